"""Text -> CSR minibatch arrays on the device (``textparse.hip``), bit for bit what the
host parser (``data.parse_text(..., ignore_slot=True)``, csrc/core/data.cc) produces.

The device parser is a strict fast path for LIBSVM and CRITEO text: clean input is parsed
entirely by HIP kernels; a chunk holding a line the kernels do not decide (a malformed
line, a ``#`` comment, a number outside the exact domain of csrc/core/textnum.h, a token
longer than 64 bytes) or overflowing the output buffers is handed whole to the host
parser and its result uploaded -- the caller sees the same arrays and ``deferred=True``.
Slot ids and per-slot info are not produced. A CPU buffer (or ``bytes``) takes the host
parser directly. One small header is read back per call (a stream synchronisation), so
call it per chunk of text, not per minibatch.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .native import hipops, is_gpu

_DEVICE_FORMATS = {"LIBSVM": 5, "CRITEO": 8}
# formats whose parsed chunks keep their values in the ``vals`` buffer (ones included)
_VALUED_FORMATS = (5, 2)  # LIBSVM, SPARSE (ops/pstext.py)
# header words of textparse.hip
H_ROWS, H_NNZ, H_MINW, H_MAXW, H_NONUNIT, H_BAD, H_DEFER, H_CAP = range(8)
MAX_CHUNK = 1 << 30


def supported(fmt) -> bool:
    """Whether ``fmt`` (name or data.TEXT_FORMATS id) has a device parser."""
    if isinstance(fmt, str):
        return fmt in _DEVICE_FORMATS
    return int(fmt) in _DEVICE_FORMATS.values()


def _fmt_id(fmt) -> int:
    from ..data import TEXT_FORMATS

    return TEXT_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)


class TextParseBuffers:
    """Caller-owned outputs of the device parser: ``labels`` f32 [cap_rows], ``row_ptr``
    i64 [cap_rows + 1], ``keys`` i64 [cap_nnz] (u64 bit patterns), ``vals`` f32 [cap_nnz],
    the header and the kernels' work space. ``slots`` i32 [cap_nnz] (the feature group of
    every entry, ops/pstext.py) is allocated on first use and then grown and carried like
    ``keys``."""

    def __init__(self, cap_rows: int, cap_nnz: int, device, text_bytes: int = 0):
        dev = torch.device(device)
        self.device = dev
        self.labels = torch.empty(max(1, cap_rows), dtype=torch.float32, device=dev)
        self.row_ptr = torch.zeros(max(1, cap_rows) + 1, dtype=torch.int64, device=dev)
        self.keys = torch.empty(max(1, cap_nnz), dtype=torch.int64, device=dev)
        self.vals = torch.empty(max(1, cap_nnz), dtype=torch.float32, device=dev)
        self.slots = None
        self.hdr = torch.zeros(8, dtype=torch.int32, device=dev)
        self.work = None
        if text_bytes and dev.type == "cuda":
            self.reserve_work(text_bytes)

    @property
    def cap_rows(self) -> int:
        return self.labels.numel()

    @property
    def cap_nnz(self) -> int:
        return self.keys.numel()

    def reserve_work(self, n: int, ps: bool = False, ad: bool = False):
        """Work space for ``n`` bytes of text (``ps``: for the parser of ops/pstext.py,
        ``ad``: for the one of ops/adtext.py)."""
        words = hipops().adtext_work_words if ad else \
            hipops().pstext_work_words if ps else hipops().textparse_work_words
        need = int(words(n))
        if self.work is None or self.work.numel() < need:
            self.work = torch.empty(need, dtype=torch.int32, device=self.device)

    def reserve_slots(self):
        if self.slots is None:
            self.slots = torch.empty(self.cap_nnz, dtype=torch.int32, device=self.device)

    def grow(self, rows: int, nnz: int, keep_rows: int = 0, keep_nnz: int = 0):
        """Room for ``rows`` / ``nnz`` in new tensors (earlier views stay valid); the first
        ``keep_rows`` rows / ``keep_nnz`` features are copied over."""
        if rows > self.cap_rows:
            lab = torch.empty(rows, dtype=torch.float32, device=self.device)
            rp = torch.zeros(rows + 1, dtype=torch.int64, device=self.device)
            lab[:keep_rows].copy_(self.labels[:keep_rows])
            rp[:keep_rows + 1].copy_(self.row_ptr[:keep_rows + 1])
            self.labels, self.row_ptr = lab, rp
        if nnz > self.cap_nnz:
            k = torch.empty(nnz, dtype=torch.int64, device=self.device)
            v = torch.empty(nnz, dtype=torch.float32, device=self.device)
            k[:keep_nnz].copy_(self.keys[:keep_nnz])
            v[:keep_nnz].copy_(self.vals[:keep_nnz])
            if self.slots is not None:
                sl = torch.empty(nnz, dtype=torch.int32, device=self.device)
                sl[:keep_nnz].copy_(self.slots[:keep_nnz])
                self.slots = sl
            self.keys, self.vals = k, v


@dataclass
class ParsedText:
    labels: torch.Tensor          # f32 [rows]            (views of the output buffers,
    row_ptr: torch.Tensor         # i64 [rows + 1]         behind row0 / nnz0)
    keys: torch.Tensor            # i64 [nnz], u64 bit patterns, mod hash_mod when given
    vals: torch.Tensor | None     # f32 [nnz]; None when every value is 1 (binary features)
    rows: int
    nnz: int
    bad_lines: int
    width: int                    # > 0: every row has exactly this many features
    deferred: bool                # the host parser produced the arrays
    valued: bool = False          # ``vals`` buffer region holds the values (ones included)
    out: TextParseBuffers | None = None
    slots: torch.Tensor | None = None  # i32 [nnz]: feature group per entry (ops/pstext.py)


def _as_bytes(buf, n) -> bytes:
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return bytes(buf[:n])
    return buf[:n].cpu().numpy().tobytes()


def _host_parse(raw: bytes, fmt, hash_mod: int):
    from ..data import parse_text

    return parse_text(raw, fmt, ignore_slot=True, hash_mod=hash_mod)


def _width_of(rp: np.ndarray) -> int:
    if rp.size < 2:
        return 0
    w = np.diff(rp)
    return int(w[0]) if w[0] > 0 and bool((w == w[0]).all()) else 0


def _store_host(b, out: TextParseBuffers, row0: int, nnz0: int, fmt_id: int, deferred: bool,
                slots: bool = False):
    """Upload a host-parsed batch behind row0 / nnz0 (the buffers grow when it does not
    fit: a chunk the device declined may be denser than its capacity). ``slots``: the
    batch's slot ids as well."""
    rows, nnz = b.rows, b.nnz
    if slots:
        out.reserve_slots()
    out.grow(row0 + rows, nnz0 + nnz, row0, nnz0)
    rp = np.asarray(b.row_ptr, dtype=np.int64)
    out.labels[row0:row0 + rows].copy_(torch.from_numpy(np.ascontiguousarray(b.labels)))
    out.row_ptr[row0:row0 + rows + 1].copy_(torch.from_numpy(rp + nnz0))
    out.keys[nnz0:nnz0 + nnz].copy_(
        torch.from_numpy(np.ascontiguousarray(b.keys).view(np.int64)))
    valued = fmt_id in _VALUED_FORMATS or b.vals is not None
    if b.vals is not None:
        out.vals[nnz0:nnz0 + nnz].copy_(torch.from_numpy(np.ascontiguousarray(b.vals)))
    elif valued:
        out.vals[nnz0:nnz0 + nnz].fill_(1.0)
    return ParsedText(out.labels[row0:row0 + rows], out.row_ptr[row0:row0 + rows + 1],
                      out.keys[nnz0:nnz0 + nnz],
                      None if b.vals is None else out.vals[nnz0:nnz0 + nnz], rows, nnz,
                      int(b.info.get("bad_lines", 0)), _width_of(rp), deferred, valued, out,
                      _store_slots(b, out, nnz0) if slots else None)


def _store_slots(b, out: TextParseBuffers, nnz0: int):
    nnz = b.nnz
    out.slots[nnz0:nnz0 + nnz].copy_(
        torch.from_numpy(np.ascontiguousarray(b.slots, dtype=np.int32)))
    return out.slots[nnz0:nnz0 + nnz]


def parse_text_device(buf, fmt, hash_mod: int = 0, *, out: TextParseBuffers | None = None,
                      row0: int = 0, nnz0: int = 0, n: int | None = None, host=None):
    """Parse the first ``n`` bytes of ``buf`` (uint8 tensor; all of it by default) as
    ``fmt`` text into ``out`` behind ``row0`` rows / ``nnz0`` features already there (rows
    carried over from the previous chunk). ``host``: the same bytes on the host (bytes, or
    a pinned uint8 tensor) for the fallback; the device buffer is copied back without it.
    Kernels run on the current stream. Returns a ``ParsedText``."""
    fid = _fmt_id(fmt)
    hash_mod = int(hash_mod)
    if isinstance(buf, (bytes, bytearray, memoryview)):
        buf = torch.frombuffer(bytearray(buf), dtype=torch.uint8) if len(buf) else \
            torch.empty(0, dtype=torch.uint8)
    if buf.dtype != torch.uint8 or buf.dim() != 1:
        raise ValueError("parse_text_device: buf must be a 1-d uint8 tensor")
    n = buf.numel() if n is None else int(n)
    if not 0 <= n <= buf.numel():
        raise ValueError("parse_text_device: n outside the buffer")
    row0, nnz0 = int(row0), int(nnz0)
    if not is_gpu(buf):
        o = out if out is not None else TextParseBuffers(1, 1, "cpu")
        return _store_host(_host_parse(_as_bytes(buf, n), fid, hash_mod), o, row0, nnz0, fid, False)
    if not supported(fid):
        raise ValueError(f"parse_text_device: no device parser for format {fmt!r} "
                         f"(supported: {sorted(_DEVICE_FORMATS)})")
    if n > MAX_CHUNK:
        raise ValueError("parse_text_device: at most 2^30 bytes per call")
    if out is None:  # (worst case: a row or a feature every two bytes)
        out = TextParseBuffers(row0 + n // 2 + 1, nnz0 + n // 2 + 1, buf.device)
    if row0 > out.cap_rows or nnz0 > out.cap_nnz:
        raise ValueError("parse_text_device: base offsets outside the output buffers")
    libsvm = fid == _DEVICE_FORMATS["LIBSVM"]
    if n == 0:
        out.row_ptr[row0:row0 + 1].fill_(nnz0)
        return ParsedText(out.labels[row0:row0], out.row_ptr[row0:row0 + 1],
                          out.keys[nnz0:nnz0], None, 0, 0, 0, 0, False, libsvm, out)
    out.reserve_work(n)
    hipops().textparse(buf, n, fid, hash_mod, row0, nnz0, out.labels, out.row_ptr, out.keys,
                       out.vals if libsvm else None, out.hdr, out.work)
    h = out.hdr.cpu().tolist()  # (the one read-back of the call)
    if h[H_CAP] or h[H_BAD] or h[H_DEFER]:
        if h[H_CAP]:
            out.hdr.zero_()  # (the capacity flag is sticky on the device)
        raw = _as_bytes(host if host is not None else buf, n)
        return _store_host(_host_parse(raw, fid, hash_mod), out, row0, nnz0, fid, True)
    rows, nnz = h[H_ROWS], h[H_NNZ]
    width = h[H_MINW] if rows and h[H_MINW] == h[H_MAXW] and h[H_MINW] > 0 else 0
    vals = out.vals[nnz0:nnz0 + nnz] if libsvm and h[H_NONUNIT] else None
    return ParsedText(out.labels[row0:row0 + rows], out.row_ptr[row0:row0 + rows + 1],
                      out.keys[nnz0:nnz0 + nnz], vals, rows, nnz, 0, width, False, libsvm, out)


def rebase_row_ptr(src: torch.Tensor, dst: torch.Tensor, n: int, delta: int):
    """dst[:n] = src[:n] - delta (a minibatch's row offsets out of a chunk's)."""
    if is_gpu(src):
        hipops().textparse_rebase(src, dst, int(n), int(delta))
    else:
        torch.sub(src[:n], int(delta), out=dst[:n])


def segments_valued(vals: torch.Tensor, bounds: torch.Tensor) -> torch.Tensor:
    """int32 flag per segment [bounds[s], bounds[s+1]): some value differs from 1."""
    flags = torch.zeros(max(0, bounds.numel() - 1), dtype=torch.int32, device=vals.device)
    if flags.numel() == 0:
        return flags
    if is_gpu(vals):
        hipops().textparse_seg_nonunit(vals, bounds, flags)
    else:
        b = bounds.tolist()
        for s in range(flags.numel()):
            flags[s] = int(bool((vals[b[s]:b[s + 1]] != 1).any()))
    return flags
