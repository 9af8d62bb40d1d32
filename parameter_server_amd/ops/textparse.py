"""Text -> CSR minibatch arrays on the device, bit for bit what the host parser
(``data.parse_text(..., ignore_slot=...)``, csrc/core/data.cc) produces. One entry,
``parse_text_device``, for the six formats with HIP kernels (``FORMATS``):

* LIBSVM, CRITEO (``textparse.hip``): no slot ids. The kernels hand back a malformed line, a
  ``#`` comment, a number outside the exact domain of csrc/core/textnum.h, a token longer
  than 64 bytes.
* SPARSE_BINARY ``label; grp key key ...; grp key ...;`` and SPARSE, the same with
  ``key:value`` (``pstext.hip``, host: parse_ps): with ``ignore_slot=False`` every feature
  gets its group head's value. Handed back: a long token, an inexact number, a ``#`` line, a
  second token before a line's first ``;``, a ``;`` on a line without a label, a ``:`` inside
  a SPARSE_BINARY key, a SPARSE feature that is not exactly ``digits:number``, with slots a
  group head that is no integer in [0, 2^31).
* ADFEA ``lineid 1 click key:grp key:grp ...`` and TERAFEA ``click lineid | key key ...``,
  the group in the key's top 10 bits (``adtext.hip``, host: parse_adfea / parse_terafea):
  binary, no values; ``shuffle_fea_id`` is not taken. Handed back: a long token, a ``#``
  opening a line, a label, key or -- with slots kept -- group that is no exact number, an
  ADFEA group outside [0, 2^31), a line of one or two tokens, an ADFEA line that ends on a
  key or opens with a ``:``.

Each is a strict fast path: clean input is parsed entirely by HIP kernels; a chunk holding a
line the kernels hand back, or overflowing the output buffers, goes whole to the host parser
and its result is uploaded -- the caller sees the same arrays and ``deferred=True``. Per-slot
``info`` statistics are not produced. A CPU buffer (or ``bytes``) takes the host parser
directly. One small header is read back per call (a stream synchronisation), so call it per
chunk of text, not per minibatch.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from .native import hipops, is_gpu


class TextFormat(NamedTuple):
    id: int        # data.TEXT_FORMATS
    valued: bool   # parsed chunks keep their values in the ``vals`` buffer (ones included)
    slots: bool    # ``ignore_slot=False`` yields a slot id per feature
    family: str    # the .hip file that holds its kernels


# the formats with a device parser
FORMATS = {
    "LIBSVM": TextFormat(5, True, False, "textparse"),
    "CRITEO": TextFormat(8, False, False, "textparse"),
    "SPARSE": TextFormat(2, True, True, "pstext"),
    "SPARSE_BINARY": TextFormat(3, False, True, "pstext"),
    "ADFEA": TextFormat(4, False, True, "adtext"),
    "TERAFEA": TextFormat(6, False, True, "adtext"),
}
_BY_ID = {t.id: t for t in FORMATS.values()}
_VALUED_FORMATS = tuple(t.id for t in FORMATS.values() if t.valued)
# header words of textparse.cuh
H_ROWS, H_NNZ, H_MINW, H_MAXW, H_NONUNIT, H_BAD, H_DEFER, H_CAP = range(8)
MAX_CHUNK = 1 << 30


def traits(fmt) -> TextFormat | None:
    """The table entry of ``fmt`` (name or data.TEXT_FORMATS id); None without a device parser."""
    return FORMATS.get(fmt) if isinstance(fmt, str) else _BY_ID.get(int(fmt))


def supported(fmt) -> bool:
    """Whether ``fmt`` (name or data.TEXT_FORMATS id) has a device parser."""
    return traits(fmt) is not None


def produces_slots(fmt) -> bool:
    """Whether ``fmt``'s device parser can keep slot ids (the slot-grouped and CTR formats)."""
    t = traits(fmt)
    return t is not None and t.slots


def _fmt_id(fmt) -> int:
    from ..data import TEXT_FORMATS

    return TEXT_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)


class TextParseBuffers:
    """Caller-owned outputs of the device parser: ``labels`` f32 [cap_rows], ``row_ptr``
    i64 [cap_rows + 1], ``keys`` i64 [cap_nnz] (u64 bit patterns), ``vals`` f32 [cap_nnz],
    the header and the kernels' work space. ``slots`` i32 [cap_nnz] (the feature group of
    every entry) is allocated on first use and then grown and carried like ``keys``."""

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
            self.reserve_work(text_bytes, "LIBSVM")

    @property
    def cap_rows(self) -> int:
        return self.labels.numel()

    @property
    def cap_nnz(self) -> int:
        return self.keys.numel()

    def reserve_work(self, n: int, fmt):
        """Work space for ``n`` bytes of ``fmt`` text."""
        need = int(hipops().textparse_work_words(n, _fmt_id(fmt)))
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
    slots: torch.Tensor | None = None  # i32 [nnz]: feature group per entry (ignore_slot=False)


def _as_bytes(buf, n) -> bytes:
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return bytes(buf[:n])
    return buf[:n].cpu().numpy().tobytes()


def _host_parse(raw: bytes, fmt, hash_mod: int, ignore_slot: bool):
    from ..data import parse_text

    return parse_text(raw, fmt, ignore_slot=ignore_slot, hash_mod=hash_mod)


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


def parse_text_device(buf, fmt, hash_mod: int = 0, *, ignore_slot: bool = True,
                      out: TextParseBuffers | None = None, row0: int = 0, nnz0: int = 0,
                      n: int | None = None, host=None):
    """Parse the first ``n`` bytes of ``buf`` (uint8 tensor; all of it by default) as
    ``fmt`` text into ``out`` behind ``row0`` rows / ``nnz0`` features already there (rows
    carried over from the previous chunk). ``ignore_slot=False`` (the formats of
    ``produces_slots``): ``slots`` (int32 per feature: its group head's value, ADFEA's group
    token, TERAFEA's ``key >> 54`` of the key as written) is produced as well; with
    ``ignore_slot=True`` the groups are not read and ``slots`` is None. ``host``: the same
    bytes on the host (bytes, or a pinned uint8 tensor) for the fallback; the device buffer
    is copied back without it. Kernels run on the current stream. Returns a ``ParsedText``.
    A format name that data.TEXT_FORMATS does not know is a ``KeyError``, as it is in
    ``data.parse_text``; every other rejection is a ``ValueError``."""
    fid = _fmt_id(fmt)
    t = traits(fid)
    hash_mod = int(hash_mod)
    want_slots = not ignore_slot
    if want_slots and t is not None and not t.slots:
        raise ValueError(f"parse_text_device: format {fmt!r} has no slot ids (ignore_slot=False)")
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
        return _store_host(_host_parse(_as_bytes(buf, n), fid, hash_mod, ignore_slot), o, row0,
                           nnz0, fid, False, want_slots)
    if t is None:
        raise ValueError(f"parse_text_device: no device parser for format {fmt!r} "
                         f"(supported: {sorted(FORMATS)})")
    if n > MAX_CHUNK:
        raise ValueError("parse_text_device: at most 2^30 bytes per call")
    if out is None:  # (worst case: a row or a feature every two bytes)
        out = TextParseBuffers(row0 + n // 2 + 1, nnz0 + n // 2 + 1, buf.device)
    if row0 > out.cap_rows or nnz0 > out.cap_nnz:
        raise ValueError("parse_text_device: base offsets outside the output buffers")
    if want_slots:
        out.reserve_slots()
    if n == 0:
        out.row_ptr[row0:row0 + 1].fill_(nnz0)
        return ParsedText(out.labels[row0:row0], out.row_ptr[row0:row0 + 1],
                          out.keys[nnz0:nnz0], None, 0, 0, 0, 0, False, t.valued, out,
                          out.slots[nnz0:nnz0] if want_slots else None)
    out.reserve_work(n, fid)
    hipops().textparse(buf, n, fid, hash_mod, row0, nnz0, out.labels, out.row_ptr, out.keys,
                       out.vals if t.valued else None, out.slots if want_slots else None,
                       out.hdr, out.work)
    h = out.hdr.cpu().tolist()  # (the one read-back of the call)
    if h[H_CAP] or h[H_BAD] or h[H_DEFER]:
        if h[H_CAP]:
            out.hdr.zero_()  # (the capacity flag is sticky on the device)
        raw = _as_bytes(host if host is not None else buf, n)
        return _store_host(_host_parse(raw, fid, hash_mod, ignore_slot), out, row0, nnz0, fid,
                           True, want_slots)
    rows, nnz = h[H_ROWS], h[H_NNZ]
    width = h[H_MINW] if rows and h[H_MINW] == h[H_MAXW] and h[H_MINW] > 0 else 0
    vals = out.vals[nnz0:nnz0 + nnz] if t.valued and h[H_NONUNIT] else None
    return ParsedText(out.labels[row0:row0 + rows], out.row_ptr[row0:row0 + rows + 1],
                      out.keys[nnz0:nnz0 + nnz], vals, rows, nnz, 0, width, False, t.valued, out,
                      out.slots[nnz0:nnz0 + nnz] if want_slots else None)


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
