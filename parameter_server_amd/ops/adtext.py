"""The CTR log formats (``ADFEA``: ``lineid 1 click key:grp key:grp ...`` and ``TERAFEA``:
``click lineid | key key ...``, the group in the key's top 10 bits) -> CSR minibatch arrays
and per-feature slot ids on the device (``adtext.hip``), bit for bit what the host parser
(``data.parse_text(..., ignore_slot=...)``, csrc/core/data.cc parse_adfea / parse_terafea)
produces. Both formats are binary: there are no values.

A third strict fast path next to ops/textparse.py and ops/pstext.py, with the same contract:
clean input is parsed entirely by HIP kernels; a chunk holding a line the kernels do not
decide (a token longer than 64 bytes, a ``#`` opening a line, a label, key or -- with slots
kept -- group that is no number of csrc/core/textnum.h's exact domain, an ADFEA group outside
[0, 2^31), a line of one or two tokens, an ADFEA line that ends on a key or opens with a
``:``) or overflowing the output buffers is handed whole to the host parser and its result
uploaded -- the caller sees the same arrays and ``deferred=True``. A CPU buffer (or
``bytes``) takes the host parser directly. One small header is read back per call (a stream
synchronisation), so call it per chunk of text. Per-slot ``info`` statistics are not
produced; ``shuffle_fea_id`` is not taken.
"""
from __future__ import annotations

import torch

from .native import hipops, is_gpu
from .textparse import (H_BAD, H_CAP, H_DEFER, H_MAXW, H_MINW, H_NNZ, H_ROWS, MAX_CHUNK,
                        ParsedText, TextParseBuffers, _as_bytes, _fmt_id, _store_host)

_DEVICE_FORMATS = {"ADFEA": 4, "TERAFEA": 6}


def supported(fmt) -> bool:
    """Whether ``fmt`` (name or data.TEXT_FORMATS id) has a device parser here."""
    if isinstance(fmt, str):
        return fmt in _DEVICE_FORMATS
    return int(fmt) in _DEVICE_FORMATS.values()


def _host_parse(raw: bytes, fmt, hash_mod: int, ignore_slot: bool):
    from ..data import parse_text

    return parse_text(raw, fmt, ignore_slot=ignore_slot, hash_mod=hash_mod)


def parse_ad_text_device(buf, fmt, hash_mod: int = 0, *, ignore_slot: bool = True,
                         out: TextParseBuffers | None = None, row0: int = 0, nnz0: int = 0,
                         n: int | None = None, host=None):
    """Parse the first ``n`` bytes of ``buf`` (uint8 tensor; all of it by default) as
    ``fmt`` text into ``out`` behind ``row0`` rows / ``nnz0`` features already there.
    ``ignore_slot=False``: ``slots`` (int32 per feature: ADFEA's group token, TERAFEA's
    ``key >> 54`` of the key as written) is produced as well; with ``ignore_slot=True`` the
    ADFEA group tokens are not read and ``slots`` is None. ``host``: the same bytes on the
    host (bytes, or a pinned uint8 tensor) for the fallback; the device buffer is copied
    back without it. Kernels run on the current stream. Returns a ``ParsedText``."""
    fid = _fmt_id(fmt)
    hash_mod = int(hash_mod)
    want_slots = not ignore_slot
    if isinstance(buf, (bytes, bytearray, memoryview)):
        buf = torch.frombuffer(bytearray(buf), dtype=torch.uint8) if len(buf) else \
            torch.empty(0, dtype=torch.uint8)
    if buf.dtype != torch.uint8 or buf.dim() != 1:
        raise ValueError("parse_ad_text_device: buf must be a 1-d uint8 tensor")
    n = buf.numel() if n is None else int(n)
    if not 0 <= n <= buf.numel():
        raise ValueError("parse_ad_text_device: n outside the buffer")
    row0, nnz0 = int(row0), int(nnz0)
    if not is_gpu(buf):
        o = out if out is not None else TextParseBuffers(1, 1, "cpu")
        return _store_host(_host_parse(_as_bytes(buf, n), fid, hash_mod, ignore_slot), o, row0,
                           nnz0, fid, False, want_slots)
    if not supported(fid):
        raise ValueError(f"parse_ad_text_device: no device parser for format {fmt!r} "
                         f"(supported: {sorted(_DEVICE_FORMATS)})")
    if n > MAX_CHUNK:
        raise ValueError("parse_ad_text_device: at most 2^30 bytes per call")
    if out is None:  # (worst case: a row or a feature every two bytes)
        out = TextParseBuffers(row0 + n // 2 + 1, nnz0 + n // 2 + 1, buf.device)
    if row0 > out.cap_rows or nnz0 > out.cap_nnz:
        raise ValueError("parse_ad_text_device: base offsets outside the output buffers")
    if want_slots:
        out.reserve_slots()
    if n == 0:
        out.row_ptr[row0:row0 + 1].fill_(nnz0)
        return ParsedText(out.labels[row0:row0], out.row_ptr[row0:row0 + 1],
                          out.keys[nnz0:nnz0], None, 0, 0, 0, 0, False, False, out,
                          out.slots[nnz0:nnz0] if want_slots else None)
    out.reserve_work(n, ad=True)
    hipops().adtext(buf, n, fid, hash_mod, row0, nnz0, out.labels, out.row_ptr, out.keys,
                    out.slots if want_slots else None, out.hdr, out.work)
    h = out.hdr.cpu().tolist()  # (the one read-back of the call)
    if h[H_CAP] or h[H_BAD] or h[H_DEFER]:
        if h[H_CAP]:
            out.hdr.zero_()  # (the capacity flag is sticky on the device)
        raw = _as_bytes(host if host is not None else buf, n)
        return _store_host(_host_parse(raw, fid, hash_mod, ignore_slot), out, row0, nnz0, fid,
                           True, want_slots)
    rows, nnz = h[H_ROWS], h[H_NNZ]
    width = h[H_MINW] if rows and h[H_MINW] == h[H_MAXW] and h[H_MINW] > 0 else 0
    return ParsedText(out.labels[row0:row0 + rows], out.row_ptr[row0:row0 + rows + 1],
                      out.keys[nnz0:nnz0 + nnz], None, rows, nnz, 0, width, False, False, out,
                      out.slots[nnz0:nnz0 + nnz] if want_slots else None)
