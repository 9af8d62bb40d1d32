"""``key\\tweight`` model files written and read on the device (``modeltext.hip``, the model
lines of ``textparse.hip``): the files are byte for byte what
``utils/checkpoint.write_text_model`` writes, the pairs loaded bit for bit what
``read_text_models`` yields.

Both directions are strict fast paths. The writer's formatter (csrc/core/textfmt.h) is
exact for normal f32 weights with 1e-22 <= |w| < 1e9; a chunk of entries holding any other
weight is formatted by the host code from that chunk's slice of the sorted arrays. The
reader accepts a chunk of text only when every non-empty line is plain -- digits, one tab,
a weight the scanner of csrc/core/textnum.h decides, a newline -- and otherwise parses the
chunk by the host rules, exceptions included. ``deferred_chunks`` counts those chunks. CPU
tensors / a CPU device take the host code unchanged.
"""
from __future__ import annotations

import io
import os

import numpy as np
import torch

from ..utils.checkpoint import (find_model_files, parse_model_lines, read_text_models,
                                text_model_lines, write_text_model)
from .keymix import to_unsigned_order
from .native import hipops, is_gpu

# header words of textparse.hip (ops/textparse.py)
H_ROWS, H_NNZ, H_MINW, H_MAXW, H_NONUNIT, H_BAD, H_DEFER, H_CAP = range(8)
MAX_CHUNK_ENTRIES = 1 << 24
MAX_CHUNK_BYTES = 1 << 30


# ------------------------------------------------------------------------------ writer
def sort_entries(keys: torch.Tensor, w: torch.Tensor):
    """The non-zero, non-NaN entries ordered by raw key as unsigned 64-bit integers
    (``keys``: int64 bit patterns): what ``write_text_model`` keeps, in its order."""
    keep = (w != 0) & ~torch.isnan(w)
    k, v = keys[keep], w[keep]
    sk, order = torch.sort(to_unsigned_order(k), stable=True)
    return to_unsigned_order(sk), v[order]


def write_text_model_device(path: str, keys, w, chunk_entries: int = 1 << 21,
                            stats: dict | None = None) -> tuple[int, int]:
    """Write the model file of (raw key, weight) pairs; returns (entries, deferred_chunks).
    GPU tensors (int64 key bit patterns, float32 weights) are selected, sorted and formatted
    on the device, ``chunk_entries`` at a time: chunk c is formatted into one of two device
    text buffers and copied to one of two pinned buffers while chunk c - 1 goes to the
    file. CPU tensors / arrays go to ``write_text_model``. ``stats``: filled with the
    per-chunk kernel times (ms) and the text size."""
    if not (isinstance(keys, torch.Tensor) and isinstance(w, torch.Tensor) and is_gpu(keys)
            and is_gpu(w)):
        return write_text_model(path, keys, w), 0
    if keys.dtype != torch.int64 or w.dtype != torch.float32 or keys.shape != w.shape:
        raise ValueError("write_text_model_device: int64 key bit patterns and float32 weights "
                         "of one shape")
    chunk_entries = int(chunk_entries)
    if not 1 <= chunk_entries <= MAX_CHUNK_ENTRIES:
        raise ValueError("write_text_model_device: chunk_entries must be in [1, 2^24]")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    sk, sv = sort_entries(keys.reshape(-1), w.reshape(-1))
    n = sk.numel()
    deferred = 0
    text_bytes = 0
    fmt_ms = []
    with open(path, "wb") as f:
        if n == 0:
            return 0, 0
        dev = sk.device
        ops = hipops()
        per = min(n, chunk_entries)
        cap = per * int(ops.modeltext_max_entry())
        text_dev = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
        text_pin = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        hdr_dev = [torch.zeros(3, dtype=torch.int64, device=dev) for _ in range(2)]
        hdr_pin = [torch.zeros(3, dtype=torch.int64).pin_memory() for _ in range(2)]
        work = torch.empty(int(ops.modeltext_work_bytes(per)), dtype=torch.uint8, device=dev)
        cur = torch.cuda.current_stream(dev)
        copy = torch.cuda.Stream(dev)

        def flush(item):
            if item[0] == "host":  # (a chunk the formatter declined)
                _, a, b = item
                kk = sk[a:b].cpu().numpy().view(np.uint64)
                f.write("".join(text_model_lines(kk, sv[a:b].cpu().numpy())).encode())
            else:
                _, i, nbytes, done = item
                done.synchronize()
                f.write(memoryview(text_pin[i].numpy())[:nbytes])

        pending = None
        for c, a in enumerate(range(0, n, chunk_entries)):
            b, i = min(n, a + chunk_entries), c & 1
            # (buffers i: chunk c - 2 left them when it was flushed, one iteration ago)
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record(cur)
            ops.modeltext_format(sk[a:b], sv[a:b], text_dev[i], hdr_dev[i], work)
            t1.record(cur)
            hdr_pin[i].copy_(hdr_dev[i], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(cur)
            ready.synchronize()  # (the one read-back of the chunk)
            nbytes, ndefer, over = hdr_pin[i].tolist()
            fmt_ms.append(t0.elapsed_time(t1))
            if ndefer or over:
                deferred += 1
                item = ("host", a, b)
            else:
                copy.wait_event(ready)
                with torch.cuda.stream(copy):
                    text_pin[i][:nbytes].copy_(text_dev[i][:nbytes], non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(copy)
                item = ("dev", i, nbytes, done)
                text_bytes += nbytes
            if pending is not None:
                flush(pending)  # (the file write of chunk c - 1 under the copy of chunk c)
            pending = item
        flush(pending)
        copy.synchronize()
    if stats is not None:
        stats.update(format_ms=fmt_ms, device_text_bytes=text_bytes, chunks=len(fmt_ms))
    return n, deferred


# ------------------------------------------------------------------------------ reader
def pairs_of(model: dict[int, float]) -> tuple[torch.Tensor, torch.Tensor]:
    """(raw keys as int64 bit patterns, float32 weights) of a ``read_text_models`` dict, on
    the host: the weight is (float)(the double nearest the decimal)."""
    raw = torch.from_numpy(np.fromiter(model.keys(), dtype=np.uint64,
                                       count=len(model)).view(np.int64).copy())
    w = torch.tensor(list(model.values()), dtype=torch.float64).float()
    return raw, w


class _CountingDict(dict):
    """A model dict that counts its assignments (= the files' pairs)."""

    sets = 0

    def __setitem__(self, k, v):
        self.sets += 1
        super().__setitem__(k, v)


def read_pairs_host(pattern: str) -> tuple[torch.Tensor, torch.Tensor, bool]:
    """``pairs_of(read_text_models(pattern))`` and whether some key repeated (the later
    line won)."""
    model = _CountingDict()
    for fn in find_model_files(pattern):
        with open(fn) as f:
            parse_model_lines(f, model)
    return (*pairs_of(model), model.sets != len(model))


def _host_chunk(raw: bytes) -> tuple[torch.Tensor, torch.Tensor]:
    """A chunk of whole lines by the host rules (text mode: decoding, newline translation)."""
    model: dict[int, float] = {}
    parse_model_lines(io.TextIOWrapper(io.BytesIO(raw)), model)
    return pairs_of(model)


class _LineTooLong(Exception):
    pass


def _last_newline(arr: np.ndarray, n: int) -> int:
    """Index after the last newline of arr[:n], 0 without one."""
    for lo in (max(0, n - 4096), 0):
        nl = np.flatnonzero(arr[lo:n] == 10)
        if nl.size:
            return lo + int(nl[-1]) + 1
        if lo == 0:
            break
    return 0


def iter_text_model_chunks(pattern: str, device, chunk_bytes: int = 32 << 20,
                           parse_ms: list | None = None):
    """The file loop of the device reader, one chunk at a time: yields (raw keys int64 bit
    patterns, float32 weights, deferred) per chunk of whole lines, in file order, on the GPU
    ``device``. Each file is streamed through two pinned buffers in chunks of at most
    ``chunk_bytes`` cut at a newline: file -> pinned -> HBM -> ``modeltext_parse`` on the
    current stream, and the next chunk is read from the file while the device works on the
    current one (and on whatever the consumer queued behind it).

    The tensors of a chunk the parser took are VIEWS of the reader's one pair of device
    buffers, valid until the generator is advanced: the consumer queues its work on them on
    the current stream (or clones them) first. ``deferred``: the chunk set ``H_BAD``,
    ``H_DEFER`` or ``H_CAP`` and was parsed by ``_host_chunk`` (fresh tensors). Raises
    ``_LineTooLong`` for a line longer than a chunk. ``parse_ms``: gains each chunk's parse
    kernel time."""
    dev = torch.device(device)
    files = find_model_files(pattern)
    ops = hipops()
    cap = chunk_bytes // 4 + 1  # (a line is at least "k\tw\n")
    pins = [torch.empty(chunk_bytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
    arrs = [p.numpy() for p in pins]
    text_dev = torch.empty(chunk_bytes, dtype=torch.uint8, device=dev)
    keys_buf = torch.empty(cap, dtype=torch.int64, device=dev)
    w_buf = torch.empty(cap, dtype=torch.float32, device=dev)
    hdr = torch.zeros(8, dtype=torch.int32, device=dev)
    work = torch.empty(int(ops.textparse_work_words(chunk_bytes)), dtype=torch.int32, device=dev)
    cur = torch.cuda.current_stream(dev)

    def launch(i, n):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        text_dev[:n].copy_(pins[i][:n], non_blocking=True)
        t0.record(cur)
        ops.modeltext_parse(text_dev, n, keys_buf, w_buf, hdr, work)
        t1.record(cur)
        return i, n, t0, t1

    def resolve(item):
        i, n, t0, t1 = item
        h = hdr.cpu().tolist()  # (the one read-back of the chunk)
        if parse_ms is not None:
            parse_ms.append(t0.elapsed_time(t1))
        if h[H_CAP] or h[H_BAD] or h[H_DEFER] or h[H_ROWS] != h[H_NNZ]:
            if h[H_CAP]:
                hdr.zero_()  # (the capacity flag is sticky on the device)
            k, v = _host_chunk(arrs[i][:n].tobytes())
            return k.to(dev), v.to(dev), True
        return keys_buf[:h[H_ROWS]], w_buf[:h[H_ROWS]], False

    pending = None
    slot = 0
    for fn in files:
        with open(fn, "rb") as f:
            carry = np.empty(0, dtype=np.uint8)
            while True:
                arr = arrs[slot]
                arr[:carry.size] = carry
                got = f.readinto(memoryview(arr)[carry.size:])
                n = carry.size + got
                if got:
                    cut = _last_newline(arr, n)
                    if cut == 0 and n == chunk_bytes:
                        raise _LineTooLong
                else:
                    cut = n  # (the end of the file: a last line without its newline)
                carry = arr[cut:n].copy()
                if pending is not None:
                    item, pending = pending, None
                    yield resolve(item)  # (the file read above ran under its kernels)
                if cut:
                    pending = launch(slot, cut)
                    slot ^= 1
                if not got:
                    break
    if pending is not None:
        yield resolve(pending)


def read_text_models_device(pattern: str, device, chunk_bytes: int = 32 << 20,
                            stats: dict | None = None):
    """Every ``key\\tweight`` file matching ``pattern`` (the files and the order of
    ``read_text_models``) as (raw keys int64 bit patterns, float32 weights, entries,
    deferred_chunks), the tensors on ``device`` and in file order. Each file is streamed
    through pinned memory in chunks of at most ``chunk_bytes`` cut at a newline; the next
    chunk is read from the file while the device parses the current one.

    A key that repeats is NOT resolved here (``entries`` counts pairs): in the dict reader
    the later line wins, which scattered device writes cannot promise. The caller compares
    the number of distinct keys with ``entries`` and, when they differ, loads through
    ``read_text_models`` (``ModelScorer.from_text`` does)."""
    dev = torch.device(device)
    chunk_bytes = int(chunk_bytes)
    if dev.type != "cuda":
        raw, w = pairs_of(read_text_models(pattern))
        return raw, w, raw.numel(), 0
    if not 64 <= chunk_bytes <= MAX_CHUNK_BYTES:
        raise ValueError("read_text_models_device: chunk_bytes must be in [64, 2^30]")
    parts_k, parts_w = [], []
    deferred = 0
    parse_ms = []
    try:
        for k, v, was_deferred in iter_text_model_chunks(pattern, dev, chunk_bytes, parse_ms):
            deferred += was_deferred
            if was_deferred:
                parts_k.append(k)
                parts_w.append(v)
            elif k.numel():  # (views of the reader's buffers: kept as copies)
                parts_k.append(k.clone())
                parts_w.append(v.clone())
    except _LineTooLong:  # (a line longer than a chunk: the host reader takes the model)
        raw, w = pairs_of(read_text_models(pattern))
        return raw.to(dev), w.to(dev), raw.numel(), 1
    if parts_k:
        keys, w = torch.cat(parts_k), torch.cat(parts_w)
    else:
        keys = torch.empty(0, dtype=torch.int64, device=dev)
        w = torch.empty(0, dtype=torch.float32, device=dev)
    if stats is not None:
        stats.update(parse_ms=parse_ms, chunks=len(parse_ms))
    return keys, w, keys.numel(), deferred
