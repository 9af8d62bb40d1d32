"""Per-example predictions as text, formatted on the device (``scoretext.hip``): one line a
row, ``score\\n`` or ``label\\tscore\\n``, every number as Python's ``"%.9g" % float(x)``
(nine significant digits round-trip an f32).

``format_scores_host`` is the plain Python loop and the reference of everything here. The
device formatter (csrc/core/textfmt.h ``dec_score``) is a strict fast path, exact for +-0
and for normal f32 values with 1e-22 <= |x| < 1e9; a chunk of rows holding any other value
(inf, nan, a subnormal, a larger or a smaller magnitude) is formatted whole by the host loop
from the same floats. ``deferred_chunks`` counts those chunks. CPU tensors / a CPU device
take the host loop unchanged.
"""
from __future__ import annotations

import os
import time

import torch

from .native import hipops, is_gpu

MAX_CHUNK_ROWS = 1 << 24
COLUMNS = (("score",), ("label", "score"))
VALUES = ("margin", "prob")


def format_scores_host(score, label=None) -> bytes:
    """The lines of float32 ``score`` (and ``label``, the first column then) by the Python
    loop. Tensors on any device, or anything ``torch.as_tensor`` takes."""
    s = torch.as_tensor(score).detach().to("cpu", torch.float32).reshape(-1).tolist()
    if label is None:
        return "".join(["%.9g\n" % x for x in s]).encode()
    y = torch.as_tensor(label).detach().to("cpu", torch.float32).reshape(-1).tolist()
    if len(y) != len(s):
        raise ValueError("format_scores: label and score must be equally long")
    return "".join(["%.9g\t%.9g\n" % (a, b) for a, b in zip(y, s)]).encode()


def _columns(score, label):
    """(first column, second column or None) as the kernels take them."""
    return (score, None) if label is None else (label, score)


def format_scores(score: torch.Tensor, label: torch.Tensor | None = None) -> bytes:
    """``format_scores_host`` of float32 tensors; GPU tensors are formatted by the device
    kernels (one synchronising call: for streams of rows use ``PredictionWriter``)."""
    if not is_gpu(score):
        return format_scores_host(score, label)
    if score.dtype != torch.float32 or (label is not None and (
            label.dtype != torch.float32 or label.shape != score.shape or not is_gpu(label))):
        raise ValueError("format_scores: float32 GPU tensors of one shape")
    score = score.reshape(-1).contiguous()
    label = label.reshape(-1).contiguous() if label is not None else None
    n = score.numel()
    if n == 0:
        return b""
    if n > MAX_CHUNK_ROWS:
        return b"".join(format_scores(score[a:a + MAX_CHUNK_ROWS],
                                      label[a:a + MAX_CHUNK_ROWS] if label is not None else None)
                        for a in range(0, n, MAX_CHUNK_ROWS))
    ops = hipops()
    dev = score.device
    out = torch.empty(n * int(ops.scoretext_max_line(1 if label is None else 2)),
                      dtype=torch.uint8, device=dev)
    hdr = torch.zeros(3, dtype=torch.int64, device=dev)
    work = torch.empty(int(ops.scoretext_work_bytes(n)), dtype=torch.uint8, device=dev)
    ops.scoretext_format(*_columns(score, label), out, hdr, work)
    nbytes, ndefer, over = hdr.cpu().tolist()
    if ndefer or over:
        return format_scores_host(score, label)
    return out[:nbytes].cpu().numpy().tobytes()


class PredictionWriter:
    """Streams rows of (margin[, label]) into the text file ``path``.

    ``append`` copies rows (device to device, on the current stream) into a staging chunk of
    ``chunk_rows`` rows and does not synchronise; a chunk that fills is written out, and so
    is the partial last one by ``close``. On a GPU (``text_io`` "auto" or "device") a chunk
    is formatted by the device kernels into one of two device text buffers, its 3-word
    header is read back (the chunk's one synchronisation), the text is copied to one of two
    pinned buffers on a copy stream, and chunk c - 1 goes to the file under the copy of
    chunk c. A chunk whose header reports a deferred value or an overflow is formatted
    whole by ``format_scores_host`` from the same floats (``deferred_chunks``). ``text_io``
    "host", and everything on a CPU device, is the host loop per chunk; "device" on a CPU
    device raises.

    ``columns``: ("score",) or ("label", "score"). ``value``: "margin" writes the margins,
    "prob" ``torch.sigmoid`` of the chunk (float32, on the chunk's device). A probability
    under 1e-22 -- a margin below about -50.6 -- is outside the device formatter's domain
    and defers its chunk to the host loop; the file is the same, only slower.

    ``close`` returns {"rows", "bytes", "chunks", "deferred_chunks"}. ``stats`` (a dict)
    gains the per-chunk kernel and copy times (ms, device events) and the host seconds spent
    in the stages."""

    def __init__(self, path: str, device, columns=("score",), value: str = "margin",
                 text_io: str = "auto", chunk_rows: int = 1 << 20, stats: dict | None = None):
        columns = tuple(columns)
        if columns not in COLUMNS:
            raise ValueError(f"PredictionWriter: columns must be one of {COLUMNS}, not {columns!r}")
        if value not in VALUES:
            raise ValueError(f"PredictionWriter: value must be margin or prob, not {value!r}")
        if text_io not in ("auto", "host", "device"):
            raise ValueError(f"PredictionWriter: text_io must be auto, host or device, "
                             f"not {text_io!r}")
        self.device = torch.device(device)
        if text_io == "device" and self.device.type != "cuda":
            raise ValueError("PredictionWriter: text_io='device' needs a GPU device")
        self.chunk_rows = int(chunk_rows)
        if not 1 <= self.chunk_rows <= MAX_CHUNK_ROWS:
            raise ValueError("PredictionWriter: chunk_rows must be in [1, 2^24]")
        self.path, self.columns, self.value = path, columns, value
        self.on_device = text_io != "host" and self.device.type == "cuda"
        self.with_label = len(columns) == 2
        self.rows = self.bytes = self.chunks = self.deferred_chunks = 0
        self.stats = stats
        self._fmt_ms, self._d2h_ms = [], []
        self._t = {"host_format_s": 0.0, "header_wait_s": 0.0, "d2h_wait_s": 0.0,
                   "file_write_s": 0.0}
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        self._f = open(path, "wb")
        self._fill = 0
        self._score = torch.empty(self.chunk_rows, dtype=torch.float32, device=self.device)
        self._label = torch.empty_like(self._score) if self.with_label else None
        self._bufs = None     # device path: allocated with the first chunk
        self._pending = None  # the chunk whose text is on its way to the pinned buffer
        self._summary = None

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        elif self._f is not None:  # (an error elsewhere: leave what was written)
            self._f.close()
            self._f = None
        return False

    # ------------------------------------------------------------------ rows in
    def append(self, margins: torch.Tensor, labels: torch.Tensor | None = None,
               rows: int | None = None) -> None:
        """The first ``rows`` (default: all) of ``margins`` and ``labels``, in order."""
        if self._f is None:
            raise ValueError("PredictionWriter: append after close")
        n = margins.numel() if rows is None else int(rows)
        if n < 0 or n > margins.numel():
            raise ValueError("PredictionWriter.append: rows outside margins")
        if self.with_label and (labels is None or labels.numel() < n):
            raise ValueError("PredictionWriter.append: the label column needs a label per row")
        a = 0
        while a < n:
            k = min(n - a, self.chunk_rows - self._fill)
            self._score[self._fill:self._fill + k].copy_(margins[a:a + k], non_blocking=True)
            if self.with_label:
                self._label[self._fill:self._fill + k].copy_(labels[a:a + k], non_blocking=True)
            self._fill += k
            a += k
            if self._fill == self.chunk_rows:
                self._chunk()

    # ------------------------------------------------------------------ chunks out
    def _write(self, data) -> None:
        t = time.perf_counter()
        self._f.write(data)
        self._t["file_write_s"] += time.perf_counter() - t
        self.bytes += len(data)

    def _host_text(self, score, label) -> bytes:
        t = time.perf_counter()
        text = format_scores_host(score, label)
        self._t["host_format_s"] += time.perf_counter() - t
        return text

    def _flush_pending(self) -> None:
        item, self._pending = self._pending, None
        if item is None:
            return
        if item[0] == "host":  # (a chunk the formatter declined)
            self._write(item[1])
        else:
            _, i, nbytes, start, done = item
            t = time.perf_counter()
            done.synchronize()
            self._t["d2h_wait_s"] += time.perf_counter() - t
            self._d2h_ms.append(start.elapsed_time(done))
            self._write(memoryview(self._bufs["text_pin"][i].numpy())[:nbytes])

    def _alloc(self) -> dict:
        ops = hipops()
        dev = self.device
        cap = self.chunk_rows * int(ops.scoretext_max_line(len(self.columns)))
        return dict(
            text_dev=[torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)],
            text_pin=[torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)],
            hdr_dev=[torch.zeros(3, dtype=torch.int64, device=dev) for _ in range(2)],
            hdr_pin=[torch.zeros(3, dtype=torch.int64).pin_memory() for _ in range(2)],
            work=torch.empty(int(ops.scoretext_work_bytes(self.chunk_rows)), dtype=torch.uint8,
                             device=dev),
            copy=torch.cuda.Stream(dev))

    def _chunk(self) -> None:
        """Write out the staged rows."""
        n, self._fill = self._fill, 0
        if n == 0:
            return
        score = self._score[:n]
        label = self._label[:n] if self.with_label else None
        if self.value == "prob":
            score = torch.sigmoid(score)
        c = self.chunks
        self.chunks += 1
        self.rows += n
        if not self.on_device:
            self._write(self._host_text(score, label))
            return
        if self._bufs is None:
            self._bufs = self._alloc()
        B, i = self._bufs, c & 1
        # (buffers i: chunk c - 2 left them when it was flushed, one chunk ago)
        cur = torch.cuda.current_stream(self.device)
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record(cur)
        hipops().scoretext_format(*_columns(score, label), B["text_dev"][i], B["hdr_dev"][i],
                                  B["work"])
        t1.record(cur)
        B["hdr_pin"][i].copy_(B["hdr_dev"][i], non_blocking=True)
        ready = torch.cuda.Event()
        ready.record(cur)
        t = time.perf_counter()
        ready.synchronize()  # (the one read-back of the chunk)
        self._t["header_wait_s"] += time.perf_counter() - t
        nbytes, ndefer, over = B["hdr_pin"][i].tolist()
        self._fmt_ms.append(t0.elapsed_time(t1))
        if ndefer or over:
            self.deferred_chunks += 1
            item = ("host", self._host_text(score, label))
        else:
            B["copy"].wait_event(ready)
            with torch.cuda.stream(B["copy"]):
                start = torch.cuda.Event(enable_timing=True)
                done = torch.cuda.Event(enable_timing=True)
                start.record(B["copy"])
                B["text_pin"][i][:nbytes].copy_(B["text_dev"][i][:nbytes], non_blocking=True)
                done.record(B["copy"])
            item = ("dev", i, nbytes, start, done)
        self._flush_pending()  # (the file write of chunk c - 1 under the copy of chunk c)
        self._pending = item

    def close(self) -> dict:
        """Flush the partial chunk and the file; the counters of the whole stream."""
        if self._f is not None:
            try:
                self._chunk()
                self._flush_pending()
                if self._bufs is not None:
                    self._bufs["copy"].synchronize()
            finally:
                self._f.close()
                self._f = None
            self._summary = {"rows": self.rows, "bytes": self.bytes, "chunks": self.chunks,
                             "deferred_chunks": self.deferred_chunks}
            if self.stats is not None:
                self.stats.update(format_ms=self._fmt_ms, d2h_ms=self._d2h_ms, **self._t,
                                  **self._summary)
        return self._summary
