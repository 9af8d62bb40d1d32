"""Per-feature-group (slot) batch loader for Darlin BCD with a local disk cache.

Reference ``SlotReader`` (src/data/slot_reader.cc:31-197): parses every file of
the worker's shard (thread pool), splits examples by slot, writes each slot of
each file to ``<cache><file>.{colidx,rowsiz,value}`` plus an ``.info`` summary,
reuses the cache when the ``.info`` file exists, and serves ``index(slot)``
(keys), ``offset(slot)`` (CSR row pointer over ALL examples) and
``value(slot)``; slot 0 is the label.

Here files are parsed by the C++ runtime (``_pscore.parse_text``), the cache is
``.npy`` arrays (loaded with ``allow_pickle=False``) plus a JSON ``.info``, and
slot info follows the reference ``InfoParser`` (src/data/info_parser.cc:10-48):
``max_key`` is exclusive (max + 1), label slot 0 has range [0, 1).

``parser="gpu"`` with a GPU ``device`` parses SPARSE_BINARY / SPARSE and ADFEA / TERAFEA
files (ops/textparse.py) on the device on a cache miss (<= 32 MiB chunks
cut at a newline, slot ids included); the arrays come back as an ``ExampleBatch`` and go through the same split and cache. Other
formats, ``.gz`` / ``hdfs://`` paths and CPU devices stay on the host parser, and so does
``parser="auto"``: with the split by slot on the host, which then bounds the load, the device
parser measured no faster than the host route.

``split="device"`` (where ``parser`` resolves to ``"gpu"``) splits every parsed chunk by slot
on the device as well (ops/slotsplit.py): the parsed arrays never cross to the host, the
chunks of a file and the files of a rank are joined on the device, and only the split arrays
come back, once -- or, with ``resident=True``, not at all: ``groups[g]`` then holds device
tensors (int64 offsets, int64 raw key bits, f32 values or None), the form
``DarlinTrainer`` takes as it is. The cache files are the host route's byte for byte (written
from a copy when resident); a cache hit returns numpy arrays on every route. Measured
(benchmarks/bench_slotreader.py, 2 M rows in 8 files): 0.72-0.76 s, resident 0.62-0.65 s,
against 0.90-0.96 s on the host route; it is opt-in all the same, the defaults and ``"auto"``
are unchanged. ``split_deferred_chunks`` counts the chunks ``SlotData.from_batch`` took after
all (more than 4096 slot ids, a row naming a group twice, too many cells). TERAFEA does
not promise that a row's groups are contiguous: such chunks take that way.
"""
from __future__ import annotations

import json
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np

from . import ExampleBatch, merge_example_info, parse_text, read_file

_CHUNK = 32 << 20  # bytes of text per device parse


@dataclass
class SlotData:
    """Examples of one worker split by feature group.

    ``groups[g] = (offset int64[rows+1], keys uint64[nnz], vals float32[nnz] | None)``
    as numpy arrays, or as torch tensors (keys: int64 raw uint64 bits) of one device.
    """

    labels: np.ndarray
    groups: dict = field(default_factory=dict)

    @property
    def rows(self) -> int:
        return int(self.labels.size)

    def info(self) -> dict:
        """ExampleInfo-like summary: {num_ex, slots: {id: {min_key, max_key, nnz_ele, nnz_ex}}}."""
        slots = {0: {"min_key": 0, "max_key": 1, "nnz_ele": self.rows, "nnz_ex": self.rows}}
        for g, (off, keys, _) in self.groups.items():
            if _is_tensor(keys):
                if keys.numel() == 0:
                    continue
                mn, mx = (keys ^ _SIGN).aminmax()  # unsigned order by way of the sign flip
                slots[g] = {"min_key": int(mn) + (1 << 63), "max_key": int(mx) + (1 << 63) + 1,
                            "nnz_ele": int(keys.numel()),
                            "nnz_ex": int((off[1:] > off[:-1]).sum())}
                continue
            if keys.size == 0:
                continue
            slots[g] = {"min_key": int(keys.min()), "max_key": int(keys.max()) + 1,
                        "nnz_ele": int(keys.size), "nnz_ex": int(np.count_nonzero(np.diff(off)))}
        return {"num_ex": self.rows, "slots": slots}

    @staticmethod
    def from_batch(batch) -> "SlotData":
        """Split a CSR ``ExampleBatch`` (with per-nnz slot ids) into slots."""
        rows = batch.rows
        row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(batch.row_ptr))
        out = SlotData(labels=batch.labels.astype(np.float32))
        for g in np.unique(batch.slots):
            m = batch.slots == g
            r = row_of[m]
            off = np.zeros(rows + 1, dtype=np.int64)
            np.cumsum(np.bincount(r, minlength=rows), out=off[1:])
            out.groups[int(g)] = (off, batch.keys[m].astype(np.uint64),
                                  None if batch.vals is None else batch.vals[m].astype(np.float32))
        return out

    @staticmethod
    def concat(parts: list["SlotData"]) -> "SlotData":
        if len(parts) == 1:
            return parts[0]
        dev = next((t[1].device for p in parts for t in p.groups.values() if _is_tensor(t[1])),
                   None)
        if dev is not None:
            return _concat_tensors(parts, dev)
        out = SlotData(labels=np.concatenate([p.labels for p in parts]))
        gids = sorted({g for p in parts for g in p.groups})
        for g in gids:
            offs, keys, vals = [np.zeros(1, np.int64)], [], []
            binary = all(p.groups.get(g, (None, None, None))[2] is None for p in parts)
            base = 0
            for p in parts:
                if g in p.groups:
                    off, k, v = p.groups[g]
                else:
                    off, k, v = np.zeros(p.rows + 1, np.int64), np.zeros(0, np.uint64), None
                offs.append(off[1:] + base)
                base += int(off[-1])
                keys.append(k)
                if not binary:
                    vals.append(np.ones(k.size, np.float32) if v is None else v)
            out.groups[g] = (np.concatenate(offs), np.concatenate(keys),
                             None if binary else np.concatenate(vals))
        return out


class SlotReader:
    def __init__(self, files, fmt: str = "LIBSVM", cache_prefix: str | None = None,
                 ignore_slot: bool = False, hadoop_home: str = "", nthreads: int = 4,
                 parser: str = "cpu", device=None, split: str = "host", resident: bool = False):
        if parser not in ("cpu", "gpu", "auto"):
            raise ValueError(f"parser must be 'cpu', 'gpu' or 'auto', not {parser!r}")
        if split not in ("host", "device"):
            raise ValueError(f"split must be 'host' or 'device', not {split!r}")
        self.files = list(files)
        self.fmt = fmt
        self.cache = cache_prefix
        self.ignore_slot = ignore_slot
        self.hadoop = hadoop_home
        self.nthreads = max(1, nthreads)
        self.hit_cache = 0
        self.device = device
        from ..ops.textparse import produces_slots

        # the parser in use: the device parser needs a GPU and a format it knows. "auto" stays
        # on the host: the load is bound by the split by slot on the host, and the device
        # route measured no faster (benchmarks/bench_slotreader.py)
        self.parser = "gpu" if (parser == "gpu" and _is_gpu_device(device)
                                and produces_slots(fmt)) else "cpu"
        self.deferred_chunks = 0  # device route: chunks the host parser took after all
        # the split by slot in use: on the device only behind the device parser
        self.split = "device" if split == "device" and self.parser == "gpu" else "host"
        self.resident = bool(resident) and self.split == "device"
        self.split_deferred_chunks = 0  # device split: chunks SlotData.from_batch took

    @staticmethod
    def from_config(data_conf, cache_conf=None, nthreads: int = 4, parser: str = "cpu",
                    device=None, split: str = "host", resident: bool = False) -> "SlotReader":
        cache = None
        if cache_conf is not None and cache_conf.has("file") and cache_conf.file:
            cache = cache_conf.file[0]
        hadoop = data_conf.hdfs.home if data_conf.has("hdfs") else ""
        return SlotReader(list(data_conf.file), data_conf.text, cache,
                          data_conf.ignore_feature_group, hadoop, nthreads, parser, device,
                          split, resident)

    def _cache_name(self, path: str) -> str:
        return f"{self.cache}{os.path.basename(path)}"

    def _load_cached(self, path: str) -> SlotData | None:
        if not self.cache:
            return None
        base = self._cache_name(path)
        try:
            with open(base + ".info") as f:
                info = json.load(f)
        except (OSError, ValueError):
            return None
        labels = np.load(base + ".label.npy", allow_pickle=False)
        sd = SlotData(labels=labels)
        for g in info["groups"]:
            off = np.load(f"{base}.{g}.rowsiz.npy", allow_pickle=False)
            keys = np.load(f"{base}.{g}.colidx.npy", allow_pickle=False)
            vf = f"{base}.{g}.value.npy"
            vals = np.load(vf, allow_pickle=False) if os.path.exists(vf) else None
            offset = np.zeros(labels.size + 1, np.int64)
            np.cumsum(off.astype(np.int64), out=offset[1:])
            sd.groups[int(g)] = (offset, keys, vals)
        return sd

    def _store_cache(self, path: str, sd: SlotData):
        if not self.cache:
            return
        base = self._cache_name(path)
        os.makedirs(os.path.dirname(base) or ".", exist_ok=True)
        np.save(base + ".label.npy", sd.labels, allow_pickle=False)
        for g, (off, keys, vals) in sd.groups.items():
            # per-example row sizes (uint16 in the reference; uint32 here)
            np.save(f"{base}.{g}.rowsiz.npy", np.diff(off).astype(np.uint32), allow_pickle=False)
            np.save(f"{base}.{g}.colidx.npy", keys, allow_pickle=False)
            if vals is not None:
                np.save(f"{base}.{g}.value.npy", vals, allow_pickle=False)
        with open(base + ".info", "w") as f:  # written last: marks the cache complete
            json.dump({"groups": sorted(sd.groups), "info": _jsonable(sd.info())}, f)

    def _read_one(self, path: str) -> SlotData:
        sd = self._load_cached(path)
        if sd is not None:
            self.hit_cache += 1
            return sd
        on_device = self.parser == "gpu" and not self.hadoop \
            and not path.startswith("hdfs://") and not path.endswith(".gz")
        if on_device and self.split == "device":
            sd = self._split_device(path)
            if sd is not None:
                if self.resident and not self.cache:
                    return sd
                host = _to_host(sd)  # (resident: the cache files are written from a copy)
                self._store_cache(path, host)
                return sd if self.resident else host
        if on_device:
            batch = self._parse_device(path)
        else:
            batch = parse_text(read_file(path, self.hadoop), self.fmt,
                               ignore_slot=self.ignore_slot)
        sd = SlotData.from_batch(batch)
        self._store_cache(path, sd)
        return sd

    @staticmethod
    def _text_chunks(raw: bytes) -> list[bytes]:
        """``raw`` in pieces of at most ``_CHUNK`` bytes, cut behind a newline."""
        out, a = [], 0
        while a < len(raw):
            b = len(raw)
            if b - a > _CHUNK:  # cut behind the chunk's last newline (a longer line: whole)
                k = raw.rfind(b"\n", a, a + _CHUNK)
                b = k + 1 if k >= 0 else (raw.find(b"\n", a + _CHUNK) + 1 or len(raw))
            out.append(raw[a:b])
            a = b
        return out

    def _split_device(self, path: str) -> SlotData | None:
        """One plain file parsed and split by slot on the device, chunk by chunk; the groups
        are device tensors. None for a file without text (the host route's)."""
        import torch

        from ..ops.slotsplit import split_by_slot
        from ..ops.textparse import parse_text_device

        with open(path, "rb") as f:
            chunks = self._text_chunks(f.read())
        if not chunks:
            return None
        parts, nonunit = [], False
        for host in chunks:
            with torch.cuda.device(self.device):
                res = parse_text_device(
                    torch.frombuffer(bytearray(host), dtype=torch.uint8).to(self.device), self.fmt,
                    ignore_slot=self.ignore_slot, host=host)
                self.deferred_chunks += bool(res.deferred)
                n = res.nnz
                nonunit |= res.vals is not None
                # unit values are a file's decision: a file of several chunks carries the
                # ones of a valued format along until every chunk is seen
                vals = res.vals
                if vals is None and res.valued and len(chunks) > 1:
                    vals = res.out.vals[:n]
                if self.ignore_slot:  # (no kernel: one group, 1, over the rows' own offsets)
                    # (copies: the parser's buffers are sized for the worst case)
                    groups = {1: (res.row_ptr - res.row_ptr[0], res.keys.clone(),
                                  None if vals is None else vals.clone())} if n else {}
                else:
                    sp = split_by_slot(None, res.row_ptr, res.keys, vals, res.slots)
                    self.split_deferred_chunks += bool(sp.deferred)
                    groups = sp.groups
                parts.append(SlotData(res.labels.cpu().numpy(), groups))
        if not nonunit:  # (every value is 1: binary features, as the host parser has it)
            for p in parts:
                p.groups = {g: (o, k, None) for g, (o, k, _) in p.groups.items()}
        return SlotData.concat(parts)

    def _parse_device(self, path: str) -> ExampleBatch:
        """One plain file through the device parser, chunk by chunk, as an ExampleBatch."""
        import torch

        from ..ops.textparse import parse_text_device

        with open(path, "rb") as f:
            raw = f.read()
        parts = []
        for host in self._text_chunks(raw):
            with torch.cuda.device(self.device):
                res = parse_text_device(
                    torch.frombuffer(bytearray(host), dtype=torch.uint8).to(self.device), self.fmt,
                    ignore_slot=self.ignore_slot, host=host)
                self.deferred_chunks += bool(res.deferred)
                n = res.nnz
                # (the host parser files every feature under slot 1 when slots are ignored)
                slots = np.ones(n, np.int32) if res.slots is None else res.slots.cpu().numpy()
                parts.append(ExampleBatch(
                    res.labels.cpu().numpy(), res.row_ptr.cpu().numpy(),
                    res.keys.cpu().numpy().view(np.uint64),
                    np.ones(n, np.float32) if res.valued and res.vals is None else
                    (None if res.vals is None else res.vals.cpu().numpy()), slots))
        if not parts:
            return parse_text(raw, self.fmt, ignore_slot=self.ignore_slot)
        if any(p.vals is not None and bool((p.vals != 1).any()) for p in parts):
            return ExampleBatch.concat(parts)
        for p in parts:  # (every value is 1: binary features, as the host parser has it)
            p.vals = None
        return ExampleBatch.concat(parts)

    def read(self) -> SlotData:
        self.hit_cache = 0
        self.deferred_chunks = 0
        self.split_deferred_chunks = 0
        with ThreadPoolExecutor(self.nthreads) as pool:
            parts = list(pool.map(self._read_one, self.files))
        if not parts:
            return SlotData(labels=np.zeros(0, np.float32))
        return SlotData.concat(parts)


_SIGN = -(1 << 63)


def _is_tensor(x) -> bool:
    return x is not None and not isinstance(x, np.ndarray) and hasattr(x, "numel")


def _to_host(sd: SlotData) -> SlotData:
    """Tensor groups as the numpy arrays of the host route (one copy each)."""
    def host(x, view=None):
        if not _is_tensor(x):
            return x
        x = x.cpu().numpy()
        return x if view is None else x.view(view)
    return SlotData(sd.labels, {g: (host(o), host(k, np.uint64), host(v))
                                for g, (o, k, v) in sd.groups.items()})


def _concat_tensors(parts: list[SlotData], dev) -> SlotData:
    """``SlotData.concat`` on the device: ``torch.cat`` with rebased offsets (numpy groups
    of a part, a cache hit among resident files, are uploaded)."""
    import torch

    def up(x, dtype):
        if _is_tensor(x):
            return x.to(dev, dtype)
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev, dtype)

    out = SlotData(labels=np.concatenate([p.labels for p in parts]))
    for g in sorted({g for p in parts for g in p.groups}):
        offs, keys, vals = [torch.zeros(1, dtype=torch.int64, device=dev)], [], []
        binary = all(p.groups.get(g, (None, None, None))[2] is None for p in parts)
        base = 0
        for p in parts:
            if g not in p.groups:
                offs.append(torch.full((p.rows,), base, dtype=torch.int64, device=dev))
                continue
            off, k, v = p.groups[g]
            k = up(k, torch.int64)
            offs.append(up(off, torch.int64)[1:] + base)
            base += int(k.numel())
            keys.append(k)
            if not binary:
                vals.append(torch.ones(k.numel(), dtype=torch.float32, device=dev)
                            if v is None else up(v, torch.float32))
        out.groups[g] = (torch.cat(offs), torch.cat(keys), None if binary else torch.cat(vals))
    return out


def _is_gpu_device(device) -> bool:
    if device is None:
        return False
    import torch

    return torch.device(device).type == "cuda"


def _jsonable(info: dict) -> dict:
    return {"num_ex": info["num_ex"], "slots": {str(k): v for k, v in info["slots"].items()}}


def merge_slot_info(infos: list[dict]) -> dict:
    """Sum of per-worker infos (reference mergeExampleInfo, data/common.cc:120-150)."""
    slots = merge_example_info([{int(k): v for k, v in i["slots"].items()} for i in infos])
    return {"num_ex": sum(i["num_ex"] for i in infos), "slots": slots}
