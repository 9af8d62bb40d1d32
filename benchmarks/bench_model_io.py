"""Saving and loading a ``key\\tweight`` text model on one GPU: the device paths
(ops/modeltext.py: modeltext.hip, the model lines of textparse.hip) against the host code
(utils/checkpoint.py) on the same table, alternating in one process.

    python benchmarks/bench_model_io.py --entries 20000000

* The model: ``--entries`` distinct random 64-bit keys with non-zero weights of trained
  magnitude (normal / 10) in a ``KVTable`` at load <= 0.5.
* Save, as ``SparseLRTrainer.save_model`` does it: occupied slots -> raw keys -> file;
  ``text_io="host"`` (copy to the host, ``write_text_model``) and ``"device"`` in
  alternation, ``--repeats`` times; the two files are compared byte for byte.
* Load, as ``ModelScorer.from_text`` does it: file -> pairs -> a new table; ``"host"`` (the
  dict reader) and ``"device"`` in alternation; the two tables are compared.
* Stages of the device paths, each timed on its own: selection + sort, the format kernels
  per chunk, a device-to-host copy of the text, a plain write of the text to a file; a
  plain read of the file, the parse kernels per chunk, the table insert.
* Warm start (``--rows warm`` runs this row alone), from the same file into a fresh
  ``SparseLRTrainer``: ``load_model`` (file -> parse -> kv_seed per chunk, one stream)
  against the composed path -- ``read_text_models_device`` (the whole model in HBM) + ``mix``
  + owner mask + the FTRL ``z`` in torch + ``KVTable.load`` -- in alternation, best of
  ``--repeats``; the two tables are compared; peak HBM of each above what was allocated
  before it (``torch.cuda.max_memory_allocated``); kv_seed's own time (events around it).

Prints one JSON line; progress goes to stderr."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def log(*a):
    print("[bench_model_io]", *a, file=sys.stderr, flush=True)


def warm_start_row(pat: str, N: int, a, res: dict):
    """load_model against the composed path on fresh trainers; fills ``res``."""
    import torch

    from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
    from parameter_server_amd.ops.keymix import mix
    from parameter_server_amd.ops.modeltext import read_text_models_device

    dev = torch.device("cuda")
    cap = 1 << max(10, (4 * N - 1).bit_length() - 1)  # load in (0.25, 0.5]
    cfg = SparseLRConfig(num_features=0, minibatch=1024, table_capacity=cap)

    def fused(tr):
        evs = []
        seed = tr.table.seed

        def timed(*args, **kw):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            seed(*args, **kw)
            e1.record()
            evs.append((e0, e1))
        tr.table.seed = timed
        r = tr.load_model(pat, chunk_bytes=a.chunk_bytes)
        torch.cuda.synchronize()
        assert r["seeded"] == N and r["deferred_chunks"] == 0, r
        return sum(e0.elapsed_time(e1) for e0, e1 in evs) / 1e3

    def composed(tr):
        rk, ww, entries, deferred = read_text_models_device(pat, dev, chunk_bytes=a.chunk_bytes)
        h = mix(rk, tr.bits)
        own = tr.part.owner_of(h) == tr.rank
        c = tr.cfg
        z = -(ww * ((0.0 + c.beta) / c.alpha + c.l2) + torch.copysign(torch.full_like(ww, c.l1), ww))
        tr.table.load(h[own], ww[own], z[own], torch.zeros_like(ww)[own])
        assert entries == N and deferred == 0
        return 0.0

    times = {"load_model": [], "composed": []}
    peaks, kernel, tabs = {}, [], {}
    fused(SparseLRTrainer(cfg, device=dev))  # (warm-up)
    for r in range(a.repeats):
        for name, fn in (("composed", composed), ("load_model", fused)):
            tabs.pop(name, None)
            tr = SparseLRTrainer(cfg, device=dev)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            ks = fn(tr)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            times[name].append(t)
            peaks[name] = torch.cuda.max_memory_allocated() - base
            if name == "load_model":
                kernel.append(ks)
            tabs[name] = tr
            log(f"warm start {name} #{r}: {t:.3f} s, {N / t / 1e6:.2f} M entries/s, "
                f"peak HBM above the trainer {peaks[name] / 2 ** 20:.0f} MiB")
    (ak, aw, az, an), (bk, bw, bz, bn) = (tabs[m].table.occupied()
                                          for m in ("load_model", "composed"))
    ao, bo = torch.argsort(ak), torch.argsort(bk)
    assert torch.equal(ak[ao], bk[bo]) and torch.equal(aw[ao].view(torch.int32),
                                                       bw[bo].view(torch.int32))
    torch.testing.assert_close(az[ao], bz[bo], rtol=1e-6, atol=0)
    for name in times:
        t = min(times[name])
        res[f"warm_{name}_s"] = round(t, 4)
        res[f"warm_{name}_entries_per_s"] = round(N / t)
        res[f"warm_{name}_peak_hbm_bytes"] = int(peaks[name])
    res["warm_kv_seed_kernels_s"] = round(min(kernel), 4)
    res["warm_table_capacity"] = cap
    res["warm_tables_identical"] = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=20_000_000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--chunk-entries", type=int, default=1 << 21)
    ap.add_argument("--chunk-bytes", type=int, default=32 << 20)
    ap.add_argument("--dir", default=None, help="where the model files go (default: a temp dir)")
    ap.add_argument("--rows", choices=("all", "warm"), default="all",
                    help="warm: only the warm-start row (the file is written by one device save)")
    a = ap.parse_args()

    import torch

    from parameter_server_amd.models import ModelScorer
    from parameter_server_amd.ops.keymix import mix, unmix
    from parameter_server_amd.ops.modeltext import (read_text_models_device, sort_entries,
                                                    write_text_model_device)
    from parameter_server_amd.utils.checkpoint import write_text_model

    dev = torch.device("cuda")
    N, bits = a.entries, 64
    g = torch.Generator(device=dev).manual_seed(1)
    half = lambda: torch.randint(0, 1 << 32, (N + N // 64,), generator=g, device=dev,  # noqa: E731
                                 dtype=torch.int64)
    raw = torch.unique((half() << 32) | half())[:N]  # (the top half wraps: keys above 2^63)
    raw = raw[torch.randperm(raw.numel(), generator=g, device=dev)]
    w = torch.randn(raw.numel(), generator=g, device=dev) * 0.1
    w[w == 0] = 0.1
    sc = ModelScorer.from_pairs(mix(raw, bits), w, bits, dev)
    del raw, w
    table = sc.table
    N = table.census()[1]
    log(f"table: {N} non-zero weights, capacity {table.capacity}")
    out = a.dir or tempfile.mkdtemp(prefix="model_io_")
    os.makedirs(out, exist_ok=True)

    def sync():
        torch.cuda.synchronize()

    def save(mode, path):
        sync()
        t0 = time.perf_counter()
        keys, ww = table.occupied_weights()
        rk = unmix(keys, bits)
        stats = {}
        if mode == "device":
            n, deferred = write_text_model_device(path, rk, ww, chunk_entries=a.chunk_entries,
                                                  stats=stats)
        else:
            n, deferred = write_text_model(path, rk.cpu(), ww.cpu()), 0
        sync()
        return time.perf_counter() - t0, n, deferred, stats

    res = {"entries": N, "chunk_entries": a.chunk_entries, "chunk_bytes": a.chunk_bytes}
    paths = {m: os.path.join(out, m, "m_S0") for m in ("host", "device")}
    save("device", paths["device"])  # (warm-up: allocator, pinned memory, file cache)
    if a.rows == "warm":
        warm_start_row(os.path.join(out, "device", "m_S.*"), N, a, res)
        if a.dir is None:
            shutil.rmtree(out, ignore_errors=True)
        print(json.dumps(res))
        return
    times = {"host": [], "device": []}
    for r in range(a.repeats):
        for mode in ("host", "device"):
            t, n, deferred, stats = save(mode, paths[mode])
            times[mode].append(t)
            log(f"save {mode} #{r}: {t:.3f} s, {n / t / 1e6:.2f} M entries/s, deferred {deferred}")
            if mode == "device":
                res["save_deferred_chunks"] = deferred
                res["save_format_ms_per_chunk"] = [round(x, 3) for x in stats["format_ms"]]
    size = os.path.getsize(paths["device"])
    with open(paths["host"], "rb") as f, open(paths["device"], "rb") as h:
        same = all(x == y for x, y in iter(lambda: (f.read(1 << 24), h.read(1 << 24)),
                                           (b"", b"")))
    assert same and size == os.path.getsize(paths["host"]), "device file differs from host file"
    res.update(text_bytes=size, files_identical=True)
    for mode in ("host", "device"):
        t = min(times[mode])
        res[f"save_{mode}_s"] = round(t, 4)
        res[f"save_{mode}_entries_per_s"] = round(N / t)
        res[f"save_{mode}_text_gb_per_s"] = round(size / t / 1e9, 4)

    # the device save's stages, one at a time
    keys, ww = table.occupied_weights()
    rk = unmix(keys, bits)
    sync()
    t0 = time.perf_counter()
    sk, sv = sort_entries(rk, ww)
    sync()
    res["save_stage_select_sort_s"] = round(time.perf_counter() - t0, 4)
    res["save_stage_format_kernels_s"] = round(sum(res["save_format_ms_per_chunk"]) / 1e3, 4)
    del keys, ww, rk, sk, sv
    text_dev = torch.empty(size, dtype=torch.uint8, device=dev)
    text_pin = torch.empty(size, dtype=torch.uint8).pin_memory()
    sync()
    t0 = time.perf_counter()
    text_pin.copy_(text_dev, non_blocking=True)
    sync()
    res["save_stage_d2h_copy_s"] = round(time.perf_counter() - t0, 4)
    t0 = time.perf_counter()
    with open(os.path.join(out, "plain_write"), "wb") as f:
        f.write(memoryview(text_pin.numpy()))
    res["save_stage_file_write_s"] = round(time.perf_counter() - t0, 4)
    os.remove(os.path.join(out, "plain_write"))

    # ---- load
    pat = os.path.join(out, "device", "m_S.*")
    times = {"host": [], "device": []}
    tabs = {}
    ModelScorer.from_text(pat, bits, dev, text_io="device")  # (warm-up)
    for r in range(a.repeats):
        for mode in ("host", "device"):
            tabs.pop(mode, None)
            sync()
            t0 = time.perf_counter()
            s = ModelScorer.from_text(pat, bits, dev, text_io=mode)
            sync()
            t = time.perf_counter() - t0
            times[mode].append(t)
            tabs[mode] = s
            log(f"load {mode} #{r}: {t:.3f} s, {s.entries / t / 1e6:.2f} M entries/s, "
                f"deferred {s.deferred_chunks}")
    assert tabs["host"].entries == tabs["device"].entries == N
    (hk, hw), (dk, dw) = tabs["host"].table.occupied_weights(), \
        tabs["device"].table.occupied_weights()
    ho, do = torch.argsort(hk), torch.argsort(dk)
    assert torch.equal(hk[ho], dk[do]) and torch.equal(hw[ho].view(torch.int32),
                                                       dw[do].view(torch.int32))
    res.update(tables_identical=True, load_deferred_chunks=tabs["device"].deferred_chunks)
    del tabs, hk, hw, dk, dw, ho, do
    for mode in ("host", "device"):
        t = min(times[mode])
        res[f"load_{mode}_s"] = round(t, 4)
        res[f"load_{mode}_entries_per_s"] = round(N / t)
        res[f"load_{mode}_text_gb_per_s"] = round(size / t / 1e9, 4)

    # the device load's stages, one at a time
    t0 = time.perf_counter()
    with open(paths["device"], "rb") as f:
        got = f.readinto(memoryview(text_pin.numpy()))
    res["load_stage_file_read_s"] = round(time.perf_counter() - t0, 4)
    assert got == size
    sync()
    t0 = time.perf_counter()
    text_dev.copy_(text_pin, non_blocking=True)
    sync()
    res["load_stage_h2d_copy_s"] = round(time.perf_counter() - t0, 4)
    del text_dev, text_pin
    stats = {}
    sync()
    t0 = time.perf_counter()
    rk, ww, entries, deferred = read_text_models_device(pat, dev, chunk_bytes=a.chunk_bytes,
                                                        stats=stats)
    sync()
    res["load_stage_read_and_parse_s"] = round(time.perf_counter() - t0, 4)
    res["load_parse_ms_per_chunk"] = [round(x, 3) for x in stats["parse_ms"]]
    res["load_stage_parse_kernels_s"] = round(sum(stats["parse_ms"]) / 1e3, 4)
    t0 = time.perf_counter()
    s = ModelScorer.from_pairs(mix(rk, bits), ww, bits, dev)
    occ = s.table.census()[0]
    sync()
    res["load_stage_table_insert_s"] = round(time.perf_counter() - t0, 4)
    assert occ == entries == N
    del s, rk, ww
    warm_start_row(pat, N, a, res)
    if a.dir is None:
        shutil.rmtree(out, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
