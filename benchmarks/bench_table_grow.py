"""Growing a KV table on one GPU: ``kv_init`` of the new table + ``kv_rehash``
(csrc/hip/kv_table.hip, what ``KVTable.grow`` launches) against what torch ops could do
before -- ``occupied()`` into a new ``KVTable``, then ``load()`` (which loses acc / cnt /
flags) -- and against a plain ``copy_`` that moves the same number of bytes.

    python benchmarks/bench_table_grow.py --log profiles/table_grow.log

Tables of 2^22 .. 2^28 slots doubled, at load 0.25 and 0.5, with hashed and with ordered
homes; one process, the paths alternated, best of ``--repeats``. Bytes of a growth = old
table read + occupied slots written + new table initialised; the ``copy_`` yardstick reads
half of that and writes half of that. Timings are device events around each path (the
torch path ends in its ``check_ok`` host sync). Prints one line per configuration and one
JSON line at the end."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_LOG = None


def log(*a):
    line = " ".join(str(x) for x in a)
    print(line, file=sys.stderr, flush=True)
    if _LOG is not None:
        _LOG.write(line + "\n")
        _LOG.flush()


def timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def populate(table, n, dev, seed):
    """``n`` random keys of the table's range, zero state (duplicates: ~n^2 / 2^63)."""
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    done = 0
    while done < n:
        c = min(1 << 24, n - done)
        keys = torch.randint(0, 1 << 62, (c,), generator=g, device=dev, dtype=torch.int64)
        table.resolve(keys, insert=True, with_w=False)
        done += c
    table.check_ok()
    return table.census()[0]


def bench_one(lg, load, ordered, a, dev):
    import torch

    from parameter_server_amd.ops.kv_table import KVTable
    from parameter_server_amd.ops.native import hipops

    H = hipops()
    cap, new_cap = 1 << lg, 1 << (lg + 1)
    kr = (0, 1 << 62) if ordered else None
    old = KVTable(cap, dev, key_range=kr)
    occ = populate(old, int(cap * load), dev, seed=lg * 7 + ordered)
    total = 32 * (cap + occ + new_cap)

    def native():
        new = torch.empty((new_cap, 4), dtype=torch.int64, device=dev)
        H.kv_init(new)
        moved = H.kv_rehash(old.slots, new, old.home_base, old.home_m, old._err)
        return new, moved

    def torch_ops():  # what a user could write before: keys and (w, z, n) only
        t = KVTable(new_cap, dev, key_range=kr)
        t.load(*old.occupied())
        return t

    src = torch.empty(total // 16, dtype=torch.int64, device=dev)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    new, moved = native()  # (warm-up, and the count checked once)
    assert int(moved.item()) == occ == int(H.kv_census(new).cpu()[0])
    del new
    copy()
    ms = {"rehash": [], "torch": [], "copy": []}
    for _ in range(a.repeats):
        t, out = timed(native)
        ms["rehash"].append(t)
        del out
        if not a.skip_torch:
            t, out = timed(torch_ops)
            ms["torch"].append(t)
            del out
        t, _ = timed(copy)
        ms["copy"].append(t)
    old.check_ok()
    best = {k: min(v) for k, v in ms.items() if v}
    res = {"log2_slots": lg, "load": load, "homes": "ordered" if ordered else "hashed",
           "occupied": occ, "bytes": total,
           "rehash_ms": round(best["rehash"], 3), "copy_ms": round(best["copy"], 3),
           "rehash_gbs": round(total / best["rehash"] / 1e6, 1),
           "copy_gbs": round(total / best["copy"] / 1e6, 1),
           "rehash_over_copy": round(best["rehash"] / best["copy"], 2)}
    if "torch" in best:
        res.update(torch_ms=round(best["torch"], 3),
                   torch_over_rehash=round(best["torch"] / best["rehash"], 1))
    log(f"2^{lg}->2^{lg + 1} load {load:.2f} {res['homes']:7s} occ {occ:>10d}  "
        f"init+rehash {res['rehash_ms']:9.3f} ms {res['rehash_gbs']:7.1f} GB/s  "
        f"copy_ {res['copy_ms']:9.3f} ms {res['copy_gbs']:7.1f} GB/s  "
        f"ratio {res['rehash_over_copy']:5.2f}"
        + (f"  occupied+load {res['torch_ms']:10.3f} ms ({res['torch_over_rehash']}x)"
           if "torch_ms" in res else ""))
    del src, dst, old
    torch.cuda.empty_cache()
    return res


def main():
    global _LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-log2", type=int, default=22)
    ap.add_argument("--max-log2", type=int, default=28)
    ap.add_argument("--loads", default="0.25,0.5")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    import torch

    from parameter_server_amd.ops.native import hipops

    if not torch.cuda.is_available():
        raise SystemExit("bench_table_grow needs a GPU")
    hipops()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        _LOG = open(a.log, "w")
    dev = torch.device("cuda", 0)
    log(f"bench_table_grow: {torch.cuda.get_device_name(0)}, best of {a.repeats}, "
        f"bytes = 32 x (old slots + occupied + new slots)")
    rows = []
    for lg in range(a.min_log2, a.max_log2 + 1):
        for load in (float(x) for x in a.loads.split(",")):
            for ordered in (0, 1):
                rows.append(bench_one(lg, load, ordered, a, dev))
    print(json.dumps({"bench": "table_grow", "repeats": a.repeats, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
