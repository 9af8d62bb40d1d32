"""Darlin's load: ``SlotReader.read()`` over slot-grouped SPARSE_BINARY files, the host route
(C++ parser) against the device route (pstext.hip), alternating in one process on the same
files, no cache. Prints one JSON line.

    python benchmarks/bench_slotreader.py --rows 2000000 --files 8 --parser cpu,gpu,cpu,gpu
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parser", default="cpu,gpu,cpu,gpu")
    ap.add_argument("--dir", default="")
    a = ap.parse_args()
    import torch

    from bench_app import write_files
    from parameter_server_amd import data
    from parameter_server_amd.data.slot_reader import SlotData, SlotReader

    d = a.dir or tempfile.mkdtemp(prefix="psamd_slots_")
    write_files(d, "ctr", a.rows, a.files)
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.startswith("part-"))
    mb = sum(os.path.getsize(f) for f in files) / 1e6
    runs = []
    for parser in a.parser.split(","):
        r = SlotReader(files, "SPARSE_BINARY", nthreads=a.threads, parser=parser, device="cuda")
        t0 = time.time()
        sd = r.read()
        dt = time.time() - t0
        runs.append({"parser": r.parser, "read_s": round(dt, 3), "rows": sd.rows,
                     "groups": len(sd.groups), "deferred_chunks": r.deferred_chunks,
                     "examples_per_s": sd.rows / dt, "text_mb_per_s": mb / dt})
        print(f"[bench_slotreader] {r.parser}: {dt:.2f} s", file=sys.stderr, flush=True)
        del sd
    # where the time goes: the parse alone of one file on either route, and the split by slot
    raw = open(files[0], "rb").read()
    t0 = time.time()
    b = data.parse_text(raw, "SPARSE_BINARY", ignore_slot=False, nthreads=a.threads)
    t_host = time.time() - t0
    r = SlotReader(files[:1], "SPARSE_BINARY", parser="gpu", device="cuda")
    r._parse_device(files[0])
    torch.cuda.synchronize()
    t0 = time.time()
    r._parse_device(files[0])
    t_dev = time.time() - t0
    t0 = time.time()
    SlotData.from_batch(b)
    t_split = time.time() - t0
    print(json.dumps({"bench": "slot_reader", "files": a.files, "text_mb": round(mb, 1),
                      "threads": a.threads, "runs": runs,
                      "one_file": {"rows": b.rows, "host_parse_s": round(t_host, 3),
                                   "device_parse_and_copy_back_s": round(t_dev, 3),
                                   "split_by_slot_s": round(t_split, 3)}}), flush=True)


if __name__ == "__main__":
    main()
