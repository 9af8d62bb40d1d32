"""Darlin's load: ``SlotReader.read()`` over slot-grouped SPARSE_BINARY files, the host route
(C++ parser, split by slot on the host) against the device routes (pstext.hip, then the split
on the host, on the device (slotsplit.hip), or on the device with the groups left there),
alternating in one process on the same files, no cache. Prints one JSON line.

    python benchmarks/bench_slotreader.py --rows 2000000 --files 8 --warmup 1 \\
        --parser cpu,gpu,gpu,gpu,cpu,gpu,gpu,gpu \\
        --split host,host,device,resident,host,host,device,resident

``--format ADFEA`` / ``TERAFEA`` reads CTR-log text instead (adtext.hip on the device
routes): ``data.synthetic.sparse_groups``-shaped rows, ``--present`` of ``--groups`` feature
groups per row with one key each, written by a fast fixed-width writer.

``--split`` pairs with ``--parser`` entry by entry (a shorter list repeats its last entry):
``host``, ``device``, or ``resident`` (``device`` with ``resident=True``). ``--warmup N``
reads every distinct route N times first, untimed. ``--csc`` also builds a ``DarlinTrainer``
from resident and from host-route data and reports its ``prep_times`` on a second line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _digits(out, v, nd):
    """``v`` as ``nd`` zero-padded decimal digits into the last axis of ``out``."""
    v = v.copy()
    for p in range(nd - 1, -1, -1):
        out[..., p] = ord("0") + (v % 10).astype(np.uint8)
        v //= 10


def write_group_files(d, fmt, rows, files, groups, present, seed=0, N=10 ** 6):
    """``sparse_groups``-shaped rows as ADFEA ("lineid 1 click key:grp ...") or TERAFEA
    ("click lineid | key ...", key = grp << 54 | id) text: ``present`` of ``groups`` groups per
    row in ascending order, one key each, fixed-width tokens built by digit arithmetic."""
    rng = np.random.default_rng(seed)
    per = rows // files
    for f in range(files):
        g = np.sort(np.argsort(rng.random((per, groups)), axis=1)[:, :present] + 1, axis=1)
        k = (N * rng.random((per, present)) ** 3).astype(np.uint64)
        y = rng.random(per) < 0.3
        i = np.arange(per, dtype=np.uint64)
        if fmt == "ADFEA":
            tok, head = 1 + 7 + 1 + 4, 8 + 4  # " kkkkkkk:gggg"; "iiiiiiii 1 c"
            out = np.full((per, head + present * tok + 1), ord(" "), dtype=np.uint8)
            _digits(out[:, :8], i, 8)
            out[:, 9] = ord("1")
            out[:, 11] = np.where(y, ord("1"), ord("0"))
            body = out[:, head:-1].reshape(per, present, tok)
            _digits(body[:, :, 1:8], k, 7)
            body[:, :, 8] = ord(":")
            _digits(body[:, :, 9:13], g.astype(np.uint64), 4)
        else:
            tok, head = 1 + 20, 1 + 1 + 8 + 2  # " " 20 digits; "c iiiiiiii |"
            out = np.full((per, head + present * tok + 1), ord(" "), dtype=np.uint8)
            out[:, 0] = np.where(y, ord("1"), ord("0"))
            _digits(out[:, 2:10], i, 8)
            out[:, 11] = ord("|")
            body = out[:, head:-1].reshape(per, present, tok)
            _digits(body[:, :, 1:21], (g.astype(np.uint64) << np.uint64(54)) | k, 20)
        out[:, -1] = ord("\n")
        out.tofile(os.path.join(d, f"part-{f:03d}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", default="SPARSE_BINARY",
                    choices=["SPARSE_BINARY", "ADFEA", "TERAFEA"])
    ap.add_argument("--groups", type=int, default=100)
    ap.add_argument("--present", type=int, default=20)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parser", default="cpu,gpu,cpu,gpu")
    ap.add_argument("--split", default="host")
    ap.add_argument("--warmup", type=int, default=0)
    ap.add_argument("--csc", action="store_true")
    ap.add_argument("--dir", default="")
    a = ap.parse_args()
    import torch

    from bench_app import write_files
    from parameter_server_amd import data
    from parameter_server_amd.data.slot_reader import SlotData, SlotReader

    d = a.dir or tempfile.mkdtemp(prefix="psamd_slots_")
    fmt = a.format
    if fmt == "SPARSE_BINARY":
        write_files(d, "ctr", a.rows, a.files)
    else:
        write_group_files(d, fmt, a.rows, a.files, a.groups, a.present)
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.startswith("part-"))
    mb = sum(os.path.getsize(f) for f in files) / 1e6
    parsers = a.parser.split(",")
    splits = a.split.split(",")
    splits += [splits[-1]] * (len(parsers) - len(splits))
    routes = list(zip(parsers, splits))

    def reader(parser, split):
        return SlotReader(files, fmt, nthreads=a.threads, parser=parser, device="cuda",
                          split="host" if split == "host" else "device",
                          resident=split == "resident")

    def read(parser, split):
        r = reader(parser, split)
        t0 = time.time()
        sd = r.read()
        torch.cuda.synchronize()
        return r, sd, time.time() - t0

    for _ in range(a.warmup):
        for parser, split in dict.fromkeys(routes):
            read(parser, split)
    runs = []
    for parser, split in routes:
        r, sd, dt = read(parser, split)
        runs.append({"parser": r.parser, "split": r.split, "resident": r.resident,
                     "read_s": round(dt, 3), "rows": sd.rows,
                     "groups": len(sd.groups), "deferred_chunks": r.deferred_chunks,
                     "split_deferred_chunks": r.split_deferred_chunks,
                     "examples_per_s": sd.rows / dt, "text_mb_per_s": mb / dt})
        print(f"[bench_slotreader] {r.parser} / {r.split}{' resident' if r.resident else ''}: "
              f"{dt:.2f} s", file=sys.stderr, flush=True)
        del sd
    # where the time goes: the parse alone of one file on either route, and the split by slot
    raw = open(files[0], "rb").read()
    t0 = time.time()
    b = data.parse_text(raw, fmt, ignore_slot=False, nthreads=a.threads)
    t_host = time.time() - t0
    r = SlotReader(files[:1], fmt, parser="gpu", device="cuda")
    r._parse_device(files[0])
    torch.cuda.synchronize()
    t0 = time.time()
    r._parse_device(files[0])
    t_dev = time.time() - t0
    t0 = time.time()
    SlotData.from_batch(b)
    t_split = time.time() - t0
    one = {"rows": b.rows, "host_parse_s": round(t_host, 3),
           "device_parse_and_copy_back_s": round(t_dev, 3), "split_by_slot_s": round(t_split, 3)}
    if any(s != "host" for s in splits):
        one.update(_device_split_times(files[0], fmt))
    out = {"bench": "slot_reader", "format": fmt, "files": a.files, "text_mb": round(mb, 1),
           "threads": a.threads, "runs": runs, "one_file": one}
    print(json.dumps(out), flush=True)
    if a.csc:  # (a line of its own: the trainers take longer than everything above)
        print(json.dumps({"bench": "slot_reader_darlin_prep", "rows": a.rows,
                          "prep_times": _csc_times(read)}), flush=True)


def _device_split_times(path: str, fmt: str) -> dict:
    """One file on the device: the parse alone (nothing copied back), the split of the parsed
    chunks alone, and the whole resident read of the file."""
    import torch

    from parameter_server_amd.data.slot_reader import SlotReader
    from parameter_server_amd.ops.slotsplit import split_by_slot
    from parameter_server_amd.ops.textparse import parse_text_device

    def parse():
        with open(path, "rb") as f:
            chunks = SlotReader._text_chunks(f.read())
        return [parse_text_device(torch.frombuffer(bytearray(c), dtype=torch.uint8).to("cuda"),
                                  fmt, ignore_slot=False, host=c) for c in chunks]

    def split(parsed):
        return [split_by_slot(None, p.row_ptr, p.keys, p.vals, p.slots) for p in parsed]

    split(parse())
    torch.cuda.synchronize()
    t0 = time.time()
    parsed = parse()
    torch.cuda.synchronize()
    t1 = time.time()
    sp = split(parsed)
    torch.cuda.synchronize()
    t2 = time.time()
    r = SlotReader([path], fmt, parser="gpu", split="device", resident=True,
                   device="cuda")
    r.read()
    torch.cuda.synchronize()
    return {"chunks": len(parsed), "device_parse_s": round(t1 - t0, 4),
            "device_split_s": round(t2 - t1, 4), "split_deferred_chunks": sum(s.deferred for s in sp),
            "resident_read_s": round(time.time() - t2, 4)}


def _csc_times(read) -> dict:
    """``DarlinTrainer``'s preprocessing from resident data and from the host route's."""
    import torch

    from parameter_server_amd.models.darlin import DarlinConfig, DarlinTrainer

    out = {}
    cfg = DarlinConfig(l1=1.0, max_pass=1, seed=0)
    for name, route in (("host_data", ("cpu", "host")), ("resident_data", ("gpu", "resident")),
                        ("host_data_again", ("cpu", "host")),
                        ("resident_data_again", ("gpu", "resident"))):
        _, sd, _ = read(*route)
        tr = DarlinTrainer(sd, cfg, device=torch.device("cuda"))
        out[name] = {k: round(v, 4) for k, v in tr.prep_times.items()}
        del tr, sd
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
