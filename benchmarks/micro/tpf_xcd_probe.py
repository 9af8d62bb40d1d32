#!/usr/bin/env python3
"""Device-only times of the flat bucket-geometry kernels (csrc/hip/tploc_bucket.hip, tploc_step.hip) on one
localised 65,536 x 39 Criteo-shaped minibatch after a few training steps, for comparing two
trees (e.g. block -> bucket-group maps: tpf_xcd_group_of): the bucket kernel alone
(localize_tpf stage 2), the tpf_step pull / update / both, and the 8-owner exchange's
tpf_unpack_w / tpf_pack_grads / tpf_pack_keys on buffers of their own. Every figure is the time per launch
of 30 back-to-back launches (a native launch list; the two exchange kernels, which have no
launch-list op, as a captured graph), repeated ``--reps`` times: [min, median, max] us, so
the spread of a kernel's own repeats stands next to its time. One JSON line, fixed key
order."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer  # noqa: E402
from parameter_server_amd.ops.native import hipops  # noqa: E402
from parameter_server_amd.ops.synthetic import criteo_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--table-log2", type=int, default=31)  # the bench's: 64 GiB of slots
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
args = ap.parse_args()

os.environ["PSAMD_FLAT"] = "1"
dev = torch.device("cuda")
H = hipops()
B, IT, G = 65536, 30, 8


def _timed(run):
    run()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        run()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / IT * 1e3)
    return [round(min(out), 2), round(statistics.median(out), 2), round(max(out), 2)]


def time_list(add):
    L = H.LaunchList()
    for _ in range(IT):
        add(L)
    return _timed(L.run)


def time_graph(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(IT):
            fn()
    return _timed(g.replay)


cfg = SparseLRConfig(num_features=10 ** 9, minibatch=B, table_capacity=1 << args.table_log2)
tr = SparseLRTrainer(cfg, device=dev)
for t in range(4):
    k, lab = criteo_batch(B, seed=5, row0=t * B, num_features=cfg.num_features, device=dev)
    tr.step(k, lab, width=39)
k, lab = criteo_batch(B, seed=5, row0=4 * B, num_features=cfg.num_features, device=dev)
loc = tr.localize(k, buf=0)
tr.step(k, lab, width=39, loc=loc)  # psum / slot_u of this minibatch are valid now
torch.cuda.synchronize()
n, bits, tb = loc.nnz, loc.bits, tr.table
it_, iv, isd, seed = tb.init.args()
common = (tb.slots, it_, iv, isd, seed, tb._err, tb._inserted, tb.home_base, tb.home_m,
          *tr.rule.args(), tr.stats)
groups = H.tpf_groups(n, bits)
row = {"label": args.label, "groups": groups, "table_log2": args.table_log2}
row["step_pull"] = time_list(lambda L: L.add_tpf_step(
    n, bits, None, None, loc.bufs, loc.w_ent, *common, None, None, None))
row["step_update"] = time_list(lambda L: L.add_tpf_step(
    n, bits, loc.bufs, loc.psum, None, None, *common, None, None, None))
row["step_both"] = time_list(lambda L: L.add_tpf_step(
    n, bits, loc.bufs, loc.psum, loc.bufs, loc.w_ent, *common, None, None, None))
# the 8-owner exchange kernels on rows of their own (C keys per owner row, 32-bit keys)
assert H.tpf_exchange_ok(n, bits, G)
C, kw = 1 << 16, 1
Hrow = 4 + C * kw + C
send = torch.zeros(G * Hrow, dtype=torch.int32, device=dev)
wrecv = torch.rand(G * C, dtype=torch.float32, device=dev)
w_ent = torch.zeros_like(loc.w_ent)
row["unpack_w"] = time_graph(lambda: H.tpf_unpack_w(
    n, bits, G, loc.cnt, loc.ent_pos, loc.ent_j, C, wrecv, w_ent, 0))
row["pack_grads"] = time_graph(lambda: H.tpf_pack_grads(
    n, bits, G, loc.cnt, loc.ent_pos, loc.ent_j, C, kw, Hrow, loc.psum, send, None, None, None,
    None, None, None))
row["pack_keys"] = time_graph(lambda: H.tpf_pack_keys(
    n, bits, G, loc.cnt, loc.uniqf, C, kw, Hrow, send, None))
# last: a rebuilt bucket may order its keys differently from the slots pulled above
lz = tr._localizers[0]
f = lz.flat
row["bucket"] = time_list(lambda L: L.add_localize_tpf(
    k, n, bits, lz.ptemp, f.dcnt, f.rep, f.uniqf, f.ent_pos, f.ent_j, f.cnt, f.err, False,
    None, 2))
torch.cuda.synchronize()
assert int(f.err.item()) == 0
print(json.dumps(row), flush=True)
