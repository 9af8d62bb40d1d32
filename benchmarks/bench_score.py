"""Scoring throughput on one GPU: the fused table-probe kernel (ops/score.py,
csrc/hip/predict.hip) against the path the training step's ops already compose --
``Localizer`` + ``KVTable.resolve(insert=False)`` + ``linear_fwd`` -- on the same
minibatches, alternating in one process.

    python benchmarks/bench_score.py                       # kernel paths
    python benchmarks/bench_score.py --app-rows 1000000    # + the eval app, end to end

* Criteo shape: B = 65,536 x 39 binary features hashed into 10^9, generated on the device
  (``criteo_gen``); the table is populated by training ``--train-steps`` minibatches, and
  the scored minibatches are fresh rows (most of their tail keys are absent from the
  model, the hot keys present).
* rcv1 shape: 32,768 valued CSR rows of 5..145 features over 47,236 keys, all in the
  model; the fused kernel in its whole-wave form (the host's choice) and the 8-lane form.
* ``--lanes-sweep``: the two lane-group forms over mean row lengths 40..5000 on a table
  that misses L2 (where the host's 64-occurrence threshold comes from).
* Before timing, both paths' margins are compared within the row bound
  (n_r + 2) 2^-23 sum |w x|.
* ``--app-rows``: the evaluation route of app/gpu.py on Criteo-shaped LIBSVM files
  (bench_app.py's generator), next to the CPU evaluator ``evaluate_model`` on the same
  files and model.

Prints one JSON line; timings are device events around ``--iters`` minibatches after
``--warmup``, repeated ``--repeats`` times per path in alternation."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def log(*a):
    print("[bench_score]", *a, file=sys.stderr, flush=True)


class Composed:
    """Margins + metrics + histogram of a minibatch by localise -> resolve -> forward."""

    def __init__(self, table, bits, max_nnz, B, device):
        import torch

        from parameter_server_amd.ops.linear import AUC_BINS, HIST_STRIPES, new_accum
        from parameter_server_amd.ops.localize import Localizer

        self.table = table
        self.lz = Localizer(max_nnz, bits, device, mode="tp")
        self.metrics = new_accum(device)
        self.hist = torch.zeros(HIST_STRIPES * 2 * AUC_BINS, dtype=torch.int32, device=device)
        self.xw = torch.empty(B, dtype=torch.float32, device=device)
        self.coef = torch.empty(B, dtype=torch.float32, device=device)

    def __call__(self, keys, labels, B, width=0, row_ptr=None, vals=None):
        from parameter_server_amd.ops.linear import linear_forward
        from parameter_server_amd.ops.localize import ensure_local_col

        loc = self.lz(keys)
        _, w = self.table.resolve(loc.uniq, insert=False, n_dev=loc.n_uniq)
        linear_forward(ensure_local_col(loc), w, labels, B=B, width=width, row_ptr=row_ptr,
                       vals=vals, xw=self.xw, coef=self.coef, metrics=self.metrics,
                       hist=self.hist)
        return self.xw


def row_bounds(table, bits, keys, B, width=0, row_ptr=None, vals=None):
    """(n_r + 2) 2^-23 sum |w x| per row, in f64 on the device."""
    import torch

    from parameter_server_amd.ops.keymix import mix
    from parameter_server_amd.ops.linear import _rows_of

    _, w = table.resolve(mix(keys, bits), insert=False)
    a = w.double().abs() * (vals.double().abs() if vals is not None else 1.0)
    rows = _rows_of(B, width, row_ptr, keys.device)
    s = torch.zeros(B, dtype=torch.float64, device=keys.device).index_add_(0, rows, a)
    n = torch.bincount(rows, minlength=B).double()
    return (n + 2) * 2.0 ** -23 * s


def timed(fn, batches, warmup, iters):
    import torch

    for i in range(warmup):
        fn(batches[i % len(batches)])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fn(batches[i % len(batches)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(name, paths, batches, B, a):
    """Alternate the paths ``a.repeats`` times; ms per minibatch and examples/s each."""
    ms = {k: [] for k in paths}
    for _ in range(a.repeats):
        for k, fn in paths.items():
            ms[k].append(timed(fn, batches, a.warmup, a.iters))
    out = {}
    for k, v in ms.items():
        med = sorted(v)[len(v) // 2]
        out[k] = {"ms_per_minibatch": [round(x, 4) for x in v], "median_ms": round(med, 4),
                  "spread_ms": round(max(v) - min(v), 4),
                  "examples_per_s": round(B / med * 1e3)}
        log(f"{name:7s} {k:12s} ms/minibatch {v}  median {med:.4f}  "
            f"{B / med * 1e3 / 1e6:.1f} M examples/s")
    return out


def bench_criteo(a, dev):
    import torch

    from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
    from parameter_server_amd.ops.keymix import mix
    from parameter_server_amd.ops.score import ScoreAccum, score
    from parameter_server_amd.ops.synthetic import criteo_batch

    B, N = a.minibatch, 10 ** 9
    cfg = SparseLRConfig(num_features=N, minibatch=B, table_capacity=a.table_capacity)
    tr = SparseLRTrainer(cfg, device=dev)
    keys = torch.empty(B * 39, dtype=torch.int64, device=dev)
    labels = torch.empty(B, dtype=torch.float32, device=dev)
    for t in range(a.train_steps):
        criteo_batch(B, seed=1, row0=t * B, num_features=N, device=dev, keys=keys, labels=labels)
        tr.step(keys, labels, width=39)
    sc = tr.scorer()  # flushes; the trainer's own table
    tr.check_ok()
    occ, nnz_w = tr.table.census()
    log(f"trained {a.train_steps} steps of {B}: {occ} keys in {tr.table.capacity} slots, "
        f"{nnz_w} non-zero weights, {tr.progress()}")
    batches = [criteo_batch(B, seed=1, row0=(a.train_steps + 10 + i) * B, num_features=N,
                            device=dev) for i in range(a.batches)]
    table, bits = tr.table, tr.bits
    acc = sc.acc  # (sc.result() below: the figures over everything the fused path scored)
    comp = Composed(table, bits, B * 39, B, dev)
    fused = lambda b: score(table, b[0], bits, width=39, labels=b[1], acc=acc)  # noqa: E731
    composed = lambda b: comp(b[0], b[1], B, width=39)  # noqa: E731
    k0, l0 = batches[0]
    mf, mc = fused((k0, l0)), composed((k0, l0)).clone()
    bound = row_bounds(table, bits, k0, B, width=39)
    worst = float(((mf - mc).double().abs() - bound).max())
    assert worst <= 0, f"fused and composed margins differ by more than the row bound: {worst}"
    hit = float((table.resolve(mix(k0, bits), insert=False)[0] >= 0).double().mean())
    log(f"criteo margins agree within the row bound; {hit:.3f} of the occurrences hit the model")
    res = compare("criteo", {"fused": fused, "composed": composed}, batches, B, a)
    res.update(B=B, width=39, occupied=occ, capacity=table.capacity, hit_fraction=round(hit, 4),
               result=sc.result())
    return res


def bench_rcv1(a, dev):
    import torch

    from parameter_server_amd.ops.keymix import mix
    from parameter_server_amd.ops.kv_table import KVTable
    from parameter_server_amd.ops.score import ScoreAccum, score

    B, F, bits = 32768, 47236, 16
    g = torch.Generator(device=dev).manual_seed(5)
    table = KVTable(1 << 17, dev)
    table.load(mix(torch.arange(F, device=dev), bits), torch.randn(F, generator=g, device=dev))
    batches = []
    for i in range(a.batches):
        lens = torch.randint(5, 146, (B,), generator=g, device=dev)
        rp = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        n = int(rp[-1])
        keys = (F * torch.rand(n, generator=g, device=dev) ** 3).long().clamp_(max=F - 1)
        vals = torch.rand(n, generator=g, device=dev) * 0.9 + 0.1
        labels = torch.where(torch.rand(B, generator=g, device=dev) < 0.3, 1.0, -1.0)
        batches.append((keys, labels, rp, vals))
    nmax = max(b[0].numel() for b in batches)
    acc = ScoreAccum(dev)
    comp = Composed(table, bits, nmax, B, dev)

    def fused(lanes):
        return lambda b: score(table, b[0], bits, row_ptr=b[2], vals=b[3], labels=b[1], acc=acc,
                               lanes=lanes)

    composed = lambda b: comp(b[0], b[1], B, row_ptr=b[2], vals=b[3])  # noqa: E731
    b0 = batches[0]
    bound = row_bounds(table, bits, b0[0], B, row_ptr=b0[2], vals=b0[3])
    mc = composed(b0).clone()
    for lanes in (0, 8):
        worst = float(((fused(lanes)(b0) - mc).double().abs() - bound).max())
        assert worst <= 0, f"rcv1 lanes={lanes}: margins differ by more than the row bound"
    log("rcv1 margins agree within the row bound")
    res = compare("rcv1", {"fused_wave": fused(0), "fused_8lane": fused(8), "composed": composed},
                  batches, B, a)
    res.update(B=B, mean_nnz_per_row=round(nmax / B, 1))
    return res


def bench_lanes(a, dev):
    """The 8-lane against the whole-wave form by mean row length: ~2.5 M valued
    occurrences per minibatch over a 4 M-key table (128 MiB of slots: misses L2)."""
    import torch

    from parameter_server_amd.ops.keymix import mix
    from parameter_server_amd.ops.kv_table import KVTable
    from parameter_server_amd.ops.score import ScoreAccum, score

    F, bits = 1 << 22, 22
    g = torch.Generator(device=dev).manual_seed(5)
    table = KVTable(1 << 23, dev)
    table.load(mix(torch.arange(F, device=dev), bits), torch.randn(F, generator=g, device=dev))
    acc = ScoreAccum(dev)
    out = {}
    for mean in (40, 75, 150, 300, 1200, 5000):
        B = max(64, 2_500_000 // mean)
        lens = torch.randint(mean // 2, mean * 3 // 2 + 1, (B,), generator=g, device=dev)
        rp = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        n = int(rp[-1])
        keys = (F * torch.rand(n, generator=g, device=dev) ** 3).long().clamp_(max=F - 1)
        b = (keys, torch.where(torch.rand(B, generator=g, device=dev) < 0.3, 1.0, -1.0), rp,
             torch.rand(n, generator=g, device=dev))
        paths = {f"lanes{ln}": (lambda b, ln=ln: score(table, b[0], bits, row_ptr=b[2], vals=b[3],
                                                       labels=b[1], acc=acc, lanes=ln))
                 for ln in (8, 64)}
        out[str(mean)] = compare(f"len{mean}", paths, [b], B, a)
    return out


def bench_app(a, dev):
    """The eval route end to end on Criteo-shaped files, beside evaluate_model."""
    import numpy as np
    from bench_app import write_files

    from parameter_server_amd.app.gpu import run_model_evaluation
    from parameter_server_amd.app.linear_method.model_evaluation import evaluate_model
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.checkpoint import read_text_models, write_text_model
    from parameter_server_amd.utils.config import load_app_config

    N = 10 ** 8
    d = tempfile.mkdtemp(prefix="psamd_score_")
    write_files(d, "criteo", a.app_rows, a.app_files, N=N)
    rng = np.random.default_rng(3)
    mk = np.unique((N * rng.random(a.app_model_keys) ** 4).astype(np.uint64))
    os.makedirs(os.path.join(d, "model"))
    write_text_model(os.path.join(d, "model", "m_S0"), mk,
                     rng.normal(0, 0.3, mk.size).astype(np.float32))
    conf = os.path.join(d, "eval.conf")
    with open(conf, "w") as f:
        f.write(f"""linear_method {{
validation_data {{ format: TEXT text: LIBSVM file: "{d}/part.*" }}
model_input {{ format: TEXT file: "{d}/model/m_S.*" }}
loss {{ type: LOGIT }}
}}""")
    lm = load_app_config(conf).linear_method
    out = {"rows": a.app_rows, "files": a.app_files, "model_keys": int(mk.size), "runs": []}
    for parser in a.app_parser.split(","):
        flags = types.SimpleNamespace(parser=parser, num_features=float(N), minibatch=a.minibatch,
                                      max_nnz_per_example=39, num_threads=16, device="cuda",
                                      seed=0, table_capacity=0, quiet=True, data_cache="off",
                                      io_threads=16)
        r = run_model_evaluation(lm, LocalComm(dev), dev, flags)
        log(f"app parser={r['parser']}: {r['examples'] / r['seconds'] / 1e6:.2f} M examples/s "
            f"({r['seconds']:.2f} s incl. loading {r['model_entries']} model entries) "
            f"auc {r['auc']:.6f} accuracy {r['accuracy']:.6f}")
        out["runs"].append({k: r[k] for k in ("parser", "examples", "seconds", "auc", "accuracy",
                                              "loss", "auc_tie_bound", "model_entries")})
    t0 = time.time()
    model = read_text_models(os.path.join(d, "model", "m_S.*"))
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.startswith("part-"))
    ref = evaluate_model(model, files, "LIBSVM")
    ref["seconds"] = time.time() - t0
    log(f"evaluate_model (CPU): {ref['examples'] / ref['seconds'] / 1e6:.3f} M examples/s "
        f"({ref['seconds']:.2f} s) auc {ref['auc']:.6f} accuracy {ref['accuracy']:.6f}")
    out["evaluate_model"] = ref
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minibatch", type=int, default=65536)
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--table-capacity", type=int, default=1 << 28)
    ap.add_argument("--batches", type=int, default=8, help="distinct scored minibatches cycled")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-rcv1", action="store_true")
    ap.add_argument("--lanes-sweep", action="store_true",
                    help="also time the 8-lane and whole-wave forms over row lengths 40..5000")
    ap.add_argument("--app-rows", type=int, default=0)
    ap.add_argument("--app-files", type=int, default=8)
    ap.add_argument("--app-model-keys", type=int, default=2_000_000)
    ap.add_argument("--app-parser", default="cpu,gpu")
    a = ap.parse_args()
    import torch

    from parameter_server_amd.ops.native import hipops

    if not torch.cuda.is_available():
        raise SystemExit("bench_score needs a GPU")
    hipops()
    dev = torch.device("cuda", 0)
    out = {"bench": "score", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
           "criteo": bench_criteo(a, dev)}
    if not a.skip_rcv1:
        out["rcv1"] = bench_rcv1(a, dev)
    if a.lanes_sweep:
        out["lanes_sweep"] = bench_lanes(a, dev)
    if a.app_rows:
        out["app"] = bench_app(a, dev)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
