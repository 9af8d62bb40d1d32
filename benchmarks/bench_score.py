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
* ``--predict-output DIR``: the cost of writing per-example predictions
  (ops/scoretext.py). Criteo-shaped files are parsed once into a binary cache; then the
  cached evaluation pass (``ModelScorer.evaluate`` over ``DeviceFeeder``, repeated until
  ``--predict-rows`` rows went by) runs with no output, with the host writer and with the
  device writer, alternated ``--repeats`` times in this process, the prediction file in
  DIR. Reports examples/s of each, the device writer's per-chunk kernel and copy times
  (device events around the launches) and its largest stage. Runs alone (the kernel paths
  above are skipped).

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


def bench_predict(a, dev):
    """The cached evaluation pass with and without a prediction writer."""
    import numpy as np
    import torch
    from bench_app import write_files

    from parameter_server_amd.data.feeder import DeviceFeeder
    from parameter_server_amd.models import ModelScorer
    from parameter_server_amd.ops.keymix import key_bits_for
    from parameter_server_amd.ops.scoretext import PredictionWriter
    from parameter_server_amd.utils.checkpoint import write_text_model

    N, B = 10 ** 8, a.minibatch
    d = a.predict_output
    os.makedirs(os.path.join(d, "model"), exist_ok=True)
    per_pass = a.predict_file_rows // a.app_files * a.app_files
    passes = max(1, -(-a.predict_rows // per_pass))
    write_files(d, "criteo", per_pass, a.app_files, N=N)
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.startswith("part-"))
    rng = np.random.default_rng(3)
    mk = np.unique((N * rng.random(a.app_model_keys) ** 4).astype(np.uint64))
    write_text_model(os.path.join(d, "model", "m_S0"), mk,
                     rng.normal(0, 0.3, mk.size).astype(np.float32))
    pattern, bits = os.path.join(d, "model", "m_S.*"), key_bits_for(N)
    cache = os.path.join(d, "cache")

    def feeder(parser="cpu"):
        return DeviceFeeder(files, "LIBSVM", B, B * 39, dev, num_features=N, passes=1,
                            shuffle=False, nthreads=16, ignore_slot=True, cache_dir=cache,
                            io_threads=a.io_threads, parser=parser)

    f = feeder("auto")
    for b in f.iter_pass(0):  # (the text pass: writes the cache)
        f.release(b)
    torch.cuda.synchronize()
    log(f"cache built: {f.num_examples} rows a pass, {passes} passes a run "
        f"({passes * f.num_examples} rows), parser {f.parser}")

    def run(mode):
        sc = ModelScorer.from_text(pattern, bits, dev)
        stats = {}
        path = os.path.join(d, f"pred_{mode}")
        w = None if mode == "none" else PredictionWriter(
            path, dev, columns=tuple(a.predict_columns.split(",")), text_io=mode, stats=stats,
            chunk_rows=a.predict_chunk_rows)
        torch.cuda.synchronize()
        t0 = time.time()
        rows = cached = 0
        for _ in range(passes):
            f = feeder()
            sc.evaluate(f, predictions=w) if w is not None else sc.evaluate(f)
            rows += f.num_examples
            cached += f.cached_passes
        if w is not None:
            w.close()
        torch.cuda.synchronize()
        s = time.time() - t0
        assert cached == passes, "the pass did not stream the cache"
        assert w is None or stats["rows"] == rows
        r = {"mode": mode, "rows": rows, "seconds": round(s, 4),
             "examples_per_s": round(rows / s), "auc": sc.result()["auc"]}
        if w is not None:
            r.update(bytes=stats["bytes"], chunks=stats["chunks"],
                     deferred_chunks=stats["deferred_chunks"],
                     file_write_s=round(stats["file_write_s"], 4),
                     host_format_s=round(stats["host_format_s"], 4))
        if mode == "device":
            fm, dm = sorted(stats["format_ms"]), sorted(stats["d2h_ms"])
            stages = {"kernels": sum(fm) / 1e3, "d2h": sum(dm) / 1e3,
                      "file_write": stats["file_write_s"]}
            r.update(format_ms_per_chunk_median=round(fm[len(fm) // 2], 4),
                     format_ms_per_chunk_max=round(fm[-1], 4),
                     format_rows_per_s=round(rows / max(sum(fm) / 1e3, 1e-9)),
                     d2h_ms_per_chunk_median=round(dm[len(dm) // 2], 4) if dm else None,
                     header_wait_s=round(stats["header_wait_s"], 4),
                     d2h_wait_s=round(stats["d2h_wait_s"], 4),
                     stage_seconds={k: round(v, 4) for k, v in stages.items()},
                     largest_stage=max(stages, key=stages.get))
        log(json.dumps(r))
        return r

    run("none")  # (warm-up: page cache, allocator, pinned slots)
    runs = [run(m) for _ in range(max(2, a.repeats)) for m in ("none", "host", "device")]
    with open(os.path.join(d, "pred_host"), "rb") as fh, \
            open(os.path.join(d, "pred_device"), "rb") as fd:
        same = all(x == y for x, y in iter(lambda: (fh.read(1 << 24), fd.read(1 << 24)),
                                           (b"", b"")))
    assert same, "host and device prediction files differ"
    best = {m: max(r["examples_per_s"] for r in runs if r["mode"] == m)
            for m in ("none", "host", "device")}
    out = {"B": B, "rows_per_run": runs[0]["rows"], "passes_per_run": passes,
           "columns": a.predict_columns, "chunk_rows": a.predict_chunk_rows, "runs": runs,
           "best_examples_per_s": best, "files_identical": same,
           "device_over_host": round(best["device"] / best["host"], 3),
           "device_over_none": round(best["device"] / best["none"], 3)}
    log(f"best examples/s {best}; device / host {out['device_over_host']}")
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
    ap.add_argument("--predict-output", default="",
                    help="directory for the prediction-writer benchmark (runs alone)")
    ap.add_argument("--predict-rows", type=int, default=120_000_000,
                    help="rows per timed run (the cached pass feeds ~10^8 rows a second: fewer "
                         "rows time the feeder's start-up)")
    ap.add_argument("--predict-file-rows", type=int, default=4_000_000,
                    help="rows of Criteo-shaped text generated and cached (one pass)")
    ap.add_argument("--predict-columns", default="score", choices=("score", "label,score"))
    ap.add_argument("--predict-chunk-rows", type=int, default=1 << 20)
    ap.add_argument("--io-threads", type=int, default=16)
    a = ap.parse_args()
    import torch

    from parameter_server_amd.ops.native import hipops

    if not torch.cuda.is_available():
        raise SystemExit("bench_score needs a GPU")
    hipops()
    dev = torch.device("cuda", 0)
    if a.predict_output:
        print(json.dumps({"bench": "score_predict_output", "repeats": max(2, a.repeats),
                          "predict_output": bench_predict(a, dev)}), flush=True)
        return
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
