#!/usr/bin/env python3
"""Factorization machine (reference src/app/factor_machine, fm.m): k-dim bf16 factor rows +
linear weights sharded over the ranks, packed [v | w] push/pull over RCCL.
Metric: examples/sec (whole node), weak scaling (fixed minibatch per GPU).

    python benchmarks/bench_fm.py --steps 20
    torchrun --nproc-per-node N benchmarks/bench_fm.py ...
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def rcv1_batches(B, n, dev):
    """n rcv1-shaped minibatches (keys, labels, vals, row_ptr): 50..100 valued features per
    row out of 47,236, skewed ids (a few frequent terms, a long tail)."""
    g = torch.Generator().manual_seed(1)
    out = []
    for _ in range(n):
        wid = torch.randint(50, 101, (B,), generator=g)
        rp = torch.zeros(B + 1, dtype=torch.int64)
        rp[1:] = wid.cumsum(0)
        nnz = int(rp[-1])
        k = (torch.rand(nnz, generator=g) ** 3 * 47236).long()
        out.append((k.to(dev), torch.where(torch.rand(B, generator=g) < 0.5, 1.0, -1.0).to(dev),
                    torch.rand(nnz, generator=g).to(dev), rp.to(dev)))
    return out


def score_mode(args):
    """1 GPU: scoring held-out minibatches with the fused kernel (``FMTrainer.scorer()``:
    fm_predict.hip, margins only and labels + accumulator) and with the composed route
    (``FMTrainer.predict``: mix, resolve, where, fm_csr forward), alternated window by window
    in this one process, on a table filled by a few training steps. Criteo-shaped B x 39 for
    D in {16, 32} (both routes) and {64, 128} (the scorer alone: ``predict`` refuses them on
    a GPU), then an rcv1-shaped valued CSR minibatch at D = 16. Times by a host clock around
    synchronised windows of ``--steps`` (at least 200) minibatches."""
    from parameter_server_amd.models.fm import FMConfig, FMTrainer
    from parameter_server_amd.ops.native import hipops
    from parameter_server_amd.ops.synthetic import criteo_batch

    dev = torch.device("cuda", 0)
    B, N, S, n = args.minibatch, int(args.num_features), 39, max(args.steps, 200)

    def measure(tag, tr, train, held, lanes):
        """held: (keys, labels, the scorer's keywords, predict's keywords) per minibatch"""
        for i in range(args.train_steps):
            train(i)
        sc = tr.scorer()
        routes = {"fused_margins": lambda b: sc.predict(b[0], **b[2]),
                  "fused_labels_acc": lambda b: sc.score(b[0], b[1], margins=False, **b[2])}
        if tr.cfg.embedding_dim in (8, 16, 32):
            routes["composed_predict"] = lambda b: tr.predict(b[0], B, **b[3])
            a, c = routes["fused_margins"](held[0]), routes["composed_predict"](held[0])
            print(f"{tag}: max |fused - composed| margin = {float((a - c).abs().max()):.3g}, "
                  f"max |margin| = {float(c.abs().max()):.3g}", flush=True)
        ms = {name: [] for name in routes}
        for fn in routes.values():
            for i in range(args.warmup):
                fn(held[i % len(held)])
        for r in range(args.repeats):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    fn(held[i % len(held)])
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / n * 1e3)
            print(f"{tag} window {r}: " + "  ".join(f"{k} {v[-1]:.4f} ms" for k, v in ms.items()),
                  flush=True)
        occ, _ = tr.shard.table.census()
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        out = {"keys_in_table": occ, "table_slots": tr.shard.capacity, "lanes": lanes,
               "eval": sc.result(), "ms": ms, "median_ms": med}
        if "composed_predict" in med:
            out["composed_over_fused_margins"] = med["composed_predict"] / med["fused_margins"]
        return out

    res = {}
    H = hipops()
    for D in (16, 32, 64, 128):
        tr = FMTrainer(FMConfig(localize=args.localize, num_features=N, embedding_dim=D,
                                minibatch=B, table_capacity=args.table_slots, seed=0), device=dev)
        crit = [criteo_batch(B, seed=77, row0=i * B, num_features=N, device=dev)
                for i in range(args.train_steps + 8)]
        held = [(k, y, dict(width=S), {}) for k, y in crit[args.train_steps:]]
        res[f"criteo_D{D}"] = measure(f"criteo D={D}", tr, lambda i: tr.step(*crit[i]), held,
                                      H.fm_csr_lanes(B * S, B))
        del tr, crit, held
        torch.cuda.empty_cache()
    rcv = rcv1_batches(B, 8, dev)
    tr = FMTrainer(FMConfig(localize=args.localize, num_features=47236, embedding_dim=16,
                            minibatch=B, max_nnz=B * 100, table_capacity=1 << 17, seed=0),
                   device=dev)
    held = [(k, y, dict(row_ptr=rp, vals=v), dict(row_ptr=rp, vals=v)) for k, y, v, rp in rcv[4:]]

    def train_rcv(i):
        k, y, v, rp = rcv[i % 4]
        tr.step(k, y, vals=v, row_ptr=rp)

    res["rcv1_D16"] = measure("rcv1 D=16", tr, train_rcv, held,
                              H.fm_csr_lanes(rcv[4][0].numel(), B))
    res["rcv1_D16"]["nnz"] = rcv[4][0].numel()
    print(json.dumps({
        "metric": "FM scoring time per minibatch, fused kernel (FMScorer) vs FMTrainer.predict, "
                  "1 GPU", "unit": "ms/minibatch (median of windows)",
        "minibatches_per_window": n, "windows": args.repeats, "minibatch": B,
        "train_steps": args.train_steps, "lane_thresholds": "fm_csr_lanes, not swept", **res}),
          flush=True)


def ffm_score_mode(args):
    """1 GPU: scoring held-out minibatches against a field-aware FM (k = 2, F = 39) with the
    fused kernel (``FFMTrainer.scorer()``: ffm_predict.hip, margins only and labels +
    accumulator) and with the composed route (``FFMTrainer.predict``: mix, resolve, where,
    then ffm_margins or the two ffm_csr_margins launches), alternated window by window in this
    one process on a table filled by a few training steps. Shapes: Criteo's B x 39 fixed rows;
    the same rows as CSR with a quarter of the slots missing; CSR rows of 65..130 occurrences
    (B / 4 rows), which the composed route serves from its global-memory kernel. Per route and
    window: a host clock around the synchronised window, and device events around the same
    launches (for the fused routes, one kernel per minibatch: the kernel's own time)."""
    from parameter_server_amd.models.ffm import FFMConfig, FFMTrainer
    from parameter_server_amd.ops.synthetic import criteo_batch

    dev = torch.device("cuda", 0)
    B, N, S = args.minibatch, int(args.num_features), 39
    tr = FFMTrainer(FFMConfig(k=2, localize=args.localize, num_features=N, minibatch=B,
                              table_capacity=min(args.table_slots, 1 << 24), seed=0), device=dev)
    crit = [criteo_batch(B, seed=77, row0=i * B, num_features=N, device=dev)
            for i in range(args.train_steps + 4)]
    for i in range(args.train_steps):
        tr.step(*crit[i])
    sc = tr.scorer()
    g = torch.Generator(device=dev).manual_seed(5)
    slot_of = torch.arange(S, dtype=torch.int32, device=dev).repeat(B)
    fixed, missing, wide = [], [], []
    for k39, y in crit[args.train_steps:]:
        fixed.append((k39, y, B, dict(width=S), {}))
        keep = torch.rand(B * S, device=dev, generator=g) < 0.75
        rp = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(keep.view(B, S).sum(1), 0)
        kw = dict(row_ptr=rp, fields=slot_of[keep])
        missing.append((k39[keep], y, B, kw, kw))
        Bw = B // 4
        rp = torch.zeros(Bw + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(torch.randint(65, 131, (Bw,), device=dev, generator=g), 0)
        nnz = int(rp[-1])
        pick = torch.randint(0, B * S, (nnz,), device=dev, generator=g)
        kw = dict(row_ptr=rp, fields=slot_of[pick])  # a held-out key in its own slot's field
        wide.append((k39[pick], y[:Bw].contiguous(), Bw, kw, kw))

    def measure(tag, held, n):
        """held: (keys, labels, rows, the scorer's keywords, predict's keywords)"""
        routes = {"fused_margins": lambda b: sc.predict(b[0], **b[3]),
                  "fused_labels_acc": lambda b: sc.score(b[0], b[1], margins=False, **b[3]),
                  "composed_predict": lambda b: tr.predict(b[0], b[2], **b[4])}
        a, c = routes["fused_margins"](held[0]), routes["composed_predict"](held[0])
        print(f"{tag}: max |fused - composed| margin = {float((a - c).abs().max()):.3g}, "
              f"max |margin| = {float(c.abs().max()):.3g}", flush=True)
        host, devt = {r: [] for r in routes}, {r: [] for r in routes}
        for fn in routes.values():
            for i in range(args.warmup):
                fn(held[i % len(held)])
        for r in range(max(args.repeats, 5)):
            for name, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for i in range(n):
                    fn(held[i % len(held)])
                e1.record()
                torch.cuda.synchronize()
                host[name].append((time.perf_counter() - t0) / n * 1e3)
                devt[name].append(e0.elapsed_time(e1) / n)
            print(f"{tag} window {r}: " + "  ".join(
                f"{k} {host[k][-1]:.4f} ms (events {devt[k][-1]:.4f})" for k in routes), flush=True)
        med = lambda d: {k: sorted(v)[len(v) // 2] for k, v in d.items()}
        span = lambda d: {k: [min(v), max(v)] for k, v in d.items()}
        mh, md = med(host), med(devt)
        return {"rows": held[0][2], "nnz": held[0][0].numel(), "minibatches_per_window": n,
                "median_ms": mh, "min_max_ms": span(host), "median_event_ms": md,
                "min_max_event_ms": span(devt),
                "composed_over_fused_margins": mh["composed_predict"] / mh["fused_margins"],
                "composed_over_fused_margins_events":
                    md["composed_predict"] / md["fused_margins"]}

    n = max(args.steps, 100)
    res = {"criteo_fixed_39": measure("criteo fixed", fixed, n),
           "criteo_csr_quarter_missing": measure("criteo csr missing", missing, n),
           "csr_wide_65_130": measure("csr wide", wide, max(n // 5, 20))}
    occ, _ = tr.shard.table.census()
    print(json.dumps({
        "metric": "FFM scoring time per minibatch, fused kernel (FFMScorer) vs "
                  "FFMTrainer.predict, 1 GPU, F = 39, k = 2, rows of 80 columns",
        "unit": "ms/minibatch (median of windows)", "windows": max(args.repeats, 5),
        "minibatch": B, "train_steps": args.train_steps, "keys_in_table": occ,
        "table_slots": tr.shard.capacity, "eval": sc.result(),
        "not_measured": ["per-phase cycles", "k = 4 and k = 8 shapes",
                         "F = 64 (one wave per block)", "the grid cap and waves per block"],
        **res}), flush=True)


def fwfm_score_mode(args):
    """1 GPU: scoring held-out minibatches against a field-weighted FM (D = 16, F = 39) with the
    fused kernel (``FwFMTrainer.scorer()``: fwfm_predict.hip, margins only and labels +
    accumulator) and with the composed route (``FwFMTrainer.predict``: mix, resolve, where, then
    fwfm_margins or fwfm_csr_margins), alternated window by window in this one process on a
    table filled by a few training steps. Shapes: Criteo's B x 39 fixed rows; the same rows as
    CSR with a quarter of the slots missing; CSR rows of which a quarter are widened to 65..130
    occurrences. Per route and window: a host clock around the synchronised window, and device
    events around the same launches (for the fused routes, one kernel per minibatch: the
    kernel's own time)."""
    from parameter_server_amd.models.fwfm import FwFMConfig, FwFMTrainer
    from parameter_server_amd.ops.synthetic import criteo_batch

    dev = torch.device("cuda", 0)
    B, N, S = args.minibatch, int(args.num_features), 39
    tr = FwFMTrainer(FwFMConfig(embedding_dim=16, localize=args.localize, num_features=N,
                                minibatch=B, table_capacity=min(args.table_slots, 1 << 24),
                                seed=0), device=dev)
    crit = [criteo_batch(B, seed=77, row0=i * B, num_features=N, device=dev)
            for i in range(args.train_steps + 4)]
    for i in range(args.train_steps):
        tr.step(*crit[i])
    sc = tr.scorer()
    g = torch.Generator(device=dev).manual_seed(5)
    slot_of = torch.arange(S, dtype=torch.int32, device=dev).repeat(B)
    fixed, missing, wide = [], [], []
    for k39, y in crit[args.train_steps:]:
        fixed.append((k39, y, dict(width=S), {}))
        keep = torch.rand(B * S, device=dev, generator=g) < 0.75
        rp = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(keep.view(B, S).sum(1), 0)
        kw = dict(row_ptr=rp, fields=slot_of[keep])
        missing.append((k39[keep], y, kw, kw))
        # a quarter of the rows take the keys of the rows after them (fields repeat there:
        # the diagonal of R acts), as --fwfm's wide route
        width = torch.where(torch.rand(B, device=dev, generator=g) < 0.25,
                            torch.randint(65, 131, (B,), device=dev, generator=g), S)
        rp = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(width, 0)
        row = torch.repeat_interleave(torch.arange(B, device=dev), width)
        pos = torch.arange(int(rp[-1]), device=dev) - rp[row]
        kw = dict(row_ptr=rp, fields=(pos % S).int())
        wide.append((k39.view(B, S)[(row + pos // S) % B, pos % S].contiguous(), y, kw, kw))

    def measure(tag, held, n):
        """held: (keys, labels, the scorer's keywords, predict's keywords)"""
        routes = {"fused_margins": lambda b: sc.predict(b[0], **b[2]),
                  "fused_labels_acc": lambda b: sc.score(b[0], b[1], margins=False, **b[2]),
                  "composed_predict": lambda b: tr.predict(b[0], B, **b[3])}
        a, c = routes["fused_margins"](held[0]), routes["composed_predict"](held[0])
        print(f"{tag}: max |fused - composed| margin = {float((a - c).abs().max()):.3g}, "
              f"max |margin| = {float(c.abs().max()):.3g}", flush=True)
        host, devt = {r: [] for r in routes}, {r: [] for r in routes}
        for fn in routes.values():
            for i in range(args.warmup):
                fn(held[i % len(held)])
        for r in range(max(args.repeats, 5)):
            for name, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for i in range(n):
                    fn(held[i % len(held)])
                e1.record()
                torch.cuda.synchronize()
                host[name].append((time.perf_counter() - t0) / n * 1e3)
                devt[name].append(e0.elapsed_time(e1) / n)
            print(f"{tag} window {r}: " + "  ".join(
                f"{k} {host[k][-1]:.4f} ms (events {devt[k][-1]:.4f})" for k in routes), flush=True)
        med = lambda d: {k: sorted(v)[len(v) // 2] for k, v in d.items()}
        span = lambda d: {k: [min(v), max(v)] for k, v in d.items()}
        mh, md = med(host), med(devt)
        return {"rows": B, "nnz": held[0][0].numel(), "minibatches_per_window": n,
                "median_ms": mh, "min_max_ms": span(host), "median_event_ms": md,
                "min_max_event_ms": span(devt),
                "composed_over_fused_margins": mh["composed_predict"] / mh["fused_margins"],
                "composed_over_fused_margins_events":
                    md["composed_predict"] / md["fused_margins"]}

    n = max(args.steps, 100)
    res = {"criteo_fixed_39": measure("criteo fixed", fixed, n),
           "criteo_csr_quarter_missing": measure("criteo csr missing", missing, n),
           "csr_quarter_wide_65_130": measure("csr quarter wide", wide, n)}
    occ, _ = tr.shard.table.census()
    print(json.dumps({
        "metric": "FwFM scoring time per minibatch, fused kernel (FwFMScorer) vs "
                  "FwFMTrainer.predict, 1 GPU, F = 39, D = 16",
        "unit": "ms/minibatch (median of windows)", "windows": max(args.repeats, 5),
        "minibatch": B, "train_steps": args.train_steps, "keys_in_table": occ,
        "table_slots": tr.shard.capacity, "eval": sc.result(),
        "R_min_max": [float(tr.R.min()), float(tr.R.max())],
        "not_measured": ["per-phase cycles", "other D and F", "a table that misses L2",
                         "other gang sizes and waves per block than the launcher's"],
        **res}), flush=True)


def csr_mode(args):
    """1 GPU: the same Criteo-shaped minibatches through the fixed-width step and through the
    ``row_ptr`` step (fm_csr), alternated window by window in this one process, then an
    rcv1-shaped minibatch (about 75 valued features per row, 47,236 features), which only
    the ``row_ptr`` step can take. Step times by a host clock around synchronised windows."""
    from parameter_server_amd.models.fm import FMConfig, FMTrainer
    from parameter_server_amd.ops.native import hipops
    from parameter_server_amd.ops.synthetic import criteo_batch

    dev = torch.device("cuda", 0)
    B, N, S = args.minibatch, int(args.num_features), 39
    tr = FMTrainer(FMConfig(localize=args.localize, num_features=N, embedding_dim=args.dim,
                            minibatch=B, compact_rows=bool(args.compact_rows),
                            table_capacity=args.table_slots, seed=0), device=dev)
    crit = [criteo_batch(B, seed=77, row0=i * B, num_features=N, device=dev) for i in range(8)]
    uniform = torch.arange(B + 1, device=dev) * S

    rcv = rcv1_batches(B, 4, dev)
    tr_rcv = FMTrainer(FMConfig(localize=args.localize, num_features=47236,
                                embedding_dim=args.dim, minibatch=B, max_nnz=B * 100,
                                compact_rows=bool(args.compact_rows), table_capacity=1 << 17,
                                seed=0), device=dev)

    def fixed(i):
        tr.step(*crit[i % len(crit)])

    def csr(i):
        k, lab = crit[i % len(crit)]
        tr.step(k, lab, row_ptr=uniform)

    def rcv1(i):
        k, lab, v, rp = rcv[i % len(rcv)]
        tr_rcv.step(k, lab, vals=v, row_ptr=rp)

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for fn in (fixed, csr, rcv1):
        for i in range(args.warmup):
            fn(i)
    ms = {"fixed": [], "csr": [], "rcv1": []}
    for r in range(args.repeats):
        for name, fn in (("fixed", fixed), ("csr", csr), ("rcv1", rcv1)):
            ms[name].append(window(fn))
        print(f"window {r}: " + "  ".join(f"{n} {v[-1]:.3f} ms" for n, v in ms.items()),
              flush=True)
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    H = hipops()
    print(json.dumps({
        "metric": "FM step time, fixed-width route vs row_ptr route (fm_csr), 1 GPU",
        "unit": "ms/step (median of windows)", "steps_per_window": args.steps,
        "windows": args.repeats, "minibatch": B, "embedding_dim": args.dim,
        "criteo_fixed_ms": med["fixed"], "criteo_row_ptr_ms": med["csr"],
        "rcv1_row_ptr_ms": med["rcv1"], "all_ms": ms,
        "lanes": {"criteo": H.fm_csr_lanes(B * S, B),
                  "rcv1": H.fm_csr_lanes(rcv[0][0].numel(), B)},
        "rcv1_nnz": rcv[0][0].numel(),
        "train": {"criteo": tr.progress(), "rcv1": tr_rcv.progress()},
    }), flush=True)


def ffm_mode(args):
    """1 GPU: the field-aware FM step (models/ffm.py, ffm.hip) on Criteo-shaped minibatches, for
    k = 2 with one field per slot (rows of 80) and k = 4 with the 13 integer slots on one field
    (F = 27, rows of 112). Beside it, alternated window by window in this one process: the same
    trainer with the kernel replaced by its vectorised PyTorch form on CUDA tensors (expand +
    ``_fwd_bwd_torch``: what there is without the kernel), and the plain FM step at D = 16 as
    context. The k = 2 shape also runs through the CSR step (ffm_csr.hip, a field id per
    occurrence): (a) the same full-width minibatches, against the fixed-width step above, and
    (b) the minibatches with each slot present with probability 0.75 (as bench_csr.py).
    Step times by a host clock around synchronised windows."""
    from parameter_server_amd.models.ffm import FFMConfig, FFMTrainer
    from parameter_server_amd.models.fm import FMConfig, FMTrainer
    from parameter_server_amd.ops import embedding as E
    from parameter_server_amd.ops.synthetic import criteo_batch

    class TorchFFM(FFMTrainer):
        def _fwd_bwd_hip(self, rows_src, rows_idx, vals, B, loc, w_wide, labels):
            S = self.cfg.slots
            X0 = E.expand(loc.local_col, B * S, rows_src, idx=rows_idx)
            return self._fwd_bwd_torch(X0, vals, B, S, loc.local_col, w_wide, labels)

    dev = torch.device("cuda", 0)
    B, N = args.minibatch, int(args.num_features)
    slots = min(args.table_slots, 1 << 24)  # five tables side by side
    crit = [criteo_batch(B, seed=77, row0=i * B, num_features=N, device=dev) for i in range(8)]
    common = dict(localize=args.localize, num_features=N, minibatch=B, table_capacity=slots, seed=0)
    shapes = {"k2_F39": dict(k=2), "k4_F27": dict(k=4, fields=[0] * 13 + list(range(1, 27)))}
    trainers = {"fm_D16": FMTrainer(FMConfig(embedding_dim=16, **common), device=dev)}
    for tag, kw in shapes.items():
        trainers[f"ffm_{tag}"] = FFMTrainer(FFMConfig(**kw, **common), device=dev)
        trainers[f"ffm_{tag}_torch"] = TorchFFM(FFMConfig(**kw, **common), device=dev)

    routes = {name: (lambda i, tr=tr: tr.step(*crit[i % len(crit)]))
              for name, tr in trainers.items()}
    # the CSR step: full rows (row_ptr = 39 b, fields = the slot index), then missing slots
    slot_of = torch.arange(39, dtype=torch.int32, device=dev).repeat(B)
    uniform = torch.arange(B + 1, device=dev) * 39
    g = torch.Generator(device=dev).manual_seed(5)
    sparse = []
    for k39, lab in crit:
        keep = torch.rand(B * 39, device=dev, generator=g) < 0.75
        rp = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(keep.view(B, 39).sum(1), 0)
        sparse.append((k39[keep], lab, rp, slot_of[keep]))
    for tag in ("ffm_k2_F39_csr_full", "ffm_k2_F39_csr_missing"):
        trainers[tag] = FFMTrainer(FFMConfig(k=2, **common), device=dev)

    def csr_full(i, tr=trainers["ffm_k2_F39_csr_full"]):
        k39, lab = crit[i % len(crit)]
        tr.step(k39, lab, row_ptr=uniform, fields=slot_of)

    def csr_missing(i, tr=trainers["ffm_k2_F39_csr_missing"]):
        k, lab, rp, fl = sparse[i % len(sparse)]
        tr.step(k, lab, row_ptr=rp, fields=fl)

    routes["ffm_k2_F39_csr_full"], routes["ffm_k2_F39_csr_missing"] = csr_full, csr_missing

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for fn in routes.values():
        for i in range(args.warmup):
            fn(i)
    ms = {name: [] for name in routes}
    for r in range(args.repeats):
        for name, fn in routes.items():
            ms[name].append(window(fn))
        print(f"window {r}: " + "  ".join(f"{n} {v[-1]:.3f} ms" for n, v in ms.items()),
              flush=True)
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    print(json.dumps({
        "metric": "FFM step time (ffm.hip) vs the same step with the PyTorch forward / backward, "
                  "and the FM step at D = 16, 1 GPU",
        "unit": "ms/step (median of windows)", "steps_per_window": args.steps,
        "windows": args.repeats, "minibatch": B, "slots": 39, "median_ms": med,
        "min_ms": {n: min(v) for n, v in ms.items()}, "max_ms": {n: max(v) for n, v in ms.items()},
        "torch_over_hip": {t: med[f"ffm_{t}_torch"] / med[f"ffm_{t}"] for t in shapes},
        "csr_over_fixed": med["ffm_k2_F39_csr_full"] / med["ffm_k2_F39"],
        "csr_missing_nnz": [int(x[0].numel()) for x in sparse[:2]],
        "row_width": {t: trainers[f"ffm_{t}"].Dr for t in shapes},
        "train": {n: tr.progress() for n, tr in trainers.items()}, "all_ms": ms}), flush=True)


def fwfm_mode(args):
    """1 GPU: the field-weighted FM step (models/fwfm.py, fwfm.hip; D = 16, one field per slot,
    F = 39) on Criteo-shaped minibatches against the FM step at D = 16 and the FFM step at
    k = 2 (rows of 80), and the FwFM's CSR step (fwfm_csr.hip) on the same rows, on rows with
    slots missing and on rows widened past 64 positions, all in this one process, alternated
    window by window. Step times by a host clock around synchronised windows."""
    from parameter_server_amd.models.ffm import FFMConfig, FFMTrainer
    from parameter_server_amd.models.fm import FMConfig, FMTrainer
    from parameter_server_amd.models.fwfm import FwFMConfig, FwFMTrainer
    from parameter_server_amd.ops.synthetic import criteo_batch

    dev = torch.device("cuda", 0)
    B, N = args.minibatch, int(args.num_features)
    slots = min(args.table_slots, 1 << 24)  # three tables side by side
    crit = [criteo_batch(B, seed=77, row0=i * B, num_features=N, device=dev) for i in range(8)]
    common = dict(localize=args.localize, num_features=N, minibatch=B, table_capacity=slots, seed=0)
    trainers = {"fm_D16": FMTrainer(FMConfig(embedding_dim=16, **common), device=dev),
                "fwfm_D16_F39": FwFMTrainer(FwFMConfig(embedding_dim=16, **common), device=dev),
                "ffm_k2_F39": FFMTrainer(FFMConfig(k=2, **common), device=dev)}
    routes = {name: (lambda i, tr=tr: tr.step(*crit[i % len(crit)]))
              for name, tr in trainers.items()}
    # the CSR step (fwfm_csr.hip, a field id per occurrence): (a) the same full rows (row_ptr =
    # 39 b, fields = the slot index) against the fixed-width step above, (b) each slot present
    # with probability 0.75, (c) a quarter of the rows widened to 65..130 positions with the
    # keys of the rows after them (fields repeat there: the diagonal of R acts)
    slot_of = torch.arange(39, dtype=torch.int32, device=dev).repeat(B)
    uniform = torch.arange(B + 1, device=dev) * 39
    g = torch.Generator(device=dev).manual_seed(5)
    full, missing, wide = [], [], []
    for k39, lab in crit:
        full.append((k39, lab, uniform, slot_of))
        keep = torch.rand(B * 39, device=dev, generator=g) < 0.75
        rp = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(keep.view(B, 39).sum(1), 0)
        missing.append((k39[keep], lab, rp, slot_of[keep]))
        width = torch.where(torch.rand(B, device=dev, generator=g) < 0.25,
                            torch.randint(65, 131, (B,), device=dev, generator=g), 39)
        rp = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(width, 0)
        row = torch.repeat_interleave(torch.arange(B, device=dev), width)
        pos = torch.arange(int(rp[-1]), device=dev) - rp[row]
        wide.append((k39.view(B, 39)[(row + pos // 39) % B, pos % 39].contiguous(), lab, rp,
                     (pos % 39).int()))
    wide_cfg = dict(common, slots=64, fields=[i % 39 for i in range(64)])  # max_nnz = 64 B
    for tag, data, kw in (("full", full, common), ("missing", missing, common),
                          ("wide", wide, wide_cfg)):
        tr = trainers[f"fwfm_csr_{tag}"] = FwFMTrainer(FwFMConfig(embedding_dim=16, **kw),
                                                       device=dev)

        def csr(i, tr=tr, data=data):
            k, lab, rp, fl = data[i % len(data)]
            tr.step(k, lab, row_ptr=rp, fields=fl)

        routes[f"fwfm_csr_{tag}"] = csr

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for fn in routes.values():
        for i in range(args.warmup):
            fn(i)
    ms = {name: [] for name in routes}
    for r in range(args.repeats):
        for name, fn in routes.items():
            ms[name].append(window(fn))
        print(f"window {r}: " + "  ".join(f"{n} {v[-1]:.3f} ms" for n, v in ms.items()),
              flush=True)
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    R = trainers["fwfm_D16_F39"].R
    print(json.dumps({
        "metric": "FwFM step time (fwfm.hip) vs the FM step at D = 16 and the FFM step at k = 2, "
                  "1 GPU",
        "unit": "ms/step (median of windows)", "steps_per_window": args.steps,
        "windows": args.repeats, "minibatch": B, "slots": 39, "median_ms": med,
        "min_ms": {n: min(v) for n, v in ms.items()}, "max_ms": {n: max(v) for n, v in ms.items()},
        "fwfm_over_fm": med["fwfm_D16_F39"] / med["fm_D16"],
        "fwfm_over_ffm": med["fwfm_D16_F39"] / med["ffm_k2_F39"],
        "csr_over_fixed": med["fwfm_csr_full"] / med["fwfm_D16_F39"],
        "csr_nnz": {"full": B * 39, "missing": [int(x[0].numel()) for x in missing[:2]],
                    "wide": [int(x[0].numel()) for x in wide[:2]]},
        "R_min_max": [float(R.min()), float(R.max())],
        "train": {n: tr.progress() for n, tr in trainers.items()}, "all_ms": ms}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fwfm", action="store_true",
                    help="1 GPU: the field-weighted FM step (D = 16, F = 39) vs the FM step at "
                         "D = 16 and the FFM step at k = 2, alternated")
    ap.add_argument("--fwfm-score", action="store_true",
                    help="1 GPU: the fused FwFM scorer (FwFMScorer, D = 16, F = 39) vs "
                         "FwFMTrainer.predict on fixed rows, CSR rows with slots missing and CSR "
                         "rows of which a quarter are wider than 64, alternated")
    ap.add_argument("--ffm", action="store_true",
                    help="1 GPU: the field-aware FM step (k = 2, and k = 4 on 27 fields) vs the same "
                         "step with the PyTorch forward / backward and the FM step, alternated")
    ap.add_argument("--csr", action="store_true",
                    help="1 GPU: fixed-width step vs the row_ptr step on the same minibatches, "
                         "alternated, and an rcv1-shaped valued minibatch")
    ap.add_argument("--score", action="store_true",
                    help="1 GPU: the fused scoring kernel (FMScorer) vs FMTrainer.predict on "
                         "held-out minibatches, alternated; D in {16, 32, 64, 128} and rcv1. With "
                         "--ffm: the fused FFM scorer (FFMScorer) vs FFMTrainer.predict on fixed "
                         "rows, CSR rows with slots missing and CSR rows wider than 64")
    ap.add_argument("--train-steps", type=int, default=20,
                    help="--score: training steps that fill the table first")
    ap.add_argument("--repeats", type=int, default=5, help="--csr / --score: windows per route")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--localize", default="sort", choices=("sort", "part"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--num-features", type=float, default=1e9)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--compact-rows", type=int, default=1,
                    help="1 GPU: gather each unique key's row once per step (0: per occurrence "
                         "through the slot index)")
    ap.add_argument("--table-slots", type=int, default=1 << 28, help="slots per GPU")
    ap.add_argument("--prefetch", type=int, default=1,
                    help="generate + localise minibatch t+1 on a side stream during step t")
    args = ap.parse_args()
    if args.fwfm_score:
        return fwfm_score_mode(args)
    if args.fwfm:
        return fwfm_mode(args)
    if args.ffm and args.score:
        return ffm_score_mode(args)
    if args.ffm:
        return ffm_mode(args)
    if args.csr:
        return csr_mode(args)
    if args.score:
        return score_mode(args)
    from parameter_server_amd.models.fm import FMConfig, FMTrainer
    from parameter_server_amd.ops.synthetic import criteo_batch
    from parameter_server_amd.parallel.comm import init_from_env

    comm, dev = init_from_env("cuda")
    G, rank = comm.world, comm.rank
    B, N = args.minibatch, int(args.num_features)
    cfg = FMConfig(localize=args.localize, num_features=N, embedding_dim=args.dim, minibatch=B, compact_rows=bool(args.compact_rows),
                   table_capacity=args.table_slots, seed=0)
    tr = FMTrainer(cfg, comm, dev)
    bufs = [(torch.empty(B * 39, dtype=torch.int64, device=dev),
             torch.empty(B, dtype=torch.float32, device=dev)) for _ in range(2)]
    t = [0]
    locs = [None, None]
    side = torch.cuda.Stream(dev, priority=int(os.environ.get("PSAMD_PREP_PRIORITY", "-1")))  # own HW queues
    main_s = torch.cuda.current_stream(dev)
    ev_prep = [torch.cuda.Event() for _ in range(2)]
    ev_step = [torch.cuda.Event() for _ in range(2)]

    def prep(i):  # minibatch i into buffer i % 2, on the side stream
        b = i % 2
        side.wait_event(ev_step[b])  # the step that last read this buffer is done
        with torch.cuda.stream(side):
            k, lab = bufs[b]
            criteo_batch(B, seed=77 + rank, row0=i * B, num_features=N, device=dev, keys=k,
                         labels=lab)
            locs[b] = tr.localize(k, buf=b)
            ev_prep[b].record(side)

    def step():
        i = t[0]
        b = i % 2
        if args.prefetch:
            if i == 0:
                prep(0)
            prep(i + 1)
            main_s.wait_event(ev_prep[b])
            tr.step(bufs[b][0], bufs[b][1], loc=locs[b])
            ev_step[b].record(main_s)
        else:
            k, lab = bufs[0]
            criteo_batch(B, seed=77 + rank, row0=i * B, num_features=N, device=dev, keys=k,
                         labels=lab)
            tr.step(k, lab)
        t[0] += 1

    for _ in range(args.warmup):
        step()
    tr.progress()
    comm.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    comm.barrier()
    dt = time.perf_counter() - t0
    x = torch.tensor([dt], dtype=torch.float64, device=dev if G > 1 else "cpu")
    comm.all_reduce_(x, op="max")
    dt = float(x.item())
    p = tr.progress()
    occ, _ = tr.shard.table.census()
    if rank == 0:
        print(json.dumps({
            "metric": "examples/sec (whole node) factorization machine, 1e9 hashed features",
            "value": G * B * args.steps / dt, "unit": "examples/sec", "n_gpus": G,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "dtype": "bf16 rows (fp32 math)",
            "config": {"num_features": N, "embedding_dim": args.dim, "slots": 39,
                       "global_batch": G * B, "table_slots_per_gpu": tr.shard.capacity,
                       "shard_gb": tr.shard.nbytes() / 2 ** 30},
            "train": {**p, "rows_rank0": occ},
        }), flush=True)
    if G > 1:
        import torch.distributed as dist

        dist.destroy_process_group()


if __name__ == "__main__":
    main()
