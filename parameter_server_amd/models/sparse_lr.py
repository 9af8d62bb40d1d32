"""Sparse logistic regression trained through the sharded HBM parameter server.

This is the MI355X-native counterpart of the reference's async-SGD linear
method (src/app/linear_method/async_sgd.h: AsyncSGDWorker::computeGradient
:241-289 and AsyncSGDServer with FTRL/SGD/AdaGrad entries :101-178,
MinibatchReader::read src/learner/sgd.h:131-150). One process per GPU; every
rank is a colocated worker (data shard ``rank``) and server shard (key range
``rank`` of the mixed key space).

One training step on a rank (all on the GPU, no host round trip when G == 1):
  localise      mix -> radix sort -> RLE  (unique keys, local cols, CSC order)
  [tail filter] CountMin insert/query of per-key counts, drop rare keys
  pull          G == 1: lookup-or-insert in the local HBM table;
                G  > 1 (exchange="padded", default): keys are sorted by owner ->
                fixed-capacity row per peer [keys(t) | grads(t-1)] with the
                counts in the row header -> equal-split all-to-all -> owner applies
                the pushes of t-1, then resolves the pulls of t -> all-to-all of
                weights. No host sync, so the step replays from HIP graphs between
                the two collectives (exchange="exact": count all-gather + sized
                all-to-all-v, one host sync per step)
  forward       Xw, loss, dL/dXw, accuracy, AUC histogram (one kernel)
  backward      segmented reduction over the CSC order -> grad per unique key
  push          G == 1: optimizer update at the cached slots (key caching: the
                push never re-sends or re-hashes keys);
                G  > 1: gradients ride the next step's exchange [FixingFloat nb-byte
                codes] -> owner applies one optimizer step per source row in rank
                order (reference semantics: one FTRL step per push message) or
                sums them first (``push_mode='aggregate'``, synchronous SGD).
"""
from __future__ import annotations

import math
import os
import time
from dataclasses import dataclass, field

import torch

from ..ops.countmin import CountMinSketch
from ..ops.keymix import key_bits_for, unmix
from ..ops.kv_table import InitRule, KVTable, UpdateRule, next_pow2
from ..ops.linear import (AUC_BINS, HIST_STRIPES, accum_total, auc_from_hist, fused_update_ok,
                          linear_fwd_bwd, loss_id, new_accum)
from ..ops.localize import Localizer
from ..ops.native import hipops
from ..parallel.comm import Comm, LocalComm
from ..parallel.consistency import ExchangeSchedule, MergedSchedule, parse_consistency
from ..parallel.partition import KeyPartition
from ..utils.trace import enabled as trace_enabled
from ..utils.trace import trace_range
from .sparse_lr_exact import ExactExchange
from .sparse_lr_growth import TableGrowth
from .sparse_lr_p2p import P2PExchange
from .sparse_lr_padded import PaddedExchange


# tp_fwd_bwd_csr encodes an occurrence's row as its offset from the tile's first row in 19
# bits: minibatches of this many rows or more take the compact path
_CSR_MAX_ROWS = (1 << 19) - 1


# the flat step's (sum, count) gradient accumulators hold |gradient| <= B < 2^25 (binary
# features, ops/linear.fused_update_ok): larger minibatches take the compact path too
_FLAT_MAX_ROWS = 1 << 25


def route(B: int, width, nnz: int, *, row_ptr: bool = False, rows: bool = False,
          vals: bool = False, flat_loc: bool = True, width_ok: bool = True,
          exchange_ok: bool = True, allow_csr: bool = True, prefetch: bool = False) -> str:
    """The layout that runs a minibatch of ``B`` rows and ``nnz`` occurrences (fixed
    ``width``, or None with a row_ptr): "flat" (fixed width, binary features: the fused
    flat forward/backward), "flat_csr" (valued and / or variable-width rows on the flat
    layout: tp_fwd_bwd_csr) or "compact" (a compact localisation and the generic step).
    Pure host logic, shared by ``step``, ``step_segments`` and the merged sequential API.

    ``row_ptr`` / ``rows`` / ``vals``: whether the minibatch comes with them. ``flat_loc``:
    its localisation is flat (or still to do, with the flat mode active). ``width_ok``:
    tp_fwd_bwd has an instance for ``width``. ``exchange_ok``: the flat exchange kernels
    serve this size (tpf_exchange_ok; true on one GPU). The entry point's restrictions:
    ``prefetch`` -- one GPU, a prefetch callback wants the generic step's blocking point;
    ``allow_csr=False`` -- the sequential ``step`` of the two-collective padded exchange
    has always localised valued and variable-width minibatches compactly, and the CSR
    kernel sums a key's occurrences in another order, so routing them flat would change
    its results at rounding level."""
    if not flat_loc or not exchange_ok or prefetch:
        return "compact"
    if row_ptr or vals:
        return "flat_csr" if allow_csr and B < _CSR_MAX_ROWS else "compact"
    if rows or not width or nnz != B * width or B >= _FLAT_MAX_ROWS or not width_ok:
        return "compact"
    return "flat"


@dataclass
class SparseLRConfig:
    num_features: int = 10 ** 9          # hashed feature space (keys in [0, N)); 0 = raw u64
    minibatch: int = 10000               # examples per worker step (reference SGDConfig.minibatch)
    max_nnz_per_example: int = 39
    loss: str = "logit"
    algo: str = "ftrl"                   # ftrl | adagrad | sgd
    lr_type: str = "decay"               # constant | decay
    alpha: float = 0.01
    beta: float = 10.0
    l1: float = 10.0
    l2: float = 1.0
    grad_scale: float = 1.0
    max_delta: float = 0.0               # per-update |dw| clip (trust region), 0 = off
    table_capacity: int = 0              # slots per shard (power of 2); 0 = auto
    table_load: float = 0.5              # auto capacity = num_features / G / load
    max_table_bytes: int = 96 << 30      # cap for the auto size and for growth (per GPU)
    # grow the table on the device instead of failing when it fills (sparse_lr_growth.py):
    # once the host's upper bound of the occupied slots passes table_grow_check x capacity
    # the exact count is taken, and a table more than table_grow_at full is rehashed into
    # one at most table_grow_at / 2 full. Off: the capacity is fixed, as before
    table_growth: bool = False
    table_grow_check: float = 0.75
    table_grow_at: float = 0.5
    init: InitRule = field(default_factory=InitRule)
    # ssp (lag >= 1) owner apply of the carried pushes: "post" = after the exchange's
    # pulls are resolved and the weights sent back (off the worker's critical path),
    # "pre" = before resolving them; same visibility (parallel/consistency.py)
    ssp_apply: str = "post"
    tail_feature_freq: int = 0           # keep keys seen > freq times (0 = off)
    countmin_n: float = 1e8
    countmin_k: int = 2
    consistency: str = "bsp"             # bsp | ssp:<tau> | asp
    push_mode: str = "sequential"        # sequential | aggregate
    localize: str = "auto"               # auto (= tp where supported, else sort) | tp | sort |
                                         # part (tp: <= 34-bit keys, part: <= 32-bit keys)
    fixing_float_bytes: int = 0          # 0 = off, else 1..7 bytes per pushed gradient
    # multi-GPU data plane: "padded" = fixed-capacity rows per peer with device-side
    # counts (no host sync, graph-replayable); "exact" = count exchange + sized
    # all-to-all-v (one host sync per step); "p2p" = one-sided peer-HBM pulls and
    # inbox pushes, no collective per step (asynchronous only, parallel/p2p.py)
    exchange: str = "padded"
    p2p_queue: int = 16                  # p2p: inbox entries per source (staleness bound)
    p2p_rounds: int = 2                  # p2p: inbox entries applied per source per step
    exchange_capacity: int = 0           # keys per peer per step; 0 = auto (first step)
    exchange_slack: float = 1.5          # auto capacity = slack * max per-peer count + 1024
    # padded exchange pipelining depth: pushes of step t ride the exchange of step
    # t + 1 + lag, so the exchanges of steps t+1 .. t+lag can run while step t
    # computes; the pull of step t then misses exactly the `lag` most recent steps of
    # pushes. -1 = from `consistency` (bsp -> 0, ssp:tau -> tau, asp -> 1)
    exchange_lag: int = -1
    asp_depth: int = 4                   # asp: exchanges whose push applies may be in flight
    # padded exchange with lag >= 1: ONE all-to-all per step carrying [keys(t+1) |
    # grads(t-d) | weights of keys(t)] (parallel/consistency.MergedSchedule) instead of
    # two (keys + grads, then weights). "auto": on for ssp:tau >= 2; "on" also for
    # ssp:1 (worker and exchange then serialise) and asp (staleness exactly 3); "off":
    # two collectives
    exchange_merge: str = "auto"
    seed: int = 0

    def update_rule(self) -> UpdateRule:
        return UpdateRule(self.algo, self.lr_type, self.alpha, self.beta, self.l1, self.l2,
                          self.grad_scale, self.max_delta)


# Per-algorithm server defaults for the pushed minibatch-SUM gradients (the reference's
# push format, async_sgd.h:263-289). FTRL-proximal is the reference CTR online config
# (example/linear/ctr/online_l1lr.conf: L1 10 / L2 1, DECAY alpha .01 beta 10). AdaGrad
# normalises by the accumulated gradient norm like FTRL, so the same step trains. Plain
# SGD takes the raw minibatch sum: a hot key's gradient is ~B x larger than a rare
# key's, and with G workers an owner applies up to G pushes of a key per step, so its
# step is 30x smaller (benchmarks/train_check.py, 65,536 x 39 Criteo-shaped, 50 steps:
# alpha .01 diverges at 1 GPU (loss 4.7); .001 trains at 1 GPU (0.556) but diverges with
# 8 asynchronous peers + 2-byte fixing-float (2.56); .0003 trains there (0.621, AUC .734);
# profiles/r3_train_sweep.log).
ALGO_DEFAULTS = {
    "ftrl": dict(lr_type="decay", alpha=0.01, beta=10.0, l1=10.0, l2=1.0, grad_scale=1.0,
                 max_delta=0.0),
    "adagrad": dict(lr_type="decay", alpha=0.01, beta=10.0, l1=10.0, l2=1.0, grad_scale=1.0,
                    max_delta=0.0),
    "sgd": dict(lr_type="decay", alpha=0.0003, beta=10.0, l1=10.0, l2=1.0, grad_scale=1.0,
                max_delta=0.0),
}


def algo_defaults(algo: str) -> dict:
    return dict(ALGO_DEFAULTS[algo.lower()])


class SparseLRTrainer(PaddedExchange, ExactExchange, P2PExchange, TableGrowth):
    """The trainer: construction, localisation, routing, ``step`` and the 1-GPU plans,
    reporting and checkpointing. The multi-GPU data planes are mixins: the padded and
    merged exchange (sparse_lr_padded.py), the exact / fused exchange and the generic
    pull / push (sparse_lr_exact.py), the one-sided peer exchange (sparse_lr_p2p.py); so is
    the opt-in table growth (sparse_lr_growth.py)."""

    def __init__(self, cfg: SparseLRConfig, comm: Comm | None = None, device="cpu"):
        # (checked before anything is allocated: the table may be most of the HBM)
        if cfg.exchange not in ("padded", "exact", "p2p"):
            raise ValueError(f"exchange must be 'padded', 'exact' or 'p2p', not {cfg.exchange!r}")
        if cfg.exchange_merge not in ("auto", "on", "off"):
            raise ValueError(f"exchange_merge must be auto / on / off, not {cfg.exchange_merge!r}")
        if cfg.ssp_apply not in ("post", "pre"):
            raise ValueError(f"ssp_apply must be 'post' or 'pre', not {cfg.ssp_apply!r}")
        self.cfg = cfg
        self.comm = comm or LocalComm(device)
        self.G, self.rank = self.comm.world, self.comm.rank
        self._growth_supported(cfg, self.G)
        self.device = torch.device(device)
        self.gpu = self.device.type == "cuda"
        self.bits = key_bits_for(cfg.num_features)
        self.part = KeyPartition(self.bits, self.G)
        self.rule = cfg.update_rule()
        self.tau = parse_consistency(cfg.consistency)
        cap = cfg.table_capacity or self.auto_capacity(cfg, self.G, self.bits)
        # ordered home slots over this shard's mixed-key range: sorted unique keys then
        # walk the (up to 64 GB) table in increasing address order
        # (the loopback emulation's one rank owns every peer's range: order over all)
        self._loopback = getattr(self.comm, "backend", "") == "loopback"
        rng = ((self.part.range_of(0)[0], self.part.range_of(self.G - 1)[1]) if self._loopback
               else self.part.range_of(self.rank))
        self.table = KVTable(cap, self.device, cfg.init, key_range=rng)
        self.max_nnz = cfg.minibatch * cfg.max_nnz_per_example
        # tail filter (reference MinibatchReader::read, sgd.h:131-150): a CountMin sketch
        # partitioned by mixed-key range (ops/countmin.py), so the flat localiser's bucket
        # workgroups insert and query it inside their own launch
        self.filter = (CountMinSketch(int(cfg.countmin_n), cfg.countmin_k, self.device,
                                      key_bits=self.bits)
                       if cfg.tail_feature_freq > 0 else None)
        # 1 GPU: entry scan + optimizer update fused (PSAMD_FUSED_UPDATE=0: scan, then
        # kv_update); read once, not per step (host issue time)
        self._fused_update = os.environ.get("PSAMD_FUSED_UPDATE", "1") != "0"
        mode = cfg.localize
        # the flat layout (Localizer "tpf": fixed per-bucket regions, ops/localize.FlatLoc):
        # 1 GPU: the step's pull fused into the previous step's update (tpf_step); G > 1
        # on the padded exchange: owner rows packed straight from the bucket regions (G a
        # power of two dividing the bucket groups, tpf_exchange_ok). PSAMD_FLAT=0: "tp"
        flat_env = os.environ.get("PSAMD_FLAT", "1") != "0"
        self._flat_x = False  # G > 1: the padded exchange on the flat layout
        # (the tail filter runs inside the flat bucket kernel: tpf_filter_unit)
        if self.G == 1:
            flat_ok = self.gpu and self._fused_update and flat_env
        else:
            flat_ok = self._flat_x = bool(
                self.gpu and flat_env and cfg.exchange == "padded"
                and self.bits <= 34 and hipops().tploc_supported(self.max_nnz, self.bits)
                and hipops().tpf_exchange_ok(self.max_nnz, self.bits, self.G))
        if mode == "auto":  # tile dedup + key-range buckets (Localizer falls back to sort
            mode = "tpf" if flat_ok else "tp"  # for > 34-bit keys or > 5.2 M keys)
        if mode == "tpf" and not flat_ok:
            mode = "tp"
        self._flat_x = self._flat_x and mode == "tpf"
        if cfg.tail_feature_freq > 0 and mode == "tp":
            mode = "sort"  # the tail filter needs per-key nnz counts (seg_start over nnz)
        # local columns on demand: the fused tp forward/backward reads the entry map
        self.localizer = self._new_localizer(mode)
        self.localize_mode = self.localizer.mode  # after the Localizer's fallbacks
        self._localizers = [self.localizer]  # + a second buffer set for prefetching (G > 1)
        self._compact = None  # flat mode: a "tp" Localizer for steps the flat path cannot run
        # flat mode: (id, generation) of the FlatLoc whose pull the previous step issued
        # ahead (fused into its update launch); valid for the very next step only
        self._pre = None
        dev = self.device
        self.metrics = new_accum(dev)  # [loss, correct, n, auc_sum, auc_n, ...] (striped)
        self.stats = new_accum(dev)    # [nnz delta, sum w^2, sum dw^2] (striped)
        self.hist = torch.zeros(HIST_STRIPES * 2 * AUC_BINS, dtype=torch.int32, device=dev)
        self.coef = torch.empty(cfg.minibatch, dtype=torch.float32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)  # device step clock
        if self.gpu:
            self.slot_buf = torch.empty(self.max_nnz, dtype=torch.int64, device=dev)
            self.w_buf = torch.empty(self.max_nnz, dtype=torch.float32, device=dev)
            self.touched = None
        # multi-GPU: fuse push(t-1) into the pull exchange of step t (2 all-to-alls/step)
        self.p2p = self.G > 1 and cfg.exchange == "p2p"
        if self.p2p and (not self.gpu or self.filter is not None
                         or cfg.push_mode == "aggregate" or not math.isinf(self.tau)):
            raise ValueError("exchange='p2p' is the asynchronous GPU data plane: consistency "
                             "'asp', no tail filter, sequential pushes")
        self.px = None  # PeerExchange (p2p, set up on the first step)
        self.padded = self.G > 1 and cfg.exchange == "padded"
        self.fused = (self.G > 1 and self.filter is None and cfg.fixing_float_bytes == 0
                      and not self.padded and not self.p2p)
        self.xc = None  # padded-exchange state (allocated on the first step)
        # consistency on the padded exchange: the pushes of step t ride exchange t+1+lag
        # and are applied before its pulls, so the pull of step t sees exactly the
        # pushes of steps <= t-1-lag (bsp: lag 0; ssp:tau: lag tau). asp: lag 1 and the
        # owner applies pushes on their own stream, which later pulls do not wait for
        # (only buffer reuse bounds it: async_depth exchanges in flight).
        self.sched = ExchangeSchedule(self.tau, cfg.exchange_lag, cfg.asp_depth,
                                      post=cfg.ssp_apply == "post")
        self.lag, self.asp, self.async_depth = self.sched.lag, self.sched.asp, self.sched.depth
        # rings of R exchange buffers indexed by step (>= 2: the exchange of step t+1
        # runs while the worker half of step t still reads its weights)
        self.R = self.sched.R
        # (auto: ssp:tau >= 2, and asp for FTRL / AdaGrad, served on the merged exchange
        # with staleness exactly 3 (an admissible asp schedule; both train there at 8
        # emulated peers + fixing-float, tests/test_train_quality_gpu.py; config 4 FTRL FF 1 B
        # 0.1299 -> 0.1205 ms, profiles/r6_asp_merged.log). Plain SGD diverged at
        # staleness 3 (loss 1.03 after 50 steps) and at staleness 2 the merged exchange
        # serialises with the worker (0.143 vs 0.130 ms): asp SGD keeps the two-collective
        # exchange, whose owner applies run beside the pulls)
        asp_merge = math.isinf(self.tau) and cfg.algo.lower() in ("ftrl", "adagrad")
        self.merged = bool(
            self.padded and cfg.exchange_merge != "off"
            and self.tau > 0 and (cfg.exchange_merge == "on" or asp_merge
                                  or (not math.isinf(self.tau) and self.tau >= 2)))
        self.msched = None
        if self.merged:  # one collective per step (MergedSchedule)
            self.msched = MergedSchedule(self.tau, cfg.exchange_lag)
            self.lag, self.asp, self.async_depth = self.msched.lag, False, 0
            self.R = self.msched.R
        self._mx_pend = None      # sequential API: the minibatch whose worker half is due
        self._mx_next = None      # index of the next merged exchange (None: bootstrap due)
        self._mx_external = False  # exchanges issued by a caller's pipeline (bench.py)
        self._xt = 0  # padded steps computed (worker halves run)
        self._xx = 0  # padded exchanges issued (exchange halves run)
        self.pending = None
        self._prefetch = None
        self._coef_views = {}  # B -> self.coef[:B]
        self._row_ptrs = {}    # (B, width) -> the arithmetic row_ptr of a fixed width
        self._rows = None      # scratch: the row of every occurrence (csr_rows)
        self._tf = None        # tail-filter workspaces (_tail_filter)
        self._pf = None        # filtered-pull workspaces, 1 GPU (_pull_filtered)
        self._mx_own = {}      # merged sequential API: private localisers (_mx_private_loc)
        # FixingFloat pushes: the stochastic-rounding seed (the device step clock varies it)
        self._ff_seed = (cfg.seed * 7919 + 17) & ((1 << 64) - 1)
        self._plans = {}  # 1 GPU: native launch lists of the fused step (_step_plan)
        self._growth_setup()
        self.step_count = 0
        self.examples = 0
        self.comm_bytes = 0
        self.t0 = time.time()

    def prefill(self, count: int, chunk: int = 1 << 24, seed: int = 12345) -> int:
        """Insert ``count`` random keys of this shard's mixed-key range (zero state), so
        a benchmark can measure the populated-table regime (probe lengths, TLB / DRAM
        page behaviour of a large table) instead of an almost empty one. Returns the
        occupied slots afterwards. (Reference: KVStore grows its hash map with every
        new key, src/parameter/kv_store.h:37-57.)"""
        from ..ops.keymix import random_keys_in_range

        self._pre = None  # (a pull issued ahead would miss nothing here, but stay strict)
        # the table's own key range (the loopback emulation's one rank owns all G ranges)
        lo, hi = self.table.key_range or self.part.range_of(self.rank)
        g = torch.Generator(device=self.device).manual_seed(seed + self.rank)
        done = 0
        while done < count:
            n = min(chunk, count - done)
            if self._growth is not None:
                self._growth.admit(n)
            mk = random_keys_in_range(lo, hi, n, g, self.device)
            self.table.resolve(mk, insert=True, with_w=False)
            done += n
        self.table.check_ok()
        return self.table.census()[0]

    @staticmethod
    def auto_capacity(cfg: SparseLRConfig, G: int, bits: int) -> int:
        n = cfg.num_features if cfg.num_features else (1 << 27)
        want = next_pow2(int(math.ceil(n / G / cfg.table_load)))
        cap_max = 1 << max(6, (cfg.max_table_bytes // 32).bit_length() - 1)
        return max(1024, min(want, cap_max))

    # ------------------------------------------------------------------ step
    def localize(self, keys: torch.Tensor, buf: int = 0, stage: int = 0):
        """Localise a minibatch into buffer set ``buf`` (0 or 1). Used to prefetch the
        next minibatch on a side stream while the current step waits for its
        exchange (``step(..., loc=..., prefetch=...)``). ``stage`` (flat layout + tail
        filter): 4 = tile + bucket, 3 = the filter (``Localizer``)."""
        while len(self._localizers) <= buf:
            self._localizers.append(self._new_localizer(self.localize_mode))
        return self._localizers[buf](keys, stage) if stage else self._localizers[buf](keys)

    def _new_localizer(self, mode: str) -> Localizer:
        """A localisation workspace of this trainer (flat: with the fused tail filter)."""
        tf = ((self.filter, self.cfg.tail_feature_freq)
              if self.filter is not None and mode == "tpf" else None)
        return Localizer(self.max_nnz, self.bits, self.device, mode=mode, lazy_cols=True,
                         sorted_keys=self._flat_x if mode == "tpf" else False, tail_filter=tf)

    def step(self, keys: torch.Tensor, labels: torch.Tensor, *, width: int | None = None,
             row_ptr: torch.Tensor | None = None, vals: torch.Tensor | None = None,
             rows: torch.Tensor | None = None, loc=None, prefetch=None, next_loc=None):
        """One minibatch: pull, forward, backward, push. ``keys`` are raw feature ids
        in CSR order (fixed ``width`` per row, or ``row_ptr``). ``loc``: an already
        localised minibatch (``localize``); ``prefetch``: called once the step's
        exchange counts are in flight and before the step blocks on them (multi-GPU),
        so the caller can enqueue the next minibatch's work on another stream.
        ``next_loc`` (1 GPU, flat layout): the NEXT minibatch, already localised; its
        pull runs in this step's update launch (after the update, in the same
        workgroups), and the next ``step(loc=next_loc)`` skips its own pull. The table
        is fully updated when this step's work completes either way."""
        if self._growth is not None:  # (before anything of this step is issued)
            self._growth_step(keys, loc, next_loc)
        pre, self._pre = self._pre, None  # a pull issued ahead serves the next step only
        if self.localize_mode == "tpf" and self.G == 1:
            B = labels.numel()
            width = self._width(width, row_ptr)
            how = self._route(B, width, keys.numel() if loc is None else loc.nnz, row_ptr, rows,
                              vals, loc, prefetch=prefetch is not None)
            if how != "compact":
                if loc is None:
                    loc = self.localizer(keys)
                pre = pre == (id(loc), loc.gen)
                if how == "flat":  # one native launch list per (buffers, labels, next)
                    plan, nxt = self.flat_plan(loc, labels, B, width, next_loc, pre)
                    plan.run()
                    self.flat_done(B, nxt)
                else:
                    # valued and / or variable-width rows: the same flat step with the CSR
                    # fused forward + tile backward (tp_fwd_bwd_csr)
                    csr = self._csr_operands(B, width, loc.nnz, row_ptr, rows, vals)
                    if rows is None:
                        hipops().csr_rows(csr[0], csr[1])
                    self._flat_step_csr(loc, labels, B, csr, next_loc, pre)
                return
            # not expressible on the flat layout: the same keys through a compact
            # localisation and the generic step below
            loc = self._compact_localizer()(keys)
        if self.p2p:
            if loc is None:
                loc = self.localizer(keys)
            return self._p2p_step(loc, labels, width, prefetch)
        if self.merged:
            return self._mx_step(keys, labels, width=width, row_ptr=row_ptr, vals=vals,
                                 rows=rows, loc=loc, prefetch=prefetch)
        if self.padded:
            if loc is None:
                with trace_range("localize"):
                    # (flat mode only: elsewhere the trainer's own localiser is the compact one)
                    if self.localize_mode == "tpf" and self._route(
                            labels.numel(), self._width(width, row_ptr), keys.numel(), row_ptr,
                            rows, vals, None, allow_csr=False) == "compact":
                        loc = self._compact_localizer()(keys)
                    else:
                        loc = self.localizer(keys)
            segs = self.step_segments(keys, labels, width=width, row_ptr=row_ptr, vals=vals,
                                      rows=rows, loc=loc)
            for kind, fn in segs:
                if kind == "comm" and prefetch is not None:
                    prefetch()  # overlap the next minibatch with this step's exchange
                    prefetch = None
                fn()
            return
        B = labels.numel()
        width = self._width(width, row_ptr)
        if (self.G == 1 and self.gpu and self.filter is None and self._fused_update
                and row_ptr is None and rows is None and vals is None and prefetch is None
                and not trace_enabled()):
            if loc is None:
                loc = self.localizer(keys)
            plan = self._step_plan(loc, labels, B, width)
            if plan is not None:  # resolve + fused forward/backward + fused scan/update
                plan.run()
                self.step_count += 1
                self.examples += B
                return
        if row_ptr is not None and rows is None:
            rows = self._csr_rows(row_ptr, keys.numel())
        if loc is None:
            with trace_range("localize"):
                loc = self.localizer(keys)
        self._prefetch = prefetch
        with trace_range("pull"):
            if self.filter is not None:
                w_local, push = self._pull_filtered(loc)
            elif self.G == 1 and self.gpu:
                slot, w_local = self.slot_buf, self.w_buf
                hipops().kv_resolve(self.table.slots, loc.uniq, loc.n_uniq, slot, w_local, True,
                                    *self.table.resolve_args())
                push = ("local", slot, loc.n_uniq)
            elif self.fused:
                w_local, push = self._exchange_fused(loc)
            else:
                w_local, push = self._pull(loc.uniq, loc.n_uniq)
        if self._prefetch is not None:  # single-GPU / non-fused paths: no blocking point
            self._prefetch()
            self._prefetch = None
        # 1 GPU: the entry scan applies the FTRL / AdaGrad / SGD update and the AUC
        # epilogue itself (tp_seg_update)
        fused_update = (push[0] == "local" and push[2] is not None and self._fused_update
                        and fused_update_ok(loc, w_local, B=B, width=width or 0, row_ptr=row_ptr,
                                            rows=rows, vals=vals))
        with trace_range("compute"):
            if fused_update:
                linear_fwd_bwd(loc, w_local, labels, B=B, width=width, vals=vals,
                               loss=self.cfg.loss, coef=self._coef(B), metrics=self.metrics,
                               hist=self.hist, update=(self.table.slots, push[1], self.rule,
                                                       self.stats, self.step_dev))
            else:
                _, grad = linear_fwd_bwd(loc, w_local, labels, B=B, width=width or 0,
                                         row_ptr=row_ptr, rows=rows, vals=vals,
                                         loss=self.cfg.loss, coef=self.coef[:B],
                                         metrics=self.metrics, hist=self.hist)
        if not fused_update:
            with trace_range("push"):
                if push[0] == "fused":
                    # deferred: travels with the next step's pull exchange (_exchange_fused)
                    _, slot, send_c, recv_c, U = push
                    self.pending = (slot, send_c, recv_c, grad[:U].clone())
                    folded = False
                else:
                    folded = self._push(grad, push, fold_auc=True)
            if not folded:
                auc_from_hist(self.hist, self.metrics, self.step_dev)
        self.step_count += 1
        self.examples += B

    def _csr_rows(self, row_ptr: torch.Tensor, nnz: int) -> torch.Tensor:
        """Row id of every CSR position (int32)."""
        if self.gpu:
            rows = torch.empty(nnz, dtype=torch.int32, device=row_ptr.device)
            hipops().csr_rows(row_ptr, rows)
            return rows
        B = row_ptr.numel() - 1
        return torch.repeat_interleave(torch.arange(B, dtype=torch.int32),
                                       (row_ptr[1:] - row_ptr[:-1]).long())

    def _compact_localizer(self, buf: int = 0) -> Localizer:
        """Flat mode: the "tp" Localizer (workspace ``buf``) for minibatches the flat
        layout cannot express (valued or variable-width rows)."""
        if self._compact is None:
            self._compact = []
        while len(self._compact) <= buf:
            self._compact.append(self._new_localizer(self._compact_mode()))
        return self._compact[buf]

    def _compact_mode(self) -> str:
        """(tail filter: "sort", whose segments count occurrences; tp's count entries)"""
        return "sort" if self.filter is not None else "tp"

    # ------------------------------------------------ routing and minibatch operands
    _WIDTH_OK: dict = {}  # width -> tp_fwd_bwd_supported(width)

    def _route(self, B: int, width, nnz: int, row_ptr, rows, vals, loc, **entry) -> str:
        """``route`` of a minibatch of this trainer (``entry``: the calling entry point's
        restrictions). Asks the native library only where a flat layout is in play."""
        if not (getattr(loc, "flat", False) if loc is not None else self.localize_mode == "tpf"):
            return "compact"
        ok = self._WIDTH_OK.get(width) if width else False
        if ok is None:
            ok = self._WIDTH_OK[width] = bool(hipops().tp_fwd_bwd_supported(width))
        return route(B, width, nnz, row_ptr=row_ptr is not None, rows=rows is not None,
                     vals=vals is not None, width_ok=ok,
                     exchange_ok=self.G == 1 or bool(hipops().tpf_exchange_ok(nnz, self.bits,
                                                                              self.G)),
                     **entry)

    def _width(self, width, row_ptr):
        """A minibatch's fixed row width: given, else the configured one (None with a
        ``row_ptr`` and no width: variable-width rows)."""
        return width or (None if row_ptr is not None else self.cfg.max_nnz_per_example)

    def _coef(self, B: int) -> torch.Tensor:
        v = self._coef_views.get(B)
        if v is None:
            v = self._coef_views[B] = self.coef[:B]
        return v

    def _csr_operands(self, B: int, width, nnz: int, row_ptr, rows, vals):
        """(row_ptr, rows, vals) of a minibatch for the CSR kernels: ``row_ptr`` given, or
        a fixed width's arithmetic one (cached per shape); ``rows`` (the row of every
        occurrence) given, or the trainer's scratch, which the caller fills from
        ``row_ptr`` (csr_rows) where its consumer is issued -- at replay time inside a
        capturable segment."""
        if row_ptr is None:
            row_ptr = self._row_ptrs.get((B, width))
            if row_ptr is None:
                row_ptr = self._row_ptrs[B, width] = torch.arange(
                    0, (B + 1) * width, width, dtype=torch.int64, device=self.device)
        return row_ptr, rows if rows is not None else self._rows_buf(nnz), vals

    def _compact_rows(self, row_ptr, rows, nnz: int):
        """``rows`` of a variable-width minibatch on the compact layout: given, the
        scratch (GPU: filled by csr_rows next to its consumer) or computed here (CPU)."""
        if row_ptr is None or rows is not None:
            return rows
        return self._rows_buf(nnz) if self.gpu else self._csr_rows(row_ptr, nnz)

    def _rows_buf(self, nnz: int) -> torch.Tensor:
        rb = self._rows
        if rb is None or rb.numel() < nnz:
            rb = self._rows = torch.empty(max(nnz, self.max_nnz), dtype=torch.int32,
                                          device=self.device)
        return rb[:nnz]

    # ----------------------------------------------- flat 1-GPU step (Localizer "tpf")
    def _tpf_common(self) -> tuple:
        """The table, optimizer and statistics arguments of every tpf_step launch."""
        return (self.table.slots, *self.table.resolve_args(), *self.rule.args(), self.stats)

    def _flat_step_csr(self, loc, labels, B: int, csr, next_loc, pre: bool):
        """The flat 1-GPU step for valued / variable-width rows (``csr``: (row_ptr, rows,
        vals)): pull (unless issued ahead), the CSR fused forward + tile backward, then
        tpf_step (update of this minibatch + pull of ``next_loc``). Issued op by op:
        minibatch shapes vary."""
        nxt = next_loc if (next_loc is not None and getattr(next_loc, "flat", False)
                           and next_loc.nnz == loc.nnz and next_loc is not loc) else None
        H, common = hipops(), self._tpf_common()
        n, bits = loc.nnz, loc.bits
        if not pre:
            H.tpf_step(n, bits, None, None, loc.bufs, loc.w_ent, *common, None, None, None)
        H.tp_fwd_bwd_csr(loc.rep, loc.dcnt, None, n, *csr, loc.w_ent, labels, B,
                         loss_id(self.cfg.loss), self._coef(B), self.metrics, self.hist,
                         AUC_BINS, loc.psum, None, None, None, None, False)
        H.tpf_step(n, bits, loc.bufs, loc.psum, nxt.bufs if nxt is not None else None,
                   nxt.w_ent if nxt is not None else None, *common, self.hist, self.metrics,
                   self.step_dev)
        self.flat_done(B, nxt)

    def flat_done(self, B: int, nxt):
        """Host bookkeeping of a flat step whose launches were issued (``flat_plan``)."""
        if nxt is not None:
            self._pre = (id(nxt), nxt.gen)
        self.step_count += 1
        self.examples += B

    def flat_plan(self, loc, labels, B: int, width: int, next_loc, pre: bool, fb_record=None):
        """(LaunchList of one flat step: pull (unless issued ahead) -> fused forward + tile
        backward -> tpf_step, the update of this minibatch and then the pull of ``next_loc``
        (same size) in the same launch; the next FlatLoc that launch pulls or None);
        cached per (buffers, labels, next buffers). bench.py splices it into its native
        multi-stream iteration lists. ``fb_record``: an event recorded between the fused
        forward/backward and the step kernel (a preparation stream may wait for it)."""
        nxt = next_loc if (next_loc is not None and getattr(next_loc, "flat", False)
                           and next_loc.nnz == loc.nnz and next_loc is not loc) else None
        key = (id(loc), id(labels), B, width, loc.nnz, pre, id(nxt) if nxt is not None else 0,
               id(self.rule), id(self.table.init), id(fb_record))
        plan = self._plans.get(key)
        if plan is None:
            H, common = hipops(), self._tpf_common()
            n, bits = loc.nnz, loc.bits
            plan = H.LaunchList()
            if not pre:  # this minibatch's pull on its own
                plan.add_tpf_step(n, bits, None, None, loc.bufs, loc.w_ent, *common, None, None,
                                  None)
            plan.add_tp_fwd_bwd(loc.rep, loc.dcnt, None, n, width, None, loc.w_ent, labels, B,
                                loss_id(self.cfg.loss), self.coef[:B], self.metrics, self.hist,
                                AUC_BINS, loc.psum, None, None, None, None, False)
            if fb_record is not None:
                plan.add_record(fb_record)
            plan.add_tpf_step(n, bits, loc.bufs, loc.psum,
                              nxt.bufs if nxt is not None else None,
                              nxt.w_ent if nxt is not None else None, *common, self.hist,
                              self.metrics, self.step_dev)
            if len(self._plans) >= 32:  # (callers passing fresh label tensors every step)
                self._plans.clear()
            self._plans[key] = plan
        return plan, nxt

    def prep_plan(self, buf: int, keys: torch.Tensor, labels: torch.Tensor, *, seed: int,
                  row0: int, row_step: int, num_features: int, alpha: float = 1.1, gate=None,
                  bucket_after=None, bucket_done=None):
        """Flat mode: a native launch list that generates the next synthetic minibatch of
        workspace ``buf`` (rows row0, row0 + row_step, ... on successive runs) and
        localises it (tile + flat bucket kernels): ONE host call per data preparation.
        ``gate``: an event the localisation waits for after the generator (bench.py: the
        training step's fused forward/backward, so the two LDS-heavy 1024-thread kernels
        do not share the CUs). ``bucket_after`` / ``bucket_done`` (tail filter): the
        filter kernel (CountMin insert + query + compaction, after the bucket kernel)
        waits for the previous minibatch's filter kernel and records its own, so sketch
        updates run in minibatch order while the generators, tile and bucket kernels of
        several preparations still overlap. Returns a callable -> the FlatLoc of
        ``buf``."""
        from ..ops.synthetic import CRITEO_1TB_CARDS, _set_cards

        if self.localize_mode != "tpf":
            raise ValueError("prep_plan needs the flat (tpf) localisation")
        while len(self._localizers) <= buf:
            self._localizers.append(self._new_localizer(self.localize_mode))
        lz = self._localizers[buf]
        f = lz.flat
        B = labels.numel()
        n = keys.numel()
        _set_cards(self.device, CRITEO_1TB_CARDS)
        H = hipops()
        plan = H.LaunchList()
        plan.add_criteo_gen(seed & ((1 << 64) - 1), row0, row_step, B, num_features, alpha, keys,
                            labels)
        if gate is not None:
            plan.add_wait(gate)
        if bucket_after is None and bucket_done is None:
            plan.add_localize_tpf(keys, n, self.bits, lz.ptemp, f.dcnt, f.rep, f.uniqf,
                                  f.ent_pos, f.ent_j, f.cnt, f.err, self._flat_x,
                                  filt=lz.filt_args())
        else:
            for stage in ((1, 2, 3) if lz.filt_args() is not None else (1, 2)):
                if stage == 3 and bucket_after is not None:
                    plan.add_wait(bucket_after)
                plan.add_localize_tpf(keys, n, self.bits, lz.ptemp, f.dcnt, f.rep, f.uniqf,
                                      f.ent_pos, f.ent_j, f.cnt, f.err, self._flat_x,
                                      filt=lz.filt_args(), stage=stage)
            if bucket_done is not None:
                plan.add_record(bucket_done)

        def run():
            plan.run()
            return done()

        def done():  # (host bookkeeping: also after the list ran inside another one)
            f.nnz = n
            f.gen += 1
            return f
        run.plan, run.done = plan, done
        return run

    def _step_plan(self, loc, labels, B: int, width: int):
        """The 1-GPU fused step (kv_resolve, tp_fwd_bwd, tp_seg_update: the same launches
        ``step`` issues one by one below) as a native ``LaunchList`` over the fixed
        workspaces of one localisation buffer and one label buffer: arguments are
        validated once, and a step is one host call (profiles/r3_s3_host_issue.log).
        None when the fused tp path does not apply to this minibatch."""
        t = loc.tile
        if t is None:
            return None
        # (object ids: a cached plan holds its tensors, so no other tensor takes their id)
        key = (id(t.rep), id(loc.uniq), id(labels), B, width, loc.nnz, id(self.rule),
               id(self.table.init))
        plan = self._plans.get(key)
        if plan is None:
            if not fused_update_ok(loc, self.w_buf, B=B, width=width):
                return None
            H, tb = hipops(), self.table
            plan = H.LaunchList()
            plan.add_kv_resolve(tb.slots, loc.uniq, loc.n_uniq, self.slot_buf, self.w_buf, True,
                                *tb.resolve_args())
            coef = self.coef[:B]
            plan.add_tp_fwd_bwd(t.rep, t.dcnt, t.ent_uid, loc.nnz, width, None, self.w_buf, labels,
                                B, loss_id(self.cfg.loss), coef, self.metrics, self.hist,
                                AUC_BINS, t.psum, loc.pos_s, loc.segid, t.n_ent, loc.grad, False)
            plan.add_tp_seg_update(loc.pos_s, loc.segid, loc.nnz, t.n_ent, t.psum, loc.seg_start,
                                   loc.n_uniq, t.pieces, self.slot_buf, tb.slots,
                                   *self.rule.args(), self.stats, self.hist, self.metrics,
                                   self.step_dev)
            if len(self._plans) >= 16:  # (callers passing fresh label tensors every step)
                self._plans.clear()
            self._plans[key] = plan
        return plan

    # ------------------------------------------- shared by the multi-GPU data planes
    def consistency_desc(self) -> str:
        """The consistency the data plane actually enforces (reported by bench.py)."""
        if self.G == 1:
            return "bsp (1 shard: every pull sees every earlier push)"
        if self.p2p:
            return (f"asp-p2p (one-sided pulls from the owners' HBM and inbox pushes, no "
                    f"collective per step; owners apply at their own pace, a pusher waits "
                    f"only {self.cfg.p2p_queue} steps ahead of an owner)")
        if self.merged:
            ms = self.msched
            base = "asp (bounded here: " if ms.asp else f"ssp:{int(self.tau)} ("
            return (f"{base}pull of step t sees exactly the pushes of steps <= t-1-{ms.lag}; "
                    f"one all-to-all per step carrying keys(t+1), pushes(t-{ms.d}) and the "
                    f"weights of keys(t), owner apply {'after' if ms.post else 'before'} "
                    f"its resolve)")
        if not self.padded or self.lag == 0 and not self.asp:
            return "bsp (pull of step t sees every push of steps <= t-1)"
        if self.asp:
            return (f"asp (pushes applied asynchronously to pulls; pull of step t misses "
                    f">= {self.lag} and, bounded only by the {self.R}-entry ring, "
                    f"<= {self.lag + self.async_depth} steps of pushes)")
        return (f"ssp:{int(self.tau)} (pull of step t sees exactly the pushes of steps "
                f"<= t-1-{self.lag})")

    def _agree_capacity(self, count) -> int:
        """Keys per peer row, the same on every rank: configured, or (collective) slack x
        the largest per-peer count over all ranks + 1024 (``count()``: this rank's
        largest); a multiple of 64, at most a whole minibatch."""
        C = int(self.cfg.exchange_capacity)
        if C <= 0:
            cnt = self.comm.all_reduce_(self._to_comm(count().to(torch.float64).reshape(1)),
                                        op="max")
            C = int(math.ceil(float(cnt.item()) * self.cfg.exchange_slack)) + 1024
        return min(max(64, (C + 63) // 64 * 64), max(64, self.max_nnz))

    def _row_geometry(self, C: int, merged: bool = False):
        """(kw, nb, w0, H) of an exchange row [4 header words | C keys of kw words |
        gradients: C floats, or C FixingFloat codes of nb bytes | merged: C weights from
        word w0], H words long (a multiple of 4).

        merged exchange: each row also carries the owner's weights answering the keys the
        row's receiver sent in the previous exchange. The owner resolves and applies in
        two launches: one launch of both halves measured the SUM of their kernel times,
        56.4 vs 22.3 + 34.4 us at 8 emulated peers, and it puts the apply on the path to
        the next collective: 0.175 vs 0.155 ms / step, profiles/r5_owner_fused.log"""
        kw = 1 if self.bits <= 32 else 2
        nb = int(self.cfg.fixing_float_bytes)  # FixingFloat: nb-byte codes instead of f32
        w0 = 4 + C * kw + ((C * nb + 3) // 4 if nb else C)
        return kw, nb, w0, (w0 + (C if merged else 0) + 3) // 4 * 4

    def _to_comm(self, t: torch.Tensor) -> torch.Tensor:
        """A tensor where the communicator reduces it (RCCL: device, gloo: host)."""
        return t.to(self.comm.device) if self.comm.backend == "nccl" else t.cpu()

    def _overflow_error(self, what: str, count, C: int) -> RuntimeError:
        return RuntimeError(
            f"{what} overflow at step {self.step_count}: {count} keys exceeded the per-peer "
            f"capacity {C} (pulled as 0, pushes dropped); set exchange_capacity or "
            f"exchange_slack higher, or exchange='exact'")

    def flush(self):
        """Apply the deferred pushes of the last step (fused / padded multi-GPU modes).
        Collective."""
        if self.p2p:
            if self.px is not None:
                xc = self.xc
                self.px.drain(self.rule, self.stats, xc.a_slot, xc.a_w, xc.link, xc.nxt)
            return
        if self.merged:
            if self._mx_external:
                return  # a caller's pipeline owns the in-flight exchanges (mx_drain)
            if self._mx_pend is not None:  # the last minibatch: exchange without keys
                self._mx_run_exchange(self._xt, None)
                self._mx_finish_pending()
            self.mx_drain()
            self._x_check_overflow()
            return
        if self.padded:
            if self.xc is not None:
                self._x_flush()
            return
        if not self.fused or self.pending is None:
            return
        self._fused_flush()

    # ------------------------------------------------------------ reporting
    def check_ok(self, collective: bool | None = None):
        """Host sync: raise if any device-side capacity was exceeded since the start --
        the table (full: a key could not be inserted), a localisation workspace (a tile
        or bucket overflowed its LDS hash or its fixed entry region: the step kernels
        would have dropped those occurrences' gradients and read stale weights) or the
        padded exchange rows. All error words are sticky, so a check at any later point
        still sees an overflow. Called by ``progress()`` and by bench.py after timing
        (same fail-loudly rule as the exchange overflow, ``_x_poll_overflow``).

        With G > 1 (``collective`` default) the three error classes are max-all-reduced
        first, so every rank raises together: a rank-local raise would leave its peers
        blocked in their next collective until the communicator timeout."""
        if not self.gpu:
            return
        lzs = [lz for lz in list(self._localizers) + list(self._compact or [])
               + list(self._mx_own.values())
               if getattr(lz, "err", None) is not None]
        words = [self.table._err] + [lz.err for lz in lzs]
        if self.xc is not None:
            words.append(self.xc.ovf)
        v = torch.cat([w.reshape(-1)[:1].to(torch.int64) for w in words])
        nl = len(lzs)
        # [table full, OR-ish (max) of the localisation error bits, exchange overflow]
        summary = torch.stack([v[0], v[1:1 + nl].max() if nl else v[0] * 0,
                               v[-1] if len(words) > 1 + nl else v[0] * 0])
        if collective is None:
            collective = self.G > 1
        if collective:
            summary = self.comm.all_reduce_(self._to_comm(summary), op="max")
        tab, loc_e, ovf = summary.cpu().tolist()
        local = v.cpu().tolist()
        if tab:
            raise RuntimeError("KVTable full: increase table_capacity (keys were not inserted)")
        if loc_e:
            bad = [lz.mode for lz, e in zip(lzs, local[1:1 + nl]) if e]
            mode = bad[0] if bad else "tpf/tp (on a peer rank)"
            raise RuntimeError(
                f"localize_{mode} overflow (error bits {loc_e:#x}): a tile or bucket "
                f"exceeded its LDS hash / entry region, so some occurrences were dropped "
                f"from the step; the minibatch is too skewed for the {mode} layout "
                f"(PSAMD_FLAT=0 or localize='sort')")
        if ovf:
            raise self._overflow_error("exchange", ovf, self.xc.C)

    def progress(self, reset: bool = True) -> dict:
        """Merged progress across ranks (reference ISGDScheduler::showProgress, sgd.h:45-80).
        Collective when G > 1 (also applies deferred pushes). Raises on a device-side
        overflow (``check_ok``) instead of reporting a silently corrupted run."""
        self.flush()
        self.check_ok()
        m = torch.cat([accum_total(self.metrics)[:8], accum_total(self.stats)[:3]])
        if self.G > 1:
            m = self.comm.all_reduce_(self._to_comm(m))
        m = m.cpu()
        n = max(float(m[2]), 1.0)
        out = {
            "examples": float(m[2]),
            "loss": float(m[0]) / n,
            # reference Evaluation::accuracy folds to max(acc, 1-acc) (evaluation.h:61)
            "accuracy": max(float(m[1]) / n, 1.0 - float(m[1]) / n) if m[2] > 0 else 0.0,
            "auc": float(m[3]) / max(float(m[4]), 1.0),
            "nnz_w": float(m[8]),
            "updt_ratio": math.sqrt(float(m[10])) / math.sqrt(max(float(m[9]), 1e-20)),
        }
        out["table_capacity"] = self.table.capacity
        out["table_grown"] = self._growth.grown if self._growth is not None else 0
        if reset:
            self.metrics.zero_()
            self.stats.view(-1, 16)[:, 1:].zero_()  # keep the cumulative nnz column
        return out

    # ------------------------------------------------------------ checkpoint
    def save_model(self, prefix: str, node_id: str | None = None, text_io: str = "auto") -> str:
        """Reference checkpoint layout: ``<prefix>_<NodeID>`` with one ``key\\tweight``
        line per non-zero weight (src/parameter/kv_store.h:63-73). ``text_io``: "device"
        formats the text on the GPU (ops/modeltext.py; the same bytes), "host" is
        ``utils/checkpoint.write_text_model``, "auto" the device path when the table is on a
        GPU. ``last_save`` holds the entry count and the chunks the device formatter left
        to the host."""
        from ..ops.modeltext import write_text_model_device
        from ..utils.checkpoint import write_text_model

        if text_io not in ("auto", "host", "device"):
            raise ValueError(f"save_model: text_io must be auto, host or device, not {text_io!r}")
        if text_io == "device" and not self.table.gpu:
            raise ValueError("save_model: text_io='device' needs the table on a GPU")
        self.flush()

        keys, w = self.table.occupied_weights()
        raw = unmix(keys, self.bits)
        path = f"{prefix}_{node_id or f'S{self.rank}'}"
        if text_io != "host" and self.table.gpu:
            entries, deferred = write_text_model_device(path, raw, w)
        else:
            entries, deferred = write_text_model(path, raw.cpu(), w.cpu()), 0
        self.last_save = {"path": path, "entries": entries, "deferred_chunks": deferred}
        return path

    def state_dict(self) -> dict:
        self.flush()
        keys, w, z, n = self.table.occupied()
        return {"keys": unmix(keys, self.bits).cpu(), "w": w.cpu(), "z": z.cpu(), "n": n.cpu(),
                "step": self.step_count, "bits": self.bits, "rank": self.rank, "world": self.G}

    def load_state_dict(self, sd: dict):
        from ..ops.keymix import mix

        keys = mix(sd["keys"].to(self.device), self.bits)
        own = self.part.owner_of(keys) == self.rank
        # growth on: room for this rank's keys first (collective when G > 1)
        self._growth_load(own)
        self._table_changed()  # the table changes under any pull issued ahead
        self.table.load(keys[own], sd["w"].to(self.device)[own], sd["z"].to(self.device)[own],
                        sd["n"].to(self.device)[own])
        self.step_count = int(sd.get("step", 0))

    def load_model(self, pattern: str, text_io: str = "auto", n0: float = 0.0,
                   chunk_bytes: int = 32 << 20) -> dict:
        """Warm start: continue training from stored ``key\\tweight`` model files (what
        ``save_model``, the reference and Darlin write: weights only). ``pattern``,
        ``text_io`` and the fallback rules are ``ModelScorer.from_text``'s: a regex or glob
        of ``<prefix>_<NodeID>`` files; "auto" parses the text on the GPU when the table is
        on one, "host" is the dict reader, "device" on a CPU table raises. Collective when
        G > 1: every rank reads every file and keeps the keys it owns, so a model saved by
        any number of ranks loads into any world size.

        Every kept weight is seeded with the optimizer state that reproduces it
        (``KVTable.seed``): FTRL gets the ``z`` whose proximal step gives back ``w``, so the
        first update continues from the stored weight instead of forgetting it. ``n0 >= 0``
        is the prior gradient norm of every key (0: fresh per-key learning rates).

        Streaming: each chunk of at most ``chunk_bytes`` goes file -> pinned -> HBM ->
        ``modeltext_parse`` -> ``kv_seed`` on one stream, the next chunk's file read under
        the current chunk's kernels; the model is never held whole. A chunk the device parser
        declines is parsed by the host rules and seeded all the same (``deferred_chunks``).
        A key that repeats (the kernel's ``overwritten`` count) or a line longer than a
        chunk restarts the load through the dict reader, where the later line wins
        (``deferred_chunks`` >= 1). With ``table_growth`` the table makes room before each
        chunk; without it a table that fills raises 'KVTable full'.

        Defined on a fresh trainer only (no step taken, empty table): ``ValueError``
        otherwise, and when a key lies outside [0, 2^bits) (the model was stored with another
        ``num_features``). The tail filter's CountMin sketch is not part of a text model
        and starts empty: with ``tail_feature_freq`` on, a seeded key is filtered from the
        minibatches until the sketch has seen it more than that many times; its stored
        weight is kept meanwhile. Returns (and leaves in ``last_load``) {"entries",
        "seeded", "foreign", "deferred_chunks", "table_capacity"}: ``entries`` the pairs
        read, ``seeded`` / ``foreign`` those this rank kept / left to the other ranks."""
        from ..ops.modeltext import (MAX_CHUNK_BYTES, _LineTooLong, iter_text_model_chunks,
                                     read_pairs_host)

        if text_io not in ("auto", "host", "device"):
            raise ValueError(f"load_model: text_io must be auto, host or device, not {text_io!r}")
        if text_io == "device" and not self.table.gpu:
            raise ValueError("load_model: text_io='device' needs the table on a GPU")
        chunk_bytes = int(chunk_bytes)
        if not 64 <= chunk_bytes <= MAX_CHUNK_BYTES:
            raise ValueError("load_model: chunk_bytes must be in [64, 2^30]")
        if n0 < 0:
            raise ValueError("load_model: n0 must be >= 0")
        if self.step_count != 0 or self.table.census()[0] != 0:
            raise ValueError("load_model needs a fresh trainer: no step taken and an empty table")
        self.flush()
        self._table_changed()  # the table changes under any pull issued ahead
        tb, g = self.table, self._growth
        lo, hi = tb.key_range or self.part.range_of(self.rank)
        counts = tb.new_seed_counts()
        entries = deferred = 0

        def seed(raw, w):
            nonlocal entries
            entries += raw.numel()
            self._growth_room(raw.numel(), exact=False)  # (collective when G > 1)
            tb.seed(raw, w, self.bits, lo, hi, self.rule, n0, stats=self.stats, counts=counts)

        def seed_host():
            """The whole model by the dict reader (the later line of a repeated key wins:
            reported as at least one deferred chunk)."""
            nonlocal deferred
            raw, w, repeated = read_pairs_host(pattern)
            deferred = max(int(repeated), deferred)
            seed(raw, w)

        def restart():
            """Everything seeded so far dropped; the whole model by the dict reader."""
            nonlocal entries, deferred
            tb.clear()
            counts.zero_()
            self.stats.view(-1, 16)[:, 0].zero_()  # the cumulative nnz column
            if g is not None:
                g.bound = 0
            entries, deferred = 0, max(1, deferred)
            seed_host()

        if text_io != "host" and tb.gpu:
            try:
                for raw, w, was_deferred in iter_text_model_chunks(pattern, self.device,
                                                                   chunk_bytes):
                    deferred += was_deferred
                    seed(raw, w)
            except _LineTooLong:
                restart()
        else:
            seed_host()
        c = tb.seed_counts(counts)
        repeats = c["overwritten"]
        if self.G > 1 and not self._loopback:  # (a repeat on any rank: all restart together)
            repeats = int(self.comm.all_reduce_(self._to_comm(
                torch.tensor([float(repeats)], dtype=torch.float64)), op="max").item())
        if repeats and not c["out_of_range"]:
            restart()
            c = tb.seed_counts(counts)
        if c["out_of_range"]:
            raise ValueError(
                f"load_model: {c['out_of_range']} keys of {pattern!r} lie outside [0, 2^{self.bits}): "
                f"the model was stored with another num_features")
        if tb.gpu:
            self.check_ok()  # (a table that filled: 'KVTable full', on every rank together)
        self.last_load = {"entries": entries, "seeded": c["seeded"], "foreign": c["foreign"],
                          "deferred_chunks": deferred, "table_capacity": tb.capacity}
        return dict(self.last_load)

    # ------------------------------------------------------------ scoring
    def scorer(self):
        """A ``ModelScorer`` (models/scorer.py) over the current weights, after ``flush()``.
        Collective when G > 1.

        One rank: the trainer's own table, aliased (zero copy, ordered homes honoured); it
        sees later steps too, after their ``flush()``. G > 1: a REPLICA of the whole model
        on every rank, as scoring probes every key locally -- each rank takes the non-zero
        (mixed key, w) of its shard, the ranks all-gather them (counts, then rows padded to
        the largest shard) and each loads the union into a scratch hashed-home table at
        load <= 0.5. That costs 32 B per slot, i.e. 64-128 B per non-zero weight of the
        WHOLE model on every rank; ``KVTable.check_ok`` raises if it does not fit."""
        from .scorer import ModelScorer

        self.flush()
        if self.G == 1 or self._loopback:
            return ModelScorer.from_table(self.table, self.bits, self.cfg.loss)
        keys, w, _, _ = self.table.occupied()
        nz = w != 0
        keys, w = keys[nz].contiguous(), w[nz].contiguous()
        counts = self.comm.all_gather_counts(
            torch.tensor([keys.numel()], dtype=torch.int64)).reshape(-1).tolist()
        C = max(1, max(counts))
        dev = keys.device
        pk = torch.zeros(C, dtype=torch.int64, device=dev)
        pw = torch.zeros(C, dtype=torch.float32, device=dev)
        pk[:keys.numel()] = keys
        pw[:w.numel()] = w
        ak = torch.empty(self.G * C, dtype=torch.int64, device=dev)
        aw = torch.empty(self.G * C, dtype=torch.float32, device=dev)
        self.comm.all_gather_into_async(ak, pk).wait()
        self.comm.all_gather_into_async(aw, pw).wait()
        sel = torch.cat([torch.arange(r * C, r * C + n, device=dev)
                         for r, n in enumerate(counts)])
        return ModelScorer.from_pairs(ak[sel], aw[sel], self.bits, self.device,
                                      loss=self.cfg.loss)

    def evaluate(self, feeder, comm=None) -> dict:
        """Score one pass of a ``DeviceFeeder`` with the current weights; the result dict
        of ``ModelScorer.result`` (over all ranks of ``comm`` when given)."""
        return self.scorer().evaluate(feeder).result(comm)

    def predict(self, keys: torch.Tensor, *, row_ptr=None, width=None, vals=None):
        """Margins of raw-key rows under the current weights (``ModelScorer.predict``)."""
        return self.scorer().predict(keys, row_ptr=row_ptr, width=width, vals=vals)
