"""Field-weighted factorization machine (FwFM, Pan et al., WWW 2018) on the sharded embedding
table: the FM's table (one vector of D bf16 per key) plus one small dense parameter, a
symmetric ``R`` [F, F] of field-pair strengths. Rows have ``slots`` positions; ``fields`` maps
position -> field in [0, F), one map for all rows, as ``FFMConfig.fields``:

    m        = sum_i x_i w_i + sum_{i<j} x_i x_j R[f_i][f_j] <v_i, v_j>
    P[f]     = sum_{i: f_i = f} x_i v_i,   T = R P,   q_f = sum_{i: f_i = f} x_i^2 |v_i|^2
    m        = lin + 1/2 (sum_f <P[f], T[f]> - sum_f R[f][f] q_f)
    dX0[i]   = c x_i (T[f_i] - R[f_i][f_i] x_i v_i),   c = -y sigma(-y m)
    dR[f,g]  = sum_b c <P[f], P[g]> (f != g),   dR[f,f] = 1/2 sum_b c (|P[f]|^2 - q_f)

With ``R = 1`` (``r_init``, the default) the model is the FM; same-field pairs count, weighted
by the diagonal of R. ``R`` is replicated on every rank and read as symmetric from its upper
triangle. The step is the FFM's fixed-width step with ``fwfm_fwd_bwd`` (fwfm.hip: one wavefront
per example, both matrix products on the fp32 matrix instructions) in the middle, then the
fixed-order reduction of the dR partials and the AdaGrad step of R (``fwfm_dr_reduce``; G > 1:
sum, all-reduce, update).

``step(..., row_ptr=, fields=)`` / ``predict(..., row_ptr=, fields=)`` take CSR minibatches with
a field id per occurrence (libffm's ``field:index:value`` rows; the device text parsers' CSR
arrays): rows of any width, fields missing, repeated, in any order. ``fields`` [nnz] int32 then
replaces the position -> field map (``cfg.fields`` is not consulted, ``cfg.slots`` only sizes
``max_nnz = minibatch * slots``); a field outside [0, F) keeps the occurrence's linear term and
takes it out of every pair. A field may repeat in one row and not in the next, so the diagonal
of R is kept out of ``T`` and acts per row, where the field occurs n_f >= 2 times:

    T0       = R0 P  (R0: R with a zero diagonal),   s_f = n_f >= 2 ? 1/2 (|P[f]|^2 - q_f) : 0
    m        = lin + 1/2 sum_f <P[f], T0[f]> + sum_f R[f][f] s_f
    dX0[p]   = c x_p (T0[f_p] + (n_{f_p} >= 2 ? R[f_p][f_p] (P[f_p] - x_p v_p) : 0))
    dR[f,g]  = sum_b c <P[f], P[g]> (f != g),   dR[f,f] = sum_b c s_f

which on rows of one width and one map is the model above. The step is ``FFMTrainer``'s CSR
sequence with ``fwfm_csr`` (fwfm_csr.hip: one kernel for every width, a row walked in rounds
of 64 occurrences) in the middle and the same reduce + update of R after it.

``scorer()`` gives an ``FwFMScorer`` (models/scorer.py) on the trainer's own shard and live R:
margins, loss / accuracy sums and the AUC histogram of held-out rows in one launch per
minibatch (fwfm_predict.hip); ``FwFMScorer.from_state_dict`` scores a snapshot of any world
size.

Not here yet: the app's ``.conf`` route.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, field

import torch

from ..ops import embedding as E
from ..ops.keymix import key_bits_for
from ..ops.kv_table import UpdateRule, next_pow2
from ..ops.linear import AUC_BINS, auc_from_hist, linear_backward, new_accum
from ..ops.localize import Localizer
from ..ops.native import hipops
from ..ops.score import fwfm_forward, fwfm_forward_csr
from ..parallel.comm import Comm, LocalComm
from ..parallel.partition import KeyPartition
from .ffm import FFMTrainer
from .fm import FMTrainer
from .wide_deep import EmbeddingPS

MAX_PARTS = 512  # blocks of the training launch = partials of dR (two per CU)


@dataclass
class FwFMConfig:
    num_features: int = 10 ** 8
    embedding_dim: int = 16              # D: 8, 16 or 32
    fields: list | None = None           # position -> field; None: identity over slots
    num_fields: int = 0                  # F; 0: max(fields) + 1
    slots: int = 39                      # positions per example (<= 64)
    minibatch: int = 10000
    emb_lr: float = 0.02
    emb_init_scale: float = 0.01
    lambda_v: float = 10.0               # L2 on the factors (once per unique key and step)
    r_lr: float = 0.02                   # AdaGrad on R
    r_init: float = 1.0                  # R = r_init everywhere: 1.0 starts as the FM
    lambda_r: float = 0.0                # L2 on R
    wide: UpdateRule = field(default_factory=lambda: UpdateRule("adagrad", "constant", 0.05,
                                                                 1e-6, 0.0, 1.0))
    table_capacity: int = 0
    table_load: float = 0.5
    max_table_bytes: int = 96 << 30
    exchange: str = "padded"             # G > 1 on GPU: sync-free fixed rows | "exact"
    exchange_slack: float = 1.5
    exchange_capacity: int = 0
    compact_rows: bool = True            # 1 GPU: gather each unique key's row once per step
    localize: str = "sort"
    seed: int = 0

    def geometry(self):
        """(fields, F), checked: everything the kernel's launcher would refuse."""
        S, D = self.slots, self.embedding_dim
        if not 1 <= S <= 64:
            raise ValueError(f"slots must be in 1..64, not {S}")
        if D not in (8, 16, 32):
            raise ValueError(f"embedding_dim must be 8, 16 or 32, not {D}")
        fields = list(range(S)) if self.fields is None else [int(f) for f in self.fields]
        if len(fields) != S:
            raise ValueError(f"fields has {len(fields)} entries for {S} slots")
        F = self.num_fields or max(fields) + 1
        if min(fields) < 0 or max(fields) >= F or F > 64:
            raise ValueError(f"every field must lie in [0, {F}), F <= 64")
        return fields, F


class FwFMTrainer(EmbeddingPS):
    _dense_state = ("R", "R_acc")

    def __init__(self, cfg: FwFMConfig, comm: Comm | None = None, device="cpu"):
        self.cfg = cfg
        self.fields, self.F = cfg.geometry()
        self.comm = comm or LocalComm(device)
        self.G, self.rank = self.comm.world, self.comm.rank
        self.device = dev = torch.device(device)
        self.gpu = dev.type == "cuda"
        self.bits = key_bits_for(cfg.num_features)
        self.part = KeyPartition(self.bits, self.G)
        D, S, B, F = cfg.embedding_dim, cfg.slots, cfg.minibatch, self.F
        per_slot = 32 + 2 * D + 5
        cap = cfg.table_capacity or next_pow2(int(math.ceil(cfg.num_features / self.G /
                                                            cfg.table_load)))
        cap = max(1024, min(cap, 1 << max(10, (cfg.max_table_bytes // per_slot).bit_length() - 1)))
        self.shard = E.EmbeddingShard(cap, D, dev, init_scale=cfg.emb_init_scale,
                                      seed=cfg.seed * 7919 + 17)
        self.max_nnz = B * S
        self.localizer = Localizer(self.max_nnz, self.bits, dev, mode=cfg.localize)
        self.coef = torch.empty(B, dtype=torch.float32, device=dev)
        self.metrics = new_accum(dev)
        self.stats = new_accum(dev)
        self.hist = torch.zeros(2 * AUC_BINS, dtype=torch.int32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._fields_t = torch.tensor(self.fields, dtype=torch.long, device=dev)
        self.R = torch.full((F, F), float(cfg.r_init), dtype=torch.float32, device=dev)
        self.R_acc = torch.zeros(F, F, dtype=torch.float32, device=dev)
        self.dR = torch.zeros(F, F, dtype=torch.float32, device=dev)
        if self.gpu:
            self.slot_buf = torch.empty(self.max_nnz, dtype=torch.int64, device=dev)
            self.w_buf = torch.empty(self.max_nnz, dtype=torch.float32, device=dev)
            self.dX0 = torch.empty(self.max_nnz, D, dtype=torch.bfloat16, device=dev)
            self.dE = torch.empty(self.max_nnz, D, dtype=torch.float32, device=dev)
            self.rows_u = torch.empty(self.max_nnz, D, dtype=torch.bfloat16, device=dev)
            Fp = (F + 15) // 16 * 16
            self.dR_part = torch.empty(min(MAX_PARTS, (B + 7) // 8), Fp * Fp,
                                       dtype=torch.float32, device=dev)
            self.row_of = None  # [max_nnz] int32, on the first CSR step
        self.step_count = 0
        self.examples = 0
        self.t0 = time.time()

    # ------------------------------------------------------------------ step
    def step(self, keys: torch.Tensor, labels: torch.Tensor, vals: torch.Tensor | None = None,
             loc=None, row_ptr: torch.Tensor | None = None, fields: torch.Tensor | None = None):
        """One minibatch: ``keys`` [B*S] raw feature ids (row-major, S per example),
        ``labels`` [B] in {-1, +1} (or {0, 1}), optional feature values ``vals`` [B*S]. With
        ``row_ptr`` [B + 1] (int64) and ``fields`` [nnz] (int32, on the trainer's device) the
        rows have any width and every occurrence names its own field (``cfg.fields`` is not
        used): row b holds keys[row_ptr[b]:row_ptr[b + 1]].
        Nothing here reads device data on the host."""
        if row_ptr is not None or fields is not None:
            return self._step_csr(keys, labels, vals, loc, row_ptr, fields)
        cfg = self.cfg
        S, D = cfg.slots, cfg.embedding_dim
        B = labels.numel()
        nnz = B * S
        if keys.numel() != nnz:
            raise ValueError(f"expected {nnz} keys, got {keys.numel()}")
        if B > self.coef.numel():
            raise ValueError(f"{B} rows in a minibatch, cfg.minibatch is {self.coef.numel()}")
        if vals is not None and vals.numel() != nnz:
            raise ValueError(f"expected {nnz} values, got {vals.numel()}")
        loc = self.localizer(keys) if loc is None else loc
        if self.G == 1:
            if self.gpu:
                slot, w_wide = self.shard.resolve(loc.uniq, loc.n_uniq, self.slot_buf, self.w_buf)
            else:
                slot, w_wide = self.shard.resolve(loc.uniq[:loc.num_unique()])
            rows_src, rows_idx = self.shard.rows, slot
            if self.gpu and cfg.compact_rows:
                hipops().emb_gather_rows(slot, self.shard.rows, self.rows_u, loc.n_uniq)
                rows_src, rows_idx = self.rows_u, None
            push = ("local", slot)
        else:
            rows_u, w_wide, push = self._pull(loc)
            rows_src, rows_idx = rows_u, None
        if self.gpu:
            dX0 = self.dX0[:nnz]
            hipops().fwfm_fwd_bwd(rows_src, rows_idx, vals, B, S, self.fields, self.F, self.R,
                                  loc.local_col, w_wide, labels, self.coef, dX0, self.dR_part,
                                  self.metrics, self.hist, AUC_BINS)
            dE = E.grad_reduce(loc, dX0, D, nnz, out=self.dE)
            l2_cap = nnz if rows_idx is not None else min(nnz, rows_src.shape[0])
            hipops().fm_l2(dE, rows_src, rows_idx, loc.n_uniq, l2_cap, cfg.lambda_v)
        else:
            X0 = E.expand(loc.local_col, nnz, rows_src, idx=rows_idx)
            dX0, dR = self._fwd_bwd_torch(X0, vals, B, S, loc.local_col, w_wide, labels)
            self.dR.copy_(dR)
            U = loc.num_unique()
            dE = E.grad_reduce(loc, dX0, D, U)
            v = (rows_src[rows_idx[:U]] if rows_idx is not None else rows_src[:U]).float()
            dE += cfg.lambda_v * v
        g_wide, _ = linear_backward(loc, self.coef[:B], B=B, width=S, vals=vals)
        self._push(loc, push, dE, g_wide)
        self._update_r()
        auc_from_hist(self.hist, self.metrics, self.step_dev)
        self.step_count += 1
        self.examples += B

    def _update_r(self):
        """dR of all ranks, then AdaGrad on the replicated R: g = dR + lambda_r R,
        acc += g^2, R -= r_lr g / (sqrt(acc) + 1e-8)."""
        cfg = self.cfg
        if self.gpu:
            one = self.G == 1
            hipops().fwfm_dr_reduce(self.dR_part, self.dR, self.F, True, one, self.R, self.R_acc,
                                    cfg.r_lr, cfg.lambda_r)
            if not one:
                self.comm.all_reduce_(self.dR)
                hipops().fwfm_dr_reduce(None, self.dR, self.F, False, True, self.R, self.R_acc,
                                        cfg.r_lr, cfg.lambda_r)
            return
        if self.G > 1:
            self.comm.all_reduce_(self.dR)
        g = self.dR + cfg.lambda_r * self.R
        self.R_acc += g * g
        self.R -= cfg.r_lr * g / (self.R_acc.sqrt() + 1e-8)

    def _forward_math(self, X0, vals, B, S, local_col, w_wide, dtype, R=None):
        """(margin [B], x [B, S], x v [B, S, D], P [B, F, D], q [B, F], T [B, F, D], diag R
        [F]) in ``dtype``; R is read as symmetric from its upper triangle."""
        return fwfm_forward(X0, vals, B, S, self._fields_t, self.F, self.R if R is None else R,
                            local_col, w_wide, dtype)

    def _fwd_bwd_math(self, X0, vals, B, S, local_col, w_wide, labels, dtype=torch.float32,
                      R=None):
        """(margin [B], coef [B], dX0 [B*S, D], dR [F, F] symmetric) in ``dtype``, nothing
        rounded to bf16."""
        m, x, xv, P, q, T, rd = self._forward_math(X0, vals, B, S, local_col, w_wide, dtype, R)
        y = torch.where(labels[:B] > 0, 1.0, -1.0).to(dtype)
        c = -y * torch.sigmoid(-y * m)
        f = self._fields_t.to(X0.device)
        dX = (c[:, None] * x)[..., None] * (T[:, f, :] - rd[f][None, :, None] * xv)
        dR = torch.einsum("b,bfd,bgd->fg", c, P, P)
        # a field of fewer than two positions has no same-field pair: |P[f]|^2 = q_f, and
        # the diagonal entry is 0 by construction, not by cancellation
        pairs = torch.bincount(f, minlength=self.F) >= 2
        diag = torch.where(pairs, 0.5 * (torch.diagonal(dR) - c @ q), torch.zeros((), dtype=dtype))
        up = torch.triu(dR, 1)
        return m, c, dX.reshape(B * S, -1), up + up.T + torch.diag(diag)

    def _fwd_bwd_torch(self, X0, vals, B, S, local_col, w_wide, labels, dtype=torch.float32):
        """fwfm_fwd_bwd in PyTorch: the CPU route, and in ``dtype=torch.float64`` the
        reference the kernel is tested against. Returns (dX0 bf16, dR in ``dtype``)."""
        m, c, dX, dR = self._fwd_bwd_math(X0, vals, B, S, local_col, w_wide, labels, dtype)
        return self._account(m, c, dX, labels, B), dR

    _account = FFMTrainer._account

    # ------------------------------------------------------------------ CSR rows
    _check_csr = FFMTrainer._check_csr

    def _step_csr(self, keys, labels, vals, loc, row_ptr, fields):
        """step() on CSR rows with a field per occurrence: ``FFMTrainer._step_csr``'s sequence
        with ``fwfm_csr`` (fwfm_csr.hip) as its forward / backward, which also writes the row
        id of every occurrence for the wide gradient, then the reduce + update of R.
        ``cfg.slots`` sizes ``max_nnz`` and is no limit on a row's width. Nothing here reads
        device data on the host."""
        cfg = self.cfg
        D = cfg.embedding_dim
        B, nnz = labels.numel(), keys.numel()
        self._check_csr(nnz, B, row_ptr, fields, vals)
        if nnz > self.max_nnz:
            raise ValueError(f"{nnz} keys in a minibatch, max_nnz is {self.max_nnz}")
        if B > self.coef.numel():
            raise ValueError(f"{B} rows in a minibatch, cfg.minibatch is {self.coef.numel()}")
        loc = self.localizer(keys) if loc is None else loc
        if self.G == 1:
            if self.gpu:
                slot, w_wide = self.shard.resolve(loc.uniq, loc.n_uniq, self.slot_buf, self.w_buf)
            else:
                slot, w_wide = self.shard.resolve(loc.uniq[:loc.num_unique()])
            rows_src, rows_idx = self.shard.rows, slot
            if self.gpu and cfg.compact_rows:
                hipops().emb_gather_rows(slot, self.shard.rows, self.rows_u, loc.n_uniq)
                rows_src, rows_idx = self.rows_u, None
            push = ("local", slot)
        else:
            rows_u, w_wide, push = self._pull(loc)
            rows_src, rows_idx = rows_u, None
        if self.gpu:
            if self.row_of is None:
                self.row_of = torch.empty(self.max_nnz, dtype=torch.int32, device=self.device)
            dX0, row_of = self.dX0[:nnz], self.row_of[:nnz]
            hipops().fwfm_csr(row_ptr, fields, nnz, rows_src, rows_idx, vals, B, self.F, self.R,
                              loc.local_col, w_wide, labels, self.coef, dX0, row_of, self.dR_part,
                              self.metrics, self.hist, AUC_BINS)
            dE = E.grad_reduce(loc, dX0, D, nnz, out=self.dE)
            l2_cap = nnz if rows_idx is not None else min(nnz, rows_src.shape[0])
            hipops().fm_l2(dE, rows_src, rows_idx, loc.n_uniq, l2_cap, cfg.lambda_v)
        else:
            X0 = E.expand(loc.local_col, nnz, rows_src, idx=rows_idx)
            row_of = torch.repeat_interleave(torch.arange(B), row_ptr[1:] - row_ptr[:-1])
            dX0, dR = self._fwd_bwd_torch_csr(X0, vals, row_of, fields, loc.local_col, w_wide,
                                              labels)
            self.dR.copy_(dR)
            U = loc.num_unique()
            dE = E.grad_reduce(loc, dX0, D, U)
            v = (rows_src[rows_idx[:U]] if rows_idx is not None else rows_src[:U]).float()
            dE += cfg.lambda_v * v
        g_wide, _ = linear_backward(loc, self.coef[:B], B=B, rows=row_of, vals=vals)
        self._push(loc, push, dE, g_wide)
        self._update_r()
        auc_from_hist(self.hist, self.metrics, self.step_dev)
        self.step_count += 1
        self.examples += B

    def _forward_math_csr(self, X0, vals, row_of, fld, B, local_col, w_wide, dtype, R=None):
        """ops/score.py ``fwfm_forward_csr`` (shared with ``fwfm_score``'s CPU path) on this
        trainer's F and R."""
        return fwfm_forward_csr(X0, vals, row_of, fld, B, self.F, self.R if R is None else R,
                                local_col, w_wide, dtype)

    def _fwd_bwd_math_csr(self, X0, vals, row_of, fld, local_col, w_wide, labels,
                          dtype=torch.float32, R=None):
        """(margin [B], coef [B], dX0 [nnz, D], dR [F, F] symmetric) in ``dtype``, nothing
        rounded to bf16."""
        B = labels.numel()
        m, xq, xv, cell, P, T0, s, rsel = self._forward_math_csr(X0, vals, row_of, fld, B,
                                                                 local_col, w_wide, dtype, R)
        y = torch.where(labels > 0, 1.0, -1.0).to(dtype)
        c = -y * torch.sigmoid(-y * m)
        D = xv.shape[1]
        own = rsel.reshape(-1)[cell][:, None] * (P.reshape(-1, D)[cell] - xv)
        dX = (c[row_of.long()] * xq)[:, None] * (T0.reshape(-1, D)[cell] + own)
        up = torch.triu(torch.einsum("b,bfd,bgd->fg", c, P, P), 1)
        return m, c, dX, up + up.T + torch.diag(c @ s)

    def _fwd_bwd_torch_csr(self, X0, vals, row_of, fld, local_col, w_wide, labels,
                           dtype=torch.float32):
        """fwfm_csr in PyTorch: the CPU route, and in ``dtype=torch.float64`` the reference
        the kernel is tested against. ``row_of`` [nnz] is the row of every occurrence (rows in
        order), ``fld`` [nnz] its field. Returns (dX0 bf16, dR in ``dtype``)."""
        m, c, dX, dR = self._fwd_bwd_math_csr(X0, vals, row_of, fld, local_col, w_wide, labels,
                                              dtype)
        return self._account(m, c, dX, labels, labels.numel()), dR

    # ------------------------------------------------------------------ eval
    def predict(self, keys: torch.Tensor, B: int, vals: torch.Tensor | None = None,
                row_ptr: torch.Tensor | None = None, fields: torch.Tensor | None = None):
        """Margins of B examples (no update, no insert; unseen keys contribute 0). G == 1.
        Rows of ``cfg.slots`` keys, or CSR rows with ``row_ptr`` [B + 1] and ``fields`` [nnz]
        as ``step``. A GPU trainer scores with the forward-only kernels (``fwfm_margins`` /
        ``fwfm_csr_margins``), slots and wide weights per occurrence."""
        if self.G != 1:
            raise NotImplementedError("predict() reads the local shard (G == 1)")
        from ..ops.keymix import mix

        S = self.cfg.slots
        nnz = keys.numel()
        csr = row_ptr is not None or fields is not None
        if csr:
            self._check_csr(nnz, B, row_ptr, fields, vals)
        elif nnz != B * S:
            raise ValueError(f"expected {B * S} keys, got {nnz}")
        mk = mix(keys.to(self.device), self.bits)
        slot, w = self.shard.table.resolve(mk, insert=False)
        ok = slot >= 0
        w = torch.where(ok, w, torch.zeros_like(w))
        if self.gpu:
            margins = torch.empty(B, dtype=torch.float32, device=self.device)
            if csr:
                hipops().fwfm_csr_margins(row_ptr, fields, nnz, self.shard.rows, slot, vals, B,
                                          self.F, self.R, None, w, margins)
            else:
                hipops().fwfm_margins(self.shard.rows, slot, vals, B, S, self.fields, self.F,
                                      self.R, None, w, margins)
            return margins
        X0 = torch.zeros(nnz, self.cfg.embedding_dim, device=self.device)
        X0[ok] = self.shard.rows[slot[ok]].float()
        if csr:
            r = torch.repeat_interleave(torch.arange(B), row_ptr[1:] - row_ptr[:-1])
            return self._forward_math_csr(X0, vals, r, fields, B, torch.arange(nnz), w,
                                          torch.float32)[0]
        return self._forward_math(X0, vals, B, S, torch.arange(nnz), w, torch.float32)[0]

    def scorer(self):
        """An ``FwFMScorer`` on this trainer's own shard and R (no copy: later steps stay
        visible), with ``cfg.fields`` as its position -> field map: held-out loss, accuracy
        and AUC through the fused scoring kernel, rows of any width. G == 1. Nothing is
        synchronised here: score on the stream the steps run on, after them."""
        if self.G != 1:
            raise NotImplementedError(
                "scorer() reads the local shard (G == 1); score a sharded model with "
                "FwFMScorer.from_state_dict(FwFMTrainer.merge_state_dicts(<every rank's "
                "state_dict()>), device)")
        from .scorer import FwFMScorer

        return FwFMScorer.from_shard(self.shard, self.bits, self.F, self.R, fields=self.fields)

    progress = FMTrainer.progress
