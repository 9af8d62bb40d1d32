"""Field-aware factorization machine (FFM, Juan et al. 2016) on the sharded embedding table.

Not a reference model (the reference stops at a sketch of the plain FM, see models/fm.py):
it is the model its Criteo-shaped data asks for. Rows have ``slots`` positions; ``fields``
maps position -> field in [0, F), one map for all rows (identity by default; it may repeat
a field, e.g. Criteo's 13 integer slots on one field, F = 27). A key owns F vectors of k
bf16, v_{i,f} = row_i[f k, + k), in a table row of Dr = F k rounded up to 8 columns
(Dr <= 128, what ``EmbeddingShard`` stores; the padding is never read, its gradient is 0):

    m          = sum_i x_i w_i + sum_{i<j} x_i x_j <v_{i,f_j}, v_{j,f_i}>
    G[i,f,:]   = sum_{j != i, f_j = f} x_j row_j[f_i k, + k)
    m          = lin + 1/2 sum_i x_i <row_i, G[i]>
    dX0[i,f,:] = c x_i G[i,f,:],  c = -y sigma(-y m)         (logistic loss, as the FM)

All pairs count, same-field pairs included (as libffm); a key that occurs twice in a row is
two positions. The step is ``FMTrainer``'s fixed-width step with ``ffm_fwd_bwd`` (ffm.hip:
one wavefront per example on an LDS tile of its rows) in place of ``fm_fwd_bwd_gather``:
localise -> pull rows + w -> forward / backward -> per-key reduction of dX0 + L2 -> AdaGrad
rows; wide gradient by the sparse-LR segmented reduction. G > 1 pulls / pushes packed
``[v | w]`` records (``EmbeddingPS``).

``step(..., row_ptr=, fields=)`` / ``predict(..., row_ptr=, fields=)`` take CSR minibatches with
a field id per occurrence (libffm's ``field:index:value`` rows; the device text parsers' CSR
arrays with one slot id per feature): rows of any width, fields missing, repeated, in any
order. ``fields`` [nnz] int32 then replaces the position -> field map; a field outside [0, F)
keeps the occurrence's linear term and takes it out of every pair. The step is the same
sequence with ``ffm_csr`` (ffm_csr.hip) as its forward / backward: rows of up to ``cfg.slots``
positions run on the per-wave LDS tile with field lists built in the wave, wider rows on a
second launch that reads partners from global memory.

Scoring a stored model is ``FFMScorer`` (models/scorer.py, ``scorer()`` below): margins, loss /
accuracy sums and the AUC histogram of raw keys in one launch of the fused probe + field-sum
kernel (ffm_predict.hip), rows of any width, from a live shard or a snapshot.
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
from ..ops.score import ffm_pairs, ffm_pairs_csr
from ..parallel.comm import Comm, LocalComm
from ..parallel.partition import KeyPartition
from .fm import FMTrainer
from .wide_deep import EmbeddingPS


@dataclass
class FFMConfig:
    num_features: int = 10 ** 8
    k: int = 2                           # factors per (key, field): 2, 4 or 8
    fields: list | None = None           # position -> field; None: identity over slots
    num_fields: int = 0                  # F; 0: max(fields) + 1
    slots: int = 39                      # positions per example (<= 64)
    minibatch: int = 10000
    emb_lr: float = 0.02
    emb_init_scale: float = 0.01
    lambda_v: float = 10.0               # L2 on the factors (once per unique key and step)
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
        """(fields, F, Dr), checked: everything the kernel's launcher would refuse."""
        S, k = self.slots, self.k
        if not 1 <= S <= 64:
            raise ValueError(f"slots must be in 1..64, not {S}")
        if k not in (2, 4, 8):
            raise ValueError(f"k must be 2, 4 or 8, not {k}")
        fields = list(range(S)) if self.fields is None else [int(f) for f in self.fields]
        if len(fields) != S:
            raise ValueError(f"fields has {len(fields)} entries for {S} slots")
        F = self.num_fields or max(fields) + 1
        if min(fields) < 0 or max(fields) >= F:
            raise ValueError(f"every field must lie in [0, {F})")
        Dr = (F * k + 7) // 8 * 8
        if Dr > 128:
            raise ValueError(f"row width {Dr} ({F} fields of k = {k}) exceeds 128")
        return fields, F, Dr

    @property
    def embedding_dim(self) -> int:      # the table's row width (EmbeddingPS reads it)
        return self.geometry()[2]


class FFMTrainer(EmbeddingPS):
    def __init__(self, cfg: FFMConfig, comm: Comm | None = None, device="cpu"):
        self.cfg = cfg
        self.fields, self.F, self.Dr = cfg.geometry()
        self.comm = comm or LocalComm(device)
        self.G, self.rank = self.comm.world, self.comm.rank
        self.device = dev = torch.device(device)
        self.gpu = dev.type == "cuda"
        self.bits = key_bits_for(cfg.num_features)
        self.part = KeyPartition(self.bits, self.G)
        Dr, S, B = self.Dr, cfg.slots, cfg.minibatch
        per_slot = 32 + 2 * Dr + 5
        cap = cfg.table_capacity or next_pow2(int(math.ceil(cfg.num_features / self.G /
                                                            cfg.table_load)))
        cap = max(1024, min(cap, 1 << max(10, (cfg.max_table_bytes // per_slot).bit_length() - 1)))
        self.shard = E.EmbeddingShard(cap, Dr, dev, init_scale=cfg.emb_init_scale,
                                      seed=cfg.seed * 7919 + 17)
        self.max_nnz = B * S
        self.localizer = Localizer(self.max_nnz, self.bits, dev, mode=cfg.localize)
        self.coef = torch.empty(B, dtype=torch.float32, device=dev)
        self.metrics = new_accum(dev)
        self.stats = new_accum(dev)
        self.hist = torch.zeros(2 * AUC_BINS, dtype=torch.int32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._fields_t = torch.tensor(self.fields, dtype=torch.long, device=dev)
        if self.gpu:
            self.slot_buf = torch.empty(self.max_nnz, dtype=torch.int64, device=dev)
            self.w_buf = torch.empty(self.max_nnz, dtype=torch.float32, device=dev)
            self.dX0 = torch.empty(self.max_nnz, Dr, dtype=torch.bfloat16, device=dev)
            self.dE = torch.empty(self.max_nnz, Dr, dtype=torch.float32, device=dev)
            self.rows_u = torch.empty(self.max_nnz, Dr, dtype=torch.bfloat16, device=dev)
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
        used): row b holds keys[row_ptr[b]:row_ptr[b + 1]]."""
        if row_ptr is not None or fields is not None:
            return self._step_csr(keys, labels, vals, loc, row_ptr, fields)
        cfg = self.cfg
        S, Dr = cfg.slots, self.Dr
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
                # each unique key's row gathered once into a compact buffer; the forward's
                # per-occurrence loads then read that buffer
                hipops().emb_gather_rows(slot, self.shard.rows, self.rows_u, loc.n_uniq)
                rows_src, rows_idx = self.rows_u, None
            push = ("local", slot)
        else:
            rows_u, w_wide, push = self._pull(loc)
            rows_src, rows_idx = rows_u, None
        if self.gpu:
            dX0 = self._fwd_bwd_hip(rows_src, rows_idx, vals, B, loc, w_wide, labels)
            dE = E.grad_reduce(loc, dX0, Dr, nnz, out=self.dE)
            # pulled rows (G > 1) hold the U unique keys' rows only: no more than that
            l2_cap = nnz if rows_idx is not None else min(nnz, rows_src.shape[0])
            hipops().fm_l2(dE, rows_src, rows_idx, loc.n_uniq, l2_cap, cfg.lambda_v)
        else:
            X0 = E.expand(loc.local_col, nnz, rows_src, idx=rows_idx)
            dX0 = self._fwd_bwd_torch(X0, vals, B, S, loc.local_col, w_wide, labels)
            U = loc.num_unique()
            dE = E.grad_reduce(loc, dX0, Dr, U)
            v = (rows_src[rows_idx[:U]] if rows_idx is not None else rows_src[:U]).float()
            dE += cfg.lambda_v * v
        g_wide, _ = linear_backward(loc, self.coef[:B], B=B, width=S, vals=vals)
        self._push(loc, push, dE, g_wide)
        auc_from_hist(self.hist, self.metrics, self.step_dev)
        self.step_count += 1
        self.examples += B

    def _fwd_bwd_hip(self, rows_src, rows_idx, vals, B, loc, w_wide, labels):
        """The GPU step's forward / backward: coef, metrics, hist and dX0 [B*S, Dr] in one
        launch, rows read through local_col (and rows_idx)."""
        dX0 = self.dX0[:B * self.cfg.slots]
        hipops().ffm_fwd_bwd(rows_src, rows_idx, vals, B, self.cfg.slots, self.fields, self.F,
                             self.cfg.k, loc.local_col, w_wide, labels, self.coef, dX0,
                             self.metrics, self.hist, AUC_BINS)
        return dX0

    def _pairs_torch(self, X0, x, dtype):
        """G [B, S, F, k] and the pair part of the margin [B] of expanded rows X0
        [B*S, Dr] with values x [B, S] (ops/score.py ``ffm_pairs``)."""
        return ffm_pairs(X0, x, self._fields_t.to(X0.device), self.F, self.cfg.k, dtype)

    def _fwd_bwd_math(self, X0, vals, B, S, local_col, w_wide, labels, dtype=torch.float32):
        """(margin [B], coef [B], dX0 [B*S, Dr]) in ``dtype``, nothing rounded to bf16."""
        dev = X0.device
        x = (vals[:B * S].to(dtype) if vals is not None else
             torch.ones(B * S, dtype=dtype, device=dev)).reshape(B, S)
        G, pair = self._pairs_torch(X0, x, dtype)
        lc = local_col[:B * S].long().reshape(B, S)
        m = (w_wide.to(dtype)[lc] * x).sum(1) + pair
        y = torch.where(labels[:B] > 0, 1.0, -1.0).to(dtype)
        c = -y * torch.sigmoid(-y * m)
        dX = torch.zeros(B, S, self.Dr, dtype=dtype, device=dev)
        dX[:, :, :self.F * self.cfg.k] = ((c[:, None] * x)[..., None, None] * G).reshape(B, S, -1)
        return m, c, dX.reshape(B * S, self.Dr)

    def _fwd_bwd_torch(self, X0, vals, B, S, local_col, w_wide, labels, dtype=torch.float32):
        """ffm_fwd_bwd in PyTorch: the CPU route, and in ``dtype=torch.float64`` the
        reference the kernel is tested against."""
        m, c, dX = self._fwd_bwd_math(X0, vals, B, S, local_col, w_wide, labels, dtype)
        return self._account(m, c, dX, labels, B)

    def _account(self, m, c, dX, labels, B):
        """What the kernels write beside dX0: coef, loss / accuracy / count, the AUC bins."""
        y = torch.where(labels[:B] > 0, 1.0, -1.0).to(m.dtype)
        self.coef[:B] = c
        self.metrics[0] += torch.nn.functional.softplus(-y * m).double().sum()
        self.metrics[1] += ((y > 0) == (m > 0)).double().sum()
        self.metrics[2] += B
        nb = AUC_BINS
        pb = torch.clamp((torch.sigmoid(m) * nb).long(), 0, nb - 1)
        self.hist += torch.bincount(pb + torch.where(y > 0, nb, 0), minlength=2 * nb).to(
            self.hist.dtype)
        return dX.to(torch.bfloat16)

    # ------------------------------------------------------------------ CSR rows
    def _check_csr(self, nnz: int, B: int, row_ptr, fields, vals) -> None:
        """Everything a CSR minibatch can get wrong, before anything is launched (shapes and
        dtypes only: the widths and the field ids are device data)."""
        if row_ptr is None or fields is None:
            raise ValueError("CSR rows need both row_ptr [B + 1] and fields [nnz]")
        if row_ptr.numel() != B + 1:
            raise ValueError(f"row_ptr has {row_ptr.numel()} entries for {B} rows, not {B + 1}")
        if row_ptr.dtype != torch.int64:
            raise ValueError("row_ptr must be int64")
        if fields.numel() != nnz:
            raise ValueError(f"expected {nnz} fields, got {fields.numel()}")
        if fields.dtype != torch.int32:
            raise ValueError("fields must be int32")
        if fields.device.type != self.device.type:
            raise ValueError(f"fields must be on the trainer's device ({self.device})")
        if vals is not None and vals.numel() != nnz:
            raise ValueError(f"expected {nnz} values, got {vals.numel()}")

    def _step_csr(self, keys, labels, vals, loc, row_ptr, fields):
        """step() on CSR rows with a field per occurrence: ``FMTrainer._step_csr``'s sequence
        with ``ffm_csr`` (ffm_csr.hip) as its forward / backward; the kernel also writes the
        row id of every occurrence for the wide gradient. ``cfg.slots`` is the row capacity
        of the LDS tile, not a limit: wider rows take the kernel's global-memory path.
        Nothing here reads device data on the host."""
        cfg = self.cfg
        Dr = self.Dr
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
            hipops().ffm_csr(row_ptr, fields, nnz, rows_src, rows_idx, vals, B, cfg.slots, self.F,
                             cfg.k, loc.local_col, w_wide, labels, self.coef, dX0, row_of,
                             self.metrics, self.hist, AUC_BINS)
            dE = E.grad_reduce(loc, dX0, Dr, nnz, out=self.dE)
            l2_cap = nnz if rows_idx is not None else min(nnz, rows_src.shape[0])
            hipops().fm_l2(dE, rows_src, rows_idx, loc.n_uniq, l2_cap, cfg.lambda_v)
        else:
            X0 = E.expand(loc.local_col, nnz, rows_src, idx=rows_idx)
            row_of = torch.repeat_interleave(torch.arange(B), row_ptr[1:] - row_ptr[:-1])
            dX0 = self._fwd_bwd_torch_csr(X0, vals, row_of, fields, loc.local_col, w_wide, labels)
            U = loc.num_unique()
            dE = E.grad_reduce(loc, dX0, Dr, U)
            v = (rows_src[rows_idx[:U]] if rows_idx is not None else rows_src[:U]).float()
            dE += cfg.lambda_v * v
        g_wide, _ = linear_backward(loc, self.coef[:B], B=B, rows=row_of, vals=vals)
        self._push(loc, push, dE, g_wide)
        auc_from_hist(self.hist, self.metrics, self.step_dev)
        self.step_count += 1
        self.examples += B

    def _pairs_torch_csr(self, X0, x, row_of, fld, B, dtype):
        """``_pairs_torch`` on CSR rows (ops/score.py ``ffm_pairs_csr``): G [nnz, F, k], the
        pair part of the margin [B] and x [nnz] with the fields outside [0, F) masked."""
        return ffm_pairs_csr(X0, x, row_of, fld, B, self.F, self.cfg.k, dtype)

    def _fwd_bwd_math_csr(self, X0, vals, row_of, fld, local_col, w_wide, labels,
                          dtype=torch.float32):
        """(margin [B], coef [B], dX0 [nnz, Dr]) in ``dtype``, nothing rounded to bf16."""
        nnz, B, dev = row_of.numel(), labels.numel(), X0.device
        x = vals[:nnz].to(dtype) if vals is not None else torch.ones(nnz, dtype=dtype, device=dev)
        G, pair, xq = self._pairs_torch_csr(X0, x, row_of, fld, B, dtype)
        m = torch.zeros(B, dtype=dtype, device=dev).index_add_(
            0, row_of.long(), w_wide.to(dtype)[local_col[:nnz].long()] * x) + pair
        y = torch.where(labels > 0, 1.0, -1.0).to(dtype)
        c = -y * torch.sigmoid(-y * m)
        dX = torch.zeros(nnz, self.Dr, dtype=dtype, device=dev)
        dX[:, :self.F * self.cfg.k] = ((c[row_of.long()] * xq)[:, None, None] * G).reshape(nnz, -1)
        return m, c, dX

    def _fwd_bwd_torch_csr(self, X0, vals, row_of, fld, local_col, w_wide, labels,
                           dtype=torch.float32):
        """ffm_csr in PyTorch: the CPU route, and in ``dtype=torch.float64`` the reference
        the kernels are tested against. ``row_of`` [nnz] is the row of every occurrence
        (rows in order), ``fld`` [nnz] its field."""
        m, c, dX = self._fwd_bwd_math_csr(X0, vals, row_of, fld, local_col, w_wide, labels, dtype)
        return self._account(m, c, dX, labels, labels.numel())

    # ------------------------------------------------------------------ eval
    def predict(self, keys: torch.Tensor, B: int, vals: torch.Tensor | None = None,
                row_ptr: torch.Tensor | None = None,
                fields: torch.Tensor | None = None) -> torch.Tensor:
        """Margins of B examples (no update, no insert; unseen keys contribute 0). G == 1.
        Rows of ``cfg.slots`` keys, or CSR rows with ``row_ptr`` [B + 1] and ``fields``
        [nnz] as ``step``. A GPU trainer scores with the forward-only kernels
        (``ffm_margins`` / ``ffm_csr_margins``), slots and wide weights per occurrence."""
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
                hipops().ffm_csr_margins(row_ptr, fields, nnz, self.shard.rows, slot, vals, B, S,
                                         self.F, self.cfg.k, None, w, margins)
            else:
                hipops().ffm_margins(self.shard.rows, slot, vals, B, S, self.fields, self.F,
                                     self.cfg.k, None, w, margins)
            return margins
        X0 = torch.zeros(nnz, self.Dr, device=self.device)
        X0[ok] = self.shard.rows[slot[ok]].float()
        x = vals.float() if vals is not None else torch.ones(nnz)
        if csr:
            r = torch.repeat_interleave(torch.arange(B), row_ptr[1:] - row_ptr[:-1])
            pair = self._pairs_torch_csr(X0, x, r, fields, B, torch.float32)[1]
            return torch.zeros(B).index_add_(0, r, w * x) + pair
        x = x.reshape(B, S)
        return (w.reshape(B, S) * x).sum(1) + self._pairs_torch(X0, x, torch.float32)[1]

    def scorer(self):
        """An ``FFMScorer`` on this trainer's own shard (no copy), with ``cfg.fields`` as its
        position -> field map: held-out loss, accuracy and AUC through the fused scoring
        kernel, rows of any width. G == 1. Nothing is synchronised here: score on the stream
        the steps run on, after them."""
        if self.G != 1:
            raise NotImplementedError(
                "scorer() reads the local shard (G == 1); score a sharded model with "
                "FFMScorer.from_state_dict(FFMTrainer.merge_state_dicts(<every rank's "
                "state_dict()>), device, num_fields, k)")
        from .scorer import FFMScorer

        return FFMScorer.from_shard(self.shard, self.bits, self.F, self.cfg.k, fields=self.fields)

    progress = FMTrainer.progress
