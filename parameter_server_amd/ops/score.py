"""Score minibatches of raw keys against a ``KVTable``: margins, loss / accuracy sums and
a bucketed-AUC histogram for a whole validation set.

GPU: one ``predict_rows`` launch per minibatch (csrc/hip/predict.hip) -- the kernel mixes
the raw keys itself and probes the table read-only, an absent key contributing 0 (the
reference's ModelEvaluation rule, src/app/linear_method/model_evaluation.h:9-74). CPU: the
same math with plain PyTorch ops (mix, ``resolve(insert=False)`` + ``gather``,
``index_add_`` in f32, the loss / accuracy / bin formulas of ops/linear.py).

The caller makes the table current first (``SparseLRTrainer.flush()``): the kernel reads
weights plainly.
"""
from __future__ import annotations

import torch

from .keymix import mix
from .linear import (AUC_BINS, HIST_STRIPES, _rows_of, accum_total, loss_id,
                     loss_terms_torch, new_accum)
from .native import hipops, is_gpu


class ScoreAccum:
    """What scoring adds into: the striped f64 sums ``[loss, correct, count]`` (ops/linear
    ``new_accum``) and ``HIST_STRIPES`` copies of the 2 x ``AUC_BINS`` histogram (negatives,
    then positives) in int64, so the counts of a long file cannot wrap. All additive: ranks
    and minibatches may split the rows in any way."""

    def __init__(self, device):
        self.metrics = new_accum(device)
        self.hist = torch.zeros(HIST_STRIPES * 2 * AUC_BINS, dtype=torch.int64, device=device)

    def sums(self) -> torch.Tensor:
        """float64 [3]: loss sum, correct, count."""
        return accum_total(self.metrics)[:3].clone()

    def counts(self) -> torch.Tensor:
        """int64 [2 * AUC_BINS]: the histogram summed over its stripes."""
        return self.hist.view(-1, 2 * AUC_BINS).sum(0)


def auc_from_counts(counts) -> tuple[float, float]:
    """(bucketed AUC, tie mass) of a 2 x AUC_BINS histogram (negatives, then positives):
    AUC = sum_b pos_b (2 neg_below_b + neg_b) / (2 P N), in Python integers; the tie mass
    sum_b pos_b neg_b / (2 P N) bounds its distance from the exact (sorted) AUC of the same
    scores -- only pairs that share a bin are counted differently, as half a pair each."""
    c = counts.view(-1, 2 * AUC_BINS).sum(0).tolist() if isinstance(counts, torch.Tensor) \
        else list(counts)
    neg, pos = c[:AUC_BINS], c[AUC_BINS:]
    P, N = sum(pos), sum(neg)
    if P == 0 or N == 0:
        return float("nan"), 0.0
    below = area2 = tie2 = 0
    for nb, pb in zip(neg, pos):
        area2 += pb * (2 * below + nb)
        tie2 += pb * nb
        below += nb
    return area2 / (2 * P * N), tie2 / (2 * P * N)


def score(table, keys: torch.Tensor, bits: int, *, row_ptr=None, width=None, vals=None,
          labels=None, margins: bool = True, acc: ScoreAccum | None = None, loss="logit",
          B: int | None = None, lanes: int = 0):
    """Margins (float32 [B], or None with ``margins=False``) of the rows of raw ``keys``
    (int64 [nnz]; ``row_ptr`` int64 [B + 1], or a fixed ``width``; ``vals`` float32 [nnz] or
    binary) against ``table`` (keys stored mixed over ``bits``). With ``labels`` and ``acc``
    the loss / correct / count sums and the AUC histogram are added into ``acc``.
    ``lanes``: lanes per row on the GPU (0: from nnz / B; 8 or 64)."""
    if (row_ptr is None) == (not width):
        raise ValueError("score needs row_ptr or a fixed width, not both")
    if acc is not None and labels is None:
        raise ValueError("score: an accumulator needs labels")
    keys = keys.contiguous()
    nnz = keys.numel()
    if B is None:
        B = row_ptr.numel() - 1 if row_ptr is not None else nnz // int(width)
    dev = keys.device
    L = loss_id(loss)
    m = torch.empty(B, dtype=torch.float32, device=dev) if (margins or not is_gpu(keys)) else None
    if B == 0:
        return m if margins else None
    if is_gpu(keys):
        hipops().predict_rows(table.slots, table.home_base, table.home_m, keys, bits, row_ptr,
                              int(width or 0), vals, labels, B, L, m,
                              acc.metrics if acc is not None else None,
                              acc.hist if acc is not None else None, AUC_BINS, lanes)
        return m
    slot, _ = table.resolve(mix(keys, bits), insert=False, with_w=False)
    contrib = table.gather(slot)  # absent key: slot -1 -> 0
    if vals is not None:
        contrib = contrib * vals[:nnz].float()
    rp = row_ptr[:B + 1] if row_ptr is not None else None
    rows = _rows_of(B, int(width or 0), rp, dev)
    m.zero_().index_add_(0, rows, contrib[:rows.numel()])
    if acc is not None:
        _accumulate(acc, m, labels, B, L)
    return m if margins else None


def _accumulate(acc: ScoreAccum, m: torch.Tensor, labels: torch.Tensor, B: int, L: int):
    """The CPU path's sums and bins of B margins ``m`` into ``acc``."""
    y = labels[:B].float()
    # (terms in f64: torch's vectorised f32 softplus differs in the last bit between a
    # row's place in the SIMD body and in the scalar tail, so f32 terms would make the
    # sum depend on how the rows are cut into minibatches)
    lo, _, _ = loss_terms_torch(m.double(), y.double(), L)
    mt = acc.metrics  # CPU code adds into stripe 0
    mt[0] += float(lo.sum())
    mt[1] += float(((y > 0) == (m > 0)).double().sum())
    mt[2] += float(B)
    p = torch.sigmoid(m)
    b = torch.clamp((p * AUC_BINS).long(), 0, AUC_BINS - 1)
    off = torch.where(y > 0, AUC_BINS, 0)
    acc.hist[:2 * AUC_BINS] += torch.bincount(b + off, minlength=2 * AUC_BINS)


def fm_score(shard, keys: torch.Tensor, bits: int, *, row_ptr=None, width=None, vals=None,
             labels=None, margins: bool = True, acc: ScoreAccum | None = None, loss="logit",
             B: int | None = None, lanes: int = 0):
    """``score`` for a factorization machine: ``shard`` is an ``EmbeddingShard`` (the KV
    table with the wide weights and the bf16 factor rows at the same slot index, any
    ``dim`` that is a multiple of 8 up to 128); margin = x.w + 1/2 sum_f [(sum_i x_i
    v_if)^2 - sum_i x_i^2 v_if^2], a key the model does not hold contributing nothing.
    GPU: one ``fm_predict_rows`` launch (csrc/hip/fm_predict.hip); CPU: the PyTorch ops of
    ``FMTrainer.predict``. ``lanes``: lanes per row on the GPU (0: from nnz / B; 16, 32, 64)."""
    if (row_ptr is None) == (not width):
        raise ValueError("fm_score needs row_ptr or a fixed width, not both")
    if acc is not None and labels is None:
        raise ValueError("fm_score: an accumulator needs labels")
    keys = keys.contiguous()
    nnz = keys.numel()
    if B is None:
        B = row_ptr.numel() - 1 if row_ptr is not None else nnz // int(width)
    dev = keys.device
    L = loss_id(loss)
    table = shard.table
    if is_gpu(keys):
        m = torch.empty(B, dtype=torch.float32, device=dev) if margins else None
        if B:
            hipops().fm_predict_rows(table.slots, table.home_base, table.home_m, shard.rows, keys,
                                     bits, row_ptr, int(width or 0), vals, labels, B, L, m,
                                     acc.metrics if acc is not None else None,
                                     acc.hist if acc is not None else None, AUC_BINS, lanes)
        return m
    if B == 0:
        return torch.empty(0, dtype=torch.float32) if margins else None
    D = shard.dim
    slot, w = table.resolve(mix(keys, bits), insert=False)
    ok = slot >= 0
    w = torch.where(ok, w, torch.zeros_like(w))
    V = torch.zeros(nnz, D, device=dev)
    V[ok] = shard.rows[slot[ok]].float()
    if vals is not None:
        V = V * vals.float()[:, None]
        w = w * vals.float()
    if row_ptr is None:
        S = int(width)
        V = V[:B * S].reshape(B, S, D)
        s = V.sum(1)
        m = w[:B * S].reshape(B, S).sum(1) + 0.5 * (s * s - (V * V).sum(1)).sum(1)
    else:
        r = torch.repeat_interleave(torch.arange(B), row_ptr[1:B + 1] - row_ptr[:B])
        n = r.numel()
        s = torch.zeros(B, D).index_add_(0, r, V[:n])
        q = torch.zeros(B).index_add_(0, r, (V[:n] * V[:n]).sum(1))
        m = torch.zeros(B).index_add_(0, r, w[:n]) + 0.5 * ((s * s).sum(1) - q)
    if acc is not None:
        _accumulate(acc, m, labels, B, L)
    return m if margins else None


def ffm_pairs(X0, x, fl, F: int, k: int, dtype):
    """The field-aware pairs of fixed-width rows in PyTorch: expanded rows X0 [B*S, Dr],
    values x [B, S], ``fl`` [S] (long) position -> field in [0, F). Gather [B, S, S, k], mask
    the diagonal, scatter-add by the partner's field. Returns G [B, S, F, k] with G[b, i, f] =
    sum_{j != i, f_j = f} x_j v_{j, f_i} and the pair part of the margin [B]."""
    B, S = x.shape
    V = X0[:B * S, :F * k].to(dtype).reshape(B, S, F, k)
    P = V[:, :, fl, :].transpose(1, 2)  # P[b, i, j] = v_{j, f_i}
    off = 1.0 - torch.eye(S, dtype=dtype, device=X0.device)
    P = P * (x[:, None, :] * off)[..., None]
    G = torch.zeros(B, S, F, k, dtype=dtype, device=X0.device).index_add_(2, fl, P)
    return G, 0.5 * (x * (V * G).sum((2, 3))).sum(1)


def ffm_pairs_csr(X0, x, row_of, fld, B: int, F: int, k: int, dtype):
    """``ffm_pairs`` on CSR rows with a field per occurrence: the rows are gathered into a
    padded [B, W] block (W the widest row) where an absent position, or an occurrence whose
    field is outside [0, F), has x = 0 and so enters no pair. Returns G [nnz, F, k] (zero for
    such an occurrence), the pair part of the margin [B] and the masked x [nnz]."""
    nnz, dev = row_of.numel(), X0.device
    r = row_of.long()
    width = torch.bincount(r, minlength=B)
    W = max(int(width.max()) if nnz else 0, 1)
    col = torch.arange(nnz, device=dev) - (torch.cumsum(width, 0) - width)[r]
    f = fld[:nnz].long()
    ok = (f >= 0) & (f < F)
    x = x * ok
    Vp = torch.zeros(B, W, F, k, dtype=dtype, device=dev)
    Vp[r, col] = X0[:nnz, :F * k].to(dtype).reshape(nnz, F, k)
    xp = torch.zeros(B, W, dtype=dtype, device=dev)
    xp[r, col] = x
    fp = torch.zeros(B, W, dtype=torch.long, device=dev)
    fp[r, col] = torch.where(ok, f, 0)
    bi = torch.arange(B, device=dev)[:, None, None]
    ji = torch.arange(W, device=dev)[None, None, :]
    P = Vp[bi, ji, fp[:, :, None]]  # P[b, i, j] = v_{j, f_i}
    off = 1.0 - torch.eye(W, dtype=dtype, device=dev)
    P = P * (xp[:, None, :] * off)[..., None]
    G = torch.zeros(B, W, F, k, dtype=dtype, device=dev).scatter_add_(
        2, fp[:, None, :, None].expand(B, W, W, k), P)
    pair = 0.5 * (xp * (Vp * G).sum((2, 3))).sum(1)
    return G[r, col] * ok[:, None, None], pair, x


def ffm_score(shard, keys: torch.Tensor, bits: int, *, num_fields: int, k: int, row_ptr=None,
              width=None, fields=None, vals=None, labels=None, margins: bool = True,
              acc: ScoreAccum | None = None, loss="logit", B: int | None = None):
    """``score`` for a field-aware factorization machine: ``shard`` is an ``EmbeddingShard``
    whose rows hold ``num_fields`` vectors of ``k`` bf16 (models/ffm.py); margin = x.w +
    sum_{i<j} x_i x_j <v_{i,f_j}, v_{j,f_i}>, a key the model does not hold contributing
    nothing. With ``row_ptr``, ``fields`` is int32 [nnz], the field of every occurrence (one
    outside [0, F) keeps its linear term and enters no pair); with a fixed ``width`` it is the
    position -> field map (int32 [width] on the keys' device, or a list; None: identity).
    GPU: one ``ffm_predict_rows`` launch (csrc/hip/ffm_predict.hip), rows of any width; CPU:
    the PyTorch ops of ``FFMTrainer.predict``, in f32."""
    if (row_ptr is None) == (not width):
        raise ValueError("ffm_score needs row_ptr or a fixed width, not both")
    if acc is not None and labels is None:
        raise ValueError("ffm_score: an accumulator needs labels")
    F, k = int(num_fields), int(k)
    if k not in (2, 4, 8) or F < 1 or F * k > shard.dim:
        raise ValueError(f"ffm_score: {F} fields of k = {k} (2, 4 or 8) do not fit rows of "
                         f"{shard.dim} columns")
    keys = keys.contiguous()
    nnz = keys.numel()
    dev = keys.device
    if row_ptr is not None:
        if fields is None or not isinstance(fields, torch.Tensor) or \
                fields.dtype != torch.int32 or fields.numel() != nnz:
            raise ValueError(f"ffm_score: rows by row_ptr need fields, int32 [{nnz}]")
    elif fields is None:
        if int(width) > F:
            raise ValueError(f"ffm_score: rows of {int(width)} positions on {F} fields need a "
                             "position -> field map")
    else:
        if not isinstance(fields, torch.Tensor):
            fields = torch.tensor([int(f) for f in fields], dtype=torch.int32, device=dev)
        if fields.dtype != torch.int32 or fields.numel() != int(width):
            raise ValueError(f"ffm_score: the position -> field map must be int32 [{int(width)}]")
    if fields is not None and fields.device.type != dev.type:
        raise ValueError(f"ffm_score: fields must be on the keys' device ({dev})")
    if B is None:
        B = row_ptr.numel() - 1 if row_ptr is not None else nnz // int(width)
    L = loss_id(loss)
    table = shard.table
    if is_gpu(keys):
        m = torch.empty(B, dtype=torch.float32, device=dev) if margins else None
        if B:
            csr = row_ptr is not None
            hipops().ffm_predict_rows(table.slots, table.home_base, table.home_m, shard.rows, keys,
                                      bits, F, k, row_ptr, int(width or 0),
                                      fields if csr else None, None if csr else fields, vals,
                                      labels, B, L, m, acc.metrics if acc is not None else None,
                                      acc.hist if acc is not None else None, AUC_BINS)
        return m
    if B == 0:
        return torch.empty(0, dtype=torch.float32) if margins else None
    slot, w = table.resolve(mix(keys, bits), insert=False)
    ok = slot >= 0
    w = torch.where(ok, w, torch.zeros_like(w))
    X0 = torch.zeros(nnz, shard.dim, device=dev)
    X0[ok] = shard.rows[slot[ok]].float()
    x = vals.float() if vals is not None else torch.ones(nnz)
    if row_ptr is not None:
        r = torch.repeat_interleave(torch.arange(B), row_ptr[1:B + 1] - row_ptr[:B])
        n = r.numel()
        pair = ffm_pairs_csr(X0[:n], x[:n], r, fields, B, F, k, torch.float32)[1]
        m = torch.zeros(B).index_add_(0, r, w[:n] * x[:n]) + pair
    else:
        S = int(width)
        fl = torch.arange(S) if fields is None else fields.long()
        if int(fl.min()) < 0 or int(fl.max()) >= F:
            raise ValueError(f"ffm_score: every field of the position map must lie in [0, {F})")
        x = x[:B * S].reshape(B, S)
        m = (w[:B * S].reshape(B, S) * x).sum(1) + ffm_pairs(X0, x, fl, F, k, torch.float32)[1]
    if acc is not None:
        _accumulate(acc, m, labels, B, L)
    return m if margins else None


def fwfm_forward(X0, vals, B: int, S: int, fl, F: int, R, local_col, w_wide, dtype):
    """The field-weighted FM's forward on fixed-width rows in PyTorch (``FwFMTrainer``'s CPU
    route and float64 reference, and ``fwfm_score``'s CPU path): expanded rows X0 [B*S, D],
    ``fl`` [S] (long) position -> field in [0, F). Returns (margin [B], x [B, S], x v
    [B, S, D], P [B, F, D], q [B, F], T [B, F, D], diag R [F]) in ``dtype``; R is read as
    symmetric from its upper triangle."""
    dev = X0.device
    x = (vals[:B * S].to(dtype) if vals is not None else
         torch.ones(B * S, dtype=dtype, device=dev)).reshape(B, S)
    xv = x[..., None] * X0[:B * S].to(dtype).reshape(B, S, -1)
    onehot = torch.zeros(S, F, dtype=dtype, device=dev)
    onehot[torch.arange(S, device=dev), fl.to(dev)] = 1
    P = torch.einsum("sf,bsd->bfd", onehot, xv)
    q = (xv * xv).sum(2) @ onehot
    R = R.to(dev, dtype)
    # a field of fewer than two positions has no same-field pair: its diagonal entry
    # has no part in the model and is read as 0
    rd = torch.diagonal(R) * (onehot.sum(0) >= 2)
    Rs = torch.triu(R, 1) + torch.triu(R, 1).T + torch.diag(rd)
    T = torch.einsum("fg,bgd->bfd", Rs, P)
    lc = local_col[:B * S].long().reshape(B, S)
    m = (w_wide.to(dtype)[lc] * x).sum(1) + 0.5 * ((P * T).sum((1, 2)) - q @ rd)
    return m, x, xv, P, q, T, rd


def fwfm_forward_csr(X0, vals, row_of, fld, B: int, F: int, R, local_col, w_wide, dtype):
    """The field-weighted FM's forward on CSR rows with a field per occurrence, in PyTorch
    (``FwFMTrainer``'s CPU route and float64 reference, and ``fwfm_score``'s CPU path):
    (margin [B], x [nnz] with the fields outside [0, F) masked, x v [nnz, D], the cell
    row * F + field of every occurrence [nnz], P [B, F, D], T0 [B, F, D], s [B, F],
    n_f >= 2 ? R[f][f] : 0 [B, F]) in ``dtype``; R is read as symmetric from its upper
    triangle. Per-row sums are ``index_add`` over ``row_of``; the diagonal acts by select
    on the row's own count n_f >= 2."""
    nnz, dev = row_of.numel(), X0.device
    x = vals[:nnz].to(dtype) if vals is not None else torch.ones(nnz, dtype=dtype, device=dev)
    ok = (fld[:nnz] >= 0) & (fld[:nnz] < F)
    xq = torch.where(ok, x, torch.zeros((), dtype=dtype, device=dev))
    cell = row_of.long() * F + torch.where(ok, fld[:nnz], 0).long()
    xv = xq[:, None] * X0[:nnz].to(dtype)
    P = torch.zeros(B * F, xv.shape[1], dtype=dtype, device=dev).index_add_(0, cell, xv)
    q = torch.zeros(B * F, dtype=dtype, device=dev).index_add_(0, cell, (xv * xv).sum(1))
    n = torch.zeros(B * F, dtype=dtype, device=dev).index_add_(0, cell, ok.to(dtype))
    P, pairs = P.view(B, F, -1), (n >= 2).view(B, F)
    R = R.to(dev, dtype)
    up = torch.triu(R, 1)
    T0 = torch.einsum("fg,bgd->bfd", up + up.T, P)
    zero = torch.zeros((), dtype=dtype, device=dev)
    s = torch.where(pairs, 0.5 * ((P * P).sum(2) - q.view(B, F)), zero)
    rsel = torch.where(pairs, torch.diagonal(R)[None, :], zero)
    lin = torch.zeros(B, dtype=dtype, device=dev).index_add_(
        0, row_of.long(), w_wide.to(dtype)[local_col[:nnz].long()] * x)
    m = lin + 0.5 * (P * T0).sum((1, 2)) + (rsel * s).sum(1)
    return m, xq, xv, cell, P, T0, s, rsel


def fwfm_score(shard, keys: torch.Tensor, bits: int, *, num_fields: int, R: torch.Tensor,
               row_ptr=None, width=None, fields=None, vals=None, labels=None,
               margins: bool = True, acc: ScoreAccum | None = None, loss="logit",
               B: int | None = None):
    """``score`` for a field-weighted factorization machine: ``shard`` is an ``EmbeddingShard``
    with one vector of ``dim`` in {8, 16, 32} bf16 per key (models/fwfm.py), ``R`` the float32
    [F, F] field-pair strengths on the keys' device, read as symmetric from its upper triangle;
    margin = x.w + sum_{i<j} x_i x_j R[f_i][f_j] <v_i, v_j>, a key the model does not hold
    contributing nothing. The field arguments are ``ffm_score``'s: with ``row_ptr``, ``fields``
    is int32 [nnz], the field of every occurrence (one outside [0, F) keeps its linear term and
    enters no pair); with a fixed ``width`` it is the position -> field map (int32 [width] on
    the keys' device, or a list; None: identity).
    GPU: one ``fwfm_predict_rows`` launch (csrc/hip/fwfm_predict.hip), rows of any width; CPU:
    the PyTorch ops of ``FwFMTrainer.predict`` in f32 (``fwfm_forward_csr``, and
    ``fwfm_forward`` for a fixed width: on one map the same model, summed as the trainer's
    fixed-width route sums it, so a scorer and its trainer agree to the bit)."""
    if (row_ptr is None) == (not width):
        raise ValueError("fwfm_score needs row_ptr or a fixed width, not both")
    if acc is not None and labels is None:
        raise ValueError("fwfm_score: an accumulator needs labels")
    F = int(num_fields)
    if not 1 <= F <= 64 or shard.dim not in (8, 16, 32):
        raise ValueError(f"fwfm_score: {F} fields (1..64) on rows of {shard.dim} columns "
                         "(8, 16 or 32)")
    if not isinstance(R, torch.Tensor) or R.dtype != torch.float32 or tuple(R.shape) != (F, F) \
            or not R.is_contiguous():
        raise ValueError(f"fwfm_score: R must be a contiguous float32 [{F}, {F}] tensor")
    keys = keys.contiguous()
    nnz = keys.numel()
    dev = keys.device
    if R.device.type != dev.type:
        raise ValueError(f"fwfm_score: R must be on the keys' device ({dev})")
    if row_ptr is not None:
        if fields is None or not isinstance(fields, torch.Tensor) or \
                fields.dtype != torch.int32 or fields.numel() != nnz:
            raise ValueError(f"fwfm_score: rows by row_ptr need fields, int32 [{nnz}]")
    elif fields is None:
        if int(width) > F:
            raise ValueError(f"fwfm_score: rows of {int(width)} positions on {F} fields need a "
                             "position -> field map")
    else:
        if not isinstance(fields, torch.Tensor):
            fields = torch.tensor([int(f) for f in fields], dtype=torch.int32, device=dev)
        if fields.dtype != torch.int32 or fields.numel() != int(width):
            raise ValueError(f"fwfm_score: the position -> field map must be int32 [{int(width)}]")
    if fields is not None and fields.device.type != dev.type:
        raise ValueError(f"fwfm_score: fields must be on the keys' device ({dev})")
    if B is None:
        B = row_ptr.numel() - 1 if row_ptr is not None else nnz // int(width)
    L = loss_id(loss)
    table = shard.table
    if is_gpu(keys):
        m = torch.empty(B, dtype=torch.float32, device=dev) if margins else None
        if B:
            csr = row_ptr is not None
            hipops().fwfm_predict_rows(table.slots, table.home_base, table.home_m, shard.rows,
                                       keys, bits, F, R, row_ptr, int(width or 0),
                                       fields if csr else None, None if csr else fields, vals,
                                       labels, B, L, m, acc.metrics if acc is not None else None,
                                       acc.hist if acc is not None else None, AUC_BINS)
        return m
    if B == 0:
        return torch.empty(0, dtype=torch.float32) if margins else None
    slot, w = table.resolve(mix(keys, bits), insert=False)
    ok = slot >= 0
    w = torch.where(ok, w, torch.zeros_like(w))
    X0 = torch.zeros(nnz, shard.dim, device=dev)
    X0[ok] = shard.rows[slot[ok]].float()
    if row_ptr is not None:
        r = torch.repeat_interleave(torch.arange(B), row_ptr[1:B + 1] - row_ptr[:B])
        n = r.numel()
        m = fwfm_forward_csr(X0[:n], vals, r, fields, B, F, R, torch.arange(n), w,
                             torch.float32)[0]
    else:
        S = int(width)
        fl = torch.arange(S) if fields is None else fields.long()
        if int(fl.min()) < 0 or int(fl.max()) >= F:
            raise ValueError(f"fwfm_score: every field of the position map must lie in [0, {F})")
        m = fwfm_forward(X0, vals, B, S, fl, F, R, torch.arange(B * S), w, torch.float32)[0]
    if acc is not None:
        _accumulate(acc, m, labels, B, L)
    return m if margins else None


def row_bound(keys: torch.Tensor, w_of: dict, vals=None, row_ptr=None, width=None):
    """fp64 reference margins by a dictionary loop over the raw keys (no mixing, no table)
    and the derived f32 bound per row, (n_r + 2) 2^-23 sum |w x|: n_r products rounded once
    each and at most n_r - 1 f32 additions in any order. Returns (m_ref, bound), float64."""
    k = keys.tolist()
    x = vals.double().tolist() if vals is not None else None
    if row_ptr is not None:
        rp = row_ptr.tolist()
    else:
        rp = list(range(0, len(k) + 1, int(width)))
    m, bd = [], []
    for r in range(len(rp) - 1):
        s = a = 0.0
        for i in range(rp[r], rp[r + 1]):
            t = float(w_of.get(k[i], 0.0)) * (x[i] if x is not None else 1.0)
            s += t
            a += abs(t)
        m.append(s)
        bd.append((rp[r + 1] - rp[r] + 2) * 2.0 ** -23 * a)
    return torch.tensor(m, dtype=torch.float64), torch.tensor(bd, dtype=torch.float64)
