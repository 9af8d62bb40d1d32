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
