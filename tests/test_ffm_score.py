"""Scoring a field-aware factorization machine (ops/score.py ``ffm_score``, models/scorer.py
``FFMScorer``): the CPU path, and the case builder / check that tests/test_ffm_score_gpu.py
runs again on the fused kernel (csrc/hip/ffm_predict.hip).

Reference: float64 margins from the model's raw (keys, w, bf16 rows) by sort + searchsorted
(no mixing, no table), the pair sum from its definition, a padded [B, W, W] gather over i < j:
NOT the field-sum identity the kernel rests on, so the identity is checked as well. Bound per
row, derived not measured: (2 n_r + k F (F + 1) / 2 + 8) 2^-23 Abs_r, Abs_r = sum |w x| +
1/2 sum_{f,g,e} |A|[f][g][e] |A|[g][f][e] + 1/2 sum_i x_i^2 |v_{i,f_i}|^2 with |A| built from
absolute values: every product rounded once, at most n_r additions per cell, the product of
two cells doubles that, then k F (F + 1) / 2 + 2 n_r terms in any order; unit round-off is
2^-24, so a factor 2 to spare."""
import functools
import itertools
from types import SimpleNamespace

import pytest
import torch

from parameter_server_amd.models import FFMConfig, FFMScorer, FFMTrainer
from parameter_server_amd.ops.embedding import EmbeddingShard
from parameter_server_amd.ops.keymix import mix
from parameter_server_amd.ops.linear import AUC_BINS
from parameter_server_amd.ops.score import ScoreAccum, ffm_score
from parameter_server_amd.ops.synthetic import criteo_batch, drop_slots

CASES = list(itertools.product([(3, 2), (8, 8), (13, 4), (39, 2), (64, 2)],
                               [(20, False), (40, True)]))
B, N_MODEL, N_ABSENT = 101, 700, 100


def ffm_ref(mk, mw, mrows, keys, vals, row_ptr, fld, F, k):
    """(float64 margins, bound per row) of CSR rows of raw ``keys`` with fields ``fld`` against
    the model's raw keys ``mk``, weights ``mw`` and rows ``mrows`` as stored."""
    sk, order = torch.sort(mk)
    pos = torch.searchsorted(sk, keys).clamp(max=sk.numel() - 1)
    hit, src = sk[pos] == keys, order[pos]
    x = vals.double() if vals is not None else torch.ones(keys.numel(), dtype=torch.float64)
    w = torch.where(hit, mw.double()[src], 0.0) * x
    f = fld.long()
    ok = hit & (f >= 0) & (f < F)
    f = torch.where(ok, f, 0)
    V = torch.where(ok[:, None], mrows.double()[src, :F * k], 0.0).reshape(-1, F, k)
    xm = x * ok
    n = row_ptr[1:] - row_ptr[:-1]
    nb, W = n.numel(), max(int(n.max()), 1)
    r = torch.repeat_interleave(torch.arange(nb), n)
    col = torch.arange(r.numel()) - row_ptr[:-1][r]

    def seg(t, idx=r, rows=nb):
        return torch.zeros((rows,) + t.shape[1:], dtype=torch.float64).index_add_(0, idx, t)

    Vp = torch.zeros(nb, W, F, k, dtype=torch.float64)
    xp, fp = torch.zeros(nb, W, dtype=torch.float64), torch.zeros(nb, W, dtype=torch.long)
    Vp[r, col], xp[r, col], fp[r, col] = V, xm, f
    upper = torch.triu(torch.ones(W, W, dtype=torch.float64), 1)
    pair = torch.zeros(nb, dtype=torch.float64)
    for b in range(nb):  # <v_{i,f_j}, v_{j,f_i}> over i < j, a row at a time
        vi = Vp[b][:, fp[b]]  # [i, j, k] = v_{i, f_j}
        pair[b] = ((vi * vi.transpose(0, 1)).sum(2) * upper * xp[b][:, None] * xp[b][None]).sum()
    own = V[torch.arange(r.numel()), f]
    absA = seg((xm[:, None, None] * V).abs(), r * F + f, nb * F).reshape(nb, F, F, k)
    A = seg(w.abs()) + 0.5 * (absA * absA.transpose(1, 2)).sum((1, 2, 3)) + \
        0.5 * seg(xm * xm * (own * own).sum(1))
    return seg(w) + pair, (2 * n + k * F * (F + 1) // 2 + 8) * 2.0 ** -23 * A


@functools.lru_cache(maxsize=None)
def make_case(F, k, bits, valued):
    """700 model keys and one minibatch of 101 rows (CPU tensors) with its float64 reference:
    widths around the round of 64, fields drawn at random (some repeat in a row, some are
    missing), one occurrence in ten a key the model lacks, one in twenty with field -1 or F,
    one row with the same key twice in one field."""
    g = torch.Generator().manual_seed(2000 + 64 * F + k + bits)
    Dr = (F * k + 7) // 8 * 8
    keys = torch.unique(torch.randint(0, 1 << bits, (4000,), generator=g))
    keys = keys[torch.randperm(keys.numel(), generator=g)]
    c = SimpleNamespace(F=F, k=k, Dr=Dr, bits=bits, mk=keys[:N_MODEL],
                        absent=keys[N_MODEL:N_MODEL + N_ABSENT])
    c.mrows = (torch.randn(N_MODEL, Dr, generator=g) * 0.3).to(torch.bfloat16)
    c.mw = torch.randn(N_MODEL, generator=g) * 0.1
    widths = ([0, 1, 2, 63, 64, 65, 130] * 15)[:B]
    c.row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(widths).cumsum(0)])
    nnz = int(c.row_ptr[-1])
    c.keys = c.mk[torch.randint(0, N_MODEL, (nnz,), generator=g)]
    gone = torch.rand(nnz, generator=g) < 0.1
    c.keys[gone] = c.absent[torch.randint(0, N_ABSENT, (int(gone.sum()),), generator=g)]
    c.fld = torch.randint(0, F, (nnz,), generator=g, dtype=torch.int32)
    out = torch.rand(nnz, generator=g) < 0.05
    c.fld[out] = torch.where(torch.rand(int(out.sum()), generator=g) < 0.5, -1, F).int()
    c.keys[c.row_ptr[6]:c.row_ptr[6] + 2] = c.mk[0]  # (row 6 is 130 wide)
    c.fld[c.row_ptr[6]:c.row_ptr[6] + 2] = F - 1
    c.vals = torch.rand(nnz, generator=g) + 0.5 if valued else None
    c.y = torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0)
    c.m, c.bound = ffm_ref(c.mk, c.mw, c.mrows, c.keys, c.vals, c.row_ptr, c.fld, F, k)
    c.loss = float(torch.nn.functional.softplus(-c.y.double() * c.m).sum())
    b = torch.clamp((torch.sigmoid(c.m) * AUC_BINS).long(), 0, AUC_BINS - 1)
    c.hist = torch.bincount(b + torch.where(c.y > 0, AUC_BINS, 0), minlength=2 * AUC_BINS)
    return c


def load_shard(c, device):
    """The case's model in a 1024-slot table: load 0.68, so probe chains are walked."""
    shard = EmbeddingShard(1024, c.Dr, device)
    z = torch.zeros(N_MODEL)
    shard.load_state(mix(c.mk, c.bits), c.mw, z, z, c.mrows, z)
    return shard


def within(m, ref, bound, scale=1.0):
    err = (m.cpu().double() - ref).abs()
    print(f"max |m - m64| / bound = {float((err / bound.clamp(min=1e-300)).max()):.3g}")
    return bool((err <= scale * bound).all())


def check_case(device, F, k, bits, valued):
    c = make_case(F, k, bits, valued)
    to = lambda t: None if t is None else t.to(device)
    acc = ScoreAccum(device)
    m = ffm_score(load_shard(c, device), to(c.keys), bits, num_fields=F, k=k,
                  row_ptr=to(c.row_ptr), fields=to(c.fld), vals=to(c.vals), labels=to(c.y), acc=acc)
    assert within(m, c.m, c.bound)
    sums = acc.sums().cpu()
    assert float(sums[2]) == B
    assert abs(float(sums[0]) - c.loss) <= 1e-3 * B
    assert int((acc.counts().cpu() - c.hist).abs().sum()) <= 4


@pytest.mark.parametrize("Fk,kind", CASES)
def test_cpu_path_within_bound(Fk, kind):
    check_case("cpu", *Fk, *kind)


CFG = dict(num_features=1 << 20, k=4, fields=[0] * 13 + list(range(1, 27)), minibatch=256,
           table_capacity=1 << 14)


def held_out(n=256):
    """Rows after the ones the tests train on, slots missing, a random field per occurrence."""
    k, y = criteo_batch(n, seed=3, row0=10 * n, num_features=CFG["num_features"], cards=[300] * 26)
    k, rp, v = drop_slots(k, n, keep=0.8, seed=5)
    fld = torch.randint(-1, 28, (k.numel(),), generator=torch.Generator().manual_seed(7))
    return k, rp, v, fld.int(), y


def train(device, steps):
    tr = FFMTrainer(FFMConfig(**CFG), device=device)
    for s in range(steps):
        tr.step(*criteo_batch(256, seed=3, row0=s * 256, num_features=CFG["num_features"],
                              cards=[300] * 26, device=device))
    return tr


def test_ffm_scorer_is_the_cpu_predict():
    tr = train("cpu", 2)
    k, rp, v, fld, y = held_out()
    sc = tr.scorer()
    m = sc.score(k, y, row_ptr=rp, vals=v, fields=fld)
    assert torch.equal(m, tr.predict(k, 256, vals=v, row_ptr=rp, fields=fld))
    k39 = criteo_batch(100, seed=3, row0=5000, num_features=CFG["num_features"], cards=[300] * 26)[0]
    assert torch.equal(sc.predict(k39, width=39), tr.predict(k39, 100))
    assert sc.result()["examples"] == 256 and float(m.abs().max()) > 0


def test_scorer_needs_one_rank_and_an_ffm_snapshot():
    tr = FFMTrainer(FFMConfig(**CFG), comm=SimpleNamespace(world=2, rank=0))
    with pytest.raises(NotImplementedError, match="from_state_dict"):
        tr.scorer()
    with pytest.raises(ValueError, match="not an FFMTrainer"):
        FFMScorer.from_state_dict({"model": "FMTrainer"}, "cpu", 27, 4)
