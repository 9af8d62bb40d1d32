"""Scoring a field-weighted factorization machine (ops/score.py ``fwfm_score``,
models/scorer.py ``FwFMScorer``): the CPU path, and the case builder / check that
tests/test_fwfm_score_gpu.py runs again on the fused kernel (csrc/hip/fwfm_predict.hip).

Reference: float64 margins from the model's raw (keys, w, bf16 rows) and R by sort +
searchsorted (no mixing, no table), the pair sum from its definition, sum_{i<j} x_i x_j
R[min(f_i, f_j)][max(f_i, f_j)] <v_i, v_j> over a padded [B, W, W] gather: NOT the field-sum /
Gram identity the kernel rests on, so the identity is checked as well.

Bound per row, derived not measured: (9 n_r + D + F (F + 1) / 2 + 8) 2^-23 Abs_r with
Abs_r = sum |w x| + sum_{f<g} |R[f][g]| <|P|[f], |P|[g]> + sum_{f: n_f >= 2} |R[f][f]| |s|_f,
|P| and |s| built from absolute values. In units of round-off on the term's absolute value:
every product is rounded once; a cell of P is a rounded x v plus at most n_r additions
(n_r + 1), so a Gram entry <P[f], P[g]> carries twice that, its own product and D additions,
and the product with R: 2 n_r + D + 4; a share of s_f is a chain of at most 8 n_f fused steps
(8 n_f) whose factors are a rounded x v and a cell of at most n_f additions (n_f + 2), then
the C <= 4 shares are added and multiplied by R[f][f]: at most 9 n_r + 8; a linear term is one
product. At most F (F + 1) / 2 + n_r such terms are then added in any order. No term carries
more than 9 n_r + D + 8 and the final sum adds at most F (F + 1) / 2 + n_r more, all within
2 (9 n_r + D + F (F + 1) / 2 + 8) units at Abs_r: the unit round-off is 2^-24, which is the
2^-23 of the bound with a factor of about 2 to spare where the terms are Gram entries."""
import functools
import itertools
from types import SimpleNamespace

import pytest
import torch

from parameter_server_amd.models import FwFMConfig, FwFMScorer, FwFMTrainer
from parameter_server_amd.ops.embedding import EmbeddingShard
from parameter_server_amd.ops.keymix import mix
from parameter_server_amd.ops.linear import AUC_BINS
from parameter_server_amd.ops.score import ScoreAccum, fwfm_score
from parameter_server_amd.ops.synthetic import criteo_batch, drop_slots

CASES = list(itertools.product([(3, 8), (16, 16), (17, 16), (39, 16), (64, 32)],
                               [(20, False), (40, True)]))
B, N_MODEL, N_ABSENT = 101, 700, 100


def fwfm_ref(mk, mw, mrows, R, keys, vals, row_ptr, fld):
    """(float64 margins, bound per row) of CSR rows of raw ``keys`` with fields ``fld`` against
    the model's raw keys ``mk``, weights ``mw``, rows ``mrows`` as stored and ``R`` [F, F]."""
    F, D = R.shape[0], mrows.shape[1]
    sk, order = torch.sort(mk)
    pos = torch.searchsorted(sk, keys).clamp(max=sk.numel() - 1)
    hit, src = sk[pos] == keys, order[pos]
    x = vals.double() if vals is not None else torch.ones(keys.numel(), dtype=torch.float64)
    w = torch.where(hit, mw.double()[src], 0.0) * x
    f = fld.long()
    ok = hit & (f >= 0) & (f < F)
    f = torch.where(ok, f, 0)
    xv = torch.where(ok[:, None], mrows.double()[src], 0.0) * x[:, None]
    n = row_ptr[1:] - row_ptr[:-1]
    nb, W = n.numel(), max(int(n.max()), 1)
    r = torch.repeat_interleave(torch.arange(nb), n)
    col = torch.arange(r.numel()) - row_ptr[:-1][r]

    def seg(t, idx=r, rows=nb):
        return torch.zeros((rows,) + t.shape[1:], dtype=torch.float64).index_add_(0, idx, t)

    Vp, fp = torch.zeros(nb, W, D, dtype=torch.float64), torch.zeros(nb, W, dtype=torch.long)
    Vp[r, col], fp[r, col] = xv, f
    Ru = torch.triu(R.double())  # read from the upper triangle, the diagonal included
    Rs = Ru + torch.triu(Ru, 1).T
    upper = torch.triu(torch.ones(W, W, dtype=torch.float64), 1)
    pair = (Vp @ Vp.transpose(1, 2) * Rs[fp[:, :, None], fp[:, None, :]] * upper).sum((1, 2))
    absP = seg(xv.abs(), r * F + f, nb * F).reshape(nb, F, D)
    gram = absP @ absP.transpose(1, 2)
    nf = seg(ok.double(), r * F + f, nb * F).reshape(nb, F)
    s_abs = 0.5 * (torch.diagonal(gram, dim1=1, dim2=2) -
                   seg((xv * xv).sum(1), r * F + f, nb * F).reshape(nb, F)).clamp(min=0)
    A = seg(w.abs()) + (gram * torch.triu(Ru, 1).abs()).sum((1, 2)) + \
        (torch.where(nf >= 2, s_abs, 0.0) * torch.diagonal(Ru).abs()).sum(1)
    return seg(w) + pair, (9 * n + D + F * (F + 1) // 2 + 8) * 2.0 ** -23 * A


@functools.lru_cache(maxsize=None)
def make_case(F, D, bits, valued):
    """700 model keys, R and one minibatch of 101 rows (CPU tensors) with its float64
    reference: widths around the round of 64, fields drawn at random (some repeat in a row,
    some are missing), one occurrence in ten a key the model lacks, one in twenty with field
    -1 or F, one row with the same key twice in one field. R is random with unrelated values
    below the diagonal and R[0][0] = 100; row 1 is one stored key on field 0 and row 2 two
    stored keys on fields 0 and F - 1 (F = 3: 0 and 2), where the diagonal must add exactly 0."""
    g = torch.Generator().manual_seed(3000 + 64 * F + D + bits)
    keys = torch.unique(torch.randint(0, 1 << bits, (4000,), generator=g))
    keys = keys[torch.randperm(keys.numel(), generator=g)]
    c = SimpleNamespace(F=F, D=D, bits=bits, mk=keys[:N_MODEL],
                        absent=keys[N_MODEL:N_MODEL + N_ABSENT])
    c.mrows = (torch.randn(N_MODEL, D, generator=g) * 0.3).to(torch.bfloat16)
    c.mw = torch.randn(N_MODEL, generator=g) * 0.1
    c.R = torch.triu(torch.randn(F, F, generator=g)) + \
        torch.tril(torch.randn(F, F, generator=g) * 50, -1)
    c.R[0, 0] = 100.0
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
    c.keys[c.row_ptr[1]:c.row_ptr[3]] = c.mk[1:4]  # (rows 1 and 2: widths 1 and 2)
    c.fld[c.row_ptr[1]:c.row_ptr[3]] = torch.tensor([0, 0, F - 1], dtype=torch.int32)
    c.vals = torch.rand(nnz, generator=g) + 0.5 if valued else None
    c.y = torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0)
    c.m, c.bound = fwfm_ref(c.mk, c.mw, c.mrows, c.R, c.keys, c.vals, c.row_ptr, c.fld)
    c.loss = float(torch.nn.functional.softplus(-c.y.double() * c.m).sum())
    b = torch.clamp((torch.sigmoid(c.m) * AUC_BINS).long(), 0, AUC_BINS - 1)
    c.hist = torch.bincount(b + torch.where(c.y > 0, AUC_BINS, 0), minlength=2 * AUC_BINS)
    return c


def load_shard(c, device):
    """The case's model in a 1024-slot table: load 0.68, so probe chains are walked."""
    shard = EmbeddingShard(1024, c.D, device)
    z = torch.zeros(N_MODEL)
    shard.load_state(mix(c.mk, c.bits), c.mw, z, z, c.mrows, z)
    return shard


def within(m, ref, bound, scale=1.0):
    err = (m.cpu().double() - ref).abs()
    print(f"max |m - m64| / bound = {float((err / bound.clamp(min=1e-300)).max()):.3g}")
    return bool((err <= scale * bound).all())


def check_case(device, F, D, bits, valued):
    c = make_case(F, D, bits, valued)
    to = lambda t: None if t is None else t.to(device)
    acc = ScoreAccum(device)
    m = fwfm_score(load_shard(c, device), to(c.keys), bits, num_fields=F, R=to(c.R),
                   row_ptr=to(c.row_ptr), fields=to(c.fld), vals=to(c.vals), labels=to(c.y), acc=acc)
    assert within(m, c.m, c.bound)
    sums = acc.sums().cpu()
    assert float(sums[2]) == B
    assert abs(float(sums[0]) - c.loss) <= 1e-3 * B
    assert int((acc.counts().cpu() - c.hist).abs().sum()) <= 4


@pytest.mark.parametrize("FD,kind", CASES)
def test_cpu_path_within_bound(FD, kind):
    check_case("cpu", *FD, *kind)


CFG = dict(num_features=1 << 20, embedding_dim=16, fields=[0] * 13 + list(range(1, 27)),
           minibatch=256, table_capacity=1 << 14)


def held_out(n=256):
    """Rows after the ones the tests train on, slots missing, a random field per occurrence."""
    k, y = criteo_batch(n, seed=3, row0=10 * n, num_features=CFG["num_features"], cards=[300] * 26)
    k, rp, v = drop_slots(k, n, keep=0.8, seed=5)
    fld = torch.randint(-1, 28, (k.numel(),), generator=torch.Generator().manual_seed(7))
    return k, rp, v, fld.int(), y


def train(device, steps):
    tr = FwFMTrainer(FwFMConfig(**CFG), device=device)
    for s in range(steps):
        tr.step(*criteo_batch(256, seed=3, row0=s * 256, num_features=CFG["num_features"],
                              cards=[300] * 26, device=device))
    return tr


def test_fwfm_scorer_is_the_cpu_predict():
    tr = train("cpu", 2)
    k, rp, v, fld, y = held_out()
    sc = tr.scorer()
    assert sc.R is tr.R
    m = sc.score(k, y, row_ptr=rp, vals=v, fields=fld)
    assert torch.equal(m, tr.predict(k, 256, vals=v, row_ptr=rp, fields=fld))
    k39 = criteo_batch(100, seed=3, row0=5000, num_features=CFG["num_features"], cards=[300] * 26)[0]
    assert torch.equal(sc.predict(k39, width=39), tr.predict(k39, 100))
    assert sc.result()["examples"] == 256 and float(m.abs().max()) > 0


def test_scorer_needs_one_rank_and_an_fwfm_snapshot():
    tr = FwFMTrainer(FwFMConfig(**CFG), comm=SimpleNamespace(world=2, rank=0))
    with pytest.raises(NotImplementedError, match="from_state_dict"):
        tr.scorer()
    with pytest.raises(ValueError, match="not an FwFMTrainer"):
        FwFMScorer.from_state_dict({"model": "FMTrainer"}, "cpu")
