"""Scoring a factorization machine (ops/score.py ``fm_score``, models/scorer.py ``FMScorer``):
the CPU path, and the case builder / check that tests/test_fm_score_gpu.py runs again on the
fused kernel (csrc/hip/fm_predict.hip).

Reference: float64 margins from the model's raw (keys, w, bf16 rows) by sort + searchsorted
(``fm_ref``: no mixing, no table). Bound per row, derived not measured:
(2 n_r + D + 8) 2^-23 A_r, A_r = sum |w x| + 1/2 sum_f (sum_i |x v_if|)^2 + 1/2 sum x^2 v^2:
every product rounded once, at most n_r additions per s_f in any order, the square doubles
the relative error of s_f, then D additions; unit round-off is 2^-24, so a factor 2 to spare.
``test_cpu_path_within_bound`` shows that the fp32 PyTorch path stays inside this bound, and
inside the loss / histogram caps, for every case and seed the GPU test uses."""
import functools
import itertools
from types import SimpleNamespace

import pytest
import torch

from parameter_server_amd.models import FMConfig, FMScorer, FMTrainer
from parameter_server_amd.ops.embedding import EmbeddingShard
from parameter_server_amd.ops.keymix import mix
from parameter_server_amd.ops.linear import AUC_BINS
from parameter_server_amd.ops.score import ScoreAccum, fm_score
from parameter_server_amd.ops.synthetic import criteo_batch, drop_slots

CASES = list(itertools.product([8, 24, 32, 64, 128], [16, 32, 64], [(20, True), (40, False)]))
B, N_MODEL, N_ABSENT = 101, 700, 100


def fm_ref(mk, mw, mrows, keys, vals, row_ptr):
    """(float64 margins, bound per row) of CSR rows of raw ``keys`` against the model's raw
    keys ``mk``, weights ``mw`` and rows ``mrows`` as stored; an absent key contributes 0."""
    sk, order = torch.sort(mk)
    pos = torch.searchsorted(sk, keys).clamp(max=sk.numel() - 1)
    hit, src = sk[pos] == keys, order[pos]
    x = vals.double() if vals is not None else torch.ones(keys.numel(), dtype=torch.float64)
    w = torch.where(hit, mw.double()[src], 0.0) * x
    xv = torch.where(hit[:, None], mrows.double()[src], 0.0) * x[:, None]
    n = row_ptr[1:] - row_ptr[:-1]
    r = torch.repeat_interleave(torch.arange(n.numel()), n)

    def seg(t):
        return torch.zeros((n.numel(),) + t.shape[1:], dtype=torch.float64).index_add_(0, r, t)

    s, q = seg(xv), seg((xv * xv).sum(1))
    A = seg(w.abs()) + 0.5 * (seg(xv.abs()) ** 2).sum(1) + 0.5 * q
    return seg(w) + 0.5 * ((s * s).sum(1) - q), (2 * n + mrows.shape[1] + 8) * 2.0 ** -23 * A


@functools.lru_cache(maxsize=None)
def make_case(D, L, bits, valued):
    """700 model keys and one minibatch of 101 rows (CPU tensors) with its float64 reference:
    every width around the sub-round (L / C positions) and the round (L), one occurrence in
    ten a key the model does not hold, one row with the same key twice."""
    g = torch.Generator().manual_seed(1000 + D + L + bits)
    C = 1 << max(0, (D // 8 - 1).bit_length())
    k = torch.unique(torch.randint(0, 1 << bits, (4000,), generator=g))
    k = k[torch.randperm(k.numel(), generator=g)]
    c = SimpleNamespace(D=D, L=L, bits=bits, mk=k[:N_MODEL], absent=k[N_MODEL:N_MODEL + N_ABSENT])
    c.mrows = (torch.randn(N_MODEL, D, generator=g) * 0.3).to(torch.bfloat16)
    c.mw = torch.randn(N_MODEL, generator=g) * 0.1
    widths = ([0, 1, L // C - 1, L // C, L // C + 1, L - 1, L, L + 1, 2 * L + 1, 130] * 11)[:B]
    c.row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(widths).cumsum(0)])
    nnz = int(c.row_ptr[-1])
    c.keys = c.mk[torch.randint(0, N_MODEL, (nnz,), generator=g)]
    gone = torch.rand(nnz, generator=g) < 0.1
    c.keys[gone] = c.absent[torch.randint(0, N_ABSENT, (int(gone.sum()),), generator=g)]
    c.keys[c.row_ptr[9]:c.row_ptr[9] + 2] = c.mk[0]  # (row 9 is 130 wide)
    c.vals = torch.rand(nnz, generator=g) + 0.5 if valued else None
    c.y = torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0)
    c.m, c.bound = fm_ref(c.mk, c.mw, c.mrows, c.keys, c.vals, c.row_ptr)
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


def check_case(device, D, L, bits, valued):
    c = make_case(D, L, bits, valued)
    to = lambda t: None if t is None else t.to(device)
    acc = ScoreAccum(device)
    m = fm_score(load_shard(c, device), to(c.keys), bits, row_ptr=to(c.row_ptr), vals=to(c.vals),
                 labels=to(c.y), acc=acc, lanes=L)
    err = (m.cpu().double() - c.m).abs()
    print(f"max |m - m64| / bound = {float((err / c.bound.clamp(min=1e-300)).max()):.3g}")
    assert bool((err <= c.bound).all())
    sums = acc.sums().cpu()
    assert float(sums[2]) == B
    assert abs(float(sums[0]) - c.loss) <= 1e-3 * B
    assert int((acc.counts().cpu() - c.hist).abs().sum()) <= 4


@pytest.mark.parametrize("D,L,kind", CASES)
def test_cpu_path_within_bound(D, L, kind):
    check_case("cpu", D, L, *kind)


CFG = dict(num_features=1 << 20, embedding_dim=16, minibatch=256, table_capacity=1 << 14)


def held_out(B=256):
    """Rows after the ones the tests train on (the generator's seed 3), slots missing."""
    k, y = criteo_batch(B, seed=3, row0=10 * B, num_features=CFG["num_features"],
                        cards=[300] * 26)
    return (*drop_slots(k, B, keep=0.8, seed=5), y)


def test_fm_scorer_is_the_cpu_predict():
    tr = FMTrainer(FMConfig(**CFG))
    for s in range(2):
        tr.step(*criteo_batch(256, seed=3, row0=s * 256, num_features=CFG["num_features"],
                              cards=[300] * 26))
    k, rp, v, y = held_out()
    sc = tr.scorer()
    m = sc.score(k, y, row_ptr=rp, vals=v)
    assert torch.equal(m, tr.predict(k, 256, vals=v, row_ptr=rp))
    assert torch.equal(sc.predict(k[:39 * 100], width=39), tr.predict(k[:39 * 100], 100))
    r = sc.result()
    want = float(torch.nn.functional.softplus(-torch.where(y > 0, 1.0, -1.0) * m.double()).mean())
    assert r["examples"] == 256 and abs(r["loss"] - want) < 1e-12


def test_scorer_needs_one_rank():
    tr = FMTrainer(FMConfig(**CFG), comm=SimpleNamespace(world=2, rank=0))
    with pytest.raises(NotImplementedError, match="from_state_dict"):
        tr.scorer()
    with pytest.raises(ValueError, match="not an FMTrainer"):
        FMScorer.from_state_dict({"model": "WideDeepTrainer"}, "cpu")
