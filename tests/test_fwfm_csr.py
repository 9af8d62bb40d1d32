"""FwFM on CSR rows (models/fwfm.py) on the CPU: the CSR step against the fixed-width step, the
checked errors, and test_fwfm_csr_gpu.py's cases with the facts its tolerances rest on."""
import functools
import itertools

import pytest
import torch

from parameter_server_amd.models import FwFMConfig, FwFMTrainer
from parameter_server_amd.ops.synthetic import criteo_batch

CFG = dict(num_features=1 << 21, embedding_dim=8, minibatch=256, table_capacity=1 << 15,
           emb_lr=0.05, lambda_v=0.5)
U, NR = 200, 300
# (F, D, widths of the first rows, widest random row after them, B, dR partials = blocks,
# factor scale). Widths 0, 1, 2 (equal fields: only the diagonal acts; different fields) and
# the round boundaries; B = 37 is odd; the scale keeps the float64 margins' deviation in 0.9..3.
SHAPES = [
    (1, 8, [0, 1, 2, 2, 5, 64, 65], 8, 37, 5, 0.21),       # every position in one field
    (4, 8, [0, 1, 2, 2, 63, 130], 12, 37, 5, 0.07),        # D = 8: half an MFMA N-tile
    (17, 16, [0, 2, 2, 63, 64, 65], 40, 37, 5, 0.14),      # one field past a 16-tile
    (39, 16, [0, 1, 2, 2, 63, 64, 65, 128, 129, 200], 60, 37, 5, 0.09),  # pads to 48, K = 39
    (64, 32, [2, 2, 64, 65, 129, 200], 64, 37, 5, 0.063),  # the most accumulators, one wave
    (39, 16, [70], 1, 1, 3, 0.2),     # idle waves and blocks write zeros
    (39, 16, [100, 0], 50, 1031, 7, 0.17),  # every wave accumulates many rows
]
# dR: the largest error of the fp32 PyTorch form against float64 over these cases, relative to
# max |dR| (measured, asserted below); the kernel's other sum order gets 8 times that.
DR_F32_ERR = 5.4e-7  # 5.32e-7, at (39, 16) binary without idx
GRID = [(s, v, i) for s in range(5) for v, i in itertools.product([True, False], repeat=2)] + \
       [(5, True, True), (6, False, False)]


@functools.lru_cache(maxsize=None)
def case(shape, valued, with_idx):  # inputs (CPU) and the float64 reference, built once
    F, D, special, wmax, B, _, scale = SHAPES[shape]
    cfg = FwFMConfig(num_features=1 << 20, slots=64, fields=[0] * 64, num_fields=F,
                     embedding_dim=D, minibatch=B, table_capacity=1024)
    ref = FwFMTrainer(cfg)
    g = torch.Generator().manual_seed(500 + 4 * shape + 2 * valued + with_idx)
    width = torch.cat([torch.tensor(special),
                       torch.randint(1, wmax + 1, (B - len(special),), generator=g)])
    rp = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(width, 0)])
    nnz = int(rp[-1])
    row_of = torch.repeat_interleave(torch.arange(B), width)
    fld = torch.randint(0, F, (nnz,), generator=g, dtype=torch.int32)  # scrambled, repeated
    fld[3::17], fld[5::23], fld[7::29] = -1, F, 1000  # out of range: a linear term, no pair
    for k, b in enumerate((width == 2).nonzero().flatten().tolist()):
        fld[rp[b]], fld[rp[b] + 1] = 0, (0 if k % 2 == 0 else F - 1)
    rows = (torch.randn(NR, D, generator=g) * scale).to(torch.bfloat16)
    idx = torch.randint(0, NR, (U,), generator=g)
    idx[::50] = -1
    idx = idx if with_idx else None
    w = torch.randn(U, generator=g) * 1.3 / float(width.float().mean()) ** 0.5
    lc = torch.randint(0, U, (nnz,), generator=g, dtype=torch.int32)
    lc[rp[1:][width >= 2] - 1] = lc[rp[:-1][width >= 2]]  # a key twice in a row
    vals = torch.rand(nnz, generator=g) + 0.5 if valued else None
    y = torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0)
    R = torch.rand(F, F, generator=g) * 2 - 0.5  # [-0.5, 1.5) with exact zeros
    R[torch.rand(F, F, generator=g) < 0.15] = 0
    R = torch.triu(R) + torch.triu(R, 1).T
    r = idx[lc.long()] if with_idx else lc.long()
    X0 = torch.where((r >= 0)[:, None], rows[r.clamp(min=0)], torch.zeros((), dtype=rows.dtype))
    ref.R.copy_(R)
    m, coef, dX, dR = ref._fwd_bwd_math_csr(X0, vals, row_of, fld, lc, w, y, dtype=torch.float64)
    dX0 = ref._account(m, coef, dX, y, B)
    f32 = FwFMTrainer(cfg)
    f32.R.copy_(R)
    dR32 = f32._fwd_bwd_torch_csr(X0, vals, row_of, fld, lc, w, y)[1]
    dr_max = float(dR.abs().max())
    return dict(tr=ref, rp=rp, row_of=row_of.int(), fld=fld, rows=rows, idx=idx, w=w, lc=lc,
                vals=vals, y=y, R=R, dX0=dX0, dR=dR, coef=ref.coef[:B].clone(),
                loss=float(ref.metrics[0]), hist=ref.hist.clone(), hist32=f32.hist.clone(),
                dr_max=dr_max, m_std=float(m.std()) if B > 1 else None,
                f32_err=float((dR32.double() - dR).abs().max()) / dr_max)


def test_cases_hold_what_the_bounds_rest_on():
    # dR's fp32 error, margins neither flat nor saturated, the fp32 form in the float64 bins
    cases = [case(*c) for c in GRID]
    assert max(c["f32_err"] for c in cases) <= DR_F32_ERR
    assert all(0.9 <= c["m_std"] <= 3.0 for c in cases if c["m_std"] is not None)
    assert all(torch.equal(c["hist32"], c["hist"]) for c in cases)


def test_csr_step_on_full_rows_equals_the_fixed_width_step():
    fields = [0] * 14 + list(range(1, 26))  # a 14-position field: the diagonal trains
    a, b = (FwFMTrainer(FwFMConfig(**dict(CFG, fields=fields))) for _ in range(2))
    rp = torch.arange(257) * 39
    fl = torch.tensor(fields, dtype=torch.int32).repeat(256)
    for s in range(3):
        k, l = criteo_batch(256, seed=5, row0=s * 256, num_features=1 << 20, cards=[300] * 26)
        a.step(k, l)
        b.step(k, l, row_ptr=rp, fields=fl)
    sa, sb = a.state_dict(), b.state_dict()
    assert torch.equal(sa["keys"], sb["keys"])  # then: the same sums in another order, in fp32
    torch.testing.assert_close(sa["rows"].float(), sb["rows"].float(), rtol=2 ** -7, atol=1e-5)
    torch.testing.assert_close(sa["w"], sb["w"], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(a.R, b.R, rtol=1e-4, atol=1e-6)
    assert float(a.R[0, 0]) != 1 and abs(a.progress()["loss"] - b.progress()["loss"]) < 1e-5
    k, _ = criteo_batch(256, seed=5, row0=1 << 20, num_features=1 << 20, cards=[300] * 26)
    torch.testing.assert_close(b.predict(k, 256, row_ptr=rp, fields=fl), a.predict(k, 256),
                               rtol=1e-4, atol=1e-5)


RP, FL = torch.arange(5) * 2, torch.zeros(8, dtype=torch.int32)


@pytest.mark.parametrize("bad", [
    dict(row_ptr=RP[:4]), dict(row_ptr=RP.int()), dict(fields=FL[:7]), dict(fields=FL.long()),
    dict(vals=torch.ones(7)), dict(row_ptr=None), dict(fields=None),
    dict(keys=torch.arange(80), fields=torch.zeros(80, dtype=torch.int32)),  # nnz > max_nnz
    dict(labels=torch.ones(9), row_ptr=torch.arange(10))])                   # B > minibatch
def test_csr_errors(bad):
    tr = FwFMTrainer(FwFMConfig(**dict(CFG, slots=4, minibatch=8)))
    kw = dict(dict(keys=torch.arange(8), labels=torch.ones(4), row_ptr=RP, fields=FL), **bad)
    with pytest.raises(ValueError):
        tr.step(kw.pop("keys"), kw.pop("labels"), **kw)
    if "labels" not in bad and "keys" not in bad:
        kw = dict(dict(row_ptr=RP, fields=FL), **bad)
        with pytest.raises(ValueError):
            tr.predict(torch.arange(8), 4, **kw)
