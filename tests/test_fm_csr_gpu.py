"""fm_csr (fm.hip: lane groups per row) and its forward-only form against the float64 CSR
PyTorch forward/backward of the same bf16 rows; the CSR trainer step, GPU against CPU."""
import functools
import itertools

import pytest
import torch

from parameter_server_amd.models.fm import FMConfig, FMTrainer
from parameter_server_amd.ops.linear import AUC_BINS, accum_total, new_accum
from parameter_server_amd.ops.native import hipops
from parameter_server_amd.ops.synthetic import criteo_batch, drop_slots

pytestmark = pytest.mark.gpu
CFG = dict(num_features=1 << 20, embedding_dim=16, minibatch=512, table_capacity=1 << 16,
           emb_lr=0.05, lambda_v=0.5)
# Every width around a group boundary, 25 times, and one row of 5,000 features in the
# middle: B = 301 rows (odd: no multiple of the 2 or 4 rows a wave holds).
WIDTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130] * 25
LONG, LONG_W = 150, 5000
WIDTHS.insert(LONG, LONG_W)
B, U, R = len(WIDTHS), 700, 900
# The long row has 5,000 columns of its own (U .. U + 5000) whose factor rows and wide
# weights are scaled by 0.02 and 0.015 (row values 0.006, not 0.3): at 0.3 its margin has a
# spread of ~2000 and the sigmoid saturates; so scaled, its margin is of order 1.
# The kernel sums that row in another order than torch. The fp32 torch reference itself lies
# 6.0e-8 .. 3.3e-7 from the float64 one on that row's coef (measured on the CPU, D in {8, 16,
# 32}, valued and binary; up to 4.7e-6 over all rows). Four times the largest is below the
# project's own atol for coef, which therefore holds for the long row too.
COEF_TOL = dict(rtol=1e-4, atol=max(1e-5, 4 * 3.3e-7))


@functools.lru_cache(maxsize=None)
def _case(D, valued):  # inputs (CPU) and the float64 reference of one case, built once
    g = torch.Generator().manual_seed(100 + D + valued)
    rows = torch.randn(R + LONG_W, D, generator=g) * 0.3
    rows[R:] *= 0.02
    rows = rows.to(torch.bfloat16)
    idx = torch.cat([torch.randint(0, R, (U,), generator=g), R + torch.arange(LONG_W)])
    idx[::50] = -1
    w = torch.randn(U + LONG_W, generator=g) * 0.1
    w[U:] *= 0.015
    row_ptr = torch.zeros(B + 1, dtype=torch.int64)
    row_ptr[1:] = torch.tensor(WIDTHS).cumsum(0)
    nnz = int(row_ptr[-1])
    lc = torch.randint(0, U, (nnz,), generator=g, dtype=torch.int32)
    lc[row_ptr[LONG]:row_ptr[LONG + 1]] = U + torch.arange(LONG_W, dtype=torch.int32)
    vals = torch.rand(nnz, generator=g) + 0.5 if valued else None
    y = torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0)
    row_of = torch.arange(B).repeat_interleave(torch.tensor(WIDTHS))
    r = idx[lc.long()]
    X0 = torch.where((r >= 0)[:, None], rows[r.clamp(min=0)], torch.zeros((), dtype=rows.dtype))
    ref = FMTrainer(FMConfig(**dict(CFG, embedding_dim=D, minibatch=B)))
    dref = ref._fwd_bwd_torch_csr(X0, vals, row_of, lc, w, y, dtype=torch.float64)
    return dict(rows=rows, idx=idx, w=w, row_ptr=row_ptr, nnz=nnz, lc=lc, vals=vals, y=y,
                row_of=row_of, coef=ref.coef[:B].clone(), dX0=dref,
                loss=float(ref.metrics[0]), hist=ref.hist.clone())


@pytest.mark.parametrize("D,lanes,valued",
                         itertools.product([8, 16, 32], [16, 32, 64], [True, False]))
def test_fm_csr_matches_float64(D, lanes, valued):
    c = _case(D, valued)
    rp, lc, rows, idx, w, y = (c[k].cuda() for k in ("row_ptr", "lc", "rows", "idx", "w", "y"))
    vals, nnz = c["vals"].cuda() if valued else None, c["nnz"]
    coef = torch.empty(B, device="cuda")
    dX0 = torch.empty(nnz, D, dtype=torch.bfloat16, device="cuda")
    row_of = torch.empty(nnz, dtype=torch.int32, device="cuda")
    met = new_accum("cuda")
    hist = torch.zeros(2 * AUC_BINS, dtype=torch.int32, device="cuda")
    hipops().fm_csr(rp, 0, lc, nnz, vals, rows, idx, w, y, B, coef, dX0, row_of, met, hist,
                    AUC_BINS, lanes=lanes)
    torch.testing.assert_close(coef.cpu(), c["coef"], **COEF_TOL)
    torch.testing.assert_close(dX0.float().cpu(), c["dX0"].float(), rtol=2e-2, atol=1e-3)
    assert torch.equal(row_of.cpu().long(), c["row_of"])
    m = accum_total(met).cpu()
    assert abs(float(m[0]) - c["loss"]) < 1e-3 * B
    assert float(m[2]) == B
    assert int((hist.cpu() - c["hist"]).abs().sum()) <= 4
    margins = torch.empty(B, device="cuda")  # the forward-only form gives the same coef
    hipops().fm_csr_margins(rp, 0, lc, nnz, vals, rows, idx, w, B, margins, lanes=lanes)
    implied = -c["y"] * torch.sigmoid(-c["y"] * margins.cpu())
    torch.testing.assert_close(implied, coef.cpu(), **COEF_TOL)
    torch.testing.assert_close(implied, c["coef"], **COEF_TOL)


def _same_model(a, b):
    (ka, wa, _, _), (kb, wb, _, _) = a.shard.table.occupied(), b.shard.table.occupied()
    oa, ob = torch.argsort(ka.cpu()), torch.argsort(kb.cpu())
    assert torch.equal(ka.cpu()[oa], kb.cpu()[ob])
    assert torch.allclose(wa.cpu()[oa], wb.cpu()[ob], atol=2e-3)
    assert abs(a.progress()["loss"] - b.progress()["loss"]) < 2e-3


def test_fm_csr_trainer_gpu_matches_cpu():
    cpu = FMTrainer(FMConfig(**CFG))
    gpu = FMTrainer(FMConfig(**CFG), device="cuda")
    for s in range(4):  # three steps, then a held-out batch
        k, l = criteo_batch(512, seed=2, row0=s * 512, num_features=CFG["num_features"],
                            cards=[300] * 26)
        k, rp, v = drop_slots(k, 512, keep=0.8, seed=s)
        if s < 3:
            cpu.step(k, l, vals=v, row_ptr=rp)
            gpu.step(k.cuda(), l.cuda(), vals=v.cuda(), row_ptr=rp.cuda())
    _same_model(cpu, gpu)
    # wide weights within 2e-3 of each other, at most 39 of them in a row, each times a
    # value below 1.5, bound how far the two margins can lie apart
    mc = cpu.predict(k, 512, vals=v, row_ptr=rp)
    mg = gpu.predict(k.cuda(), 512, vals=v.cuda(), row_ptr=rp.cuda())
    assert torch.allclose(mg.cpu(), mc, atol=39 * 1.5 * 2e-3)


def test_fm_csr_uniform_row_ptr_matches_fixed_width():
    fixed = FMTrainer(FMConfig(**CFG), device="cuda")
    csr = FMTrainer(FMConfig(**CFG), device="cuda")
    rp = torch.arange(513, device="cuda") * 39
    for s in range(3):
        k, l = criteo_batch(512, seed=2, row0=s * 512, num_features=CFG["num_features"],
                            cards=[300] * 26, device="cuda")
        fixed.step(k, l)
        csr.step(k, l, row_ptr=rp)
    _same_model(fixed, csr)
