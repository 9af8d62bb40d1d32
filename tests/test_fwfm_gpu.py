"""fwfm_fwd_bwd / fwfm_margins / fwfm_dr_reduce (fwfm.hip: one wavefront per example, T = R P
and dR on the fp32 matrix instructions) against the float64 PyTorch forward / backward of the
same bf16 rows; the FwFM trainer, GPU against CPU."""
import functools
import itertools

import pytest
import torch

from parameter_server_amd.models import FwFMConfig, FwFMTrainer
from parameter_server_amd.ops.linear import AUC_BINS, accum_total, new_accum
from parameter_server_amd.ops.native import hipops
from parameter_server_amd.ops.synthetic import criteo_batch

gpu = pytest.mark.gpu
U, NR = 200, 300
# (S, fields (None: identity), D, factor scale, B, dR partials = blocks). B = 37: odd, no
# multiple of the waves a block holds. The scale keeps the float64 margins at a standard
# deviation of about 1 to 3 (the linear part is 1, the pair part 0.73 scale^2
# sqrt(D S (S - 1) / 2), 0.73 the root mean square of R).
SHAPES = [
    (1, None, 8, 1.0, 37, 5),     # no pair: dX0 and dR are zero
    (2, None, 8, 0.55, 37, 5),    # one pair, half an MFMA N-tile
    (39, None, 16, 0.14, 37, 5),  # F = 39 pads to 48 rows, K = 39 is no multiple of 4
    # a 14-position field (one position apart from the others): the diagonal term and q_f
    (40, [0] * 13 + list(range(1, 27)) + [0], 16, 0.14, 37, 5),
    (17, None, 16, 0.21, 37, 5),  # one row past a 16-tile
    (16, None, 32, 0.18, 37, 5),  # exact tiles
    (64, [i % 16 for i in range(64)], 32, 0.09, 37, 5),
    (64, None, 32, 0.09, 37, 5),  # the largest region and the most accumulators
    (39, None, 16, 0.14, 1, 3),   # idle waves and blocks contribute zeros
    (39, None, 16, 0.14, 1031, 7),  # every wave accumulates many rows
]
# dR: the largest error of the fp32 PyTorch form against the float64 one over these cases,
# relative to max |dR|, is DR_F32_ERR (measured; test_cases_hold_what_the_bounds_rest_on
# asserts it on the CPU). The kernel's other sum order (wave, block, runs of blocks) and its
# fp32 sums over B * D terms get 8 times that.
DR_F32_ERR = 9.6e-7  # 9.54e-7, at (64, i % 16, 32) binary without idx
DR_TOL = 8 * DR_F32_ERR
# (shape, valued, with idx); the B = 1 and B = 1031 cases run one combination each
GRID = [(s, v, i) for s in range(8) for v, i in itertools.product([True, False], repeat=2)] + \
       [(8, True, True), (9, False, False)]


@functools.lru_cache(maxsize=None)
def _case(shape, valued, with_idx):  # inputs (CPU) and the float64 reference, built once
    S, fields, D, scale, B, _ = SHAPES[shape]
    ref = FwFMTrainer(FwFMConfig(num_features=1 << 20, slots=S, fields=fields, embedding_dim=D,
                                 minibatch=B, table_capacity=1024))
    g = torch.Generator().manual_seed(100 + 4 * shape + 2 * valued + with_idx)
    rows = (torch.randn(NR, D, generator=g) * scale).to(torch.bfloat16)
    idx = torch.randint(0, NR, (U,), generator=g)
    idx[::50] = -1
    idx = idx if with_idx else None
    w = torch.randn(U, generator=g) / S ** 0.5
    lc = torch.randint(0, U, (B, S), generator=g, dtype=torch.int32)
    lc[:, -1] = lc[:, 0]  # a key twice in a row
    lc = lc.flatten()
    vals = torch.rand(B * S, generator=g) + 0.5 if valued else None
    y = torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0)
    R = torch.rand(ref.F, ref.F, generator=g) * 2 - 0.5  # [-0.5, 1.5) with exact zeros
    R[torch.rand(ref.F, ref.F, generator=g) < 0.15] = 0
    R = torch.triu(R) + torch.triu(R, 1).T
    r = idx[lc.long()] if with_idx else lc.long()
    X0 = torch.where((r >= 0)[:, None], rows[r.clamp(min=0)], torch.zeros((), dtype=rows.dtype))
    ref.R.copy_(R)
    m, coef, dX, dR = ref._fwd_bwd_math(X0, vals, B, S, lc, w, y, dtype=torch.float64)
    dX0 = ref._account(m, coef, dX, y, B)
    f32 = FwFMTrainer(ref.cfg)  # the fp32 form lands in the same bins: the cap below is the kernel's
    f32.R.copy_(R)
    dR32 = f32._fwd_bwd_torch(X0, vals, B, S, lc, w, y)[1]
    assert torch.equal(f32.hist, ref.hist)
    dr_max = float(dR.abs().max())
    return dict(tr=ref, rows=rows, idx=idx, w=w, lc=lc, vals=vals, y=y, R=R, dX0=dX0, dR=dR,
                coef=ref.coef[:B].clone(), loss=float(ref.metrics[0]), hist=ref.hist.clone(),
                dr_max=dr_max, m_std=float(m.std()) if B > 1 else None,
                f32_err=float((dR32.double() - dR).abs().max()) / dr_max if dr_max else 0.0)


def test_cases_hold_what_the_bounds_rest_on():
    """No GPU: the fp32 form in the float64 AUC bins (the builder's own assertion), the fp32
    error of dR the tolerance is derived from, margins neither flat nor saturated."""
    cases = [_case(*c) for c in GRID]
    assert max(c["f32_err"] for c in cases) <= DR_F32_ERR
    assert all(0.9 <= c["m_std"] <= 3.0 for c in cases if c["m_std"] is not None)


@gpu
@pytest.mark.parametrize("shape,valued,with_idx", GRID)
def test_fwfm_kernel_matches_float64(shape, valued, with_idx):
    c = _case(shape, valued, with_idx)
    tr, (S, _, D, _, B, parts) = c["tr"], SHAPES[shape]
    F, Fp = tr.F, (tr.F + 15) // 16 * 16
    rows, w, lc, y, R = (c[n].cuda() for n in ("rows", "w", "lc", "y", "R"))
    idx = c["idx"].cuda() if with_idx else None
    vals = c["vals"].cuda() if valued else None
    coef = torch.empty(B, device="cuda")
    dX0 = torch.empty(B * S, D, dtype=torch.bfloat16, device="cuda")
    met = new_accum("cuda")
    hist = torch.zeros(2 * AUC_BINS, dtype=torch.int32, device="cuda")
    dRs = []
    for rep in range(2):  # twice, each time into partials full of NaN
        part = torch.full((parts, Fp * Fp), float("nan"), device="cuda")
        dR = torch.empty(F, F, device="cuda")
        hipops().fwfm_fwd_bwd(rows, idx, vals, B, S, tr.fields, F, R, lc, w, y, coef, dX0, part,
                              met if rep == 0 else new_accum("cuda"), hist if rep == 0 else None,
                              AUC_BINS)
        hipops().fwfm_dr_reduce(part, dR, F, True, False)
        dRs.append(dR.cpu())
    tol = dict(rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(coef.cpu(), c["coef"], **tol)
    torch.testing.assert_close(dX0.float().cpu(), c["dX0"].float(), rtol=2e-2, atol=1e-3)
    m = accum_total(met).cpu()
    assert abs(float(m[0]) - c["loss"]) < 1e-3 * B
    assert float(m[2]) == B
    assert int(hist.sum()) == B and int((hist.cpu() - c["hist"]).abs().sum()) <= 2
    assert torch.equal(dRs[0], dRs[1])  # the same bits on every run
    assert torch.equal(dRs[0], dRs[0].T)
    dr_atol = DR_TOL * c["dr_max"]
    err = float((dRs[0].double() - c["dR"]).abs().max())
    print(f"dR error {err:.3g} of max |dR| {c['dr_max']:.3g}: bound {dr_atol:.3g}")
    assert err <= dr_atol
    if S == 1:
        assert float(dX0.float().abs().sum()) == 0 and float(dRs[0].abs().sum()) == 0
    margins = torch.empty(B, device="cuda")  # the forward-only form gives the same coef
    hipops().fwfm_margins(rows, idx, vals, B, S, tr.fields, F, R, lc, w, margins)
    implied = -c["y"] * torch.sigmoid(-c["y"] * margins.cpu())
    torch.testing.assert_close(implied, coef.cpu(), **tol)
    torch.testing.assert_close(implied, c["coef"], **tol)
    # sum + update in one launch against AdaGrad on the float64 dR (lr 0.05, lambda_r 0.1,
    # acc 0.25 before): |d step / d g| <= lr / sqrt(acc) = 0.1 and d acc / d g = 2 g carry
    # the error of dR; the rest is fp32 rounding of R <= 1.6 and of acc
    Rg, acc = R.clone(), torch.full((F, F), 0.25, device="cuda")
    hipops().fwfm_dr_reduce(part, dR, F, True, True, Rg, acc, 0.05, 0.1)
    g = c["dR"] + 0.1 * c["R"].double()
    a = 0.25 + g * g
    gm = float(g.abs().max())
    torch.testing.assert_close(Rg.cpu().double(), c["R"].double() - 0.05 * g / (a.sqrt() + 1e-8),
                               rtol=0, atol=0.1 * dr_atol + 4e-7)
    torch.testing.assert_close(acc.cpu().double(), a, rtol=0,
                               atol=2 * gm * dr_atol + 4e-7 * float(a.max()))


@gpu
def test_fwfm_trainer_gpu_matches_cpu():
    cfg = dict(num_features=1 << 20, embedding_dim=16, minibatch=512, table_capacity=1 << 16,
               emb_lr=0.05, lambda_v=0.5)
    cpu, dev = FwFMTrainer(FwFMConfig(**cfg)), FwFMTrainer(FwFMConfig(**cfg), device="cuda")
    for s in range(4):  # three steps, then a held-out batch
        k, l = criteo_batch(512, seed=2, row0=s * 512, num_features=cfg["num_features"],
                            cards=[300] * 26)
        if s < 3:
            cpu.step(k, l)
            dev.step(k.cuda(), l.cuda())
    (ka, wa, _, _), (kb, wb, _, _) = cpu.shard.table.occupied(), dev.shard.table.occupied()
    oa, ob = torch.argsort(ka.cpu()), torch.argsort(kb.cpu())
    assert torch.equal(ka.cpu()[oa], kb.cpu()[ob])
    assert torch.allclose(wa.cpu()[oa], wb.cpu()[ob], atol=2e-3)
    assert abs(cpu.progress()["loss"] - dev.progress()["loss"]) < 2e-3
    # R takes AdaGrad steps r_lr g / sqrt(sum g^2): the first is r_lr sign(g) on both, and a
    # later one is r_lr times a ratio in [-1, 1] that moves by no more than the relative
    # error of g. The kernel's share of that is DR_TOL; the rest is the states parting (bf16
    # rows, the wide weights' 2e-3 above). 2e-3 of r_lr per step would follow from that
    # alone; entries whose |g| is small against max |dR| carry more, so the bound is the wide
    # weights': both are AdaGrad parameters fed by the same coef, with r_lr < the wide rate
    assert float((dev.R.cpu() - cpu.R).abs().max()) <= 2e-3
    # wide weights within 2e-3 of each other, 39 of them in a row (binary values), bound how
    # far the two margins can lie apart
    assert torch.allclose(dev.predict(k.cuda(), 512).cpu(), cpu.predict(k, 512), atol=39 * 2e-3)
