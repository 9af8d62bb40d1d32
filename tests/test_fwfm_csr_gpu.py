"""fwfm_csr / fwfm_csr_margins (fwfm_csr.hip: CSR rows of any width with a field per
occurrence) against the float64 PyTorch forward / backward of the same bf16 rows; the FwFM
trainer's CSR step, GPU against CPU."""
import pytest
import torch

from parameter_server_amd.models import FwFMConfig, FwFMTrainer
from parameter_server_amd.ops.linear import AUC_BINS, accum_total, new_accum
from parameter_server_amd.ops.native import hipops
from parameter_server_amd.ops.synthetic import criteo_batch
from test_fwfm_csr import DR_F32_ERR, GRID, SHAPES, case
from test_fwfm_gpu import DR_F32_ERR as FIXED_F32_ERR, SHAPES as FIXED, _case as fixed_case

pytestmark = pytest.mark.gpu


def run(c, F, B, parts, R=None):
    """The training form twice, each time into NaN-filled partials, then the forward-only."""
    rp, fld, rows, w, lc, y = (c[n].cuda() for n in ("rp", "fld", "rows", "w", "lc", "y"))
    R = (c["R"] if R is None else R).cuda()
    idx = c["idx"].cuda() if c["idx"] is not None else None
    vals = c["vals"].cuda() if c["vals"] is not None else None
    nnz, D, Fp = fld.numel(), rows.shape[1], (F + 15) // 16 * 16
    o = dict(coef=torch.empty(B, device="cuda"), met=new_accum("cuda"), dR=[],
             hist=torch.zeros(2 * AUC_BINS, dtype=torch.int32, device="cuda"),
             row_of=torch.full((nnz,), -1, dtype=torch.int32, device="cuda"))
    for rep in range(2):
        o["dX0"] = torch.full((nnz, D), float("nan"), dtype=torch.bfloat16, device="cuda")
        part = torch.full((parts, Fp * Fp), float("nan"), device="cuda")
        dR = torch.empty(F, F, device="cuda")
        hipops().fwfm_csr(rp, fld, nnz, rows, idx, vals, B, F, R, lc, w, y, o["coef"], o["dX0"],
                          o["row_of"], part, o["met"] if rep == 0 else new_accum("cuda"),
                          o["hist"] if rep == 0 else None, AUC_BINS)
        hipops().fwfm_dr_reduce(part, dR, F, True, False)
        o["dR"].append(dR.cpu())
    o["margins"] = torch.empty(B, device="cuda")
    hipops().fwfm_csr_margins(rp, fld, nnz, rows, idx, vals, B, F, R, lc, w, o["margins"])
    return o


def check(o, c, B, F, f32_err):
    tol = dict(rtol=1e-4, atol=1e-5)  # the outputs of run() against the float64 reference in c
    torch.testing.assert_close(o["coef"].cpu(), c["coef"], **tol)
    torch.testing.assert_close(o["dX0"].float().cpu(), c["dX0"].float(), rtol=2e-2, atol=1e-3)
    bad = (c["fld"] < 0) | (c["fld"] >= F)
    assert float(o["dX0"].cpu()[bad].float().abs().sum()) == 0  # exactly, not to a tolerance
    assert torch.equal(o["row_of"].cpu(), c["row_of"])
    m = accum_total(o["met"]).cpu()
    assert abs(float(m[0]) - c["loss"]) < 1e-3 * B and float(m[2]) == B
    assert int(o["hist"].sum()) == B and int((o["hist"].cpu() - c["hist"]).abs().sum()) <= 2
    assert torch.equal(o["dR"][0], o["dR"][1]) and torch.equal(o["dR"][0], o["dR"][0].T)  # bits
    err, bound = float((o["dR"][0].double() - c["dR"]).abs().max()), 8 * f32_err * c["dr_max"]
    print(f"dR error {err:.3g} of max |dR| {c['dr_max']:.3g}: bound {bound:.3g}")
    assert err <= bound
    implied = -c["y"] * torch.sigmoid(-c["y"] * o["margins"].cpu())  # the forward-only form
    torch.testing.assert_close(implied, o["coef"].cpu(), **tol)


@pytest.mark.parametrize("shape,valued,with_idx", GRID)
def test_fwfm_csr_kernel_matches_float64(shape, valued, with_idx):
    c, (F, _, _, _, B, parts, _) = case(shape, valued, with_idx), SHAPES[shape]
    assert int(((c["fld"] < 0) | (c["fld"] >= F)).sum()) > 0
    check(run(c, F, B, parts), c, B, F, DR_F32_ERR)


def test_fwfm_csr_diagonal_is_zero_by_construction():
    # field 3 occurs exactly once in every row: dR[3][3] is 0, R[3][3] acts nowhere, to the bit
    F, B, g = 4, 37, torch.Generator().manual_seed(9)
    width = torch.cat([torch.tensor([70]), torch.randint(2, 12, (B - 1,), generator=g)])
    rp = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(width, 0)])
    fld = torch.randint(0, 3, (int(rp[-1]),), generator=g, dtype=torch.int32)
    fld[rp[:-1] + (torch.rand(B, generator=g) * width).long()] = 3
    c = dict(rp=rp, fld=fld, rows=(torch.randn(300, 8, generator=g) * 0.3).to(torch.bfloat16),
             idx=None, w=torch.randn(300, generator=g) * 0.3, vals=None,
             lc=torch.randint(0, 300, (fld.numel(),), generator=g, dtype=torch.int32),
             y=torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0))
    R = torch.rand(F, F, generator=g) + 0.2
    a, b = (run(c, F, B, 5, R=R.index_put((torch.tensor(3), torch.tensor(3)), torch.tensor(r)))
            for r in (0.7, 1e3))
    assert float(a["dR"][0][3, 3]) == 0 and float(a["dR"][0][0, 0]) != 0
    assert all(torch.equal(a[n].view(torch.uint8), b[n].view(torch.uint8))
               for n in ("coef", "dX0", "margins")) and torch.equal(a["dR"][0], b["dR"][0])


def test_fwfm_csr_on_fixed_rows_matches_the_fixed_width_reference():
    # test_fwfm_gpu.py's case with a 14-position field against its reference (_fwd_bwd_math)
    (S, fields, _, _, B, parts), c = FIXED[3], fixed_case(3, True, True)
    fld = torch.tensor(fields, dtype=torch.int32).repeat(B)
    c = dict(c, rp=torch.arange(B + 1) * S, fld=fld,
             row_of=torch.arange(B, dtype=torch.int32).repeat_interleave(S))
    check(run(c, c["tr"].F, B, parts), c, B, c["tr"].F, FIXED_F32_ERR)


def test_fwfm_csr_trainer_gpu_matches_cpu():
    cfg = dict(num_features=1 << 20, embedding_dim=16, minibatch=512, table_capacity=1 << 16,
               emb_lr=0.05, lambda_v=0.5)
    cpu, dev = FwFMTrainer(FwFMConfig(**cfg)), FwFMTrainer(FwFMConfig(**cfg), device="cuda")
    g = torch.Generator().manual_seed(7)
    field_of = torch.arange(39, dtype=torch.int32).clamp(max=37).repeat(512)  # 37, 38: one field
    for s in range(4):  # three steps, then a held-out batch
        k, l = criteo_batch(512, seed=2, row0=s * 512, num_features=cfg["num_features"],
                            cards=[300] * 26)
        keep = torch.rand(512, 39, generator=g) < 0.8  # slots dropped at random
        rp = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(keep.sum(1), 0)])
        merged = torch.ones(513, dtype=torch.bool)
        merged[[1, 2, 101, 301, 302, 303]] = False  # rows run together: up to 4 x 39 positions
        rp, k, fl, B = rp[merged], k[keep.flatten()], field_of[keep.flatten()], 512 - 6
        if s < 3:
            cpu.step(k, l[:B], row_ptr=rp, fields=fl)
            dev.step(k.cuda(), l[:B].cuda(), row_ptr=rp.cuda(), fields=fl.cuda())
    widest = int((rp[1:] - rp[:-1]).max())
    (ka, wa, _, _), (kb, wb, _, _) = cpu.shard.table.occupied(), dev.shard.table.occupied()
    oa, ob = torch.argsort(ka.cpu()), torch.argsort(kb.cpu())
    assert widest > 64 and torch.equal(ka.cpu()[oa], kb.cpu()[ob])
    assert torch.allclose(wa.cpu()[oa], wb.cpu()[ob], atol=2e-3)
    assert abs(cpu.progress()["loss"] - dev.progress()["loss"]) < 2e-3
    assert float((cpu.R[37, 37] - 1).abs()) > 0 and float(cpu.R[38, 38]) == 1
    assert float((dev.R.cpu() - cpu.R).abs().max()) <= 2e-3  # derived in test_fwfm_gpu.py
    # wide weights within 2e-3 of each other, `widest` of them in a row at the most (binary)
    got = dev.predict(k.cuda(), B, row_ptr=rp.cuda(), fields=fl.cuda()).cpu()
    assert torch.allclose(got, cpu.predict(k, B, row_ptr=rp, fields=fl), atol=widest * 2e-3)
