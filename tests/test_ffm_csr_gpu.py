"""ffm_csr / ffm_csr_margins (ffm_csr.hip: CSR rows with a field per occurrence, LDS tile for
rows of up to T positions, global-memory path for wider ones) against the float64 PyTorch
forward / backward of the same bf16 rows; the FFM trainer's CSR step, GPU against CPU."""
import functools
import itertools

import pytest
import torch

from parameter_server_amd.models import FFMConfig, FFMTrainer
from parameter_server_amd.ops.linear import AUC_BINS, accum_total, new_accum
from parameter_server_amd.ops.native import hipops
from parameter_server_amd.ops.synthetic import criteo_batch

pytestmark = pytest.mark.gpu
B, U, R = 37, 200, 300  # rows: odd, no multiple of the 3 or 4 a block holds
# (T, k, F, factor scale): Dr = F * k rounded up to 8. The scale keeps the float64 margins at
# a standard deviation of 1 to 3 (the pair part of a row of n is scale^2 sqrt(k n (n - 1) / 2)).
SHAPES = [
    (4, 8, 1, 0.5),     # Dr 8: one field, every pair a same-field pair
    (39, 2, 39, 0.2),   # Dr 80: Criteo; F * k = 78, the last chunk half padding
    (40, 4, 27, 0.16),  # Dr 112: a padding chunk
    (64, 8, 16, 0.11),  # Dr 128: full wave, largest tile; rows of 65 and 150
    (33, 2, 36, 0.21),  # Dr 72: just over half a wave, odd Dr / 8
]


@functools.lru_cache(maxsize=None)
def _case(shape, valued, with_idx):  # inputs (CPU) and the float64 reference, built once
    T, k, F, scale = SHAPES[shape]
    cfg = FFMConfig(num_features=1 << 20, slots=T, fields=[0] * T, num_fields=F, k=k,
                    minibatch=B, table_capacity=1024)
    ref = FFMTrainer(cfg)
    g = torch.Generator().manual_seed(300 + 4 * shape + 2 * valued + with_idx)
    special = [0, 1, 2, T - 1, T, T + 1] + ([65, 150] if T == 64 else [])
    width = torch.cat([torch.tensor(special),
                       torch.randint(1, T + 1, (B - len(special),), generator=g)])
    rp = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(width, 0)])
    nnz = int(rp[-1])
    row_of = torch.repeat_interleave(torch.arange(B), width)
    fld = torch.randint(0, F, (nnz,), generator=g, dtype=torch.int32)
    fld[rp[4]:rp[5]] = F // 2            # the row of T: every occurrence on one field
    fld[rp[3]:rp[4]] = 0                 # the row of T - 1: field F - 1 occurs once
    fld[rp[3]] = F - 1
    fld[3::17] = -1                      # out of range: a linear term and no pair
    fld[5::23] = F
    rows = (torch.randn(R, ref.Dr, generator=g) * scale).to(torch.bfloat16)
    idx = torch.randint(0, R, (U,), generator=g)
    idx[::50] = -1
    idx = idx if with_idx else None
    w = torch.randn(U, generator=g) / T ** 0.5
    lc = torch.randint(0, U, (nnz,), generator=g, dtype=torch.int32)
    two = width >= 2
    lc[rp[1:][two] - 1] = lc[rp[:-1][two]]  # a key twice in a row
    vals = torch.rand(nnz, generator=g) + 0.5 if valued else None
    y = torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0)
    r = idx[lc.long()] if with_idx else lc.long()
    X0 = torch.where((r >= 0)[:, None], rows[r.clamp(min=0)], torch.zeros((), dtype=rows.dtype))
    dref = ref._fwd_bwd_torch_csr(X0, vals, row_of, fld, lc, w, y, dtype=torch.float64)
    f32 = FFMTrainer(cfg)  # the fp32 form lands in the same bins: the cap below is the kernel's
    f32._fwd_bwd_torch_csr(X0, vals, row_of, fld, lc, w, y)
    assert torch.equal(f32.hist, ref.hist)
    return dict(tr=ref, rp=rp, row_of=row_of.int(), fld=fld, rows=rows, idx=idx, w=w, lc=lc,
                vals=vals, y=y, coef=ref.coef[:B].clone(), dX0=dref, loss=float(ref.metrics[0]),
                hist=ref.hist.clone())


def _run_and_check(c, T):
    """Both kernels on case c with a tile of T rows; everything checked against float64."""
    tr = c["tr"]
    F, k = tr.F, tr.cfg.k
    rp, fld, rows, w, lc, y = (c[n].cuda() for n in ("rp", "fld", "rows", "w", "lc", "y"))
    idx = c["idx"].cuda() if c["idx"] is not None else None
    vals = c["vals"].cuda() if c["vals"] is not None else None
    nnz = fld.numel()
    coef = torch.empty(B, device="cuda")
    dX0 = torch.full((nnz, tr.Dr), float("nan"), dtype=torch.bfloat16, device="cuda")
    row_of = torch.full((nnz,), -1, dtype=torch.int32, device="cuda")
    met = new_accum("cuda")
    hist = torch.zeros(2 * AUC_BINS, dtype=torch.int32, device="cuda")
    hipops().ffm_csr(rp, fld, nnz, rows, idx, vals, B, T, F, k, lc, w, y, coef, dX0, row_of, met,
                     hist, AUC_BINS)
    tol = dict(rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(coef.cpu(), c["coef"], **tol)
    torch.testing.assert_close(dX0.float().cpu(), c["dX0"].float(), rtol=2e-2, atol=1e-3)
    assert float(dX0[:, F * k:].float().abs().sum()) == 0  # the padding columns
    bad = (fld < 0) | (fld >= F)
    assert int(bad.sum()) > 0 and float(dX0[bad].float().abs().sum()) == 0
    assert torch.equal(row_of.cpu(), c["row_of"])
    m = accum_total(met).cpu()
    print(f"T={T} loss {float(m[0]):.6f} ref {c['loss']:.6f} "
          f"hist diff {int((hist.cpu() - c['hist']).abs().sum())}")
    assert abs(float(m[0]) - c["loss"]) < 1e-3 * B
    assert float(m[2]) == B
    assert int(hist.sum()) == B and int((hist.cpu() - c["hist"]).abs().sum()) <= 2
    margins = torch.empty(B, device="cuda")  # the forward-only form gives the same coef
    hipops().ffm_csr_margins(rp, fld, nnz, rows, idx, vals, B, T, F, k, lc, w, margins)
    implied = -c["y"] * torch.sigmoid(-c["y"] * margins.cpu())
    torch.testing.assert_close(implied, coef.cpu(), **tol)
    torch.testing.assert_close(implied, c["coef"], **tol)
    return coef, dX0, margins


@pytest.mark.parametrize("shape,valued,with_idx",
                         itertools.product(range(len(SHAPES)), [True, False], [True, False]))
def test_ffm_csr_kernel_matches_float64(shape, valued, with_idx):
    _run_and_check(_case(shape, valued, with_idx), SHAPES[shape][0])


@pytest.mark.parametrize("shape", [1, 2])
def test_ffm_csr_tile_and_wide_paths_agree(shape, record_property):
    """The same minibatch with every row on the tile (T = 64 >= the widest row) and with
    T = 4, which sends most rows down the global-memory path: both meet the float64
    tolerances. Whether they are bit-equal is recorded, not asserted."""
    c = _case(shape, True, True)
    tile, wide = _run_and_check(c, 64), _run_and_check(c, 4)
    equal = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(tile, wide))
    record_property("tile_and_wide_bit_equal", equal)
    print("tile and wide paths bit-equal:", equal)


def test_ffm_csr_trainer_gpu_matches_cpu():
    cfg = dict(num_features=1 << 20, k=2, minibatch=512, table_capacity=1 << 16, emb_lr=0.05,
               lambda_v=0.5)
    cpu, gpu = FFMTrainer(FFMConfig(**cfg)), FFMTrainer(FFMConfig(**cfg), device="cuda")
    g = torch.Generator().manual_seed(7)
    slot_of = torch.arange(39, dtype=torch.int32).repeat(512)
    for s in range(4):  # three steps, then a held-out batch; slots dropped at random
        k, l = criteo_batch(512, seed=2, row0=s * 512, num_features=cfg["num_features"],
                            cards=[300] * 26)
        keep = torch.rand(512, 39, generator=g) < 0.8
        rp = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(keep.sum(1), 0)])
        k, fl = k[keep.flatten()], slot_of[keep.flatten()]
        if s < 3:
            cpu.step(k, l, row_ptr=rp, fields=fl)
            gpu.step(k.cuda(), l.cuda(), row_ptr=rp.cuda(), fields=fl.cuda())
    (ka, wa, _, _), (kb, wb, _, _) = cpu.shard.table.occupied(), gpu.shard.table.occupied()
    oa, ob = torch.argsort(ka.cpu()), torch.argsort(kb.cpu())
    assert torch.equal(ka.cpu()[oa], kb.cpu()[ob])
    assert torch.allclose(wa.cpu()[oa], wb.cpu()[ob], atol=2e-3)
    assert abs(cpu.progress()["loss"] - gpu.progress()["loss"]) < 2e-3
    # wide weights within 2e-3 of each other, at most 39 of them in a row (binary values)
    got = gpu.predict(k.cuda(), 512, row_ptr=rp.cuda(), fields=fl.cuda()).cpu()
    assert torch.allclose(got, cpu.predict(k, 512, row_ptr=rp, fields=fl), atol=39 * 2e-3)
