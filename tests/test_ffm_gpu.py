"""ffm_fwd_bwd / ffm_margins (ffm.hip: one wavefront per example on an LDS tile) against the
float64 PyTorch forward / backward of the same bf16 rows; the FFM trainer, GPU against CPU."""
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
# (S, fields (None: identity), k, factor scale): Dr = F * k rounded up to 8. The scale keeps
# the float64 margins at a standard deviation of 1 to 3 (the pair part is scale^2
# sqrt(k S (S - 1) / 2), the linear part 1): at 0.3, S = 64 saturates the sigmoid.
SHAPES = [
    (1, None, 8, 1.0),    # Dr 8: no pair, m = the linear part, dX0 all zero
    (2, None, 2, 1.0),    # Dr 8: one pair; columns 4..7 are padding
    (39, None, 2, 0.2),   # Dr 80: Criteo; F * k = 78, the last chunk half padding
    # Dr 112, F = 27: a long field list (14 positions on field 0, one of them apart from the
    # others), same-field pairs, j != i inside a list, a padding chunk
    (40, [0] * 13 + list(range(1, 27)) + [0], 4, 0.16),
    (64, [i % 16 for i in range(64)], 8, 0.11),  # Dr 128: full wave, largest tile, most items
    (33, None, 2, 0.21),  # Dr 72: just over half a wave, odd Dr / 8
]


@functools.lru_cache(maxsize=None)
def _case(shape, valued, with_idx):  # inputs (CPU) and the float64 reference, built once
    S, fields, k, scale = SHAPES[shape]
    ref = FFMTrainer(FFMConfig(num_features=1 << 20, slots=S, fields=fields, k=k, minibatch=B,
                               table_capacity=1024))
    g = torch.Generator().manual_seed(100 + 4 * shape + 2 * valued + with_idx)
    rows = (torch.randn(R, ref.Dr, generator=g) * scale).to(torch.bfloat16)
    idx = torch.randint(0, R, (U,), generator=g)
    idx[::50] = -1
    idx = idx if with_idx else None
    w = torch.randn(U, generator=g) / S ** 0.5
    lc = torch.randint(0, U, (B, S), generator=g, dtype=torch.int32)
    lc[:, -1] = lc[:, 0]  # a key twice in a row
    lc = lc.flatten()
    vals = torch.rand(B * S, generator=g) + 0.5 if valued else None
    y = torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0)
    r = idx[lc.long()] if with_idx else lc.long()
    X0 = torch.where((r >= 0)[:, None], rows[r.clamp(min=0)], torch.zeros((), dtype=rows.dtype))
    dref = ref._fwd_bwd_torch(X0, vals, B, S, lc, w, y, dtype=torch.float64)
    f32 = FFMTrainer(ref.cfg)  # the fp32 form lands in the same bins: the cap below is the kernel's
    f32._fwd_bwd_torch(X0, vals, B, S, lc, w, y)
    assert torch.equal(f32.hist, ref.hist)
    return dict(tr=ref, rows=rows, idx=idx, w=w, lc=lc, vals=vals, y=y, coef=ref.coef[:B].clone(),
                dX0=dref, loss=float(ref.metrics[0]), hist=ref.hist.clone())


@pytest.mark.parametrize("shape,valued,with_idx",
                         itertools.product(range(len(SHAPES)), [True, False], [True, False]))
def test_ffm_kernel_matches_float64(shape, valued, with_idx):
    c = _case(shape, valued, with_idx)
    tr, S = c["tr"], SHAPES[shape][0]
    rows, w, lc, y = (c[n].cuda() for n in ("rows", "w", "lc", "y"))
    idx = c["idx"].cuda() if with_idx else None
    vals = c["vals"].cuda() if valued else None
    coef = torch.empty(B, device="cuda")
    dX0 = torch.empty(B * S, tr.Dr, dtype=torch.bfloat16, device="cuda")
    met = new_accum("cuda")
    hist = torch.zeros(2 * AUC_BINS, dtype=torch.int32, device="cuda")
    hipops().ffm_fwd_bwd(rows, idx, vals, B, S, tr.fields, tr.F, tr.cfg.k, lc, w, y, coef, dX0,
                         met, hist, AUC_BINS)
    tol = dict(rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(coef.cpu(), c["coef"], **tol)
    torch.testing.assert_close(dX0.float().cpu(), c["dX0"].float(), rtol=2e-2, atol=1e-3)
    assert float(dX0[:, tr.F * tr.cfg.k:].float().abs().sum()) == 0  # the padding columns
    m = accum_total(met).cpu()
    assert abs(float(m[0]) - c["loss"]) < 1e-3 * B
    assert float(m[2]) == B
    assert int(hist.sum()) == B and int((hist.cpu() - c["hist"]).abs().sum()) <= 2
    margins = torch.empty(B, device="cuda")  # the forward-only form gives the same coef
    hipops().ffm_margins(rows, idx, vals, B, S, tr.fields, tr.F, tr.cfg.k, lc, w, margins)
    implied = -c["y"] * torch.sigmoid(-c["y"] * margins.cpu())
    torch.testing.assert_close(implied, coef.cpu(), **tol)
    torch.testing.assert_close(implied, c["coef"], **tol)


def test_ffm_trainer_gpu_matches_cpu():
    cfg = dict(num_features=1 << 20, k=2, minibatch=512, table_capacity=1 << 16, emb_lr=0.05,
               lambda_v=0.5)
    cpu, gpu = FFMTrainer(FFMConfig(**cfg)), FFMTrainer(FFMConfig(**cfg), device="cuda")
    for s in range(4):  # three steps, then a held-out batch
        k, l = criteo_batch(512, seed=2, row0=s * 512, num_features=cfg["num_features"],
                            cards=[300] * 26)
        if s < 3:
            cpu.step(k, l)
            gpu.step(k.cuda(), l.cuda())
    (ka, wa, _, _), (kb, wb, _, _) = cpu.shard.table.occupied(), gpu.shard.table.occupied()
    oa, ob = torch.argsort(ka.cpu()), torch.argsort(kb.cpu())
    assert torch.equal(ka.cpu()[oa], kb.cpu()[ob])
    assert torch.allclose(wa.cpu()[oa], wb.cpu()[ob], atol=2e-3)
    assert abs(cpu.progress()["loss"] - gpu.progress()["loss"]) < 2e-3
    # wide weights within 2e-3 of each other, 39 of them in a row (binary values), bound how
    # far the two margins can lie apart
    assert torch.allclose(gpu.predict(k.cuda(), 512).cpu(), cpu.predict(k, 512), atol=39 * 2e-3)
