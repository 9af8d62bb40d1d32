"""FM on variable-width rows (models/fm.py, ``row_ptr``): the CSR PyTorch step against the
fixed-width one, a CPU run that learns, the checked errors and 2 gloo ranks."""
import socket

import pytest
import torch
import torch.multiprocessing as mp

from parameter_server_amd.models.fm import FMConfig, FMTrainer
from parameter_server_amd.ops.synthetic import criteo_batch, drop_slots

CFG = dict(num_features=1 << 20, embedding_dim=8, minibatch=256, table_capacity=1 << 15,
           emb_lr=0.05, lambda_v=0.0)


def _csr_batch(B, s, seed):
    k, l = criteo_batch(B, seed=seed, row0=s * B, num_features=CFG["num_features"],
                        cards=[300] * 26)
    return (*drop_slots(k, B, keep=0.8, seed=seed * 1000 + s), l)


def test_csr_torch_equals_fixed_width_on_uniform_rows():
    B, S, D, U = 37, 11, 8, 90
    g = torch.Generator().manual_seed(3)
    X0 = (torch.randn(B * S, D, generator=g) * 0.3).to(torch.bfloat16)
    vals = torch.rand(B * S, generator=g) + 0.5
    lc = torch.randint(0, U, (B * S,), generator=g, dtype=torch.int32)
    w = torch.randn(U, generator=g) * 0.1
    y = torch.where(torch.rand(B, generator=g) < 0.4, 1.0, -1.0)
    a, b = FMTrainer(FMConfig(**CFG)), FMTrainer(FMConfig(**CFG))
    da = a._fwd_bwd_torch(X0, vals, B, S, lc, w, y)
    db = b._fwd_bwd_torch_csr(X0, vals, torch.arange(B).repeat_interleave(S), lc, w, y)
    torch.testing.assert_close(b.coef[:B], a.coef[:B], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(db.float(), da.float(), rtol=1e-2, atol=1e-5)  # (bf16 ulp)
    torch.testing.assert_close(b.metrics, a.metrics, rtol=1e-5, atol=0)  # (fp32 loss sums)
    assert int((a.hist - b.hist).abs().sum()) <= 2


def test_csr_step_learns_on_cpu():
    tr = FMTrainer(FMConfig(**CFG))
    losses = []
    for s in range(30):
        k, rp, v, l = _csr_batch(256, s, seed=5)
        tr.step(k, l, vals=v, row_ptr=rp)
        if s % 10 == 9:
            losses.append(tr.progress()["loss"])
    assert losses[-1] < losses[0], losses


def test_csr_step_errors():
    k, rp, v, l = _csr_batch(64, 0, seed=7)
    tr = FMTrainer(FMConfig(**dict(CFG, max_nnz=k.numel() - 1)))
    with pytest.raises(ValueError, match="max_nnz"):
        tr.step(k, l, vals=v, row_ptr=rp)
    tr = FMTrainer(FMConfig(**CFG))
    with pytest.raises(ValueError, match="row_ptr"):
        tr.step(k, l, vals=v, row_ptr=rp[:-1])
    # D = 48 has no fm_csr instance: a GPU trainer refuses it before any launch
    tr = FMTrainer(FMConfig(**dict(CFG, embedding_dim=48)))
    tr.gpu = True
    with pytest.raises(ValueError, match="embedding_dim"):
        tr.step(k, l, vals=v, row_ptr=rp)


def _worker(rank, port, q):
    import torch.distributed as dist

    from parameter_server_amd.parallel.comm import DistComm

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=2)
    tr = FMTrainer(FMConfig(**CFG), DistComm("cpu"), "cpu")
    for s in range(5):
        k, rp, v, l = _csr_batch(256, s, seed=11 + rank)
        tr.step(k, l, vals=v, row_ptr=rp)
    q.put((tr.progress()["examples"], tr.shard.table.census()[0]))
    dist.destroy_process_group()


def test_csr_step_two_rank_gloo():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = [q.get(timeout=240) for _ in ps]
    [p.join(60) for p in ps]
    assert all(n == 2 * 5 * 256 and occ > 0 for n, occ in res), res
