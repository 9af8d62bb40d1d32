"""Field-aware FM (models/ffm.py) on the CPU: the vectorised PyTorch forward / backward against
autograd of a literal loop over pairs, a run that learns, the checked errors and 2 gloo
ranks against the 1-rank model."""
import socket

import pytest
import torch
import torch.multiprocessing as mp

from parameter_server_amd.models import FFMConfig, FFMTrainer
from parameter_server_amd.ops.synthetic import criteo_batch

CFG = dict(num_features=1 << 21, k=2, minibatch=256, table_capacity=1 << 15, emb_lr=0.05,
           lambda_v=0.0)


@pytest.mark.parametrize("valued", [True, False])
def test_torch_form_equals_autograd_of_the_pair_loop(valued):
    B, S, k, U = 3, 5, 2, 9
    fields = [0, 1, 2, 1, 0]  # F = 3: F * k = 6 in rows of Dr = 8
    tr = FFMTrainer(FFMConfig(**dict(CFG, slots=S, fields=fields, minibatch=B)))
    assert (tr.F, tr.Dr) == (3, 8)
    g = torch.Generator().manual_seed(1)
    X0 = torch.randn(B * S, 8, generator=g).to(torch.bfloat16).double().requires_grad_()
    x = (torch.rand(B * S, generator=g) + 0.5).double() if valued else torch.ones(B * S).double()
    lc = torch.randint(0, U, (B * S,), generator=g, dtype=torch.int32)
    w = torch.randn(U, generator=g).double()
    y = torch.tensor([1.0, -1.0, 1.0])
    m = []
    for b in range(B):
        p = range(b * S, (b + 1) * S)
        mb = sum(x[q] * w[lc[q]] for q in p)
        for i in range(S):
            for j in range(i + 1, S):
                vi = X0[p[i], fields[j] * k:(fields[j] + 1) * k]
                vj = X0[p[j], fields[i] * k:(fields[i] + 1) * k]
                mb = mb + x[p[i]] * x[p[j]] * (vi * vj).sum()
        m.append(mb)
    m = torch.stack(m)
    torch.nn.functional.softplus(-y.double() * m).sum().backward()
    got_m, got_c, got_dX = tr._fwd_bwd_math(X0.detach(), x if valued else None, B, S, lc, w, y,
                                            dtype=torch.float64)
    tol = dict(rtol=0, atol=1e-10)
    torch.testing.assert_close(got_m, m.detach(), **tol)
    torch.testing.assert_close(got_c, -y.double() * torch.sigmoid(-y.double() * m.detach()), **tol)
    torch.testing.assert_close(got_dX, X0.grad, **tol)
    assert float(X0.grad[:, 6:].abs().max()) == 0 and float(got_dX[:, 6:].abs().max()) == 0


def test_step_learns_on_cpu():
    tr = FFMTrainer(FFMConfig(**CFG))
    losses = []
    for s in range(30):
        k, l = criteo_batch(256, seed=5, row0=s * 256, num_features=1 << 20, cards=[300] * 26)
        tr.step(k, l)
        if s % 10 == 9:
            losses.append(tr.progress()["loss"])
    assert losses[-1] < losses[0], losses


@pytest.mark.parametrize("bad", [dict(slots=65), dict(k=3), dict(slots=3, fields=[0, 1, 5],
                                                                 num_fields=3),
                                 dict(slots=39, k=4)])  # (39 fields of 4: rows of 160)
def test_geometry_errors(bad):
    with pytest.raises(ValueError):
        FFMTrainer(FFMConfig(**dict(CFG, **bad)))


def _batch(s, rank):  # the two ranks' keys are disjoint: even and odd
    k, l = criteo_batch(128, seed=11, row0=(2 * s + rank) * 128, num_features=1 << 20,
                        cards=[300] * 26)
    return k * 2 + rank, l


def _model(tr):
    sd = tr.state_dict()
    return sd["keys"].numpy(), sd["w"].numpy(), sd["rows"].float().numpy()


def _worker(rank, port, q):
    import torch.distributed as dist

    from parameter_server_amd.parallel.comm import DistComm

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=2)
    tr = FFMTrainer(FFMConfig(**dict(CFG, minibatch=128)), DistComm("cpu"), "cpu")
    for s in range(3):
        tr.step(*_batch(s, rank))
    q.put((*_model(tr), tr.progress()))
    dist.destroy_process_group()


def test_two_rank_gloo_equals_one_rank():
    """Two ranks on key-disjoint minibatches are one rank on both minibatches in one: a key's
    gradient comes from its own half, and it is updated once per step either way."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = [q.get(timeout=240) for _ in ps]
    [p.join(60) for p in ps]
    one = FFMTrainer(FFMConfig(**CFG))
    for s in range(3):
        (k0, l0), (k1, l1) = _batch(s, 0), _batch(s, 1)
        one.step(torch.cat([k0, k1]), torch.cat([l0, l1]))
    keys, w, rows = (torch.cat([torch.from_numpy(r[i]) for r in res]) for i in range(3))
    k1, w1, rows1 = (torch.from_numpy(a) for a in _model(one))
    o, o1 = torch.argsort(keys), torch.argsort(k1)
    assert torch.equal(keys[o], k1[o1])
    # the exchange carries row gradients as bf16 (2^-9 relative) into a row-wise AdaGrad step
    # of at most emb_lr * sqrt(Dr) = 0.45 per coordinate: 0.45 * 2^-9 * 3 steps = 2.6e-3; each
    # step also rounds the row to bf16 again, where the two may part by one ulp (2^-8 of the
    # value at the most): 3 * 2^-8 relative
    torch.testing.assert_close(rows[o], rows1[o1], rtol=3 * 2 ** -8, atol=2.6e-3)
    torch.testing.assert_close(w[o], w1[o1], rtol=0, atol=1e-3)
    p1 = one.progress()
    assert res[0][3]["examples"] == p1["examples"] == 3 * 256
    assert abs(res[0][3]["loss"] - p1["loss"]) < 1e-3
