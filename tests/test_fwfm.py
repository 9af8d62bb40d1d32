"""Field-weighted FM (models/fwfm.py) on the CPU: the vectorised PyTorch forward / backward
against the FM pair sum (R = 1) and against autograd of a literal loop over pairs, a run that
learns, and R through a snapshot."""
import torch

from parameter_server_amd.models import FwFMConfig, FwFMTrainer
from parameter_server_amd.ops.synthetic import criteo_batch

CFG = dict(num_features=1 << 21, embedding_dim=8, minibatch=256, table_capacity=1 << 15,
           emb_lr=0.05, lambda_v=0.0)
B, S, D, U = 3, 5, 8, 9
FIELDS = [0, 1, 1, 2, 0]


def _inputs():
    tr = FwFMTrainer(FwFMConfig(**dict(CFG, slots=S, fields=FIELDS, minibatch=B)))
    g = torch.Generator().manual_seed(1)
    X0 = torch.randn(B * S, D, generator=g).to(torch.bfloat16).double()
    x = (torch.rand(B * S, generator=g) + 0.5).double()
    lc = torch.randint(0, U, (B * S,), generator=g, dtype=torch.int32)
    w = torch.randn(U, generator=g).double()
    return tr, X0, x, lc, w, torch.tensor([1.0, -1.0, 1.0])


def _pair_loop(X0, x, lc, w, R):  # margins [B] by the double loop over i < j
    m = []
    for b in range(B):
        p = range(b * S, (b + 1) * S)
        mb = sum(x[q] * w[lc[q]] for q in p)
        for i in range(S):
            for j in range(i + 1, S):
                r = R[min(FIELDS[i], FIELDS[j]), max(FIELDS[i], FIELDS[j])]
                mb = mb + r * x[p[i]] * x[p[j]] * (X0[p[i]] * X0[p[j]]).sum()
        m.append(mb)
    return torch.stack(m)


def test_r_of_ones_is_the_fm():
    tr, X0, x, lc, w, y = _inputs()
    assert float(tr.R.min()) == float(tr.R.max()) == 1.0  # r_init
    m = tr._fwd_bwd_math(X0, x, B, S, lc, w, y, dtype=torch.float64)[0]
    torch.testing.assert_close(m, _pair_loop(X0, x, lc, w, torch.ones(3, 3)), rtol=0, atol=1e-10)


def test_torch_form_equals_autograd_of_the_pair_loop():
    tr, X0, x, lc, w, y = _inputs()
    # symmetric, with a zero and a negative entry; differentiated as its upper triangle
    R = torch.tensor([[0.7, 0.0, 1.3], [0.0, -0.4, 0.9], [1.3, 0.9, 1.1]]).double()
    X0.requires_grad_()
    Ru = torch.triu(R).requires_grad_()
    m = _pair_loop(X0, x, lc, w, Ru)
    torch.nn.functional.softplus(-y.double() * m).sum().backward()
    got_m, got_c, got_dX, got_dR = tr._fwd_bwd_math(X0.detach(), x, B, S, lc, w, y,
                                                    dtype=torch.float64, R=R)
    tol = dict(rtol=0, atol=1e-10)
    torch.testing.assert_close(got_m, m.detach(), **tol)
    torch.testing.assert_close(got_c, -y.double() * torch.sigmoid(-y.double() * m.detach()), **tol)
    torch.testing.assert_close(got_dX, X0.grad, **tol)
    torch.testing.assert_close(torch.triu(got_dR), Ru.grad, **tol)
    torch.testing.assert_close(got_dR, got_dR.T, **tol)


def test_step_learns_and_r_survives_a_snapshot():
    tr = FwFMTrainer(FwFMConfig(**CFG))
    losses = []
    for s in range(30):
        k, l = criteo_batch(256, seed=5, row0=s * 256, num_features=1 << 20, cards=[300] * 26)
        tr.step(k, l)
        if s % 10 == 9:
            losses.append(tr.progress()["loss"])
    assert losses[-1] < losses[0], losses
    assert float((tr.R - 1).abs().max()) > 0 and torch.equal(tr.R, tr.R.T)
    sd = FwFMTrainer.merge_state_dicts([tr.state_dict()])
    new = FwFMTrainer(FwFMConfig(**CFG))
    new.load_state_dict(sd)
    assert torch.equal(new.R, tr.R) and torch.equal(new.R_acc, tr.R_acc)
    k, _ = criteo_batch(64, seed=5, row0=1 << 20, num_features=1 << 20, cards=[300] * 26)
    assert torch.equal(new.predict(k, 64), tr.predict(k, 64))
