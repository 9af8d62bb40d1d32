"""FFM on CSR rows with a field per occurrence (models/ffm.py) on the CPU: the padded PyTorch
form against autograd of a literal loop over pairs, the CSR step against the fixed-width step
on full rows, and the checked errors."""
import pytest
import torch

from parameter_server_amd.models import FFMConfig, FFMTrainer
from parameter_server_amd.ops.synthetic import criteo_batch

CFG = dict(num_features=1 << 21, k=2, minibatch=256, table_capacity=1 << 15, emb_lr=0.05,
           lambda_v=0.5)


@pytest.mark.parametrize("valued", [True, False])
def test_csr_torch_form_equals_autograd_of_the_pair_loop(valued):
    F, k, U = 3, 2, 9
    rp = torch.tensor([0, 0, 1, 4, 10])  # widths 0, 1, 3, 6
    fld = torch.tensor([2, 0, 1, 0, 1, -1, 2, 1, 0, 1], dtype=torch.int32)  # repeats; one -1
    B, nnz = 4, 10
    tr = FFMTrainer(FFMConfig(**dict(CFG, slots=4, num_fields=F, fields=[0, 1, 2, 0], minibatch=B)))
    assert (tr.F, tr.Dr) == (3, 8)
    g = torch.Generator().manual_seed(1)
    X0 = torch.randn(nnz, 8, generator=g).to(torch.bfloat16).double().requires_grad_()
    x = (torch.rand(nnz, generator=g) + 0.5).double() if valued else torch.ones(nnz).double()
    lc = torch.randint(0, U, (nnz,), generator=g, dtype=torch.int32)
    w = torch.randn(U, generator=g).double()
    y = torch.tensor([1.0, -1.0, 1.0, -1.0])
    m = []
    for b in range(B):
        p = range(int(rp[b]), int(rp[b + 1]))
        mb = sum((x[q] * w[lc[q]] for q in p), torch.zeros((), dtype=torch.float64))
        for i in p:
            for j in p:
                if i < j and fld[i] >= 0 and fld[j] >= 0:
                    vi = X0[i, fld[j] * k:(fld[j] + 1) * k]
                    vj = X0[j, fld[i] * k:(fld[i] + 1) * k]
                    mb = mb + x[i] * x[j] * (vi * vj).sum()
        m.append(mb)
    m = torch.stack(m)
    torch.nn.functional.softplus(-y.double() * m).sum().backward()
    row_of = torch.repeat_interleave(torch.arange(B), rp[1:] - rp[:-1])
    got_m, got_c, got_dX = tr._fwd_bwd_math_csr(X0.detach(), x if valued else None, row_of, fld,
                                                lc, w, y, dtype=torch.float64)
    tol = dict(rtol=0, atol=1e-10)
    torch.testing.assert_close(got_m, m.detach(), **tol)
    torch.testing.assert_close(got_c, -y.double() * torch.sigmoid(-y.double() * m.detach()), **tol)
    torch.testing.assert_close(got_dX, X0.grad, **tol)
    assert float(got_m[0]) == 0 and float(got_dX[5].abs().max()) == 0  # empty row; field -1
    assert float(got_dX[:, 6:].abs().max()) == 0


def test_csr_step_on_full_rows_equals_the_fixed_width_step():
    fields = [0] * 13 + list(range(1, 27))
    a = FFMTrainer(FFMConfig(**dict(CFG, fields=fields)))
    b = FFMTrainer(FFMConfig(**dict(CFG, fields=fields)))
    rp = torch.arange(257) * 39
    fl = torch.tensor(fields, dtype=torch.int32).repeat(256)
    for s in range(3):
        k, l = criteo_batch(256, seed=5, row0=s * 256, num_features=1 << 20, cards=[300] * 26)
        a.step(k, l)
        b.step(k, l, row_ptr=rp, fields=fl)
    sa, sb = a.state_dict(), b.state_dict()
    assert torch.equal(sa["keys"], sb["keys"])
    # the same sums in another order, in fp32
    torch.testing.assert_close(sa["rows"].float(), sb["rows"].float(), rtol=2 ** -7, atol=1e-5)
    torch.testing.assert_close(sa["w"], sb["w"], rtol=1e-4, atol=1e-6)
    assert abs(a.progress()["loss"] - b.progress()["loss"]) < 1e-5


RP, FL = torch.arange(5) * 2, torch.zeros(8, dtype=torch.int32)


@pytest.mark.parametrize("bad", [
    dict(row_ptr=RP[:4]), dict(row_ptr=RP.int()), dict(fields=FL[:7]), dict(fields=FL.long()),
    dict(vals=torch.ones(7)), dict(row_ptr=None), dict(fields=None),
    dict(keys=torch.arange(80), fields=torch.zeros(80, dtype=torch.int32)),  # nnz > max_nnz
    dict(labels=torch.ones(9), row_ptr=torch.arange(10))])                   # B > minibatch
def test_csr_errors(bad):
    tr = FFMTrainer(FFMConfig(**dict(CFG, slots=4, minibatch=8)))
    kw = dict(dict(keys=torch.arange(8), labels=torch.ones(4), row_ptr=RP, fields=FL), **bad)
    with pytest.raises(ValueError):
        tr.step(kw.pop("keys"), kw.pop("labels"), **kw)
    if "labels" not in bad and "keys" not in bad:
        kw = dict(dict(row_ptr=RP, fields=FL), **bad)
        with pytest.raises(ValueError):
            tr.predict(torch.arange(8), 4, **kw)
