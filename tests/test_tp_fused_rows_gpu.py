"""The fused forward + backward kernel (tploc_fused.hip tp_fwd_bwd_kernel) evaluates each
row's loss terms in ONE thread (margins and coefs go through LDS row arrays) instead of
in all eight lanes of the row's group: every register-pass instantiation and both
layouts (compact "tp", flat "tpf") against the plain PyTorch fp32 reference of
tests/test_tp_fused_gpu.py, with that file's tolerances.

Shapes are the smallest that reach each path:
  width 39, B = 631, tiles pinned to 8192 occurrences: <PER 5, NP 2>; rows straddle both
    boundaries of a tile and the last tile holds 33 occurrences (less than one row);
  width 39, B = 631, flat, unpinned: 1024-occurrence tiles, the NP = 1 instantiation;
  width 9, B = 1,900: NP = 8, up to 912 rows per tile (row threads past the first
    128-row pass);
  width 64, B = 300, valued: PER = 8.
"""
import functools

import pytest
import torch

from parameter_server_amd.ops.linear import (AUC_BINS, HIST_STRIPES, accum_total, linear_fwd_bwd,
                                             loss_id, loss_terms_torch, new_accum)
from parameter_server_amd.ops.localize import Localizer
from parameter_server_amd.ops.native import hipops
from parameter_server_amd.ops.synthetic import criteo_batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TILE = 8192  # entry stride of a tile, whatever it holds


@functools.lru_cache(maxsize=None)
def _batch(B, width, with_vals):
    """(keys, labels in {-1, +1}, real-valued labels, vals or None); built once per shape."""
    g = torch.Generator(device="cpu").manual_seed(1000 * width + B)
    if width == 39:
        keys, _ = criteo_batch(B, seed=3, row0=0, num_features=10 ** 9, device=DEV)
    else:
        keys = (torch.randint(0, 1 << 20, (B * width,), generator=g) ** 2 % 1000003).to(DEV)
    labels = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0).to(DEV)
    real = torch.randn(B, generator=g).to(DEV)
    vals = (torch.rand(B * width, generator=g) + 0.5).to(DEV) if with_vals else None
    return keys, labels, real, vals


def _key_weights(keys):
    """A weight per KEY (uniform, std 0.05): which entry or unique id a key gets varies from
    localisation to localisation, the margins (and the rows near a bin edge) must not."""
    u = ((keys * 2654435761) >> 7) % (1 << 20)
    return ((u.double() / (1 << 20) - 0.5) * 0.17).float()


class _Case:
    """One localisation of a shape in one layout: ``cols`` maps every occurrence to the
    index of its weight (unique id for "tp", tile entry for "tpf"), ``live`` marks the
    gradient slots the kernel writes, ``run(labels, loss)`` launches the fused kernel."""

    def __init__(self, layout, B, width, with_vals):
        self.B, self.width = B, width
        keys, self.labels, self.real, self.vals = _batch(B, width, with_vals)
        n = keys.numel()
        i = torch.arange(n, device=DEV)
        if layout == "tp":
            self.loc = loc = Localizer(n, 30, DEV, mode="tp", lazy_cols=True)(keys)
            U = int(loc.n_uniq.item())
            self.w = torch.zeros(U, device=DEV)
            t = loc.tile
            self.cols = t.ent_uid[(i >> 13) * TILE + (t.rep[:n].long() & 0xFFFF)].long()
            self.live = torch.ones(U, dtype=torch.bool, device=DEV)
            self.partials = t.psum
        else:
            self.loc = f = Localizer(n, 30, DEV, mode="tpf")(keys)
            self.lts = lts = hipops().tpf_tile_log2(n)
            T = (n + (1 << lts) - 1) >> lts
            self.w = torch.zeros(f.w_ent.numel(), device=DEV)
            self.cols = (i >> lts) * TILE + (f.rep[:n].long() & 0xFFFF)
            live = torch.arange(TILE, device=DEV)[None, :] < f.dcnt[:T, None]
            self.live = torch.zeros(f.w_ent.numel(), dtype=torch.bool, device=DEV)
            self.live[:T * TILE] = live.reshape(-1)
            self.partials = f.psum
        self.w[self.cols] = _key_weights(keys)  # (occurrences of one slot share their key)
        self.layout = layout

    def run(self, labels, loss):
        B, width = self.B, self.width
        coef = torch.empty(B, device=DEV)
        metrics = new_accum(DEV)
        hist = torch.zeros(HIST_STRIPES * 2 * AUC_BINS, dtype=torch.int32, device=DEV)
        if self.layout == "tp":
            self.loc.grad.zero_()  # (as the localiser leaves it: cut runs add atomically)
            _, grad = linear_fwd_bwd(self.loc, self.w, labels, B=B, width=width, vals=self.vals,
                                     loss=loss, coef=coef, metrics=metrics, hist=hist)
            assert not self.loc.tile.cols_ready  # the fused kernel ran, not the fallback
            grad = grad[:self.w.numel()]
        else:
            f = self.loc
            hipops().tp_fwd_bwd(f.rep, f.dcnt, None, f.nnz, width, self.vals, self.w, labels, B,
                                loss_id(loss), coef, metrics, hist, AUC_BINS, f.psum, None, None,
                                None, None, False)
            grad = f.psum
        torch.cuda.synchronize()
        return coef, grad, accum_total(metrics).cpu(), hist.view(-1, 2 * AUC_BINS).sum(0).cpu()

    def reference(self, labels, loss):
        """Plain torch (tests/test_tp_fused_gpu.py _reference) + the AUC bins."""
        B, width, w, col = self.B, self.width, self.w, self.cols
        x = self.vals if self.vals is not None else torch.ones_like(w[col])
        m = (w[col] * x).reshape(B, width).double().sum(1).float()
        lo, c, _ = loss_terms_torch(m, labels, loss_id(loss))
        g = torch.zeros_like(w).index_add_(0, col, c.repeat_interleave(width) * x)
        pb = (1.0 / (1.0 + torch.exp(-m))) * AUC_BINS
        b = pb.clamp(0, AUC_BINS - 1).long() + torch.where(labels > 0, AUC_BINS, 0)
        h = torch.zeros(2 * AUC_BINS, dtype=torch.int64, device=DEV).index_add_(
            0, b, torch.ones_like(b)).cpu()
        near = int(((pb - pb.round()).abs() < 1e-3).sum())  # rows a rounding may move a bin
        return m, c, lo, g, h, near


@functools.lru_cache(maxsize=None)
def _case(layout, B, width, with_vals, pin):
    # (pin: part of the key only; the caller has set PSAMD_TILE_LTS, read per call)
    return _Case(layout, B, width, with_vals)


def _check(case, loss="logit"):
    B = case.B
    labels = case.real if loss == "square" else case.labels
    coef, grad, tot, h = case.run(labels, loss)
    m, c, lo, g, h_ref, near = case.reference(labels, loss)
    torch.testing.assert_close(coef, c, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(grad[case.live], g[case.live], rtol=1e-3, atol=1e-4)
    print(f"loss sum {float(tot[0]):.6f} ref {float(lo.double().sum()):.6f}; correct "
          f"{int(tot[1])} ref {int(((m > 0) == (labels > 0)).sum())}; rows {int(tot[2])}")
    assert abs(float(tot[0]) - float(lo.double().sum())) < 1e-3 * B
    assert int(tot[1]) == pytest.approx(int(((m > 0) == (labels > 0)).sum()), abs=3)
    assert int(tot[2]) == B
    # AUC histogram as cumulative counts: a row moves to a neighbouring bin only if its
    # p * nbins rounds differently, i.e. lies within 1e-3 of an integer
    assert int(h.sum()) == B
    diff = int((h.long().cumsum(0) - h_ref.cumsum(0)).abs().max())
    print(f"histogram: max cumulative difference {diff}, rows near a bin edge {near} of {B}")
    assert near < 0.01 * B
    assert diff <= near


@pytest.mark.parametrize("loss", ["logit", "square", "hinge", "square_hinge"])
@pytest.mark.parametrize("layout", ["tpf", "tp"])
def test_width39_pinned_tiles_all_losses(layout, loss, monkeypatch):
    monkeypatch.setenv("PSAMD_TILE_LTS", "13")
    case = _case(layout, 631, 39, False, 13)
    if layout == "tpf":
        assert case.lts == 13 and int(case.loc.nnz) % TILE == 33
    _check(case, loss)


def test_width39_unpinned_flat_single_pass(monkeypatch):
    monkeypatch.delenv("PSAMD_TILE_LTS", raising=False)
    case = _case("tpf", 631, 39, False, 0)
    assert case.lts == 10  # 1024 / 39 + 2 <= 128 rows: NP = 1
    _check(case)


@pytest.mark.parametrize("layout", ["tpf", "tp"])
def test_width9_eight_row_passes(layout, monkeypatch):
    monkeypatch.setenv("PSAMD_TILE_LTS", "13")
    case = _case(layout, 1900, 9, False, 13)
    _check(case)


@pytest.mark.parametrize("layout", ["tpf", "tp"])
def test_width64_valued_rows(layout, monkeypatch):
    monkeypatch.setenv("PSAMD_TILE_LTS", "13")
    case = _case(layout, 300, 64, True, 13)
    _check(case)


@pytest.mark.parametrize("layout", ["tpf", "tp"])
def test_repeated_launches_are_bitwise_equal(layout, monkeypatch):
    monkeypatch.setenv("PSAMD_TILE_LTS", "13")
    case = _case(layout, 631, 39, False, 13)
    outs = []
    for _ in range(3):
        coef, _, _, _ = case.run(case.labels, "logit")
        outs.append((coef.view(torch.int32).clone(), case.partials.view(torch.int32).clone()))
    # (as int32: partial slots past a tile's entry count are never written)
    for c, p in outs[1:]:
        assert torch.equal(outs[0][0], c) and torch.equal(outs[0][1], p)
