"""The per-example epilogue of the linear models (csrc/hip/loss.cuh) against references
that share no code with it.

(a) auc_hist_block against integers. The kernel's 2 x area is exact in u64 and is
followed by one conversion, one multiply and one divide in double, so the device AUC
must equal 0.5 * A2 / (P * N) of Python's integers to a few ulp of double (rtol 1e-15):
random stripes, ties only, perfect separation, one-class histograms, counts whose
products need 64 bits and whose stripe sum needs all 32.

(b) loss_terms, auc_bin and the metrics through linear_forward (linear.hip) and through
the fused tile kernel (tploc_fused.hip tp_fwd_bwd, which inlines loss.cuh separately),
against float64 loss_terms_torch, at planted margins: +-0, the hinge kink +-1 and the
softplus switch +-20 with their float32 neighbours, the expf overflow / underflow region
(+-50, +-88, +-89, +-104), labels +1 / -1 / 0 and real-valued ones. Every row has one
column with the planted weight and 38 columns of a zero-weight key, so its margin is the
planted value exactly.

Tolerances. xw, coef, coef2: the project's rtol 1e-5 / atol 1e-5
(test_linear_fwd_bwd_matches_torch). On the tail margins (|m| >= 19.9: both sides of the
softplus switch at 20, and everything beyond) atol alone would accept 0 for a loss or a
coefficient of 1e-9, so those are also held RELATIVELY: float32 loss_terms_torch deviates
from float64 there by at most 4.2e-8 (loss) and 6.8e-8 (coef), measured on the CPU over
these margins and labels (logit; square 3.9e-8 / 0, hinge 0 / 0, square hinge 2.6e-8 / 0);
TAIL_RTOL is 4 x the largest, the device expf / log1pf being other implementations
(COEF_TOL in test_fm_csr_gpu.py is the precedent). A float64 value below the smallest
normal float32 is expected as 0 or a denormal: atol only.

The kernels write no per-row loss, only its sum into metrics[0], where the rows with
y m = -104, -89, ... dominate. So each tail (margin, label) class is also launched as a
batch of its own (test_tail_loss_of_each_margin_class): one row carries the class and
every other row a margin whose float32 loss is exactly 0 (y m = 150 -- expf(-150) = 7e-66
is far below the smallest denormal -- and m = y for the square loss), so that metrics[0]
IS that row's loss, held to TAIL_RTOL of its float64 value.

The variable-width form of the tile kernel (tp_fwd_bwd_csr_kernel, which inlines the
epilogue a third time and handles empty rows itself) sees the same planted rows through
the harness of test_tp_fused_rows_gpu.py, in both layouts: rows of 1 to 64 columns plus
empty ones, the planted column carrying (weight m, value 1) or (weight 1, value m), every
other column a zero-weight key with a random value."""
import functools

import pytest
import torch

from parameter_server_amd.ops import KVTable, UpdateRule
from parameter_server_amd.ops.linear import (AUC_BINS, HIST_STRIPES, LOSS_TYPES, accum_total,
                                             auc_from_hist, linear_forward, linear_fwd_bwd,
                                             loss_terms_torch, new_accum)
from parameter_server_amd.ops.localize import Localizer, ensure_local_col
from parameter_server_amd.ops.native import hipops

from test_tp_fused_rows_gpu import _Case as FusedRowsCase

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TAIL_RTOL = 4 * 6.8e-8
TINY = torch.finfo(torch.float32).tiny
TAIL_FROM = 19.9  # (the inner float32 neighbour of 20 is 19.999998)
NB = AUC_BINS


# ------------------------------------------------------------------ (a) the AUC block
def auc_int_ref(neg, pos):
    """neg / pos: Python ints per bin. (AUC as float64 or None for a one-class histogram)"""
    below = a2 = 0
    for nb, pb in zip(neg, pos):
        a2 += pb * (2 * below + nb)
        below += nb
    P, N = sum(pos), below
    return 0.5 * a2 / (P * N) if P and N else None


def _as_i32(h):  # u32 counts as the int32 bit patterns the tensor holds
    return torch.where(h >= (1 << 31), h - (1 << 32), h).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _hist(name):
    """int64 [stripes, 2, NB] (negatives, positives)."""
    g = torch.Generator().manual_seed(11)
    one = lambda: torch.zeros(1, 2, NB, dtype=torch.int64)  # noqa: E731
    if name == "random-1":
        return torch.randint(0, 50, (1, 2, NB), generator=g)
    if name == "random-8":  # different contents per stripe, some bins empty
        h = torch.randint(0, 1000, (HIST_STRIPES, 2, NB), generator=g)
        return h * (torch.rand(HIST_STRIPES, 2, NB, generator=g) < 0.6)
    h = one()
    if name == "one-bin":
        h[0, 0, 777], h[0, 1, 777] = 12345, 678
    elif name == "separated":
        h[0, 0, :1000], h[0, 1, 1000:] = 3, 5
    elif name == "inverted":
        h[0, 0, 1000:], h[0, 1, :1000] = 3, 5
    elif name == "pos-only":
        h[0, 1] = torch.randint(0, 9, (NB,), generator=g)
    elif name == "neg-only":
        h[0, 0] = torch.randint(0, 9, (NB,), generator=g)
    elif name == "2^31-1":  # P * N and pos * 2 * below need 64 bits
        h[0, 0, 5], h[0, 1, 2040] = (1 << 31) - 1, (1 << 31) - 1
    elif name == "3e9-two-stripes":  # one bin's count only fits u32 as the stripe SUM
        h = torch.zeros(HIST_STRIPES, 2, NB, dtype=torch.int64)
        h[0, 0, 300] = h[5, 0, 300] = 1_500_000_000
        h[2, 1, 300], h[7, 1, 1999], h[3, 1, 17], h[1, 0, 1500] = 3, 5, 7, 11
    return h


HISTS = ["random-1", "random-8", "one-bin", "separated", "inverted", "pos-only", "neg-only",
         "2^31-1", "3e9-two-stripes"]
EXACT = {"one-bin": 0.5, "separated": 1.0, "inverted": 0.0, "2^31-1": 1.0}


@pytest.mark.parametrize("name", HISTS)
@pytest.mark.parametrize("entry", ["auc_from_hist", "kv_update"])
def test_auc_block_equals_the_integer_auc(entry, name):
    h = _hist(name)
    tot = h.sum(0)
    want = auc_int_ref(tot[0].tolist(), tot[1].tolist())
    if name in EXACT:
        assert want == EXACT[name]
    hist = _as_i32(h).reshape(-1).to(DEV)
    metrics = new_accum(DEV)
    if want is None:  # (what a one-class step must leave alone)
        metrics.view(-1, 16)[0, 3:5] = torch.tensor([0.25, 2.0], dtype=torch.float64)
    clock = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    if entry == "auc_from_hist":
        auc_from_hist(hist, metrics, clock)
    else:
        t = KVTable(256, DEV)
        slot, _ = t.resolve(torch.arange(1, 65, dtype=torch.int64, device=DEV))
        hipops().kv_update(t.slots, slot, torch.ones(64, device=DEV), None,
                           *UpdateRule("sgd", "constant", alpha=0.5).args(), new_accum(DEV),
                           hist=hist, metrics=metrics, step_counter=clock)
        assert bool((t.gather(slot) == -0.5).all())  # (and the update itself ran)
    m = accum_total(metrics).cpu()
    assert int(hist.count_nonzero()) == 0 and int(clock.item()) == 42
    if want is None:
        assert float(m[3]) == 0.25 and float(m[4]) == 2.0
    else:
        assert float(m[4]) == 1.0
        assert abs(float(m[3]) - want) <= 1e-15 * want, (float(m[3]), want)


# ------------------------------------------------------------------ (b) loss terms
def _nbrs(c):
    c = torch.tensor(c, dtype=torch.float32)
    return [float(c), float(torch.nextafter(c, c * 2)), float(torch.nextafter(c, c * 0))]


KINK = [s * v for c in (1.0, 20.0) for v in _nbrs(c) for s in (1, -1)]
PLANTED = [0.0, -0.0] + KINK + [s * v for v in (50.0, 88.0, 89.0, 104.0) for s in (1, -1)]
ZERO_LABELLED = [0.0, -0.0] + KINK[:6] + [20.0, -20.0, 104.0, -104.0]
WIDTH = 39


@functools.lru_cache(maxsize=None)
def _rows():
    """(margins float32 [257], labels float32 [257]); the last row is the NaN one."""
    g = torch.Generator().manual_seed(5)
    m = [v for v in PLANTED for _ in (0, 1)] + ZERO_LABELLED
    lab = [y for _ in PLANTED for y in (1.0, -1.0)] + [0.0] * len(ZERO_LABELLED)
    cyc = [1.0, -1.0, 0.0, 0.5, 3.0]  # (0.5 and 3.0: real labels for the square loss)
    while len(m) < 256:
        v = (torch.rand(1, generator=g) * 16 - 8).float()
        e = torch.sigmoid(v.double()) * NB
        if float((e - torch.round(e)).abs()) >= 1e-3:  # away from every bin edge
            m.append(float(v))
            lab.append(cyc[len(m) % 5])
    m, lab = m + [float("nan")], lab + [1.0]
    return torch.tensor(m, dtype=torch.float32), torch.tensor(lab, dtype=torch.float32)


def _bins64(m, lab):
    """float64 binning. The planted rows are safe by construction: m = 0 gives p = 0.5
    exactly in any precision, and the others are >= 1e-3 from an INTERIOR edge (asserted;
    a p * NB within 1e-3 of 0 or of NB stays in the first / last bin: floor and clamp)."""
    e = torch.sigmoid(m.double()) * NB
    k = torch.round(e)
    near = ((e - k).abs() < 1e-3) & (k >= 1) & (k <= NB - 1) & (m != 0)
    assert not near[~torch.isnan(m)].any()
    b = torch.clamp(torch.floor(e), 0, NB - 1)
    b = torch.where(torch.isnan(m), torch.zeros_like(b), b)  # NaN: bin 0 of its half
    return (b.long() + torch.where(lab > 0, NB, 0))


def _check_terms(got, ref, m, what, tail_rel=True):
    ok = ~torch.isnan(m)  # the NaN row is the only one left out
    torch.testing.assert_close(got[ok].double(), ref[ok], rtol=1e-5, atol=1e-5, msg=what)
    if not tail_rel:
        return
    tail = ok & (m.abs() >= TAIL_FROM) & (ref.abs() >= TINY)
    rel = ((got.double() - ref).abs() / ref.abs())[tail]
    print(what, "largest tail relative deviation", float(rel.max()) if rel.numel() else 0.0)
    assert bool((rel <= TAIL_RTOL).all()), (what, float(rel.max()))
    sub = ok & (ref.abs() < TINY)  # 0 or a denormal
    assert bool((got[sub].abs() < TINY).all()), what


@pytest.mark.parametrize("loss", ["logit", "square", "hinge", "square_hinge"])
def test_linear_forward_loss_terms_at_planted_margins(loss):
    m, lab = _rows()
    B = m.numel()
    col = torch.zeros(B, WIDTH, dtype=torch.int32)
    col[:, 0] = torch.arange(1, B + 1, dtype=torch.int32)
    w = torch.cat([torch.zeros(1), m])
    L = LOSS_TYPES[loss]
    lo64, c64, c264 = loss_terms_torch(m.double(), lab.double(), L)
    out = {}
    for nrow in (B, B - 1):  # with the NaN row, and without it for the loss sum
        xw, c, c2 = (torch.empty(nrow, device=DEV) for _ in range(3))
        met = torch.zeros(8, dtype=torch.float64, device=DEV)
        hist = torch.zeros(2 * NB, dtype=torch.int32, device=DEV)
        linear_forward(col[:nrow].reshape(-1).to(DEV), w.to(DEV), lab[:nrow].to(DEV), B=nrow,
                       width=WIDTH, loss=loss, xw=xw, coef=c, coef2=c2, metrics=met, hist=hist)
        out[nrow] = (xw.cpu(), c.cpu(), c2.cpu(), met.cpu(), hist.cpu())
    xw, c, c2, met, hist = out[B]
    ok = ~torch.isnan(m)
    assert torch.equal(xw[ok], m[ok]) and bool(torch.isnan(xw[~ok]).all())
    _check_terms(c, c64, m, loss + " coef")
    # (coef2 = tau * (1 - tau) cancels in float32 once tau rounds to 1, at y m <= -17: the
    # float32 reference gives 0 there too, 2e-9 absolute; no relative claim is made for it)
    _check_terms(c2, c264, m, loss + " coef2", tail_rel=False)
    want_hist = torch.bincount(_bins64(m, lab), minlength=2 * NB).to(torch.int32)
    assert torch.equal(hist, want_hist)  # exactly the float64 binning: 0 examples differ
    correct = int(((lab > 0) == (m > 0)).sum())  # (m = +-0 and NaN: predicted negative)
    assert float(met[2]) == B and float(met[1]) == correct
    _, _, _, met1, hist1 = out[B - 1]
    assert torch.equal(hist1, torch.bincount(_bins64(m, lab)[:-1], minlength=2 * NB).to(torch.int32))
    assert float(met1[2]) == B - 1 and float(met1[1]) == correct  # (the NaN row was wrong)
    torch.testing.assert_close(float(met1[0]), float(lo64[:-1].sum()), rtol=1e-6, atol=0)


@pytest.mark.parametrize("loss", ["logit", "square", "hinge", "square_hinge"])
def test_fused_tile_forward_loss_terms_at_planted_margins(loss):
    """The same rows through tp_fwd_bwd on a "tp" localisation at width 39."""
    m, lab = _rows()
    B = m.numel()
    keys = torch.full((B, WIDTH), 7, dtype=torch.int64)
    keys[:, 0] = torch.arange(1000, 1000 + B)
    keys = keys.reshape(-1).to(DEV)
    loc = Localizer(keys.numel(), 30, DEV, mode="tp", lazy_cols=True)
    assert loc.mode == "tp"
    L = loc(keys)
    U = int(L.n_uniq.item())
    assert U == B + 1
    lo64, c64, _ = loss_terms_torch(m.double(), lab.double(), LOSS_TYPES[loss])
    cols = ensure_local_col(L)[:keys.numel()].view(B, WIDTH).long().clone()
    out = {}
    for nan_row in (True, False):
        mm = m.clone()
        if not nan_row:
            mm[-1] = 0.0
        w = torch.zeros(U, device=DEV)
        w[cols[:, 0]] = mm.to(DEV)
        coef = torch.empty(B, device=DEV)
        met = new_accum(DEV)
        hist = torch.zeros(HIST_STRIPES * 2 * NB, dtype=torch.int32, device=DEV)
        L = loc(keys)  # (a fresh lazy localisation: the fused kernel, not linear_forward)
        linear_fwd_bwd(L, w, lab.to(DEV), B=B, width=WIDTH, loss=loss, coef=coef, metrics=met,
                       hist=hist)
        torch.cuda.synchronize()
        assert not L.tile.cols_ready
        out[nan_row] = (coef.cpu(), accum_total(met).cpu(),
                        hist.view(-1, 2 * NB).sum(0).cpu().to(torch.int32))
        assert torch.equal(ensure_local_col(L)[:keys.numel()].view(B, WIDTH).long(), cols)
    c, met, hist = out[True]
    _check_terms(c, c64, m, loss + " fused coef")
    assert torch.equal(hist, torch.bincount(_bins64(m, lab), minlength=2 * NB).to(torch.int32))
    correct = int(((lab > 0) == (m > 0)).sum())
    assert float(met[2]) == B and float(met[1]) == correct
    c1, met1, _ = out[False]  # the last row at margin 0 (label +1): a finite loss sum
    m0 = m.clone()
    m0[-1] = 0.0
    lo0 = loss_terms_torch(m0.double(), lab.double(), LOSS_TYPES[loss])[0]
    torch.testing.assert_close(float(met1[0]), float(lo0.sum()), rtol=1e-6, atol=0)
    assert float(met1[1]) == correct


# ------------------------------------------------------------------ one launcher per path
LOSSES = ["logit", "square", "hinge", "square_hinge"]
PATHS = ["linear_forward", "tp", "csr-tpf", "csr-tp"]
TILE = 8192


def _csr_widths(nrows, empties=True):
    """1 to 64 columns per row, and six empty rows: two leading, two in the middle, two
    trailing (the kernel gives those their margin-0 terms outside its row windows)."""
    w = tuple(1 + (37 * r) % 64 for r in range(nrows))
    e = (0, 0) if empties else ()
    return e + w[:nrows // 2] + e + w[nrows // 2:] + e


@functools.lru_cache(maxsize=None)
def _launcher(path, widths=None):
    """run(m, lab, loss) -> (coef, metrics total, histogram over the stripes), on the CPU:
    one launch of ``path``'s kernel on rows whose margins are ``m`` exactly (an empty row's
    entry of ``m`` is not used: its margin is 0). The keys and their localisation are
    built once; only weights, values and labels change from run to run."""
    B = len(widths) if widths else _rows()[0].numel()
    if path == "linear_forward":
        col = torch.zeros(B, WIDTH, dtype=torch.int32)
        col[:, 0] = torch.arange(1, B + 1, dtype=torch.int32)
        col = col.reshape(-1).to(DEV)

        def run(m, lab, loss):
            xw, c, c2 = (torch.empty(B, device=DEV) for _ in range(3))
            met = torch.zeros(8, dtype=torch.float64, device=DEV)
            hist = torch.zeros(2 * NB, dtype=torch.int32, device=DEV)
            linear_forward(col, torch.cat([torch.zeros(1), m]).to(DEV), lab.to(DEV), B=B,
                           width=WIDTH, loss=loss, xw=xw, coef=c, coef2=c2, metrics=met, hist=hist)
            return c.cpu(), met.cpu(), hist.cpu()
        return run
    if path == "tp":
        keys = torch.full((B, WIDTH), 7, dtype=torch.int64)
        keys[:, 0] = torch.arange(1000, 1000 + B)
        keys = keys.reshape(-1).to(DEV)
        loc = Localizer(keys.numel(), 30, DEV, mode="tp", lazy_cols=True)
        L = loc(keys)
        U = int(L.n_uniq.item())
        cols = ensure_local_col(L)[:keys.numel()].view(B, WIDTH).long().clone()

        def run(m, lab, loss):
            w = torch.zeros(U, device=DEV)
            w[cols[:, 0]] = m.to(DEV)
            coef = torch.empty(B, device=DEV)
            met = new_accum(DEV)
            hist = torch.zeros(HIST_STRIPES * 2 * NB, dtype=torch.int32, device=DEV)
            L = loc(keys)  # (a fresh lazy localisation: the fused kernel, not linear_forward)
            linear_fwd_bwd(L, w, lab.to(DEV), B=B, width=WIDTH, loss=loss, coef=coef, metrics=met,
                           hist=hist)
            torch.cuda.synchronize()
            assert not L.tile.cols_ready
            out = (coef.cpu(), accum_total(met).cpu(),
                   hist.view(-1, 2 * NB).sum(0).cpu().to(torch.int32))
            assert torch.equal(ensure_local_col(L)[:keys.numel()].view(B, WIDTH).long(), cols)
            return out
        return run
    layout = path[4:]
    wd = torch.tensor(widths)
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), wd.cumsum(0)])
    n = int(row_ptr[-1])
    assert n > TILE  # more than one tile in the compact layout too
    rows = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), wd)
    g = torch.Generator().manual_seed(7)
    keys = torch.randint(10 ** 6, 10 ** 6 + 5000, (n,), generator=g)  # (their weights stay 0)
    full = wd > 0
    first = row_ptr[:-1][full]  # the planted column of every non-empty row
    keys[first] = 1000 + torch.arange(B)[full]
    vals0 = torch.rand(n, generator=g) + 0.5
    case = FusedRowsCase(layout, B, 0, True, batch=(keys.to(DEV), None, None, vals0.to(DEV)))
    if layout == "tpf":
        assert int(case.loc.err.item()) == 0 and (1 << case.lts) < n
    by_value = (torch.arange(B) % 2 == 1)[full]  # odd rows: weight 1, value m
    wcol = case.cols[first.to(DEV)]
    row_ptr, rows = row_ptr.to(DEV), rows.to(DEV)

    def run(m, lab, loss):
        mm = m[full]
        vals = vals0.clone()
        vals[first] = torch.where(by_value, mm, torch.ones_like(mm))
        case.vals = vals.to(DEV)
        case.w.zero_()
        case.w[wcol] = torch.where(by_value, torch.ones_like(mm), mm).to(DEV)
        coef, _, met, hist = case.run_csr(lab.to(DEV), loss, row_ptr, rows)
        return coef.cpu(), met, hist.to(torch.int32)
    return run


@functools.lru_cache(maxsize=None)
def _csr_rows():
    """_rows() laid out on _csr_widths: (margins, labels, widths); an empty row's margin
    is 0 and the six of them carry the labels +1, -1, 0, +1, -1, 0."""
    m, lab = _rows()
    widths = _csr_widths(m.numel())
    mm, ll, src, lab_e = [], [], iter(range(m.numel())), iter([1.0, -1.0, 0.0] * 2)
    for w in widths:
        i = next(src) if w else None
        mm.append(float(m[i]) if w else 0.0)
        ll.append(float(lab[i]) if w else next(lab_e))
    return torch.tensor(mm, dtype=torch.float32), torch.tensor(ll, dtype=torch.float32), widths


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("layout", ["tpf", "tp"])
def test_csr_tile_forward_loss_terms_at_planted_margins(layout, loss, monkeypatch):
    """The planted rows through tp_fwd_bwd_csr, in the flat and the compact layout."""
    monkeypatch.delenv("PSAMD_TILE_LTS", raising=False)
    m, lab, widths = _csr_rows()
    B = m.numel()
    assert int(torch.isnan(m).sum()) == 1
    run = _launcher("csr-" + layout, widths)
    c64 = loss_terms_torch(m.double(), lab.double(), LOSS_TYPES[loss])[1]
    c, met, hist = run(m, lab, loss)
    _check_terms(c, c64, m, f"{loss} csr {layout} coef")
    assert torch.equal(hist, torch.bincount(_bins64(m, lab), minlength=2 * NB).to(torch.int32))
    correct = int(((lab > 0) == (m > 0)).sum())  # (m = +-0, empty rows and NaN: negative)
    assert float(met[2]) == B and float(met[1]) == correct
    m0 = torch.nan_to_num(m, nan=0.0)  # the NaN row (label +1) at margin 0: a finite sum
    _, met0, _ = run(m0, lab, loss)
    lo0 = loss_terms_torch(m0.double(), lab.double(), LOSS_TYPES[loss])[0]
    print(loss, layout, "loss sum", float(met0[0]), "float64", float(lo0.sum()))
    assert float(met0[2]) == B and float(met0[1]) == correct
    torch.testing.assert_close(float(met0[0]), float(lo0.sum()), rtol=1e-6, atol=0)


def _tail_classes():
    """The distinct (margin, label) pairs of the planted rows with |m| >= TAIL_FROM."""
    m, lab = _rows()
    sel = ~torch.isnan(m) & (m.abs() >= TAIL_FROM)
    return list(dict.fromkeys(zip(m[sel].tolist(), lab[sel].tolist())))


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("path", PATHS)
def test_tail_loss_of_each_margin_class(path, loss, monkeypatch):
    """metrics[0] of a batch in which ONE row carries the class and all others lose exactly
    0 in float32: that row's loss, relative to its float64 value (the expf(x) branch of
    softplus below -20, the log1pf(expf(x)) side just above it, underflow beyond)."""
    monkeypatch.delenv("PSAMD_TILE_LTS", raising=False)
    B, row = _rows()[0].numel(), 100
    run = _launcher(path, _csr_widths(B, empties=False) if path.startswith("csr") else None)
    fill_m = torch.full((B,), 1.0 if loss == "square" else 150.0)
    fill_lab = torch.ones(B)
    assert float(run(fill_m, fill_lab, loss)[1][0]) == 0.0
    classes = _tail_classes()
    assert len(classes) >= 28
    worst = 0.0
    for mv, y in classes:
        m, lab = fill_m.clone(), fill_lab.clone()
        m[row], lab[row] = mv, y
        want = float(loss_terms_torch(m.double(), lab.double(), LOSS_TYPES[loss])[0].sum())
        got = float(run(m, lab, loss)[1][0])
        if want < TINY:  # 0 or a denormal
            assert 0.0 <= got < TINY, (mv, y, got, want)
        else:
            worst = max(worst, abs(got - want) / want)
            assert abs(got - want) <= TAIL_RTOL * want, (mv, y, got, want)
    print(path, loss, "largest relative deviation of a tail loss", worst)
