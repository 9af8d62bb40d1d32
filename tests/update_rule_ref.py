"""Float64 reference of the per-key optimizer recurrence, written from the formulas
(learning rate CONSTANT = alpha, DECAY = alpha / (x + beta); elastic-net proximal
operator; FTRL-proximal, proximal AdaGrad, proximal SGD with a per-key step count), and
the case grid the update-rule tests share (test_update_rule.py for the host kernels,
test_update_rule_gpu.py for the device ones).

One call applies a SEQUENCE of pushes to K independent keys at once (tensors of shape
[K], gradients [T, K]); each key sees exactly the scalar recurrence:

    g = grad * grad_scale                  NaN: the push is skipped, nothing changes
    FTRL     n' = sqrt(n^2 + g^2); z += g - (n' - n) / alpha * w; n = n'
             eta = alpha | alpha / (n' + beta);      w' = prox(-z * eta, eta)
    AdaGrad  n += g^2; eta = alpha / (beta + sqrt(n)); w' = prox(w - eta * g, eta)
    SGD      cnt += 1; eta = alpha | alpha / (beta + sqrt(cnt)); w' = prox(w - eta * g, eta)
    prox(x, eta) = 0 on the CLOSED interval |x| <= l1 * eta,
                   else (x - sign(x) * l1 * eta) / (1 + l2 * eta)
    max_delta > 0: w' = w + clamp(w' - w, -max_delta, max_delta); z and n keep their
                   unclipped values

The rule's scalars are rounded to float32 first: that is how the kernels hold them, and
the reference is of the rule with those parameters. ``dtype`` selects the arithmetic:
float64 is the reference, float32 the same code at the kernels' precision (used to show
that the project tolerances hold for the reference alone, and that no key sits so close
to a discontinuity -- the prox threshold, the clip -- that rounding decides its side)."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace

import torch

from parameter_server_amd.ops.kv_table import UpdateRule


def _f32(x: float) -> float:
    return float(torch.tensor(float(x), dtype=torch.float32))


@dataclass
class PushTrace:
    """What one push did, per key: applied (gradient not NaN), w == 0 afterwards, clipped
    by max_delta, and the relative distance of the key from the nearer discontinuity."""
    applied: torch.Tensor
    zero: torch.Tensor
    clipped: torch.Tensor
    margin: torch.Tensor


def apply_pushes(state, grads, rule: UpdateRule, dtype=torch.float64):
    """state = (w, z, n, cnt) tensors [K]; grads [T, K] (NaN = filtered push).
    Returns (new state in ``dtype``, stats, [PushTrace per push]); stats = (dnnz int,
    sum w_new^2, sum (w_new - w_old)^2), the sums in float64 over the weights rounded to
    float32 (what a float32 table stores), one term per applied push."""
    w, z, n, cnt = (t.detach().clone().to(dtype) for t in state)
    grads = grads.reshape(-1, w.numel()).to(dtype)
    alpha, beta, l1, l2, gs, md = (_f32(v) for v in (rule.alpha, rule.beta, rule.l1, rule.l2,
                                                      rule.grad_scale, rule.max_delta))
    algo, const = rule.algo.lower(), rule.lr_type.lower() == "constant"
    dnnz, sw2, sd2, trace = 0, 0.0, 0.0, []
    tiny = torch.finfo(torch.float32).tiny
    for t in range(grads.shape[0]):
        g = grads[t] * gs
        ok = ~torch.isnan(g)
        g = torch.where(ok, g, torch.zeros_like(g))
        if algo == "ftrl":
            n_new = torch.sqrt(n * n + g * g)
            z_new = z + g - (n_new - n) / alpha * w
            eta = torch.full_like(w, alpha) if const else alpha / (n_new + beta)
            x = -z_new * eta
            c_new = cnt
        elif algo == "adagrad":
            n_new = n + g * g
            z_new = z
            eta = alpha / (beta + torch.sqrt(n_new))
            x = w - eta * g
            c_new = cnt
        else:
            c_new = cnt + 1
            n_new, z_new = n, z
            eta = torch.full_like(w, alpha) if const else alpha / (beta + torch.sqrt(c_new))
            x = w - eta * g
        leta = l1 * eta
        w_new = torch.where(x.abs() <= leta, torch.zeros_like(x),
                            (x - torch.sign(x) * leta) / (1 + l2 * eta))
        # (l1 = 0: the prox is continuous and gives 0 only for x == 0 exactly: no threshold)
        margin = (x.abs() - leta).abs() / torch.maximum(x.abs(), leta).clamp(min=tiny) \
            if l1 > 0 else torch.full_like(x, math.inf)
        d = w_new - w
        clipped = torch.zeros_like(ok)
        if md > 0:
            clipped = d.abs() > md
            # (a weight clipped to exactly +-max_delta from 0 that the prox sends back to 0
            # moves by exactly max_delta in any precision: 0 -+ max_delta is exact. Not a
            # near miss: the strict comparison leaves it unclipped everywhere)
            tie = (w_new == 0) & (w.abs() == md)
            margin = torch.minimum(margin, torch.where(
                tie, torch.full_like(d, math.inf), (d.abs() - md).abs() / md))
            w_new = torch.where(d > md, w + md, torch.where(d < -md, w - md, w_new))
        w_old = w
        w = torch.where(ok, w_new, w)
        z = torch.where(ok, z_new, z)
        n = torch.where(ok, n_new, n)
        cnt = torch.where(ok, c_new, cnt)
        a, b = w.float().double()[ok], w_old.float().double()[ok]
        dnnz += int((a != 0).sum()) - int((b != 0).sum())
        sw2 += float((a * a).sum())
        sd2 += float(((a - b) ** 2).sum())
        inf = torch.full_like(margin, math.inf)
        trace.append(PushTrace(ok, w == 0, clipped & ok, torch.where(ok, margin, inf)))
    return (w, z, n, cnt), (dnnz, sw2, sd2), trace


def zero_state(K: int):
    return tuple(torch.zeros(K, dtype=torch.float64) for _ in range(4))


# ------------------------------------------------------------------ tolerances
# The project's own values for this rule (test_kv_update_matches_torch).
RTOL, ATOL = 2e-5, 2e-6
# No key of a case may be nearer than this (relative) to the prox threshold or to the clip
# bound, the planted threshold keys apart: float32 rounding (2^-24 per operation, a handful
# of operations, and a device compiler free to contract a * b + c) then cannot move a key
# across, and the zero pattern, the nnz delta and the clipped set are exact expectations.
MARGIN = 1e-6


def close(got, ref, scale=None, rtol=RTOL, atol=ATOL):
    """|got - ref| <= atol * scale + rtol * |ref| per key. ``scale`` = max(1, largest
    |gradient| pushed to the key): an absolute tolerance presumes values of order one, and
    the planted +-1e4 gradients carry state of order 1e4 whose float32 spacing is 1e-3."""
    got, ref = got.double(), ref.double()
    tol = atol * (scale.double() if scale is not None else 1.0) + rtol * ref.abs()
    bad = ~((got - ref).abs() <= tol)
    assert not bad.any(), (int(bad.sum()), got[bad][:5], ref[bad][:5])


# ------------------------------------------------------------------ the case grid
ALGOS = [("ftrl", "decay"), ("ftrl", "constant"), ("adagrad", "decay"), ("sgd", "decay"),
         ("sgd", "constant")]
BIND, BIG_L1 = "bind", "big"  # placeholders the case builder resolves from the data
# (l1, l2, beta, grad_scale, max_delta): every value of every axis, max_delta binding
# together with grad_scale != 1 twice; each runs with all five (algo, lr_type) above
PENALTIES = {
    "plain": (0.0, 0.0, 1.0, 1.0, 0.0),
    "l2-gs64-clip": (0.0, 0.5, 1.0, 1 / 64, BIND),
    "l1-beta0-gs.3-loose": (0.05, 0.0, 0.0, 0.3, 1e3),
    "l1l2-gs.3-clip": (0.05, 0.5, 1.0, 0.3, BIND),
    "l1l2-clip": (0.05, 0.5, 1.0, 1.0, BIND),
    "bigl1": (BIG_L1, 0.5, 1.0, 1.0, 0.0),
    "beta0-gs64": (0.0, 0.0, 0.0, 1 / 64, 0.0),
}
# the rows whose l1 / grad_scale is exact in float32, so that a gradient lands exactly on
# the prox threshold (_plant): these must carry the planted threshold keys
THRESHOLD_ROWS = ("l1l2-clip", "bigl1")
PUSHES = 4
INVALID_SLOTS = 3  # -1, capacity, capacity + 5 in every slot list


@dataclass
class Case:
    rule: UpdateRule
    grads: torch.Tensor       # [T, K] float32, NaN = filtered / absent
    scale: torch.Tensor       # [K] atol scale (see close)
    ref: tuple                # float64 state after all pushes
    stats: tuple
    trace: list
    thresh: torch.Tensor      # [K] bool: the planted prox-threshold keys


def _plant(g, rule_args, summed=False):
    """Planted gradients into columns 0.. of g [T, K]; returns the threshold mask."""
    l1, beta, gs, big = rule_args
    T, K = g.shape
    thresh = torch.zeros(K, dtype=torch.bool)
    if K < 16:
        return thresh
    last = T - 1
    col = 0
    if beta != 0:  # (eta = alpha / (0 + beta) needs a non-zero gradient at beta = 0)
        g[0, 0], g[0, 1], g[min(2, last), 0], g[last, 1] = 0.0, -0.0, 0.0, -0.0
        if summed:
            g[:, 0] = 0.0  # (touched, and the sum is a zero gradient)
        col = 2
    if T >= 2:
        g[1, col] = float("nan")  # NaN on the 2nd push only
    if summed:  # (the sums must stay exact in float32: no tiny / huge terms)
        return thresh
    g[0, col + 1], g[0, col + 2] = 1e-12, -1e-12
    g[min(2, last), col + 1] = -1e-12
    col += 3
    if not big:  # (the big-l1 case wants EVERY weight 0 after the first push)
        # on the LAST push: float32 FTRL state of order 1e4 cannot resolve the n' - n of a
        # later order-one gradient (spacing 1e-3), which is the rule's own property
        g[last, col], g[last, col + 1] = 1e4, -1e4
        col += 2
    if l1 > 0:
        # first push from the zero state: |x| = eta * g and the threshold l1 * eta are the
        # same product when g * grad_scale == l1 -> the closed interval's edge. Planted
        # where a float32 gradient gives that EXACTLY (grad_scale a power of two), so that
        # it holds in float32 and in float64 alike
        l1f = torch.tensor(l1, dtype=torch.float32)
        gsf = torch.tensor(gs, dtype=torch.float32)
        cand = l1f / gsf
        if float(cand.double() * gsf.double()) == float(l1f):
            g[0, col], g[0, col + 1] = cand, -cand
            thresh[col:col + 2] = True
    return thresh


@functools.lru_cache(maxsize=None)
def build_case(algo: str, lr: str, pen: str, K: int = 1000, T: int = PUSHES,
               summed: bool = False, w0: float = 0.0, absent: float = 0.0) -> Case:
    """``T`` pushes; ``absent``: that fraction of the (push, key) pairs is NaN (a source row
    without the key, or a filtered entry: both leave the key alone); ``summed``: the
    reference is ONE push of each key's gradient sum (the aggregated push), the gradients
    multiples of 2^-10 so that their float32 sum is exact in any order; ``w0``: the
    weight every key starts from (a table with a constant init).

    The case (algo, lr, penalty row, K keys), built once: gradients randn * 0.3 with
    the planted keys, the float64 reference, and the proof that the reference ALONE meets
    the tolerances the kernels are held to: its float32 run is within (RTOL, ATOL) of its
    float64 run on w, z, n, has the same zero pattern and clipped set after every push, and
    no key is within MARGIN of a discontinuity (reseeded until so; the planted threshold
    keys, expected exactly 0 by construction, apart)."""
    l1, l2, beta, gs, md = PENALTIES[pen]
    big = l1 == BIG_L1
    for seed in range(64):
        gen = torch.Generator().manual_seed(1000 * seed + K + 17 * T)
        g = (torch.randn(T, K, generator=gen) * 0.3).float()
        if big:
            g[0] *= 0.5  # first push small, so one l1 zeroes every weight, later ones leave
        if summed:
            g = torch.round(g * 1024) / 1024
        if absent:
            g[torch.rand(T, K, generator=gen) < absent] = float("nan")
            g[:, K // 3] = float("nan")  # one key in no push at all
        l1v = _f32(1.01 * float(g[0].abs().max()) * gs) if big else l1
        thresh = _plant(g, (l1v, beta, gs, big), summed) if w0 == 0 else \
            torch.zeros(K, dtype=torch.bool)
        gin = g
        if summed:  # NaN-skipping sum; a key with no finite push stays untouched (NaN)
            gin = torch.nan_to_num(g).double().sum(0, keepdim=True).float()
            assert torch.equal(gin.double(), torch.nan_to_num(g).double().sum(0, keepdim=True))
            gin[0, torch.isnan(g).all(0)] = float("nan")
        start = (torch.full((K,), float(w0), dtype=torch.float64),) + zero_state(K)[1:]
        rule = UpdateRule(algo, lr, alpha=0.1, beta=beta, l1=l1v, l2=l2, grad_scale=gs,
                          max_delta=0.0 if md == BIND else md)
        if md == BIND:  # binds for most keys on the first push: 0.3 x the median first step
            st1, _, _ = apply_pushes(start, gin[:1], rule)
            step = (st1[0] - start[0]).abs()
            step = step[(step > 0) & (gin[0].abs() < 10)]
            rule = replace(rule, max_delta=_f32(0.3 * float(step.median())))
        ref, stats, trace = apply_pushes(start, gin, rule)
        lo, stats32, trace32 = apply_pushes(start, gin, rule, dtype=torch.float32)
        same = all(torch.equal(a.zero, b.zero) and torch.equal(a.clipped, b.clipped)
                   for a, b in zip(trace, trace32))
        # (the threshold keys are exempt on the push that plants them, the first, only)
        far = bool((trace[0].margin[~thresh] >= MARGIN).all()) and \
            all(bool((t.margin >= MARGIN).all()) for t in trace[1:])
        if same and far:
            break
    else:
        raise AssertionError(f"no seed keeps {algo}/{lr}/{pen}/{K}/{T} off the discontinuities")
    scale = torch.nan_to_num(g).abs().amax(0).clamp(min=1.0)
    for a, b in zip(lo[:3], ref[:3]):  # the reference alone meets the project tolerance
        close(a, b, scale)
    assert torch.equal(lo[3].double(), ref[3]) and stats32[0] == stats[0]
    for a, b in zip(stats32[1:], stats[1:]):  # (and the 1e-5 of the two sums)
        assert math.isclose(a, b, rel_tol=1e-5, abs_tol=1e-30), (a, b)
    if pen in THRESHOLD_ROWS and K >= 16 and not summed and w0 == 0:
        assert thresh.any()  # every algorithm meets the closed interval's edge in these rows
    if thresh.any():
        assert bool(trace[0].zero[thresh].all())
    if md == BIND and K >= 16 and not absent:
        assert trace[0].clipped.float().mean() > 0.3, float(trace[0].clipped.float().mean())
    if md == 1e3:
        assert not any(bool(t.clipped[scale <= 1].any()) for t in trace)  # (+-1e4 keys may)
    if big and not absent and not summed and w0 == 0:
        assert bool(trace[0].zero.all()) and not bool(trace[-1].zero.all())
    return Case(rule, g, scale, ref, stats, trace, thresh)


def case_ids():
    """(algo, lr, penalty, K): the whole penalty grid at K = 1000, and the wave-boundary
    key counts (the per-wave stats sums are added by lane 63) on one clipped row."""
    ids = [(a, lr, p, 1000) for a, lr in ALGOS for p in PENALTIES]
    ids += [(a, lr, "l1l2-gs.3-clip", K) for a, lr in ALGOS for K in (1, 63, 64, 65)]
    return ids


def slot_list(slot: torch.Tensor, capacity: int):
    """``slot`` [K] with the INVALID_SLOTS invalid entries spliced in (front, middle, end);
    returns (slot list, index of every valid entry in it)."""
    K = slot.numel()
    bad = torch.tensor([-1, capacity, capacity + 5], dtype=torch.int64, device=slot.device)
    h = K // 2
    full = torch.cat([bad[:1], slot[:h], bad[1:2], slot[h:], bad[2:]])
    pos = torch.cat([torch.arange(1, 1 + h), torch.arange(2 + h, 2 + K)])
    return full, pos


def with_invalid(g: torch.Tensor, pos: torch.Tensor, total: int):
    """A gradient row [K] spread to the slot list's length; the invalid entries carry 7.0
    (a finite gradient that would show in the stats if it were applied anywhere)."""
    out = torch.full((total,), 7.0, dtype=torch.float32)
    out[pos] = g
    return out


def check_table(table, slot, case: Case, stats_total):
    """w, z, n, cnt of ``slot`` (-1: a key never inserted, all zero) and the three stats
    against the case's float64 reference; the zero pattern and the nnz delta exactly."""
    w, z, n = (table.gather(slot, f).cpu() for f in range(3))
    rw, rz, rn, rc = case.ref
    cnt = table.slots.view(torch.int32)[slot.clamp(min=0), 6].cpu()
    assert torch.equal(torch.where(slot.cpu() >= 0, cnt, 0).double(), rc)
    close(w, rw, case.scale)
    close(z, rz, case.scale)
    close(n, rn, case.scale)
    assert torch.equal(w == 0, case.trace[-1].zero)
    dnnz, sw2, sd2 = case.stats
    got = [float(v) for v in stats_total[:3]]
    assert got[0] == dnnz, (got[0], dnnz)
    assert math.isclose(got[1], sw2, rel_tol=1e-5, abs_tol=1e-30), (got[1], sw2)
    assert math.isclose(got[2], sd2, rel_tol=1e-5, abs_tol=1e-30), (got[2], sd2)
