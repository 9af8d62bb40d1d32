"""Every device entry of the shared optimizer rule (kv_slot.cuh apply_update +
soft_threshold_prox) against the float64 recurrence of tests/update_rule_ref.py:
kv_update, kv_accumulate + kv_apply_accumulated, the per-push owner applies
kv_update_rows and kv_apply_part (through the helpers of test_owner_apply_gpu.py), and the
fused 1-GPU step kernels (tpf_step, tp_seg_update) through SparseLRTrainer. The case grid
-- l1 / l2 / beta = 0, grad_scale != 1, max_delta binding and not, planted zero / NaN /
tiny / huge gradients, prox-threshold keys, invalid slots -- is the helper's; the host
twin is test_update_rule.py.

Tolerances: the project's rtol 2e-5 / atol 2e-6 on w, z, n (the helper's ``close``) and
rtol 1e-4 with atol 1e-5 (w) / 1e-4 (z, n) at trainer level; each case's builder asserts
that the float32 run of the reference itself is within them of its float64 run, and that
no key is within 1e-6 (relative) of the prox threshold or the clip bound, so the zero
pattern and the nnz delta are compared exactly."""
import functools
import math
from dataclasses import replace

import pytest
import torch

from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
from parameter_server_amd.models.sparse_lr import algo_defaults
from parameter_server_amd.ops import KVTable
from parameter_server_amd.ops.keymix import unmix
from parameter_server_amd.ops.kv_table import InitRule
from parameter_server_amd.ops.linear import accum_total, new_accum
from parameter_server_amd.ops.native import hipops
from parameter_server_amd.ops.synthetic import criteo_batch

from test_owner_apply_gpu import apply_rows, pack_rows, resolve_rows
from update_rule_ref import (ALGOS, MARGIN, apply_pushes, build_case, case_ids, check_table, close,
                             slot_list, with_invalid, zero_state)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
# kv_update's launcher caps its grid at 2048 blocks of 256 threads: one more wave than
# that makes the grid-stride loop take a second trip
BIG_K = 2048 * 256 + 65


def _table(K, init=None):
    t = KVTable(4 * K, DEV, init)
    slot, _ = t.resolve((torch.arange(1, K + 1, dtype=torch.int64) * 7919).to(DEV))
    assert torch.unique(slot).numel() == K and int(slot.min()) >= 0
    return t, slot


def _untouched(t, slot, before):
    other = torch.ones(t.capacity, dtype=torch.bool, device=DEV)
    other[slot] = False
    assert torch.equal(t.slots[other], before[other])  # nothing but the K slots moved


@pytest.mark.parametrize("algo,lr,pen,K", case_ids() + [("ftrl", "decay", "l1l2-gs.3-clip", BIG_K)])
def test_kv_update_matches_float64_reference(algo, lr, pen, K):
    case = build_case(algo, lr, pen, K)
    t, slot = _table(K)
    full, pos = slot_list(slot, t.capacity)
    before = t.slots.clone()
    stats = new_accum(DEV)
    for g in case.grads:
        t.update(full, with_invalid(g, pos, full.numel()).to(DEV), case.rule, stats)
    check_table(t, slot, case, accum_total(stats).cpu())
    _untouched(t, slot, before)


@pytest.mark.parametrize("algo,lr", ALGOS)
@pytest.mark.parametrize("pen,w0", [("l1l2-gs.3-clip", 0.0), ("l2-gs64-clip", 0.25)])
def test_accumulate_then_apply_is_one_update_of_the_sum(algo, lr, pen, w0):
    """A slot touched k times gets ONE update with grad_scale * (sum of its gradients);
    acc returns to 0, the touched mark (flag bit 0) is cleared and the published-init
    mark (bit 1, set on a table with a non-zero init) survives."""
    K = 1000
    case = build_case(algo, lr, pen, K, summed=True, absent=0.3, w0=w0)
    t, slot = _table(K, InitRule("constant", w0) if w0 else None)
    full, pos = slot_list(slot, t.capacity)
    T = case.grads.shape[0]
    slots_all = full.repeat(T)
    grads_all = torch.cat([with_invalid(g, pos, full.numel()) for g in case.grads]).to(DEV)
    touched = torch.full((slots_all.numel(),), -1, dtype=torch.int64, device=DEV)
    nt = torch.zeros(1, dtype=torch.int32, device=DEV)
    flags0 = t.slots.view(torch.int32)[:, 7].clone()
    assert bool((flags0[slot] == (2 if w0 else 0)).all())
    H = hipops()
    H.kv_accumulate(t.slots, slots_all, grads_all, None, touched, nt)
    live = ~torch.isnan(case.grads).all(0)
    assert int(nt.item()) == int(live.sum())
    gsum = torch.nan_to_num(case.grads).double().sum(0)
    assert torch.equal(t.gather(slot, 3).cpu().double(), gsum)  # (exact: multiples of 2^-10)
    assert torch.equal(t.slots.view(torch.int32)[slot, 7].cpu() & 1, live.to(torch.int32))
    before = t.slots.clone()
    stats = new_accum(DEV)
    H.kv_apply_accumulated(t.slots, touched, nt, *case.rule.args(), stats)
    check_table(t, slot, case, accum_total(stats).cpu())
    assert int(t.gather(slot, 3).abs().sum()) == 0
    assert torch.equal(t.slots.view(torch.int32)[:, 7], flags0)
    _untouched(t, slot, before)


@pytest.mark.parametrize("algo,lr", ALGOS)
@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("kernel", ["kv_update_rows", "kv_apply_part"])
def test_owner_apply_is_the_rule_push_by_push(kernel, G, algo, lr):
    """G source rows with overlapping key sets: every push is its own optimizer step, in
    source-rank order -- SGD's count advances once per push, and each push clips against
    the weight the push before left. Row s holds, sorted, the keys whose push s is finite
    and the NaN-marked ones of ``keep_nan`` (those travel too, and are skipped)."""
    K, C, lgP = 1000, 1024, 3
    case = build_case(algo, lr, "l1l2-gs.3-clip", K, T=G, absent=0.4 if G > 1 else 0.1)
    lo, span = 1 << 20, 1 << 22
    gen = torch.Generator().manual_seed(G)
    keys = torch.sort(torch.randperm(span, generator=gen)[:K]).values + lo
    keep_nan = torch.arange(K) % 5 == 0
    sent = [~torch.isnan(g) | keep_nan for g in case.grads]
    recv, H = pack_rows([(keys[sel], g[sel]) for g, sel in zip(case.grads, sent)], C)
    recv = recv.to(DEV)
    t = KVTable(1 << 12, DEV, key_range=(lo, lo + span))
    slot, rkeys, bnd = resolve_rows(t, recv, H, C, G, lgP)
    stats = torch.zeros(3, dtype=torch.float64, device=DEV)
    apply_rows(kernel, t, recv, H, C, G, slot, rkeys, bnd, lgP, case.rule, stats)
    t.check_ok()
    kslot, _ = t.resolve(keys.to(DEV), insert=False)
    assert torch.equal(kslot.cpu() >= 0, torch.stack(sent).any(0))
    check_table(t, kslot, case, stats.cpu())


# ------------------------------------------------------------------ fused step kernels
STEPS, B, WIDTH = 3, 1000, 39
# (algo, lr_type, grad_scale, binding max_delta?, l1): the three rules with the penalties
# of algo_defaults (l1 = 10). At this minibatch the largest |gradient sum| of a key is
# ~180, so grad_scale 1/64 keeps every FTRL / SGD key inside the l1 threshold: those two
# pin z, n and an all-zero model, and only the AdaGrad one trains weights and clips. The
# same three rules at l1 = 0.5 train 20 to 1100 weights and clip up to 2200 pushes.
TRAINER_RULES = [("ftrl", "constant", 1 / 64, True, None), ("adagrad", "decay", 0.3, True, None),
                 ("sgd", "constant", 1 / 64, False, None), ("ftrl", "constant", 1 / 64, True, 0.5),
                 ("adagrad", "decay", 0.3, True, 0.5), ("sgd", "constant", 1 / 64, False, 0.5)]
# trainer level (test_fused_1gpu_step_matches_fp32_reference): rtol, and atol of w, z, n
TRAINER_RTOL, TRAINER_ATOL = 1e-4, (1e-5, 1e-4, 1e-4)


def _train_ref(batches, rule, dtype=torch.float64):
    """The reference loop over raw keys in ``dtype`` arithmetic, one push per key per
    minibatch (logistic loss, binary features): returns (keys, state, nnz, smallest
    discontinuity margin, clipped pushes, [(zero pattern, clipped set) per step])."""
    allk = torch.unique(torch.cat([k for k, _ in batches]))
    K = allk.numel()
    state, margin, clipped, steps = tuple(s.to(dtype) for s in zero_state(K)), math.inf, 0, []
    for k, y in batches:
        idx = torch.searchsorted(allk, k)
        m = state[0][idx].view(-1, WIDTH).sum(1)
        yy = torch.where(y > 0, 1.0, -1.0).to(dtype)
        coef = -yy * torch.sigmoid(-yy * m)
        g = torch.zeros(K, dtype=dtype).index_add_(0, idx, coef.repeat_interleave(WIDTH))
        seen = torch.zeros(K, dtype=torch.bool)
        seen[idx] = True
        g[~seen] = float("nan")  # a key outside the minibatch is not pushed
        state, _, tr = apply_pushes(state, g[None], rule, dtype=dtype)
        margin = min(margin, float(tr[0].margin.min()))
        clipped += int(tr[0].clipped.sum())
        steps.append((tr[0].zero, tr[0].clipped))
    return allk, state, int((state[0] != 0).sum()), margin, clipped, steps


@functools.lru_cache(maxsize=None)
def _trainer_case(algo, lr, gs, bind, l1):
    """(config, minibatches, float64 reference), reseeded until the float32 run of the
    reference has the float64 run's zero pattern and clipped set after every step and no
    key is within 10 * MARGIN of a discontinuity; that float32 run must then meet the
    trainer-level tolerances the device is held to."""
    kw = dict(algo_defaults(algo), lr_type=lr, grad_scale=gs)
    if l1 is not None:
        kw["l1"] = l1
    for seed in range(31, 47):
        batches = [criteo_batch(B, seed=seed, row0=t * B, num_features=10 ** 8, device="cpu")
                   for t in range(STEPS)]
        cfg = SparseLRConfig(num_features=10 ** 8, minibatch=B, table_capacity=1 << 18,
                             algo=algo, **kw)
        if bind:  # 0.3 x the median non-zero first step; with none (all inside l1): of |z| alpha
            st = _train_ref(batches[:1], cfg.update_rule())[1]
            step = st[0].abs()[st[0] != 0]
            md = 0.3 * float(step.median()) if step.numel() else 1e-3
            cfg = replace(cfg, max_delta=float(torch.tensor(md, dtype=torch.float32)))
        ref = _train_ref(batches, cfg.update_rule())
        lo = _train_ref(batches, cfg.update_rule(), dtype=torch.float32)
        same = all(torch.equal(za, zb) and torch.equal(ca, cb)
                   for (za, ca), (zb, cb) in zip(ref[5], lo[5]))
        if same and ref[3] >= MARGIN * 10:
            break
    else:
        raise AssertionError("no seed keeps the trainer case off the discontinuities")
    for a, b, atol in zip(lo[1][:3], ref[1][:3], TRAINER_ATOL):  # the reference alone
        close(a, b, rtol=TRAINER_RTOL, atol=atol)
    assert lo[2] == ref[2] and lo[4] == ref[4]
    return cfg, batches, ref


@pytest.mark.parametrize("mode", ["tpf", "tp"])
@pytest.mark.parametrize("algo,lr,gs,bind,l1", TRAINER_RULES)
def test_fused_step_kernels_match_float64_reference(mode, algo, lr, gs, bind, l1, monkeypatch):
    monkeypatch.setenv("PSAMD_FLAT", "1" if mode == "tpf" else "0")
    cfg, batches, (allk, ref, nnz, _, clipped, _) = _trainer_case(algo, lr, gs, bind, l1)
    if l1 is not None:
        assert nnz > 10 and (clipped > 100 or not bind)  # trained weights, a binding clip
    tr = SparseLRTrainer(cfg, device=DEV)
    assert tr.localize_mode == mode
    for k, lab in batches:
        tr.step(k.to(DEV), lab.to(DEV), width=WIDTH)
    torch.cuda.synchronize()
    p = tr.progress()
    assert p["examples"] == STEPS * B
    keys, w, z, n = tr.table.occupied()
    raw = unmix(keys, tr.bits).cpu()
    o = torch.argsort(raw)
    assert torch.equal(raw[o], allk)  # exactly the keys seen
    w, z, n = w.cpu()[o], z.cpu()[o], n.cpu()[o]
    for got, want, atol in zip((w, z, n), ref[:3], TRAINER_ATOL):
        close(got, want, rtol=TRAINER_RTOL, atol=atol)
    assert torch.equal(w == 0, ref[0] == 0)
    assert p["nnz_w"] == nnz
