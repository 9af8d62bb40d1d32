"""The block -> bucket-group map of the flat bucket-geometry kernels (csrc/hip/tploc.cuh
tpf_xcd_group_of, used by the kernels of tploc_step.hip: the blocks of one XCD take a contiguous range of groups). The map is a
permutation of the groups, and the kernels that use it (tpf_step, tpf_unpack_w,
tpf_pack_grads) still compute what they did next to the ones that take their group from
blockIdx.x (tpf_bucket, tpf_filter, tpf_pack_keys; every region is indexed by the logical
group, so the two kinds mix freely): small width-39 minibatches at 2 (identity), 8, 16 (the first power of two at which the bijective form
permutes: at exactly 8 groups each XCD holds one group and the map is still the identity),
32 and 128 groups against the fp32 PyTorch loop of tests/test_tpf_gpu.py."""
import functools

import pytest
import torch

from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
from parameter_server_amd.ops.keymix import key_bits_for, unmix
from parameter_server_amd.ops.localize import TP_TILE
from parameter_server_amd.ops.native import hipops
from parameter_server_amd.ops.synthetic import criteo_batch
from test_tpf_gpu import (_reference_train, _reference_train_filtered, _skewed_batch,
                          _table_by_raw_key)

WIDTH = 39
STEPS = 6
GROUPS = {64: 2, 420: 8, 840: 16, 1000: 32, 4096: 128}  # B -> bucket groups at width 39


@pytest.mark.parametrize("groups", [1, 2, 4, 7, 8, 9, 12, 16, 128, 1023, 1024])
def test_xcd_map_is_a_permutation_in_range(groups):
    """Host call of the kernels' own function: a bijection of [0, groups), the identity
    below 8 groups, and XCD x (bid % 8) takes one contiguous, ascending range."""
    H = hipops()
    m = [H.tpf_xcd_group(b, groups) for b in range(groups)]
    assert all(0 <= g < groups for g in m)
    assert sorted(m) == list(range(groups))
    if groups < 8:
        assert m == list(range(groups))
    start = 0
    for x in range(min(8, groups)):  # the XCDs' ranges follow one another
        mine = m[x::8]
        assert mine == list(range(start, start + len(mine))), (groups, x)
        start += len(mine)
    assert start == groups
    with pytest.raises(ValueError):
        H.tpf_xcd_group(groups, groups)  # (the extra AUC block is never remapped)


def _dev():
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _batches(B: int, N: int = 10 ** 8, seed: int = 31, steps: int = STEPS):
    return tuple(criteo_batch(B, seed=seed, row0=t * B, num_features=N, device=_dev())
                 for t in range(steps))


@functools.lru_cache(maxsize=None)
def _reference(B: int):
    """The fp32 loop over the B-row minibatches, computed once and shared."""
    cfg = SparseLRConfig(num_features=10 ** 8, minibatch=B, table_capacity=1 << 22)
    return _reference_train(list(_batches(B)), cfg.update_rule(), key_bits_for(10 ** 8))


def _trainer(B: int, **kw):
    cfg = SparseLRConfig(num_features=10 ** 8, minibatch=B, table_capacity=1 << 22, **kw)
    tr = SparseLRTrainer(cfg, device=_dev())
    assert tr.localize_mode == "tpf"
    assert hipops().tpf_groups(B * WIDTH, tr.bits) == GROUPS[B]
    return tr


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 420, 840, 1000, 4096])
def test_flat_step_matches_fp32_reference_at_group_counts(B, monkeypatch):
    """6 flat steps with the pulls issued ahead (next_loc) and 6 sequential ones: w, z, n to
    rtol 1e-4 of the fp32 loop, and the same last AUC / metrics from both (the extra AUC
    workgroup is the last physical block whatever the map does to the others)."""
    monkeypatch.setenv("PSAMD_FLAT", "1")
    batches = _batches(B)
    allk, W, Z, Nn = _reference(B)
    prog = []
    for variant in ("ahead", "plain"):
        tr = _trainer(B)
        if variant == "ahead":
            loc = tr.localize(batches[0][0], buf=0)
            for t in range(STEPS):
                nxt = tr.localize(batches[t + 1][0], buf=(t + 1) % 2) if t + 1 < STEPS else None
                tr.step(batches[t][0], batches[t][1], width=WIDTH, loc=loc, next_loc=nxt)
                loc = nxt
        else:
            for k, lab in batches:
                tr.step(k, lab, width=WIDTH)
        torch.cuda.synchronize()
        tr.check_ok()
        p = tr.progress()
        assert p["examples"] == STEPS * B
        prog.append(p)
        w, z, n = _table_by_raw_key(tr, allk)
        torch.testing.assert_close(w, W, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(z, Z, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(n, Nn, rtol=1e-4, atol=1e-4)
        assert (z != 0).sum() > 100  # the comparison covers updated keys
    assert prog[0]["auc"] == prog[1]["auc"]
    # (the loss sum takes float LDS atomics in any order: equal to rounding)
    assert prog[0]["loss"] == pytest.approx(prog[1]["loss"], rel=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [420, 840])
def test_flat_tail_filter_at_8_and_16_groups(B, monkeypatch):
    """tpf_filter_kernel's compacted units consumed by the mapped tpf_step
    (tail_feature_freq 1, a small sketch): the sketch cell for cell and the weights against
    the fp32 loop with a CPU CountMin."""
    from parameter_server_amd.ops.countmin import CountMinSketch

    monkeypatch.setenv("PSAMD_FLAT", "1")
    steps, freq, N = 5, 1, 10 ** 6
    batches = [(k, lab, None, None) for k, lab in _batches(B, N, 77, steps)]
    cfg = SparseLRConfig(num_features=N, minibatch=B, max_nnz_per_example=WIDTH,
                         table_capacity=1 << 22, alpha=0.05, l1=1.0, l2=0.1,
                         tail_feature_freq=freq, countmin_n=1 << 16)
    tr = SparseLRTrainer(cfg, device=_dev())
    assert tr.localize_mode == "tpf" and tr.filter is not None
    assert hipops().tpf_groups(B * WIDTH, tr.bits) == GROUPS[B]
    for k, lab, _, _ in batches:
        tr.step(k, lab, width=WIDTH)
    torch.cuda.synchronize()
    assert tr._compact is None  # every step ran the flat path
    tr.check_ok()
    assert tr.progress()["examples"] == steps * B
    cm = CountMinSketch(cfg.countmin_n, cfg.countmin_k, "cpu", key_bits=tr.bits)
    allk, W, Z, Nn, dropped = _reference_train_filtered(batches, cfg.update_rule(), tr.bits,
                                                        freq, cm)
    assert dropped > 0  # the filter removed something
    assert torch.equal(tr.filter.cells.cpu(), cm.cells)  # same sketch, cell for cell
    w, z, n = _table_by_raw_key(tr, allk)  # only ever-kept keys were stored
    torch.testing.assert_close(w, W, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(z, Z, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(n, Nn, rtol=1e-4, atol=1e-4)
    assert (z != 0).sum() > 20


@pytest.mark.gpu
@pytest.mark.parametrize("peers", [2, 8])
def test_flat_multi_peer_matches_compact_at_32_groups(peers, monkeypatch):
    """Emulated peers over the loopback exchange at B = 1000 (32 groups: 16 / 4 per owner):
    tpf_pack_keys (unmapped) / tpf_unpack_w / tpf_pack_grads (mapped) with the owner
    boundary b / per leave the table the compact layout leaves on the same minibatches."""
    from parameter_server_amd.parallel.comm import LoopbackComm

    B = 1000
    batches = _batches(B)
    outs = []
    for flat in ("1", "0"):
        monkeypatch.setenv("PSAMD_FLAT", flat)
        cfg = SparseLRConfig(num_features=10 ** 8, minibatch=B, consistency="ssp:2",
                             table_capacity=1 << 22, alpha=0.05, l1=1.0, l2=0.1)
        tr = SparseLRTrainer(cfg, LoopbackComm(peers, "cuda"), _dev())
        assert (tr.localize_mode == "tpf") == (flat == "1")
        if flat == "1":
            assert hipops().tpf_groups(B * WIDTH, tr.bits) == GROUPS[B]
        for k, lab in batches:
            tr.step(k, lab, width=WIDTH)
        p = tr.progress()
        tr.check_ok()
        kk, w, z, n = tr.table.occupied()
        o = torch.argsort(kk)
        outs.append((kk[o].cpu(), w[o].cpu(), n[o].cpu(), p))
    assert torch.equal(outs[0][0], outs[1][0])
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(outs[0][2], outs[1][2], rtol=1e-4, atol=1e-4)
    assert abs(outs[0][3]["loss"] - outs[1][3]["loss"]) < 1e-4
    assert (outs[0][2] != 0).sum() > 100


def _overflow_pair_batch(step: int, B: int, pair: int, bits: int = 20):
    """tests/test_tpf_gpu.py _skewed_batch at width 39 for any bucket pair: 1500 distinct
    keys in each of pair ``pair``'s two fine buckets, every one of them in the first two
    8192-occurrence tiles (6000 entries > the bucket kernel's LDS capacity), so that pair
    falls back to its two fine buckets as separate units. Raw keys."""
    g = torch.Generator().manual_seed(200 + step)
    n = B * WIDTH
    nbk = 2 * GROUPS[B]
    shift = bits - (nbk.bit_length() - 1)
    lo = (2 * pair) << shift
    k0 = lo + torch.randperm(1 << shift, generator=g)[:1500]
    k1 = lo + (1 << shift) + torch.randperm(1 << shift, generator=g)[:1500]
    hot = torch.cat([k0, k1])
    mixed = torch.randint(0, (1 << bits) - (2 << shift), (n,), generator=g)
    mixed = torch.where(mixed >= lo, mixed + (2 << shift), mixed)  # (outside the pair)
    for t in range(2):
        room = min(TP_TILE, n - t * TP_TILE)
        pos = t * TP_TILE + torch.randperm(room, generator=g)[:hot.numel()]
        mixed[pos] = hot
    keys = unmix(mixed.to(_dev()), bits)
    labels = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0).to(_dev())
    return keys, labels


@pytest.mark.gpu
@pytest.mark.parametrize("B,pair", [(420, 5), (840, 5)])
def test_flat_overflowing_pair_at_8_and_16_groups(B, pair, monkeypatch):
    """The two-unit fallback (tpf_unit_light) of one overflowing pair, not the first, at 8
    and 16 groups: its counts land in ITS group's cnt row and 3 steps train like the fp32
    loop."""
    monkeypatch.setenv("PSAMD_FLAT", "1")
    monkeypatch.setenv("PSAMD_TILE_LTS", "13")  # (the batches are built for 8192-key tiles)
    bits = 20
    batches = [_overflow_pair_batch(s, B, pair, bits) for s in range(3)]
    cfg = SparseLRConfig(num_features=1 << bits, minibatch=B, max_nnz_per_example=WIDTH,
                         table_capacity=1 << 22, l1=0.1, l2=0.1, alpha=0.1)
    tr = SparseLRTrainer(cfg, device=_dev())
    assert tr.localize_mode == "tpf" and tr.bits == bits
    G = hipops().tpf_groups(B * WIDTH, bits)
    assert G == GROUPS[B]
    f = tr.localizer(batches[0][0])
    torch.cuda.synchronize()
    c = f.cnt[:4 * G].view(G, 4).cpu()
    # that pair ran as two units, in ITS row (the other pairs' near-distinct random keys
    # may give up on the hash build and fall back too: not asserted)
    assert c[pair].tolist() == [1500, 3000, 1500, 3000], c
    for k, lab in batches:
        tr.step(k, lab, width=WIDTH)
    torch.cuda.synchronize()
    assert int(tr.localizer.err.item()) == 0
    allk, W, Z, Nn = _reference_train(batches, cfg.update_rule(), bits)
    w, z, n = _table_by_raw_key(tr, allk)
    torch.testing.assert_close(w, W, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(z, Z, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(n, Nn, rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
def test_flat_overflowing_first_pair_at_16_groups_width_16(monkeypatch):
    """tests/test_tpf_gpu.py _skewed_batch as it stands (2048 x 16: 16 groups, the first
    pair overflows), one localisation: group 0 holds the two units under the map."""
    monkeypatch.setenv("PSAMD_FLAT", "1")
    monkeypatch.setenv("PSAMD_TILE_LTS", "13")
    bits = 20
    keys, labels = _skewed_batch(0, bits)
    cfg = SparseLRConfig(num_features=1 << bits, minibatch=labels.numel(),
                         max_nnz_per_example=16, table_capacity=1 << 22)
    tr = SparseLRTrainer(cfg, device=_dev())
    G = hipops().tpf_groups(keys.numel(), bits)
    assert G == 16
    f = tr.localizer(keys)
    torch.cuda.synchronize()
    assert int(f.err.item()) == 0
    c = f.cnt[:4 * G].view(G, 4).cpu()
    assert c[0].tolist() == [1500, 3000, 1500, 3000], c
