"""The PyTorch path of ops/slotsplit.py (``split_by_slot`` on CPU tensors: a stable sort by
slot index plus searchsorted) against ``SlotData.from_batch`` on the same arrays, array for
array in dtype and contents, and ``SlotData.concat`` / ``info()`` on tensor groups against
the numpy results."""
import numpy as np
import pytest
import torch

from parameter_server_amd.data import ExampleBatch
from parameter_server_amd.data.slot_reader import SlotData
from parameter_server_amd.data.synthetic import sparse_groups
from parameter_server_amd.ops.slotsplit import SlotSplit, split_by_slot


def batch_of(sd: SlotData) -> ExampleBatch:
    """The CSR batch a parser makes of ``sd``'s text: per row the groups ascending."""
    gids = sorted(sd.groups)
    row = np.concatenate([np.repeat(np.arange(sd.rows), np.diff(sd.groups[g][0])) for g in gids])
    slot = np.concatenate([np.full(sd.groups[g][1].size, g, np.int32) for g in gids])
    keys = np.concatenate([sd.groups[g][1] for g in gids]).astype(np.uint64)
    valued = any(sd.groups[g][2] is not None for g in gids)
    order = np.lexsort((np.arange(row.size), slot, row))
    vals = None
    if valued:
        vals = np.concatenate([np.ones(sd.groups[g][1].size, np.float32) if sd.groups[g][2] is None
                               else sd.groups[g][2] for g in gids])[order]
    rp = np.zeros(sd.rows + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=sd.rows), out=rp[1:])
    return ExampleBatch(sd.labels, rp, keys[order], vals, slot[order])


def hand_batch(rows, valued=False, seed=0) -> ExampleBatch:
    """``rows``: per row the list of (slot id, number of keys)."""
    rng = np.random.default_rng(seed)
    rp, slots = [0], []
    for r in rows:
        for g, k in r:
            slots += [g] * k
        rp.append(len(slots))
    n = len(slots)
    keys = rng.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n).astype(np.uint64)
    vals = (rng.integers(1, 9, n) / 4).astype(np.float32) if valued else None
    return ExampleBatch(np.ones(len(rows), np.float32), np.array(rp, np.int64), keys, vals,
                        np.array(slots, np.int32))


def same_groups(got: dict, ref: dict):
    assert list(got) == sorted(ref)  # (ascending)
    for g in ref:
        for u, v in zip(got[g], ref[g]):
            assert (u is None) == (v is None)
            if v is not None:
                assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v)


def check_cpu(b: ExampleBatch) -> SlotSplit:
    ref = SlotData.from_batch(b).groups
    got = split_by_slot(b.labels, b.row_ptr, b.keys, b.vals, b.slots)
    assert got.deferred is False and got.cause is None
    same_groups(got.numpy(), ref)
    t = lambda x, dt: None if x is None else torch.from_numpy(  # noqa: E731
        x.view(np.int64) if x.dtype == np.uint64 else x).to(dt)
    got = split_by_slot(None, t(b.row_ptr, torch.int64) + 5, t(b.keys, torch.int64),
                        t(b.vals, torch.float32), t(b.slots, torch.int32))
    same_groups(got.numpy(), ref)  # (tensors; the base of row_ptr does not matter)
    return got


def valued(sd: SlotData, seed: int) -> SlotData:
    rng = np.random.default_rng(seed)
    sd.groups = {g: (o, k, rng.integers(1, 9, k.size).astype(np.float32) / 4)
                 for g, (o, k, _) in sd.groups.items()}
    return sd


HAND = {
    "no rows": [],
    "rows with no features": [[], [], []],
    "some rows empty": [[], [(3, 2)], [], [], [(3, 1), (9, 2)], []],
    "a slot absent from some rows": [[(1, 2), (2, 1)], [(2, 3)], [(1, 1)], [(2, 1), (5, 4)]],
    "one slot only": [[(6, 1)], [(6, 3)], [], [(6, 2)]],
    "ids 0, 7 and 2^31 - 1": [[(0, 1), (7, 2), (2 ** 31 - 1, 1)], [(2 ** 31 - 1, 2)], [(0, 3)],
                               [(7, 1), (2 ** 31 - 1, 1)]],
    "a group repeated in a row": [[(4, 2), (9, 1), (4, 3)], [(9, 2)], [(9, 1), (4, 1), (9, 2)]],
}


@pytest.mark.parametrize("is_valued", [False, True])
def test_cpu_path_matches_from_batch_on_synthetic_groups(is_valued):
    sd = sparse_groups(700, groups=9, present=4, keys_per_group=300, seed=3)
    b = batch_of(valued(sd, 1) if is_valued else sd)
    assert (b.vals is not None) == is_valued and b.nnz > 4000
    got = check_cpu(b)
    assert len(got.groups) == 9
    same_groups(got.numpy(), sd.groups)  # (and the split undoes batch_of)


@pytest.mark.parametrize("is_valued", [False, True])
@pytest.mark.parametrize("name", list(HAND))
def test_cpu_path_matches_from_batch_on_hand_made_cases(name, is_valued):
    b = hand_batch(HAND[name], is_valued, seed=len(name))
    got = check_cpu(b)
    assert len(got.groups) == len({g for r in HAND[name] for g, _ in r})


def test_repeated_group_keeps_the_stable_order():
    b = hand_batch(HAND["a group repeated in a row"])
    off, keys, _ = split_by_slot(b.labels, b.row_ptr, b.keys, None, b.slots).numpy()[4]
    assert off.tolist() == [0, 5, 5, 6]
    assert keys.tolist() == [int(b.keys[i]) for i in (0, 1, 3, 4, 5, 9)]


def test_bad_arguments():
    b = hand_batch(HAND["one slot only"])
    with pytest.raises(ValueError):
        split_by_slot(b.labels, b.row_ptr, b.keys, None, b.slots[:-1])
    with pytest.raises(ValueError):
        split_by_slot(b.labels[:-1], b.row_ptr, b.keys, None, b.slots)
    with pytest.raises(ValueError):
        split_by_slot(None, b.row_ptr[:-1], b.keys, None, b.slots)


def as_tensors(sd: SlotData) -> SlotData:
    t = torch.from_numpy
    return SlotData(sd.labels, {g: (t(o), t(k.view(np.int64)), None if v is None else t(v))
                                for g, (o, k, v) in sd.groups.items()})


def test_concat_and_info_on_tensor_groups_match_numpy():
    parts = [sparse_groups(300, groups=6, present=3, keys_per_group=200, seed=10),
             valued(sparse_groups(200, groups=6, present=2, keys_per_group=200, seed=11), 2),
             sparse_groups(1, groups=6, present=1, keys_per_group=200, seed=12)]
    # keys above 2^63 (the unsigned min / max), and a group that one part lacks
    o, k, v = parts[0].groups[min(parts[0].groups)]
    parts[0].groups[min(parts[0].groups)] = (o, k + np.uint64((1 << 63) + 5), v)
    del parts[2].groups[max(parts[2].groups)], parts[1].groups[min(parts[1].groups)]
    ref = SlotData.concat(parts)
    got = SlotData.concat([as_tensors(p) for p in parts])
    assert all(isinstance(x, torch.Tensor) for t in got.groups.values() for x in t if x is not None)
    assert np.array_equal(got.labels, ref.labels) and got.rows == ref.rows
    same_groups(SlotSplit(got.groups).numpy(), ref.groups)
    assert got.info() == ref.info()
    for p in parts:
        assert as_tensors(p).info() == p.info()
    # numpy parts among tensor parts (a cache hit among resident files) are taken along
    mixed = SlotData.concat([as_tensors(parts[0]), parts[1], as_tensors(parts[2])])
    same_groups(SlotSplit(mixed.groups).numpy(), ref.groups)
    # binary parts stay binary
    bin_ref = SlotData.concat([parts[0], parts[2]])
    bin_got = SlotData.concat([as_tensors(parts[0]), as_tensors(parts[2])])
    assert all(v is None for _, _, v in bin_got.groups.values())
    same_groups(SlotSplit(bin_got.groups).numpy(), bin_ref.groups)
