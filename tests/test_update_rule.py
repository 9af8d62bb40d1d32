"""The host optimizer update (csrc/core/cpu_kernels.cc kv_update, ``KVTable.update`` on
"cpu") against the float64 recurrence of tests/update_rule_ref.py, over the whole case
grid: five (algorithm, rate) rules x penalties with l1 / l2 / beta = 0, grad_scale != 1,
max_delta binding and not, planted zero / NaN / tiny / huge gradients and prox-threshold
keys, slot lists with -1 and indices past the capacity. The device twin is
test_update_rule_gpu.py."""
import pytest
import torch

from parameter_server_amd.ops import KVTable

from update_rule_ref import (PUSHES, build_case, case_ids, check_table, slot_list, with_invalid)


@pytest.mark.parametrize("algo,lr,pen,K", case_ids())
def test_host_kv_update_matches_float64_reference(algo, lr, pen, K):
    case = build_case(algo, lr, pen, K)
    t = KVTable(4 * K, "cpu")
    slot, _ = t.resolve(torch.arange(1, K + 1, dtype=torch.int64) * 7919)
    assert torch.unique(slot).numel() == K
    full, pos = slot_list(slot, t.capacity)
    before = t.slots.clone()
    stats = torch.zeros(3, dtype=torch.float64)
    for p in range(PUSHES):
        t.update(full, with_invalid(case.grads[p], pos, full.numel()), case.rule, stats)
    check_table(t, slot, case, stats)
    other = torch.ones(t.capacity, dtype=torch.bool)
    other[slot] = False
    assert torch.equal(t.slots[other], before[other])  # nothing but the K slots moved
