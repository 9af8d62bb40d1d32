"""64-bit keys on the exchange rows, through a whole trainer: 2^34 features give 34-bit mixed
keys, so every peer row carries u64 keys (kw = 2) and its gradients start at word 4 + 2C.
Three emulated peers on the GPU against the same configuration on the CPU route, on the
same minibatches (generated on the host: the two generators may differ in a key or two)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, B, STEPS = 1 << 34, 128, 4


def _train(device, extra):
    from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
    from parameter_server_amd.ops.synthetic import criteo_batch
    from parameter_server_amd.parallel.comm import LoopbackComm

    cfg = SparseLRConfig(num_features=N, minibatch=B, table_capacity=1 << 15, l1=0.5, **extra)
    comm = LoopbackComm(3, "cuda") if device == "cuda" else LoopbackComm(3)
    tr = SparseLRTrainer(cfg, comm, device)
    for s in range(STEPS):
        k, l = criteo_batch(B, seed=100, row0=s * B, num_features=N, cards=[200] * 26)
        tr.step(k.to(device), l.to(device))
    tr.flush()
    if device == "cuda":
        torch.cuda.synchronize()
        tr.check_ok()
    keys, w, _, _ = tr.table.occupied()
    return tr, dict(zip(keys.cpu().tolist(), w.cpu().tolist()))


@pytest.mark.parametrize("extra", [dict(exchange_merge="off"),
                                   dict(exchange_merge="on", consistency="ssp:2")],
                         ids=["two-collective", "merged-ssp2"])
def test_three_peers_wide_keys_match_cpu_route(extra):
    tr, got = _train("cuda", extra)
    assert tr.bits == 34 and tr.xc.kw == 2
    assert tr.merged == (extra["exchange_merge"] == "on")
    ref_tr, ref = _train("cpu", extra)
    assert ref_tr.merged == tr.merged
    assert got.keys() == ref.keys() and len(ref) > 500
    assert max(k for k in ref) >= 1 << 32  # (keys that do not fit a 32-bit row word)
    assert max(abs(got[k] - ref[k]) for k in ref) < 1e-5
    assert sum(1 for v in ref.values() if v != 0) > 20  # the model moved
