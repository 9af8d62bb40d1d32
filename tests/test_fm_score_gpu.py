"""The fused FM scoring kernel (csrc/hip/fm_predict.hip) against the float64 reference and
the derived bound of tests/test_fm_score.py; determinism across table layouts; accumulation."""
import pytest
import torch

from parameter_server_amd.models import FMConfig, FMScorer, FMTrainer
from parameter_server_amd.ops.synthetic import criteo_batch
from test_fm_score import CASES, CFG, check_case, fm_ref, held_out, load_shard, make_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D,L,kind", CASES)
def test_kernel_matches_float64(D, L, kind):
    check_case("cuda", D, L, *kind)


def test_fixed_width_rows():
    c = make_case(32, 32, 20, True)
    n = c.keys.numel() // 39
    k, v = c.keys[:n * 39], c.vals[:n * 39]
    sc = FMScorer.from_shard(load_shard(c, "cuda"), c.bits)
    m = sc.predict(k.cuda(), width=39, vals=v.cuda(), lanes=32)
    ref, bound = fm_ref(c.mk, c.mw, c.mrows, k, v, torch.arange(n + 1) * 39)
    assert bool(((m.cpu().double() - ref).abs() <= bound).all())


def test_same_bits_for_any_table_layout():
    """D = 64, which FMTrainer.predict refuses on a GPU: the trainer's own shard and a shard
    rebuilt from its snapshot (another capacity, other probe chains) give the same bits."""
    cfg = dict(CFG, embedding_dim=64)
    tr = FMTrainer(FMConfig(**cfg), device="cuda")
    for s in range(3):
        tr.step(*criteo_batch(256, seed=3, row0=s * 256, num_features=cfg["num_features"],
                              cards=[300] * 26, device="cuda"))
    sd = tr.state_dict()
    k, rp, v, _ = held_out()
    live = tr.scorer().predict(k.cuda(), row_ptr=rp.cuda(), vals=v.cuda())
    stored = FMScorer.from_state_dict(sd, "cuda").predict(k.cuda(), row_ptr=rp.cuda(),
                                                          vals=v.cuda())
    assert torch.equal(live, stored)
    ref, bound = fm_ref(sd["keys"], sd["w"], sd["rows"], k, v, rp)
    assert bool(((live.cpu().double() - ref).abs() <= bound).all())
    assert float(ref.abs().max()) > 0


def test_accumulation_in_halves():
    c = make_case(64, 16, 40, False)
    shard = load_shard(c, "cuda")
    one, two = FMScorer.from_shard(shard, c.bits), FMScorer.from_shard(shard, c.bits)
    keys, rp, y = c.keys.cuda(), c.row_ptr.cuda(), c.y.cuda()
    one.score(keys, y, row_ptr=rp, margins=False)
    h = 50
    two.score(keys[:rp[h]], y[:h], row_ptr=rp[:h + 1], margins=False)
    two.score(keys[rp[h]:], y[h:], row_ptr=rp[h:] - rp[h], margins=False)
    (s1, c1), (s2, c2) = one.totals(), two.totals()
    assert torch.equal(c1, c2) and float(s1[2]) == float(s2[2]) == len(c.y)
    assert abs(float(s1[0]) - float(s2[0])) <= 1e-9 * abs(float(s1[0]))
    assert set(one.result()) == {"examples", "loss", "accuracy", "auc", "auc_tie_bound"}
