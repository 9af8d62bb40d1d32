"""The fused table-probe scoring kernel (csrc/hip/predict.hip) on the GPU: the cases,
references and bounds of tests/test_score.py, plus the fused scorer against the path
composed from the training step's ops (localise + resolve(insert=False) + linear_fwd).

The completely full table is not run here: a probe loop without its trip bound would hang
a shared machine, so that bound is checked on the CPU path and by reading the loop."""
import pytest
import torch

from test_score import (CASES, Case, check_accumulation, check_case, check_empty_model,
                        ordered_wrap_case, train_and_score)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_score_gpu_cases(name):
    check_case(Case("cuda", **CASES[name]))


def test_score_gpu_lane_forms_agree_with_cpu_within_bound():
    """Both lane-group forms on the same valued CSR rows, and the CPU path: each within
    the row bound of the fp64 reference (check_case), so within twice it of each other."""
    kw = dict(lens=tuple(range(0, 130, 3)), vals=True, seed=11)
    m8 = check_case(Case("cuda", lanes=8, **kw))
    m64 = check_case(Case("cuda", lanes=64, **kw))
    mc = check_case(Case("cpu", **kw))
    assert m8.shape == m64.shape == mc.shape


def test_score_gpu_ordered_home_chain_wraps():
    check_case(ordered_wrap_case("cuda"))


def test_score_gpu_empty_model():
    check_empty_model("cuda")


def test_score_gpu_accumulates_over_minibatches():
    check_accumulation("cuda")


def test_score_gpu_rejects_bad_shapes():
    """Sizes are validated on the host before the launch."""
    c = Case("cuda", lens=(5,) * 8, fixed=True)
    from parameter_server_amd.ops.score import score

    keys = c.dev(c.keys)
    with pytest.raises(Exception):
        score(c.table, keys, c.bits, width=5, B=9)           # 9 rows of 5 > 40 keys
    with pytest.raises(Exception):
        score(c.table, keys, c.bits, width=5, vals=c.dev(torch.ones(39)))
    with pytest.raises(Exception):
        score(c.table, keys, c.bits, row_ptr=c.dev(torch.zeros(4, dtype=torch.int64)), B=8)
    with pytest.raises(Exception):
        score(c.table, keys, c.bits, width=5, lanes=16)


def _composed_margins(table, keys, bits, labels, B, width=None, row_ptr=None, vals=None):
    """What the training step's ops already compose: localise, resolve without insert,
    the forward kernel."""
    from parameter_server_amd.ops.linear import linear_forward
    from parameter_server_amd.ops.localize import Localizer, ensure_local_col

    lz = Localizer(keys.numel(), bits, keys.device, mode="sort")
    loc = lz(keys)
    n = int(loc.n_uniq.item()) if torch.is_tensor(loc.n_uniq) else int(loc.n_uniq)
    _, w = table.resolve(loc.uniq[:n], insert=False)
    xw = torch.empty(B, dtype=torch.float32, device=keys.device)
    linear_forward(ensure_local_col(loc), w, labels, B=B, width=width or 0, row_ptr=row_ptr,
                   vals=vals, xw=xw)
    return xw


@pytest.mark.parametrize("shape", ["criteo_1000", "rcv1_300"])
def test_fused_scorer_matches_composed_path(shape):
    from parameter_server_amd.ops.score import row_bound

    if shape == "criteo_1000":
        c = Case("cuda", lens=(39,) * 1000, fixed=True, universe=4000, seed=21)
    else:
        g = torch.Generator().manual_seed(22)
        lens = tuple(torch.randint(20, 160, (300,), generator=g).tolist())
        c = Case("cuda", lens=lens, vals=True, universe=4000, seed=22)
    fused = c.run(labels=False)
    comp = _composed_margins(c.table, c.dev(c.keys), c.bits, c.dev(c.labels), c.B,
                             width=c.width, row_ptr=c.dev(c.row_ptr), vals=c.dev(c.vals))
    m_ref, bound = row_bound(c.keys, c.w_of, c.vals, c.row_ptr, c.width)
    for m in (fused, comp):  # each within the row bound of the fp64 reference ...
        assert bool(((m.cpu().double() - m_ref).abs() <= bound).all())
    # ... and of each other (both are f32 sums of the same n_r products)
    assert bool(((fused - comp).cpu().double().abs() <= bound).all())


def test_trainer_scorer_equals_saved_model_gpu(tmp_path):
    train_and_score("cuda", tmp_path)
