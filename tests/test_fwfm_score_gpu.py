"""The fused FwFM scoring kernel (csrc/hip/fwfm_predict.hip) against the float64 reference and
the derived bound of tests/test_fwfm_score.py; fixed-width rows against the same rows as CSR;
determinism across table layouts; accumulation."""
import pytest
import torch

from parameter_server_amd.models import FwFMScorer
from test_fwfm_score import (CASES, CFG, check_case, fwfm_ref, held_out, load_shard, make_case,
                             train, within)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("FD,kind", CASES)
def test_kernel_matches_float64(FD, kind):
    check_case("cuda", *FD, *kind)


def test_fixed_width_equals_csr():
    """100 rows of 39 positions, 13 of them on field 0 (F = 39, D = 16, so R[0][0] = 100 acts
    in every row): by width= with the position map, and as CSR with the map tiled."""
    c = make_case(39, 16, 40, True)
    fmap = CFG["fields"]
    k, v = c.keys[:3900].cuda(), c.vals[:3900].cuda()
    rp, fld = torch.arange(101) * 39, torch.tensor(fmap, dtype=torch.int32).repeat(100)
    sc = FwFMScorer.from_shard(load_shard(c, "cuda"), c.bits, 39, c.R.cuda(), fields=fmap)
    fixed = sc.predict(k, width=39, vals=v)
    assert torch.equal(fixed, sc.predict(k, row_ptr=rp.cuda(), vals=v, fields=fld.cuda()))
    ref, bound = fwfm_ref(c.mk, c.mw, c.mrows, c.R, k.cpu(), v.cpu(), rp, fld)
    assert within(fixed, ref, bound) and float(ref.abs().max()) > 0


def test_same_bits_for_any_table_layout():
    """The trainer's own shard and live R, and a shard rebuilt from its snapshot (another
    capacity, other probe chains) give the same bits; the tile kernel of ``predict`` sums in
    another order."""
    tr = train("cuda", 3)
    sd = tr.state_dict()
    k, rp, v, fld, _ = (t.cuda() for t in held_out())
    live = tr.scorer().predict(k, row_ptr=rp, vals=v, fields=fld)
    stored = FwFMScorer.from_state_dict(sd, "cuda", capacity=1 << 16).predict(
        k, row_ptr=rp, vals=v, fields=fld)
    assert torch.equal(live, stored)
    ref, bound = fwfm_ref(sd["keys"], sd["w"], sd["rows"], sd["R"], k.cpu(), v.cpu(), rp.cpu(),
                          fld.cpu())
    assert within(live, ref, bound) and float(ref.abs().max()) > 0
    assert within(tr.predict(k, 256, vals=v, row_ptr=rp, fields=fld), live.cpu().double(), bound, 2)


def test_accumulation_in_halves():
    c = make_case(39, 16, 40, True)
    shard, R = load_shard(c, "cuda"), c.R.cuda()
    one, two = (FwFMScorer.from_shard(shard, c.bits, 39, R) for _ in range(2))
    keys, rp, f, y = c.keys.cuda(), c.row_ptr.cuda(), c.fld.cuda(), c.y.cuda()
    one.score(keys, y, row_ptr=rp, fields=f, margins=False)
    h = 50
    two.score(keys[:rp[h]], y[:h], row_ptr=rp[:h + 1], fields=f[:rp[h]], margins=False)
    two.score(keys[rp[h]:], y[h:], row_ptr=rp[h:] - rp[h], fields=f[rp[h]:], margins=False)
    (s1, c1), (s2, c2) = one.totals(), two.totals()
    assert torch.equal(c1, c2) and float(s1[2]) == float(s2[2]) == len(c.y)
    assert abs(float(s1[0]) - float(s2[0])) <= 1e-9 * abs(float(s1[0]))
