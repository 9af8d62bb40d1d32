"""Tile dedup + bucket partition localisation (csrc/hip/tploc.hip + tploc_bucket.hip, mode "tp") against
the plain-PyTorch localisation: identical sorted unique keys and local columns; the
entry-level CSC groups every tile-distinct entry under its key; the backward
(csrc/hip/tploc_fused.hip: per-tile LDS accumulation + segmented scan over entries)
matches an fp64 reference."""
import pytest
import torch

from parameter_server_amd.ops.keymix import mix
from parameter_server_amd.ops.linear import linear_backward
from parameter_server_amd.ops.localize import Localizer, localize_torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 8192


def _check(k, bits, width=39):
    n = k.numel()
    ref = localize_torch(k, bits)
    lz = Localizer(n + 5, bits, DEV, mode="tp")
    assert lz.mode == "tp"
    loc = lz(k.to(DEV))
    lz.check()
    torch.cuda.synchronize()
    U = loc.num_unique()
    assert U == ref.uniq.numel()
    assert torch.equal(loc.uniq[:U].cpu(), ref.uniq)
    assert torch.equal(loc.local_col.cpu(), ref.local_col)
    assert torch.all(loc.grad[:U].cpu() == 0)
    # entry CSC: entries = distinct (tile, key) pairs
    mk = mix(k, bits)
    tiles = torch.arange(n) // TILE
    ent = torch.unique(tiles * (1 << 32) + ref.local_col.long())
    E = ent.numel()
    assert int(loc.tile.n_ent.item()) == E
    seg = loc.seg_start[:U + 1].cpu().long()
    assert seg[0] == 0 and seg[U] == E
    per_key = torch.bincount(ent % (1 << 32), minlength=U)
    assert torch.equal(seg[1:] - seg[:-1], per_key)
    segid = loc.segid[:E].cpu().long()
    pos = loc.pos_s[:E].cpu().long()
    assert torch.equal(segid, torch.repeat_interleave(torch.arange(U), per_key) + 1)
    # entry id -> (tile, key): the key of entry pos[q] is uniq[segid[q] - 1]
    rep = loc.tile.rep[:n].cpu().long() & 0xFFFF
    eid_of_occ = tiles * TILE + rep
    key_of_eid = torch.full(((int(tiles.max()) + 1) * TILE,), -1, dtype=torch.int64)
    key_of_eid[eid_of_occ] = mk
    assert torch.equal(key_of_eid[pos], ref.uniq[segid - 1])
    # every entry exactly once
    assert torch.equal(torch.sort(pos).values, torch.unique(eid_of_occ))
    # backward
    B = (n + width - 1) // width
    coef = torch.randn(B, device=DEV)
    g, _ = linear_backward(loc, coef, B=B, width=width)
    rows = torch.arange(n) // width
    exp = torch.zeros(U, dtype=torch.float64).index_add_(0, ref.local_col.long(),
                                                         coef.cpu().double()[rows])
    torch.testing.assert_close(g[:U].cpu().double(), exp, rtol=1e-4, atol=1e-4)
    return loc


@pytest.mark.parametrize("bits,n", [(30, 1), (30, 1000), (30, 100003), (20, 300000), (8, 5000),
                                    (31, 2000000), (27, 65536 * 39), (30, 65536 * 39),
                                    (32, 300000), (33, 100003), (34, 65536 * 39)])
def test_tploc_matches_torch(bits, n):
    g = torch.Generator().manual_seed(n + bits)
    k = torch.randint(0, 1 << min(bits + 4, 62), (n,), generator=g, dtype=torch.int64)
    if n > 10:
        k[::3] = k[0]       # heavy hitters
        k[1::7] = k[1]
    _check(k, bits)


def test_tploc_criteo_batch_and_replay():
    from parameter_server_amd.ops.synthetic import criteo_batch

    keys, _ = criteo_batch(65536, seed=3, row0=0, num_features=10 ** 9, device=DEV)
    loc = _check(keys.cpu(), 30)
    # a second call into the same workspace gives the same result (no stale state)
    lz = Localizer(keys.numel(), 30, DEV, mode="tp")
    a = lz(keys)
    u1, lc1 = a.uniq[:a.num_unique()].clone(), a.local_col.clone()
    b = lz(keys)
    assert torch.equal(b.uniq[:b.num_unique()], u1) and torch.equal(b.local_col, lc1)
    assert int(loc.tile.n_ent.item()) > 0


def test_tploc_all_distinct():
    n = 65536 * 39
    k = torch.randperm(1 << 22)[:n].to(torch.int64) * 97 + 11
    _check(k, 30)


def test_tploc_34bit_criteo_1e10():
    """10^10 hashed features = 34-bit mixed keys: the quotient-encoded tile hash keeps
    them in 32-bit LDS words; the buckets hold the top bits."""
    from parameter_server_amd.ops.synthetic import criteo_batch

    keys, _ = criteo_batch(65536, seed=5, row0=0, num_features=10 ** 10, device=DEV)
    _check(keys.cpu(), 34)


def test_tploc_pair_overflow_redo_sequence():
    """Buckets run in pairs of fine buckets; a pair that overflows (nearly distinct
    keys) flags the launch and the gated fine-bucket kernel redoes it. The flag carries
    the launch epoch, so calls before and after in the same workspace are unaffected."""
    from parameter_server_amd.ops.synthetic import criteo_batch

    n = 65536 * 39
    crit, _ = criteo_batch(65536, seed=9, row0=0, num_features=10 ** 9, device=DEV)
    dist = (torch.randperm(1 << 22)[:n].to(torch.int64) * 97 + 11).to(DEV)
    lz = Localizer(n, 30, DEV, mode="tp")
    for k in (crit, dist, crit, crit, dist, dist, crit):
        ref = localize_torch(k.cpu(), 30)
        loc = lz(k)
        lz.check()
        U = loc.num_unique()
        assert U == ref.uniq.numel()
        assert torch.equal(loc.uniq[:U].cpu(), ref.uniq)
        assert torch.equal(loc.local_col.cpu(), ref.local_col)
