"""What a move of the tp / tpf kernels between translation units (csrc/hip/tploc.hip,
tploc_bucket.hip, tploc_flat.hip, tploc_fused.hip, tploc_step.hip) can break without the
numerical tests noticing:

* the stage decompositions of localize_tpf (tploc_flat.hip): tile, bucket and filter run
  as separate calls leave exactly what one call of all stages leaves;
* the profiling hooks: tp_tile_set_prof / tp_fb_set_prof write the __device__ pointer that
  the tile kernel (tploc.hip) / the fused kernel (tploc_fused.hip) reads, so setter and
  kernel must share one device symbol.

B = 256 rows x 39 keys = 9,984 keys: the flat geometry picks ten 1024-occurrence tiles and
8 bucket groups."""
import functools

import pytest
import torch

from parameter_server_amd.ops.countmin import CountMinSketch
from parameter_server_amd.ops.keymix import mix
from parameter_server_amd.ops.linear import AUC_BINS, new_accum
from parameter_server_amd.ops.localize import TP_TILE, Localizer
from parameter_server_amd.ops.native import hipops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, WIDTH = 256, 39
N_KEYS = B * WIDTH
FREQ = 1  # tail filter: keys seen once are dropped, so the unique ids leave the minibatch


@functools.lru_cache(maxsize=None)
def _keys(bits: int) -> torch.Tensor:
    """Half the occurrences from 300 hot ids (repeated keys), half drawn over the whole id
    range (unique ones)."""
    g = torch.Generator().manual_seed(bits)
    hot = torch.randint(0, 1 << bits, (300,), generator=g)
    cold = torch.randint(0, 1 << bits, (N_KEYS,), generator=g)
    pick = torch.rand(N_KEYS, generator=g) < 0.5
    k = torch.where(pick, hot[torch.randint(0, 300, (N_KEYS,), generator=g)], cold)
    c = torch.unique(k, return_counts=True)[1]
    assert int((c > 1).sum()) > 100 and int((c == 1).sum()) > 1000
    return k.to(DEV)


def _tiles() -> int:
    H = hipops()
    assert H.tpf_tile_log2(N_KEYS) == 10
    return H.tpf_stride(N_KEYS) // TP_TILE


def _buffers(bits: int, filt: bool, fill: int = 0) -> dict:
    H = hipops()
    N, g = H.tpf_stride_max(N_KEYS), H.tpf_groups(N_KEYS, bits)
    kr, er = H.tpf_key_region(), H.tpf_entry_region()

    def buf(k, dt):
        return torch.full((k,), fill, dtype=dt, device=DEV)

    b = dict(temp=buf(H.tpf_temp_bytes(N_KEYS, bits), torch.uint8), dcnt=buf(N // TP_TILE, torch.int32),
             rep=buf(N_KEYS, torch.int16), uniqf=buf(g * kr, torch.int64),
             ent_pos=buf(g * er, torch.int32), ent_j=buf(g * er, torch.int16),
             cnt=buf(4 * g, torch.int32), err=torch.zeros(1, dtype=torch.int32, device=DEV))
    if filt:  # its own zeroed sketch; w_ent = 1 so that the filter's zeros show
        b.update(cm=CountMinSketch(1 << 16, 2, DEV, key_bits=bits), ecnt=buf(N, torch.uint8),
                 w_ent=torch.ones(N, dtype=torch.float32, device=DEV), cnt_pre=buf(4 * g, torch.int32))
    return b


def _localize(bits: int, stages, filt: bool, b: dict | None = None) -> dict:
    """localize_tpf once per stage of ``stages`` on one set of (fresh) buffers."""
    H = hipops()
    b = b or _buffers(bits, filt)
    f = (*b["cm"].args(FREQ), b["ecnt"], b["w_ent"], b["cnt_pre"]) if filt else None
    for s in stages:
        H.localize_tpf(_keys(bits), bits, b["temp"], b["dcnt"], b["rep"], b["uniqf"], b["ent_pos"],
                       b["ent_j"], b["cnt"], b["err"], False, filt=f, stage=s)
    torch.cuda.synchronize()
    assert int(b["err"].item()) == 0
    return b


def _live(bits: int, b: dict, filt: bool) -> dict:
    """The outputs a consumer reads, in a form that does not depend on the order of LDS
    atomics. dcnt, cnt, the sketch cells and cnt_pre are compared as bytes. The tile kernel
    hands out a tile's entry positions, and the bucket kernel a unit's key indices, in the
    order in which its lanes' LDS atomics land, so rep, uniqf, ent_pos, ent_j (and ecnt /
    w_ent, indexed by entry) are one of many equivalent numberings: two stage-0 calls on
    fresh buffers differed in rep, uniqf and ent_j in 12 of 12 repeats on an MI355X. What is
    fixed is what the numbering denotes, and that is compared exactly: the key (occurrence
    count, weight) of every occurrence's entry, each unit's key set, each group's set of
    (tile, key) entries -- taken from the parts of uniqf / ent_pos / ent_j that cnt declares
    live (per group: D0 keys of unit 0, D1 of unit 1, E0 then E1 entries)."""
    H = hipops()
    T = _tiles()
    g, kr, er = H.tpf_groups(N_KEYS, bits), H.tpf_key_region(), H.tpf_entry_region()
    cnt = b["cnt"].cpu().view(-1, 4)[:g]
    uq, ep = b["uniqf"].cpu(), b["ent_pos"].cpu().long()
    ej = b["ent_j"].cpu().long() & 0xFFFF
    key_of_eid = torch.full((T * TP_TILE,), -1, dtype=torch.int64)
    unit_keys, group_entries = [], []
    for i, (d0, e0, d1, e1) in enumerate(cnt.tolist()):
        assert 0 <= d0 <= kr // 2 and 0 <= d1 <= kr // 2 and 0 <= e0 + e1 <= er
        ent = []
        for kb, d, ea, eb in ((i * kr, d0, 0, e0), (i * kr + kr // 2, d1, e0, e0 + e1)):
            keys = uq[kb:kb + d]
            pos, j = ep[i * er + ea:i * er + eb], ej[i * er + ea:i * er + eb]
            assert bool((j < d).all()) and bool((key_of_eid[pos] == -1).all())  # each entry once
            key_of_eid[pos] = keys[j]
            unit_keys.append(torch.sort(keys).values)
            ent.append((pos // TP_TILE << 40) + keys[j])
        group_entries.append(torch.sort(torch.cat(ent)).values)
    occ = torch.arange(N_KEYS)
    eid = (occ >> H.tpf_tile_log2(N_KEYS)) * TP_TILE + (b["rep"].cpu().long() & 0xFFFF)
    out = dict(dcnt=b["dcnt"].cpu()[:T], cnt=cnt, occ_key=key_of_eid[eid],
               unit_keys=torch.cat(unit_keys), group_entries=torch.cat(group_entries))
    if filt:
        w = b["w_ent"].cpu()
        out.update(cells=b["cm"].cells.cpu(), cnt_pre=b["cnt_pre"].cpu(),
                   occ_ecnt=b["ecnt"].cpu()[eid], occ_w=w[eid], w_zeros=(w == 0).sum())
    return out


@functools.lru_cache(maxsize=None)
def _all_stages(bits: int, filt: bool):
    """One stage-0 call on fresh buffers: the reference of every decomposition."""
    ref = _live(bits, _localize(bits, (0,), filt), filt)
    assert int(ref["cnt"].sum()) > 0 and int(ref["dcnt"].sum()) > 0
    # every occurrence's entry carries the occurrence's own (mixed) key; with the filter the
    # keys seen once have left the minibatch
    mk = mix(_keys(bits).cpu(), bits)
    kept = ref["occ_key"] >= 0
    assert torch.equal(ref["occ_key"][kept], mk[kept])
    if filt:
        # (a CountMin estimate is never below the count: repeated keys all stay; most of
        # the keys seen once go, the rest collide in the small sketch)
        seen = torch.unique(mk, return_inverse=True, return_counts=True)
        often = seen[2][seen[1]] > FREQ
        assert bool(kept[often].all()) and int((~kept).sum()) > int((~often).sum()) // 2
    else:
        assert bool(kept.all())
    return ref


@pytest.mark.parametrize("bits", [31, 34])  # 34: the quotient-encoded tile kernel
@pytest.mark.parametrize("stages,filt", [((1, 2), False), ((4,), False),
                                         ((1, 2, 3), True), ((4, 3), True)])
def test_localize_tpf_stage_sequences_equal_one_call(bits, stages, filt):
    ref = _all_stages(bits, filt)
    got = _live(bits, _localize(bits, stages, filt), filt)
    assert got.keys() == ref.keys()
    for name in ref:
        assert torch.equal(got[name], ref[name]), (name, stages)
    if filt:  # the filter did drop keys, and zeroed their entries' weights
        assert int(got["cnt"].sum()) < int(got["cnt_pre"].sum())
        assert int(got["w_zeros"]) > 0 and bool((got["occ_w"] == (got["occ_key"] >= 0)).all())


@pytest.mark.parametrize("bits", [31, 34])
def test_localize_tpf_filter_stage_without_filter_launches_nothing(bits):
    b = _localize(bits, (3,), False, _buffers(bits, False, fill=7))
    for name in ("dcnt", "rep", "uniqf", "ent_pos", "ent_j", "cnt", "temp"):
        assert bool((b[name] == 7).all()), name


# Shader-clock marks in phase order (the TILE_MARK / FB_MARK uses; slots 8 / 9 hold the
# workgroup's start / end on the realtime counter, slot 10 the CU id).
TILE_PHASES = (0, 1, 2, 3, 4, 5, 6)
FB_PHASES = (0, 1, 11, 12, 2, 3, 4, 5, 6)


def _check_marks(prof: torch.Tensor, phases):
    p = prof.view(_tiles(), 16).cpu()
    for cols in (list(phases), [8, 9]):
        m = p[:, cols]
        assert bool((m != 0).all()), cols
        assert bool((m[:, 1:] >= m[:, :-1]).all()), cols


def test_profiling_hooks_reach_their_kernels():
    H = hipops()
    bits, T = 31, _tiles()
    keys = _keys(bits)
    lz = Localizer(N_KEYS, bits, DEV, mode="tpf")
    assert lz.mode == "tpf"
    f = lz(keys)
    labels = torch.where(torch.rand(B, device=DEV) < 0.3, 1.0, -1.0)
    w_ent = torch.randn(f.w_ent.numel(), device=DEV) * 0.01
    coef = torch.empty(B, device=DEV)
    met = new_accum(DEV)
    hist = torch.zeros(2 * AUC_BINS, dtype=torch.int32, device=DEV)

    def fused():
        H.tp_fwd_bwd(f.rep, f.dcnt, None, N_KEYS, WIDTH, None, w_ent, labels, B, 2, coef, met,
                     hist, AUC_BINS, f.psum, None, None, None, None, False)
        torch.cuda.synchronize()

    def localise():
        lz(keys)
        torch.cuda.synchronize()

    tile_prof = torch.zeros(T * 16, dtype=torch.int64, device=DEV)
    fb_prof = torch.zeros(T * 16, dtype=torch.int64, device=DEV)
    try:
        H.tp_tile_set_prof(tile_prof)
        localise()
        _check_marks(tile_prof, TILE_PHASES)
        assert not bool(fb_prof.any())  # (the fused kernel's hook is still off)
        H.tp_fb_set_prof(fb_prof)
        fused()
        _check_marks(fb_prof, FB_PHASES)
        # off again: a further run leaves zeroed buffers zero
        H.tp_tile_set_prof(None)
        H.tp_fb_set_prof(None)
        tile_prof.zero_()
        fb_prof.zero_()
        localise()
        fused()
        assert not bool(tile_prof.any()) and not bool(fb_prof.any())
    finally:
        H.tp_tile_set_prof(None)
        H.tp_fb_set_prof(None)
    lz.check()
