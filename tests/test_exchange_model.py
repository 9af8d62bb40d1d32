"""The host model of the exchange rows (tests/exchange_model.py) against what the package
states on the CPU: SparseLRTrainer._row_geometry / KVWorker's row sizes, and the CPU
FixingFloat encoder (ops.fixing_float, reference src/filter/fixing_float.h:44-95). The GPU
tests compare the pack / unpack kernels with this model, so it has to be right on its own."""
import types

import numpy as np
import pytest
import torch

import exchange_model as M

C = 257


def _layout(G):
    runs = {1: [C + 5], 3: [0, C, C + 5], 8: [0, 12, 0, 0, C, C + 5, 33, 0]}[G]
    return M.offsets(runs)


@pytest.mark.parametrize("merged", [False, True])
@pytest.mark.parametrize("nb", [0, 1, 2, 3])
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("cap", [1, 257, 4096])
def test_row_words_is_the_trainers_geometry(cap, kw, nb, merged):
    from parameter_server_amd.models import SparseLRTrainer

    me = types.SimpleNamespace(bits=32 if kw == 1 else 34,
                               cfg=types.SimpleNamespace(fixing_float_bytes=nb))
    gkw, gnb, w0, H = SparseLRTrainer._row_geometry(me, cap, merged)
    assert (gkw, gnb) == (kw, nb)
    assert M.row_words(cap, kw, nb, merged=merged) == H
    assert H % 4 == 0 and H >= w0 + (cap if merged else 0)
    assert w0 == 4 + cap * kw + (-(-cap * nb // 4) if nb else cap)


@pytest.mark.parametrize("bits,k", [(32, 1), (64, 1), (64, 3), (32, 16)])
def test_row_words_is_the_kv_workers_geometry(bits, k):
    from parameter_server_amd.parallel.comm import LoopbackComm
    from parameter_server_amd.parameter.sharded_kv import KVWorker

    kv = KVWorker(LoopbackComm(2), "cpu", dim=k, max_keys=4096, key_bits=bits, capacity=1 << 10)
    assert kv.kw == (1 if bits <= 32 else 2)
    assert M.row_words(kv.C, kv.kw, k=0) == kv.Hk
    assert M.row_words(kv.C, kv.kw, k=k) == kv.Hp
    assert M.row_words(kv.C, 0, k=k) == kv.Hv


@pytest.mark.parametrize("perm_on", [False, True])
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("G", [1, 3, 8])
def test_pack_then_unpack_is_the_identity_on_kept_keys(G, kw, perm_on):
    """The owner answers entry i of row p with f(key); unpacking the answers gives f(key)
    at every kept key's unique id and 0 at every dropped one."""
    rng = np.random.default_rng(G * 10 + kw)
    off = _layout(G)
    n = int(off[-1])
    keys = rng.integers(0, 1 << (32 if kw == 1 else 64), n, dtype=np.uint64)
    keys[:: 7] |= np.uint64(1 << (31 if kw == 1 else 63))
    if kw == 2:
        keys[1:: 5] &= np.uint64(0xFFFFFFFF00000000)
    perm = rng.permutation(n).astype(np.int32) if perm_on else None
    H = M.row_words(C, kw)
    send, ovf = M.pack_keys(keys, off, C, kw, H)
    cnt = np.minimum(np.diff(off), C)
    assert ovf == int(np.maximum(np.diff(off) - C, 0).sum())
    assert (send[:, 0] == cnt).all() and (send[:, 1:4] == M.SENTINEL).all()
    ws = C + 11
    recv_w = np.zeros((G - 1) * ws + C, dtype=np.float32)
    for p in range(G):
        row = send[p, 4:4 + C * kw]
        got = row if kw == 1 else row.view(np.uint64)
        assert np.array_equal(got[:cnt[p]], keys[off[p]:off[p] + cnt[p]] &
                              np.uint64(0xFFFFFFFF if kw == 1 else (1 << 64) - 1))
        assert (row[cnt[p] * kw:] == M.SENTINEL).all() and (send[p, 4 + C * kw:] == M.SENTINEL).all()
        recv_w[p * ws:p * ws + cnt[p]] = (got[:cnt[p]] % np.uint64(1000003)).astype(np.float32)
    w = M.unpack_w(recv_w, perm, off, C, ws, n).view(np.float32)
    uid = np.arange(n) if perm is None else perm.astype(np.int64)
    kept = (np.arange(n) - off[M.owner_of(off, np.arange(n))]) < C
    want = np.where(kept, ((keys & np.uint64(0xFFFFFFFF if kw == 1 else (1 << 64) - 1)) %
                           np.uint64(1000003)).astype(np.float32), np.float32(0))
    assert np.array_equal(w[uid], want) and (~kept).sum() == ovf
    # the gradients travel the same way: row p entry i carries grad[perm[off[p] + i]]
    grad = rng.standard_normal(n).astype(np.float32)
    sg = M.pack_grads(grad, perm, off, C, kw, M.row_words(C, kw, merged=True))
    assert (sg[:, 1] == cnt).all() and (sg[:, 0] == M.SENTINEL).all()
    for p in range(G):
        g = sg[p, 4 + C * kw:4 + C * kw + cnt[p]].view(np.float32)
        assert np.array_equal(g, grad[uid[off[p]:off[p] + cnt[p]]])


def test_owner_of_skips_empty_runs():
    off = M.offsets([0, 3, 0, 0, 2, 0])
    assert M.owner_of(off, np.arange(5)).tolist() == [1, 1, 1, 4, 4]
    assert M.owner_of(M.offsets([4]), np.arange(4)).tolist() == [0] * 4


def test_ff_ord_is_monotone_and_invertible():
    f = np.array([-np.inf, -3.4e38, -1.5, -1e-45, -0.0, 0.0, 1e-45, 2.5, 3.4e38, np.inf],
                 dtype=np.float32)
    o = M.ff_ord(f)
    assert (np.diff(o.astype(np.int64)) > 0).all()
    assert np.array_equal(M.ff_unord(o).view(np.int32), f.view(np.int32))
    assert M.ff_ord(np.float32(-0.0)) == -1 and M.ff_ord(np.float32(0.0)) == 0


def _cpu_codes(x, nb, seed):
    from parameter_server_amd.ops import fixing_float as FF

    code, mm = FF.encode(torch.from_numpy(x), nb, seed=seed)
    dec = FF.decode(code, nb, mm).numpy()
    return M.ff_codes(code.numpy(), x.size, nb), mm.numpy(), dec


@pytest.mark.parametrize("n", [1, 2, 257, 65536])
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_ff_model_reproduces_the_cpu_encoder(nb, n):
    """Codes of the CPU encoder lie within one level of the model's targets, its decoder
    agrees with ff_decode to 1 float32 ulp, and its rounding draws are unbiased and
    differ between seeds as often as independent draws would (the conditions the GPU
    tests put on xchg_ff_encode)."""
    rng = np.random.default_rng(nb * 100 + n % 97)
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    r, mm, dec = _cpu_codes(x, nb, seed=5)
    lo, hi, t = M.ff_targets(x, nb)
    assert lo == mm[0] == x.min() and hi == mm[1]
    assert hi == np.float32(x.max() + np.float32(1e-6))
    assert (r >= 0).all() and (r <= M.ff_ratio(nb)).all()
    assert np.abs(r - t).max() <= 1 + 1e-6
    want = M.ff_decode(r, lo, hi, nb)
    assert (np.abs(dec.astype(np.float64) - want) <= M.ulp32(want)).all()
    step = (float(hi) - float(lo)) / M.ff_ratio(nb)
    assert np.abs(dec.astype(np.float64) - x).max() <= step * (1 + 1e-6) + 2.4e-7 * np.abs(x).max()
    up, exp, sd = M.ff_round_stats(r, t)
    print(f"cpu encoder nb={nb} n={n}: round-ups {up:.0f}, expected {exp:.1f}, "
          f"{(up - exp) / sd if sd else 0.0:+.2f} sigma")
    assert abs(up - exp) <= 6 * sd
    if n == 65536 and nb == 1:
        r2 = _cpu_codes(x, nb, seed=6)[0]
        frac, want_frac = float((r != r2).mean()), M.ff_expected_differing(t)
        print(f"cpu encoder nb=1: differing-code fraction {frac:.3f}, expected {want_frac:.3f}")
        assert abs(want_frac - 1 / 3) < 0.01 and frac >= 0.5 * want_frac


def test_ff_targets_edge_rows():
    lo, hi, t = M.ff_targets(np.zeros(0, dtype=np.float32), 2)  # empty: the init identities
    assert (lo, hi) == (M.FF_INIT_LO, M.FF_INIT_HI) and t.size == 0
    lo, hi, t = M.ff_targets(np.full(5, 1000.0, dtype=np.float32), 1)
    assert hi == lo == np.float32(1000.0) and (t == 0).all()  # 1000 + 1e-6f == 1000 in float32
    assert (M.ff_decode(np.arange(5), lo, hi, 1) == np.float32(1000.0)).all()
    lo, hi, t = M.ff_targets(np.zeros(5, dtype=np.float32), 3)
    assert lo == 0 and hi == np.float32(1e-6) and (t == 0).all()
    assert (M.ff_decode(t, lo, hi, 3).view(np.int32) == 0).all()
    z = np.array([0.0, -0.0, 0.0], dtype=np.float32)
    mn, mx = M.ff_minmax(z)
    assert np.signbit(mn) and not np.signbit(mx)
    x = np.array([1.0, np.nan, -2.0, np.nan, 0.5], dtype=np.float32)
    lo, hi, t = M.ff_targets(x, 2)
    assert lo == -2.0 and hi == np.float32(1.0 + np.float32(1e-6))
    assert np.isnan(t[[1, 3]]).all() and t[2] == 0 and abs(t[0] - M.ff_ratio(2)) < 1
    lo, hi, t = M.ff_targets(np.array([-1e30, 1e30], dtype=np.float32), 1)
    assert t[0] == 0 and t[1] == M.ff_ratio(1)


@pytest.mark.parametrize("k", [1, 3])
def test_kvv_pack_vals_sums_duplicates_in_position_order(k):
    from parameter_server_amd.ops.localize import localize_torch

    rng = np.random.default_rng(k)
    keys = np.concatenate([rng.integers(0, 50, 300), np.full(64, 7)])
    rng.shuffle(keys)
    vals = rng.standard_normal((keys.size, k)).astype(np.float32)
    loc = localize_torch(torch.from_numpy(keys.astype(np.int64)), 32)
    U = loc.uniq.numel()
    off = M.offsets([5, 0, U - 5])
    Cc = 20
    H = M.row_words(Cc, 1, k=k)
    send, s32, s64 = M.kvv_pack_vals(vals, k, loc.pos_s.numpy(), loc.seg_start.numpy(), off, Cc, 1, H)
    lc = loc.local_col.numpy()
    for u in range(U):
        pos = np.flatnonzero(lc == u)  # ascending positions
        acc = np.zeros(k, dtype=np.float32)
        for q in pos:
            acc = acc + vals[q]
        assert np.array_equal(acc, s32[u])
        np.testing.assert_allclose(s64[u], vals[pos].astype(np.float64).sum(0), rtol=0, atol=1e-12)
    assert send[:, 1].tolist() == [5, 0, Cc] and (send[:, 0] == M.SENTINEL).all()
    v = send[2, 4 + Cc:4 + Cc + Cc * k].view(np.float32).reshape(Cc, k)
    assert np.array_equal(v, s32[5:5 + Cc])
    assert (send[2, 4 + Cc + Cc * k:] == M.SENTINEL).all() and (send[1, 2:] == M.SENTINEL).all()
