"""The pack / unpack kernels of the fixed-capacity exchange (csrc/hip/exchange.hip) and the
owner's kv_resolve_rows, called directly and compared with the host model of the row
format (tests/exchange_model.py): 32- and 64-bit keys, 1 to 64 peers with empty, full and
overflowing owner runs, and the FixingFloat codes of the gradient region. Every output
buffer starts out filled with a sentinel word, so a store outside what the row format
documents shows up as well as a wrong value does."""
import numpy as np
import pytest
import torch

import exchange_model as M

pytestmark = pytest.mark.gpu

C = 257  # not a multiple of 4: H is rounded up and the last FixingFloat code word is ragged
DEV = "cuda"
TAIL = 37  # capacity of the unique-key arrays past n_uniq; holds garbage

LAYOUTS = {
    "g1_short": [200],
    "g1_over": [C + 5],
    "g3_empty_first": [0, C, C + 5],
    "g3_off": [C, 5, 31],
    "g3_empty_mid": [60, 0, 90],
    "g8": [0, 12, 0, 0, C, C + 5, 33, 0],
    "g64": [C + 5 if p == 20 else (0 if p % 2 else 3 + p % 5) for p in range(64)],
}


def _hh():
    from parameter_server_amd.ops.native import hipops

    return hipops()


def _dev_words(a):
    """uint32 rows -> flat int32 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).to(DEV)


def _words(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _assert_words_equal(got, want, what):
    got, want = got.reshape(-1), want.reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} words differ, first at {bad[0]}: "
                           f"{got[bad[0]]:#x} != {want[bad[0]]:#x}")


def _keys(n, kw, rng):
    """kw = 1: up to 2^32 - 1, a quarter with bit 31 set (negative as int32); kw = 2: a
    quarter with bit 63 set, a fifth with a zero low word."""
    if kw == 1:
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        k[::4] |= np.uint64(1 << 31)
        k[:3] = [0xFFFFFFFF, 0x80000000, 0][:min(n, 3)]
    else:
        k = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        k[::4] |= np.uint64(1 << 63)
        k[1::5] &= np.uint64(0xFFFFFFFF00000000)
        k[:2] = [0xFFFFFFFF00000000, 1 << 63][:min(n, 2)]
    return k


class _Step:
    """The unique keys of one step: n live entries in owner order, TAIL garbage ones."""

    def __init__(self, runs, kw, perm_on, seed):
        rng = np.random.default_rng(seed)
        self.off = M.offsets(runs)
        self.G, self.n = len(runs), int(self.off[-1])
        self.cap = self.n + TAIL
        self.keys = _keys(self.cap, kw, rng)
        self.grad = rng.standard_normal(self.cap).astype(np.float32)
        self.grad[self.n:] = 777.0
        self.perm = None
        if perm_on:
            self.perm = np.concatenate([rng.permutation(self.n), np.full(TAIL, -1)]).astype(np.int32)
        self.d_off = torch.from_numpy(self.off).to(DEV)
        self.d_n = torch.tensor([self.n], dtype=torch.int32, device=DEV)
        self.d_keys = torch.from_numpy(self.keys.view(np.int64).copy()).to(DEV)
        self.d_grad = torch.from_numpy(self.grad).to(DEV)
        self.d_perm = None if self.perm is None else torch.from_numpy(self.perm).to(DEV)

    def row_values(self, p, cap=C):
        """The gradients row p carries, in entry order."""
        a = int(self.off[p])
        j = np.arange(a, a + min(int(self.off[p + 1]) - a, cap))
        return self.grad[j if self.perm is None else self.perm[j]]


# ------------------------------------------------------------------ keys, gradients, weights
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_pack_keys_rows_equal_model(name, kw):
    hh = _hh()
    st = _Step(LAYOUTS[name], kw, False, seed=len(name) + kw)
    for merged in (False, True):
        H = M.row_words(C, kw, merged=merged)
        blank = M.new_rows(st.G, H)
        send = _dev_words(blank)
        ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
        hh.xchg_pack_keys(st.d_keys, st.d_n, st.d_off, C, kw, H, send, ovf)
        want, novf = M.pack_keys(st.keys, st.off, C, kw, H, blank)
        _assert_words_equal(_words(send), want, "xchg_pack_keys")
        assert int(ovf.item()) == novf == sum(max(r - C, 0) for r in LAYOUTS[name])
        hh.xchg_pack_keys(st.d_keys, st.d_n, st.d_off, C, kw, H, send, ovf)  # ovf accumulates
        hh.xchg_pack_keys(st.d_keys, st.d_n, st.d_off, C, kw, H, send, None)
        _assert_words_equal(_words(send), want, "xchg_pack_keys, repeated")
        assert int(ovf.item()) == 2 * novf


@pytest.mark.parametrize("perm_on", [False, True])
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_pack_grads_rows_equal_model(name, kw, perm_on):
    hh = _hh()
    st = _Step(LAYOUTS[name], kw, perm_on, seed=3 * len(name) + kw)
    for merged in (False, True):
        H = M.row_words(C, kw, merged=merged)
        blank = M.new_rows(st.G, H)
        send = _dev_words(blank)
        hh.xchg_pack_grads(st.d_grad, st.d_perm, st.d_n, st.d_off, C, kw, H, send)
        want = M.pack_grads(st.grad, st.perm, st.off, C, kw, H, blank)
        _assert_words_equal(_words(send), want, "xchg_pack_grads")
        # both halves of a row: the key pack leaves word 1 and the gradients alone, the
        # gradient pack word 0 and the keys
        hh.xchg_pack_keys(st.d_keys, st.d_n, st.d_off, C, kw, H, send, None)
        both, _ = M.pack_keys(st.keys, st.off, C, kw, H, want)
        _assert_words_equal(_words(send), both, "keys after gradients")
        hh.xchg_pack_grads(st.d_grad, st.d_perm, st.d_n, st.d_off, C, kw, H, send)
        _assert_words_equal(_words(send), both, "gradients after keys")


def test_pack_grads_publishes_the_overflow_count():
    """ovf_host (a pinned host word) receives the device counter in the gradient pack."""
    hh = _hh()
    st = _Step(LAYOUTS["g8"], 2, True, seed=1)
    H = M.row_words(C, 2)
    send = _dev_words(M.new_rows(st.G, H))
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    host = torch.full((1,), -1, dtype=torch.int32).pin_memory()
    hh.xchg_pack_keys(st.d_keys, st.d_n, st.d_off, C, 2, H, send, ovf)
    hh.xchg_pack_grads(st.d_grad, st.d_perm, st.d_n, st.d_off, C, 2, H, send, ovf=ovf,
                       ovf_host=host)
    torch.cuda.synchronize()
    assert int(host[0]) == int(ovf.item()) == 5


@pytest.mark.parametrize("perm_on", [False, True])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_unpack_w_equals_model(name, perm_on):
    hh = _hh()
    st = _Step(LAYOUTS[name], 1, perm_on, seed=5 * len(name))
    rng = np.random.default_rng(9)
    for ws in (C, C + 11):
        recv_w = rng.standard_normal((st.G - 1) * ws + C).astype(np.float32)
        recv_w[recv_w == 0] = 1.0  # a dropped key's exact 0 cannot come from a reply
        blank = np.full(st.cap, M.SENTINEL, dtype=np.uint32)
        w_local = _dev_words(blank).view(torch.float32)
        hh.xchg_unpack_w(torch.from_numpy(recv_w).to(DEV), st.d_perm, st.d_n, st.d_off, C, w_local,
                         ws)
        want = M.unpack_w(recv_w, st.perm, st.off, C, ws, st.cap, blank)
        _assert_words_equal(_words(w_local), want, f"xchg_unpack_w, wstride {ws}")
        j = np.arange(st.n)
        dropped = j - st.off[M.owner_of(st.off, j)] >= C
        uid = j if st.perm is None else st.perm[j]
        assert (want[uid[dropped]] == 0).all() and (want[st.n:] == M.SENTINEL).all()
        assert dropped.sum() == sum(max(r - C, 0) for r in LAYOUTS[name])


@pytest.mark.parametrize("keys,grads", [(True, False), (False, True), (True, True)])
def test_clear_counts_zeroes_only_the_counts(keys, grads):
    hh = _hh()
    for G in (1, 8, 64):
        H = M.row_words(C, 2)
        blank = M.new_rows(G, H)
        send = _dev_words(blank)
        hh.xchg_clear_counts(send, H, keys, grads)
        if keys:
            blank[:, 0] = 0
        if grads:
            blank[:, 1] = 0
        _assert_words_equal(_words(send), blank, "xchg_clear_counts")


# ------------------------------------------------------------------------- loopback step
@pytest.mark.parametrize("kw", [1, 2])
def test_loopback_rows_resolve_on_the_owner(kw):
    """recv = send: 8 rows of sorted unique keys, many keys in several rows, resolved by
    kv_resolve_rows in one launch."""
    from parameter_server_amd.ops.kv_table import KVTable

    hh = _hh()
    rng = np.random.default_rng(40 + kw)
    runs = LAYOUTS["g8"]
    G, off = len(runs), M.offsets(runs)
    n = int(off[-1])
    pool = np.unique(_keys(500, kw, rng))
    ukeys = np.concatenate([np.sort(rng.choice(pool, r, replace=False)) for r in runs] +
                           [_keys(TAIL, kw, rng)])
    H = M.row_words(C, kw)
    send = _dev_words(M.new_rows(G, H))
    hh.xchg_pack_keys(torch.from_numpy(ukeys.view(np.int64).copy()).to(DEV),
                      torch.tensor([n], dtype=torch.int32, device=DEV),
                      torch.from_numpy(off).to(DEV), C, kw, H, send, None)
    cnt = np.minimum(np.diff(off), C)
    sent = [ukeys[off[p]:off[p] + cnt[p]] for p in range(G)]
    key_range = (0, 1 << 32) if kw == 1 else (0, (1 << 64) - 1)
    ws = C + 11

    def resolve(tb, insert):
        slot = torch.full((G * C,), -7, dtype=torch.int64, device=DEV)
        w = _dev_words(np.full((G - 1) * ws + C, M.SENTINEL, dtype=np.uint32)).view(torch.float32)
        okey = torch.full((G * C,), -7, dtype=torch.int64, device=DEV)
        it, iv, isd, seed = tb.init.args()
        hh.kv_resolve_rows(tb.slots, send, H, C, kw, slot, w, insert, it, iv, isd, seed, tb._err,
                           None, tb.home_base, tb.home_m, okey, None, 0, ws)
        torch.cuda.synchronize()
        assert int(tb._err.item()) == 0
        return slot.cpu().numpy().reshape(G, C), _words(w), okey.cpu().numpy().reshape(G, C)

    def live(ws_words, p):
        return ws_words[p * ws:p * ws + cnt[p]]

    tb = KVTable(1 << 14, DEV, key_range=key_range)
    slot, w, okey = resolve(tb, False)  # nothing inserted yet: no slot, weight 0
    for p in range(G):
        assert (slot[p, :cnt[p]] == -1).all() and (slot[p, cnt[p]:] == -7).all()
        assert (live(w, p) == 0).all()
    assert tb.census()[0] == 0
    slot, w, okey = resolve(tb, True)
    key_slot = {}
    for p in range(G):
        assert np.array_equal(okey[p, :cnt[p]].view(np.uint64), sent[p])
        assert (okey[p, cnt[p]:] == -7).all() and (slot[p, cnt[p]:] == -7).all()
        assert (slot[p, :cnt[p]] >= 0).all() and (slot[p, :cnt[p]] < tb.capacity).all()
        for k, s in zip(sent[p].tolist(), slot[p, :cnt[p]].tolist()):
            assert key_slot.setdefault(k, s) == s  # one slot per key, whichever row carries it
    assert len(set(key_slot.values())) == len(key_slot) == tb.census()[0]
    assert len(key_slot) < int(cnt.sum())  # (keys were shared between rows)
    # weights travel back at out_w[s * wstride + i]; nothing else of out_w is written
    kk = np.array(sorted(key_slot), dtype=np.uint64)
    wv = rng.standard_normal(kk.size).astype(np.float32)
    tb.set(torch.tensor([key_slot[k] for k in kk.tolist()], dtype=torch.int64, device=DEV),
           w=torch.from_numpy(wv).to(DEV))
    slot2, w, _ = resolve(tb, False)
    assert np.array_equal(slot2, slot)
    want = np.full((G - 1) * ws + C, M.SENTINEL, dtype=np.uint32)
    for p in range(G):
        want[p * ws:p * ws + cnt[p]] = wv[np.searchsorted(kk, sent[p])].view(np.uint32)
    _assert_words_equal(w, want, "kv_resolve_rows out_w")


# --------------------------------------------------------------------------- FixingFloat
FF_LAYOUTS = {  # G -> (runs, what each row's gradients are)
    1: ([C + 5], ["randn"]),
    2: ([128, 64], ["pm0", "pm0"]),  # whole waves of one owner: the wave-reduced min / max
    3: ([C, 0, 77], ["nan10", "randn", "randn"]),
    8: ([0, 1, 40, 41, 42, 43, 200, C + 5],
        ["randn", "randn", "zero", "k1000", "pm0", "big", "nan10", "randn"]),
}


def _ff_values(kind, n, rng):
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    if kind == "zero":
        x[:] = 0.0
    elif kind == "k1000":
        x[:] = 1000.0  # 1000 + 1e-6f == 1000 in float32: bin = 0
    elif kind == "pm0":
        x = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    elif kind == "big":
        x = np.where(rng.random(n) < 0.5, np.float32(1e30), np.float32(-1e30)).astype(np.float32)
    elif kind == "nan10":
        x[rng.random(n) < 0.1] = np.nan
    return x


class _FFStep(_Step):
    def __init__(self, G, kw, perm_on, seed):
        runs, kinds = FF_LAYOUTS[G]
        super().__init__(runs, kw, perm_on, seed)
        rng = np.random.default_rng(seed + 1000)
        for p, kind in enumerate(kinds):
            a, b = int(self.off[p]), int(self.off[p + 1])
            j = np.arange(a, b)
            self.grad[j if self.perm is None else self.perm[j]] = _ff_values(kind, b - a, rng)
        self.kinds = kinds
        self.d_grad = torch.from_numpy(self.grad).to(DEV)


def _check_minmax_word(word, want, vals, what):
    """Header words 2 / 3: ff_ord of the row's min / max. Where that is a zero and the row
    holds zeros of both signs, either zero is the min (max): the wave reduction in front
    of the int atomics compares floats, and -0.0 < +0.0 is false."""
    got = np.array([word], dtype=np.uint32).view(np.int32)[0]
    if want == 0 and (vals == 0).any():
        ok = {int(M.ff_ord(v)) for v in vals[vals == 0]}
        assert int(got) in ok, (what, got, ok)
    else:
        assert got == M.ff_ord(want), (what, got, M.ff_ord(want), want)


def _check_ff_rows(rows, values, kw, nb, H, key_words=None):
    """Every row of an encoded buffer against the model; returns the codes per row."""
    codes = []
    for p, vals in enumerate(values):
        row, n = rows[p], vals.size
        assert row[1] == n
        if key_words is None:
            assert row[0] == M.SENTINEL and (row[4:4 + C * kw] == M.SENTINEL).all()
        else:
            assert np.array_equal(row[[0] + list(range(4, 4 + C * kw))], key_words[p])
        mn, mx = M.ff_minmax(vals)
        ok = ~np.isnan(vals)
        _check_minmax_word(row[2], mn, vals[ok], f"row {p} min")
        _check_minmax_word(row[3], mx, vals[ok], f"row {p} max")
        lo, hi, t = M.ff_targets(vals, nb)
        by = row[4 + C * kw:].view(np.uint8)
        assert (by[n * nb:] == 0x5A).all(), f"row {p}: code bytes past the count written"
        r = M.ff_codes(by, n, nb)
        assert (r[ok] >= 0).all() and (r[ok] <= M.ff_ratio(nb)).all()
        if ok.any():
            assert np.abs(r[ok] - t[ok]).max() <= 1 + 1e-6, f"row {p} ({n} entries)"
        codes.append(r)
    return codes


def _check_ff_decode(gin, codes, values, nb):
    gin = gin.reshape(len(values), C)
    for p, (r, vals) in enumerate(zip(codes, values)):
        n = vals.size
        assert (gin[p, n:].view(np.uint32) == M.SENTINEL).all(), f"row {p}: gin past the count"
        lo, hi, _ = M.ff_targets(vals, nb)
        want = M.ff_decode(r, lo, hi, nb)
        got = gin[p, :n].astype(np.float64)
        assert (np.abs(got - want) <= M.ulp32(want)).all(), f"row {p}: decode"
        ok = ~np.isnan(vals)
        if ok.any():
            step = (float(hi) - float(lo)) / M.ff_ratio(nb) if hi > lo else 0.0
            bound = step * (1 + 1e-6) + 2.4e-7 * np.abs(vals[ok]).max()
            assert np.abs(got[ok] - vals[ok]).max() <= bound, f"row {p}: round trip"
        if n and (vals == 0).all():
            assert (gin[p, :n] == 0).all()
        if n and (vals == 1000.0).all():
            assert (gin[p, :n] == np.float32(1000.0)).all()


@pytest.mark.parametrize("step_on", [False, True])
@pytest.mark.parametrize("perm_on", [False, True])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_ff_pack_and_decode_rows(nb, kw, G, perm_on, step_on):
    """xchg_ff_pack_grads (min / max by the producer's atomics) then xchg_ff_decode."""
    hh = _hh()
    st = _FFStep(G, kw, perm_on, seed=nb * 100 + kw * 10 + G)
    H = M.row_words(C, kw, nb)
    step = torch.tensor([12345678901], dtype=torch.int64, device=DEV) if step_on else None
    send = _dev_words(M.new_rows(G, H))
    gstage = _dev_words(np.full(G * C, M.SENTINEL, dtype=np.uint32)).view(torch.float32)
    hh.xchg_ff_pack_grads(st.d_grad, st.d_perm, st.d_n, st.d_off, C, kw, H, nb, 77, step, send,
                          gstage)
    values = [st.row_values(p) for p in range(G)]
    rows = _words(send).reshape(G, H)
    codes = _check_ff_rows(rows, values, kw, nb, H)
    staged = _words(gstage).reshape(G, C)
    for p, vals in enumerate(values):  # the staging rows: the live gradients, bit for bit
        assert np.array_equal(staged[p, :vals.size], vals.view(np.uint32))
        assert (staged[p, vals.size:] == M.SENTINEL).all()
    gin = _dev_words(np.full(G * C, M.SENTINEL, dtype=np.uint32)).view(torch.float32)
    hh.xchg_ff_decode(send, C, kw, H, nb, gin)
    _check_ff_decode(gin.cpu().numpy(), codes, values, nb)
    # the same (seed, step, row) draws the same bits; the key pack leaves the codes alone
    send2 = _dev_words(M.new_rows(G, H))
    hh.xchg_pack_keys(st.d_keys, st.d_n, st.d_off, C, kw, H, send2, None)
    key_words = _words(send2).reshape(G, H)[:, [0] + list(range(4, 4 + C * kw))].copy()
    hh.xchg_ff_pack_grads(st.d_grad, st.d_perm, st.d_n, st.d_off, C, kw, H, nb, 77, step, send2,
                          gstage)
    rows2 = _words(send2).reshape(G, H)
    _check_ff_rows(rows2, values, kw, nb, H, key_words)
    _assert_words_equal(rows2[:, 1:4], rows[:, 1:4], "header of a second call")
    _assert_words_equal(rows2[:, 4 + C * kw:], rows[:, 4 + C * kw:], "codes of a second call")


@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_ff_encode_from_producer_partials(nb, kw, G):
    """xchg_ff_encode with per = 3: the rows staged by a producer, min / max from its
    workgroups' partials at gstage[G * C + 2 w]; one producer of each row contributes
    nothing (the identity pair)."""
    hh = _hh()
    per = 3
    st = _FFStep(G, kw, False, seed=nb * 100 + kw * 10 + G + 5)
    H = M.row_words(C, kw, nb)
    values = [st.row_values(p) for p in range(G)]
    gs = np.full(G * C + 2 * G * per, M.SENTINEL, dtype=np.uint32).view(np.float32)
    blank = M.new_rows(G, H)
    for p, vals in enumerate(values):
        gs[p * C:p * C + vals.size] = vals
        blank[p, 1] = vals.size
        h = vals.size // 2
        for q, part in ((0, vals[:h]), (1, vals[:0]), (2, vals[h:])):
            gs[G * C + 2 * (p * per + q):][:2] = M.ff_minmax(part)
    send = _dev_words(blank)
    step = torch.tensor([3], dtype=torch.int64, device=DEV)
    hh.xchg_ff_encode(torch.from_numpy(gs).to(DEV), C, kw, H, nb, 77, step, send, per)
    rows = _words(send).reshape(G, H)
    codes = _check_ff_rows(rows, values, kw, nb, H)
    gin = _dev_words(np.full(G * C, M.SENTINEL, dtype=np.uint32)).view(torch.float32)
    hh.xchg_ff_decode(send, C, kw, H, nb, gin)
    _check_ff_decode(gin.cpu().numpy(), codes, values, nb)


@pytest.mark.parametrize("nb", [1, 2, 3])
def test_ff_nan_marks_leave_the_other_codes_alone(nb):
    """A row with 10 % NaN against the same row with its NaNs replaced by an in-range
    value, same seed / step / row: same header, same code at every other entry."""
    hh = _hh()
    rng = np.random.default_rng(nb)
    x = _ff_values("nan10", C, rng)
    y = np.where(np.isnan(x), np.float32(0.01), x).astype(np.float32)
    assert np.isnan(x).sum() > 10
    H = M.row_words(C, 1, nb)
    off = torch.tensor([0, C], dtype=torch.int64, device=DEV)
    n = torch.tensor([C], dtype=torch.int32, device=DEV)
    out = []
    for v in (x, y):
        send = _dev_words(M.new_rows(1, H))
        gstage = torch.zeros(C, dtype=torch.float32, device=DEV)
        hh.xchg_ff_pack_grads(torch.from_numpy(v).to(DEV), None, n, off, C, 1, H, nb, 5, None, send,
                              gstage)
        out.append(_words(send).reshape(1, H)[0])
    assert np.array_equal(out[0][:4], out[1][:4])
    assert out[0][2] == M.ff_ord(np.nanmin(x)).view(np.uint32)
    assert out[0][3] == M.ff_ord(np.nanmax(x)).view(np.uint32)
    rx, ry = (M.ff_codes(o[4 + C:].view(np.uint8), C, nb) for o in out)
    ok = ~np.isnan(x)
    assert np.array_equal(rx[ok], ry[ok])


# ------------------------------------------------------------------------ rounding draws
BIG = 65536


def _encode_big(x, nb, seed, step, G=1):
    """Codes [G, C] of x split into G equal rows, by xchg_ff_pack_grads."""
    hh = _hh()
    Cb = x.size // G
    H = M.row_words(Cb, 1, nb)
    send = _dev_words(M.new_rows(G, H))
    gstage = torch.zeros(x.size, dtype=torch.float32, device=DEV)
    off = torch.arange(G + 1, dtype=torch.int64, device=DEV) * Cb
    n = torch.tensor([x.size], dtype=torch.int32, device=DEV)
    d_step = None if step is None else torch.tensor([step], dtype=torch.int64, device=DEV)
    hh.xchg_ff_pack_grads(torch.from_numpy(x).to(DEV), None, n, off, Cb, 1, H, nb, seed, d_step,
                          send, gstage)
    rows = _words(send).reshape(G, H)
    return np.stack([M.ff_codes(rows[p, 4 + Cb:].view(np.uint8), Cb, nb) for p in range(G)])


@pytest.fixture(scope="module")
def big_row():
    return (0.3 * np.random.default_rng(2024).standard_normal(BIG)).astype(np.float32)


@pytest.mark.parametrize("nb", [1, 2, 3])
def test_ff_rounding_is_unbiased(big_row, nb):
    """Over 65,536 entries the number of round-ups is within 6 standard deviations of
    sum(frac(t)): independent Bernoulli(p_i) draws have variance sum p_i (1 - p_i). (The
    device's uniform has 2^-24 granularity, which moves the mean by under 0.004.)"""
    _, _, t = M.ff_targets(big_row, nb)
    worst = 0.0
    for seed, step in ((1, 7), (2, None), (1, 8)):
        r = _encode_big(big_row, nb, seed, step)[0]
        assert (r >= 0).all() and (r <= M.ff_ratio(nb)).all() and np.abs(r - t).max() <= 1 + 1e-6
        up, exp, sd = M.ff_round_stats(r, t)
        print(f"xchg_ff_encode nb={nb} seed={seed} step={step}: round-ups {up:.0f}, expected "
              f"{exp:.1f}, {(up - exp) / sd:+.2f} sigma")
        worst = max(worst, abs(up - exp) / sd)
        assert abs(up - exp) <= 6 * sd
    print(f"xchg_ff_encode nb={nb}: worst deviation {worst:.2f} sigma")


def test_ff_rounding_bits_are_deterministic_and_fresh(big_row):
    """nb = 1. The same (seed, step, row) gives the same codes; another step, another seed
    or another row of the same call gives codes that differ at no fewer than half of the
    entries at which two independent draws are expected to: mean(2 p (1 - p)), about 1/3."""
    _, _, t = M.ff_targets(big_row, 1)
    want = M.ff_expected_differing(t)
    assert abs(want - 1 / 3) < 0.01
    a = _encode_big(big_row, 1, 11, 7)[0]
    assert np.array_equal(a, _encode_big(big_row, 1, 11, 7)[0])
    assert np.array_equal(_encode_big(big_row, 1, 11, None)[0], _encode_big(big_row, 1, 11, 0)[0])
    for what, b in (("step + 1", _encode_big(big_row, 1, 11, 8)[0]),
                    ("another seed", _encode_big(big_row, 1, 12, 7)[0]),
                    ("no step clock", _encode_big(big_row, 1, 11, None)[0])):
        frac = float((a != b).mean())
        print(f"xchg_ff_encode nb=1, {what}: differing-code fraction {frac:.3f} "
              f"(independent draws: {want:.3f})")
        assert frac >= 0.5 * want, what
    half = big_row[:BIG // 2]
    two = _encode_big(np.concatenate([half, half]), 1, 11, 7, G=2)
    want2 = M.ff_expected_differing(M.ff_targets(half, 1)[2])
    frac = float((two[0] != two[1]).mean())
    print(f"xchg_ff_encode nb=1, two rows of one call: differing-code fraction {frac:.3f} "
          f"(independent draws: {want2:.3f})")
    assert frac >= 0.5 * want2
