"""The k-value rows of the KVWorker API (csrc/hip/kvapi.hip): kvv_pack_vals, kvv_serve,
kv_serve_w, kvv_apply, kvv_unpack and kvv_single_off called directly, against the host
model of the row format (tests/exchange_model.py). Output buffers start out filled with a
sentinel word; entries past a row's live count hold in-range garbage that must not be used."""
import numpy as np
import pytest
import torch

import exchange_model as M

pytestmark = pytest.mark.gpu

C = 257
DEV = "cuda"
U = 600  # unique keys of a call
RUNS = {3: [C, C + 5, U - 2 * C - 5], 8: [0, 12, 0, 0, C, C + 5, U - 12 - 2 * C - 5, 0]}


def _hh():
    from parameter_server_amd.ops.native import hipops

    return hipops()


def _dev_words(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).to(DEV)


def _words(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _sentinel_f32(n):
    return _dev_words(np.full(n, M.SENTINEL, dtype=np.uint32)).view(torch.float32)


@pytest.fixture(scope="module")
def call():
    """About 2,000 positions over U unique 40-bit keys, one of them 64 times, localised on
    the host; seg_start carries a garbage tail past the unique count."""
    from parameter_server_amd.ops.localize import localize_torch

    rng = np.random.default_rng(31)
    uniq = rng.choice(1 << 40, U, replace=False)
    keys = np.concatenate([uniq, np.full(63, uniq[17]), rng.choice(uniq, 2000 - U - 63)])
    rng.shuffle(keys)
    loc = localize_torch(torch.from_numpy(keys.astype(np.int64)), 64)
    assert loc.uniq.numel() == U
    seg = np.concatenate([loc.seg_start.numpy(), [-5, 1 << 30, 7] * 7]).astype(np.int32)
    assert np.diff(seg[:U + 1]).max() >= 64
    return dict(nnz=keys.size, pos_s=loc.pos_s.numpy().astype(np.int32), seg_start=seg,
                local_col=loc.local_col.numpy().astype(np.int32))


@pytest.mark.parametrize("kw", [0, 1, 2])
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("G", [3, 8])
def test_pack_vals_rows_equal_model(call, G, k, kw):
    hh = _hh()
    rng = np.random.default_rng(G * 100 + k * 3 + kw)
    off = M.offsets(RUNS[G])
    assert off[-1] == U
    H = M.row_words(C, kw, k=k)
    vals = rng.standard_normal((call["nnz"], k)).astype(np.float32)
    blank = M.new_rows(G, H)
    send = _dev_words(blank)
    hh.kvv_pack_vals(torch.from_numpy(vals).to(DEV), k, torch.from_numpy(call["pos_s"]).to(DEV),
                     torch.from_numpy(call["seg_start"]).to(DEV),
                     torch.tensor([U], dtype=torch.int32, device=DEV),
                     torch.from_numpy(off).to(DEV), C, kw, H, send)
    want, s32, s64 = M.kvv_pack_vals(vals, k, call["pos_s"], call["seg_start"], off, C, kw, H, blank)
    got = _words(send).reshape(G, H)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{bad.shape[0]} words differ, first (row, word) {bad[0]}"
    # the model's float32 sums themselves: sequential sums of <= 64 addends
    absum = np.zeros((U, k))
    np.add.at(absum, call["local_col"], np.abs(vals.astype(np.float64)))
    assert (np.abs(s32 - s64) <= 64 * 2.0 ** -24 * absum).all()
    # word 0 only for a key-less row; keys, headers and dropped entries untouched
    assert (got[:, 0] == (want[:, 1] if kw == 0 else M.SENTINEL)).all()
    assert (got[:, 2:4 + C * kw] == M.SENTINEL).all()
    assert want[:, 1].tolist() == [min(r, C) for r in RUNS[G]]


def _push_rows(G, k, kw, rng, cap):
    """G received push rows [count | - | keys | C*k values] and the slots of their
    entries: slots shared between rows, distinct within a row, some missing (-1) or out of
    range; 5 % of the value components NaN marks; entries past the count hold in-range
    slots and finite values."""
    H = M.row_words(C, kw, k=k)
    counts = [C, 0, 100, 1, C - 1, 57, 200, 3][:G]
    recv = M.new_rows(G, H)
    vals = rng.standard_normal((G, C, k)).astype(np.float32)
    vals[rng.random((G, C, k)) < 0.05] = np.nan
    vals[:, :, 0][:, ::50] = np.nan
    slot = np.stack([rng.permutation(300)[:C] for _ in range(G)]).astype(np.int64)
    for s in range(G):
        recv[s, 0] = counts[s]
        live = slot[s, :counts[s]]
        live[3::11] = -1
        live[5::13] = cap + 2
        live[7::17] = np.iinfo(np.int64).min
        vals[s, counts[s]:] = np.where(np.isnan(vals[s, counts[s]:]), 1.0, vals[s, counts[s]:])
        recv[s, 4 + C * kw:4 + C * kw + C * k] = vals[s].reshape(-1).view(np.uint32)
    return H, counts, recv, vals, slot


@pytest.mark.parametrize("kw", [0, 1, 2])
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("G", [3, 8])
def test_apply_plus_and_assign(G, k, kw):
    hh = _hh()
    rng = np.random.default_rng(G * 100 + k * 3 + kw + 1)
    cap = 320
    H, counts, recv, vals, slot = _push_rows(G, k, kw, rng, cap)
    table0 = rng.standard_normal((cap, k)).astype(np.float32)
    d_recv, d_slot = _dev_words(recv), torch.from_numpy(slot.reshape(-1)).to(DEV)
    for op in (0, 1):
        table = torch.from_numpy(table0).to(DEV)
        hh.kvv_apply(d_recv, H, C, kw, d_slot, table, op)
        got = table.cpu().numpy()
        tot = table0.astype(np.float64)
        absum = np.abs(tot)
        last = table0.copy()
        touched = np.zeros((cap, k), dtype=bool)
        for s in range(G):  # source rank order
            for i in range(counts[s]):
                sl = slot[s, i]
                if not 0 <= sl < cap:
                    continue
                x = vals[s, i]
                ok = ~np.isnan(x)  # a NaN component carries no value
                tot[sl, ok] += x[ok].astype(np.float64)
                absum[sl, ok] += np.abs(x[ok])
                last[sl, ok] = x[ok]
                touched[sl] |= ok
        assert touched.any() and not touched.all() and not np.isnan(got).any()
        assert np.array_equal(got[~touched].view(np.uint32), table0[~touched].view(np.uint32))
        if op == 0:  # float atomics in any order: at most G roundings of partial sums
            assert (np.abs(got - tot) <= G * 2.0 ** -24 * absum).all()
            assert (got[touched] != table0[touched]).any()
        else:  # the highest source rank that carries the component wins, exactly
            assert np.array_equal(got.view(np.uint32), last.view(np.uint32))


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("G", [3, 8])
def test_serve_gathers_the_table_rows(G, k):
    hh = _hh()
    rng = np.random.default_rng(G * 100 + k)
    cap = 320
    H, counts, recv, _, slot = _push_rows(G, k, 1, rng, cap)
    table = rng.standard_normal((cap, k)).astype(np.float32)
    rec = _sentinel_f32(G * C * k)
    hh.kvv_serve(_dev_words(recv), H, C, torch.from_numpy(slot.reshape(-1)).to(DEV),
                 torch.from_numpy(table).to(DEV), rec)
    want = np.full((G, C, k), M.SENTINEL, dtype=np.uint32)
    for s in range(G):
        sl = slot[s, :counts[s]]
        ok = (sl >= 0) & (sl < cap)
        want[s, :counts[s]] = np.where(ok[:, None], table[np.where(ok, sl, 0)], np.float32(0)).view(
            np.uint32)
    assert np.array_equal(_words(rec).reshape(G, C, k), want)
    assert (want[0, :counts[0]][slot[0, :counts[0]] == -1] == 0).all()


def test_serve_w_gathers_the_slot_weights():
    """kv_serve_w: the same gather from the w field of a KVTable's 32-byte slots; header-only
    rows (H = 4), as the registered-key pull serves them."""
    from parameter_server_amd.ops.kv_table import KVTable

    hh = _hh()
    rng = np.random.default_rng(77)
    G, cap = 3, 1 << 10
    counts = [C, 0, 100]
    tb = KVTable(cap, DEV)
    keys = torch.from_numpy(rng.choice(1 << 40, 300, replace=False).astype(np.int64)).to(DEV)
    tslot, _ = tb.resolve(keys)
    w = rng.standard_normal(300).astype(np.float32)
    tb.set(tslot, w=torch.from_numpy(w).to(DEV))
    tslot = tslot.cpu().numpy()
    assert np.unique(tslot).size == 300 and tslot.min() >= 0
    pick = np.stack([rng.permutation(300)[:C] for _ in range(G)])
    slot = tslot[pick]
    miss = np.zeros((G, C), dtype=bool)
    miss[:, 3::11] = True
    slot[miss] = -1
    hdr = M.new_rows(G, 4)
    hdr[:, 0] = counts
    rec = _sentinel_f32(G * C)
    hh.kv_serve_w(_dev_words(hdr), 4, C, torch.from_numpy(slot.reshape(-1)).to(DEV), tb.slots, rec)
    want = np.full((G, C), M.SENTINEL, dtype=np.uint32)
    for s in range(G):
        n = counts[s]
        want[s, :n] = np.where(miss[s, :n], np.float32(0), w[pick[s, :n]]).view(np.uint32)
    assert np.array_equal(_words(rec).reshape(G, C), want)


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("G", [3, 8])
def test_unpack_scatters_records_to_request_order(call, G, k):
    hh = _hh()
    rng = np.random.default_rng(G * 100 + k + 2)
    off = M.offsets(RUNS[G])
    rec = rng.standard_normal((G, C, k)).astype(np.float32)
    rec[rec == 0] = 1.0
    lc = call["local_col"].copy()
    lc[::97] = -1  # no unique id
    lc[5::101] = U  # = off[G]
    lc[7::103] = U + 1000
    lc[11::107] = np.iinfo(np.int32).min
    nnz = lc.size
    out = _sentinel_f32(nnz * k + 8)
    hh.kvv_unpack(torch.from_numpy(rec).to(DEV), C, k, torch.from_numpy(off).to(DEV),
                  torch.from_numpy(lc).to(DEV), out)
    u = lc.astype(np.int64)
    valid = (u >= 0) & (u < U)
    p = M.owner_of(off, np.where(valid, u, 0))
    i = np.where(valid, u, 0) - off[p]
    kept = valid & (i < C)
    want = np.where(kept[:, None], rec[p, np.minimum(i, C - 1)], np.float32(0))
    got = _words(out)
    assert np.array_equal(got[:nnz * k].reshape(nnz, k), want.view(np.uint32))
    assert (got[nnz * k:] == M.SENTINEL).all()
    dropped = valid & ~kept
    assert dropped.sum() >= 5 and (~valid).sum() >= 40 and kept.sum() > 1500


def test_single_off_is_the_device_count():
    hh = _hh()
    off = torch.full((2,), -9, dtype=torch.int64, device=DEV)
    hh.kvv_single_off(torch.tensor([431, 99], dtype=torch.int32, device=DEV), off)
    assert off.tolist() == [0, 431]
