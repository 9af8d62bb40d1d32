"""The device path of the warm start -- kv_seed (kv_table.hip), the streaming
``SparseLRTrainer.load_model`` -- against the CPU reference path of the same call: the
smallest shapes at which the kernel can go wrong, streaming and deferred chunks,
continuation on the flat one-GPU step, growth on the device and the app."""
import numpy as np
import pytest
import torch

import warm_start_util as U
from parameter_server_amd.models import ModelScorer, SparseLRConfig, SparseLRTrainer
from parameter_server_amd.ops.keymix import mix, unmix
from parameter_server_amd.ops.kv_table import InitRule, KVTable, UpdateRule

pytestmark = pytest.mark.gpu
DEV = "cuda"
RULE = UpdateRule("ftrl", "decay", U.ALPHA, U.BETA, U.L1, U.L2)


def _i64(k: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(k.astype(np.uint64).view(np.int64).copy())


def _table_state(t: KVTable):
    """(mixed keys u64, w, z, n) of the occupied slots ordered by mixed key, numpy."""
    k, w, z, n = (x.cpu().numpy() for x in t.occupied())
    k = k.view(np.uint64)
    o = np.argsort(k)
    return k[o], w[o], z[o], n[o]


def _seed_both(raw, w, bits, lo, hi, cap, ordered, rule=RULE, n0=0.0, init=None):
    """The same ``KVTable.seed`` call on a GPU and on a CPU table; checks keys and w bit for
    bit, counts, n, and z against the float64 formula; returns (gpu table, counts)."""
    out = []
    for dev in (DEV, "cpu"):
        t = KVTable(cap, dev, init, key_range=(lo, hi) if ordered else None)
        stats = torch.zeros(64 * 16, dtype=torch.float64, device=dev)
        c = t.seed(raw, w, bits, lo, hi, rule, n0, stats=stats)
        t.check_ok()
        out.append((t, c, float(stats.view(-1, 16).sum(0)[0])))
    (tg, cg, ng), (tc, cc, nc) = out
    assert cg == cc, (cg, cc)
    assert ng == nc == cg["seeded"]
    kg, wg, zg, ngr = _table_state(tg)
    kc, wc, zc, ncr = _table_state(tc)
    assert np.array_equal(kg, kc) and kg.size == cg["seeded"]
    assert np.array_equal(wg.view(np.uint32), wc.view(np.uint32))
    z64, n_want = U.seed_state64(wg, rule.algo, rule.lr_type, n0, rule.alpha, rule.beta, rule.l1,
                                 rule.l2)
    assert np.array_equal(ngr, np.full(kg.size, n_want, dtype=np.float32))
    if rule.algo != "ftrl":
        assert not zg.any()
    elif kg.size:
        rel = np.abs(zg.astype(np.float64) - z64) / np.abs(z64)
        print("z max rel err", rel.max())
        assert rel.max() <= 1e-6
    return tg, cg


# --------------------------------------------- 1. the smallest shapes that can go wrong
@pytest.mark.parametrize("ordered", [True, False])
@pytest.mark.parametrize("bits", [20, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_seed_sizes(n, bits, ordered):
    k, w = U.entries(n, 10 + n, 0 if bits == 64 else 1 << 20)
    if bits == 64:
        assert n < 2 or (k >= np.uint64(1 << 63)).any()
    total = 1 << bits
    lo, hi = total // 4, total - total // 8  # (5/8 of the space is owned)
    if n >= 63:  # entries a foreign file may hold, and a key stored with more bits
        w[3], w[7], w[11] = 0.0, -0.0, np.nan
        if bits == 20:
            k[5] = (1 << 20) + 17
    _, c = _seed_both(_i64(k), torch.from_numpy(w), bits, lo, hi, 4096, ordered)
    assert sum(c.values()) == n and c["overwritten"] == 0
    if n >= 63:
        assert c["foreign"] > 0 and c["out_of_range"] == (bits == 20)
        assert 1 <= c["skipped"] <= 3


@pytest.mark.parametrize("ordered", [True, False])
def test_seed_64_slot_table_long_runs_and_wrap(ordered):
    """30 keys in 64 slots; with ordered homes 20 of them crowd the top of the range, so
    their probe runs pass slot 63 and wrap to slot 0."""
    bits = 20
    lo, hi = 1 << 18, 1 << 19
    rng = np.random.default_rng(3)
    top = hi - 1 - np.arange(20, dtype=np.int64) * 3
    rest = rng.choice(np.arange(lo, hi - 100), 10, replace=False)
    raw = unmix(torch.from_numpy(np.concatenate([top, rest]).astype(np.int64)), bits)
    w = torch.from_numpy(U.entries(30, 4, 1 << 20)[1])
    t, c = _seed_both(raw, w, bits, lo, hi, 64, ordered)
    assert c["seeded"] == 30 and t.capacity == 64
    slot, got = t.resolve(mix(raw.to(DEV), bits), insert=False)
    assert (slot >= 0).all() and torch.equal(got.cpu(), w)
    if ordered:  # the crowd's home is the last slot: its run wrapped
        assert int(slot.min()) == 0 and int(slot.max()) == 63
    # seeding the same keys again overwrites them: no new slot
    c2 = t.seed(raw, -w, bits, lo, hi, RULE)
    assert c2["seeded"] == 0 and c2["overwritten"] == 30 and t.census()[0] == 30
    # 40 more keys do not fit: the error word, no fault (trip bound mask + 1)
    more = unmix(torch.from_numpy(rng.choice(np.arange(lo, hi - 100), 40, replace=False)), bits)
    t.seed(more, torch.ones(40), bits, lo, hi, RULE)
    with pytest.raises(RuntimeError, match="KVTable full"):
        t.check_ok()
    assert t.census()[0] == 64


def test_seed_owned_range_edges():
    bits = 20
    lo, hi = 300_000, 700_000
    raw = unmix(torch.tensor([lo, hi - 1, hi, lo - 1], dtype=torch.int64), bits)
    t, c = _seed_both(raw, torch.tensor([1.0, -2.0, 3.0, 4.0]), bits, lo, hi, 64, True)
    assert c == dict(seeded=2, overwritten=0, foreign=2, out_of_range=0, skipped=0)
    k, w, _, _ = _table_state(t)
    assert k.tolist() == [lo, hi - 1] and w.tolist() == [1.0, -2.0]


@pytest.mark.parametrize("ordered", [True, False])
def test_seed_publishes_over_a_nonzero_init(ordered):
    """A constant non-zero init rule: a later resolve and the fused scorer read the seeded
    weight, not the init value (kSlotInit is set)."""
    bits, n = 20, 300
    k, w = U.entries(n, 21, 1 << 20)
    raw = _i64(k)
    t, c = _seed_both(raw, torch.from_numpy(w), bits, 0, 1 << 20, 1024, ordered,
                      init=InitRule("constant", 0.5))
    assert c["seeded"] == n
    h = mix(raw.to(DEV), bits)
    slot, got = t.resolve(h, insert=True)
    assert torch.equal(got.cpu(), torch.from_numpy(w)) and t.census()[0] == n
    margins = ModelScorer.from_table(t, bits).predict(raw.to(DEV), width=1)
    assert torch.equal(margins.cpu(), torch.from_numpy(w))
    fresh = torch.tensor([int(np.setdiff1d(np.arange(1 << 20), k)[0])], device=DEV)
    assert t.resolve(mix(fresh, bits), insert=True)[1].item() == 0.5


@pytest.mark.parametrize("algo,lr_type,n0", [("adagrad", "decay", 3.5), ("sgd", "constant", 0.0),
                                             ("ftrl", "constant", 3.5)])
def test_seed_other_rules(algo, lr_type, n0):
    k, w = U.entries(500, 22, 1 << 20)
    rule = UpdateRule(algo, lr_type, U.ALPHA, U.BETA, U.L1, U.L2)
    t, c = _seed_both(_i64(k), torch.from_numpy(w), 20, 0, 1 << 20, 2048, True, rule, n0)
    assert c["seeded"] == 500


# -------------------------------------------------------------------------- 2. streaming
def _trainer(num_features, **kw):
    kw.setdefault("minibatch", 1024)
    kw.setdefault("max_nnz_per_example", 16)
    return SparseLRTrainer(SparseLRConfig(num_features=num_features, **kw), device=DEV)


def _same_state(a, b):
    for x, y in zip(U.sorted_state(a), U.sorted_state(b)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_streaming_matches_host_load(tmp_path):
    n = 200_000
    k, w = U.entries(n, 30, 0)
    U.write_model(str(tmp_path / "m_S0"), k, w)
    pat = str(tmp_path / "m_S.*")
    host = _trainer(0, table_capacity=1 << 19)
    rh = host.load_model(pat, text_io="host")
    assert rh["entries"] == rh["seeded"] == n and rh["deferred_chunks"] == 0
    for kw in (dict(chunk_bytes=4096), dict()):
        tr = _trainer(0, table_capacity=1 << 19)
        r = tr.load_model(pat, text_io="device", **kw)
        assert r == rh
        _same_state(tr, host)
        assert tr.progress()["nnz_w"] == n


def test_streaming_defers_only_the_odd_chunk(tmp_path):
    n = 20_000
    k, w = U.entries(n, 31, 1 << 20)
    U.write_model(str(tmp_path / "m_S0"), k, w)
    with open(tmp_path / "m_S0") as f:
        lines = f.readlines()
    free = int(np.setdiff1d(np.arange(1 << 20), k)[0])
    lines[n // 2:n // 2] = [f"{free}\tnan\n", "\n"]
    with open(tmp_path / "m_S0", "w") as f:
        f.writelines(lines)
    pat = str(tmp_path / "m_S.*")
    host = _trainer(1 << 20, table_capacity=1 << 16)
    rh = host.load_model(pat, text_io="host")
    tr = _trainer(1 << 20, table_capacity=1 << 16)
    r = tr.load_model(pat, chunk_bytes=4096)
    assert r["deferred_chunks"] == 1 and rh["deferred_chunks"] == 0
    assert r["entries"] == rh["entries"] == n + 1 and r["seeded"] == rh["seeded"] == n
    _same_state(tr, host)


def test_repeated_key_on_the_device_path(tmp_path):
    k, w = U.entries(5000, 32, 1 << 20)
    U.write_model(str(tmp_path / "m_S0"), k, w)
    with open(tmp_path / "m_S0", "a") as f:
        f.write(f"{int(k[0])}\t0.75\n")
    tr = _trainer(1 << 20, table_capacity=1 << 14)
    r = tr.load_model(str(tmp_path / "m_S.*"), chunk_bytes=8192)
    assert r["deferred_chunks"] >= 1 and r["entries"] == r["seeded"] == 5000
    sk, sw, _, _ = U.sorted_state(tr)
    assert sw[np.searchsorted(sk, k[0])] == 0.75 and tr.progress()["nnz_w"] == 5000


def test_out_of_range_and_full_table(tmp_path):
    k, w = U.entries(3000, 33, 1 << 20)
    U.write_model(str(tmp_path / "m_S0"), k, w)
    with pytest.raises(ValueError, match="num_features"):
        _trainer(1 << 16, table_capacity=1 << 13).load_model(str(tmp_path / "m_S.*"))
    with pytest.raises(RuntimeError, match="KVTable full"):
        _trainer(1 << 20, table_capacity=1024).load_model(str(tmp_path / "m_S.*"))


# ------------------------------------------------------------- 3. continuation (flat step)
def test_continuation_flat_step(tmp_path):
    N, B, width = 1 << 20, 1024, 16
    k, w = U.entries(20_000, 34, N)
    o = np.argsort(k)
    k, w = k[o], w[o]
    U.write_model(str(tmp_path / "m_S0"), k, w)
    pat = str(tmp_path / "m_S.*")
    batches = U.minibatches(5, B, width, N, seed=35, device=DEV)
    # (half of every minibatch's keys are stored ones, so the first pull reads many)
    stored = torch.from_numpy(k.astype(np.int64)).to(DEV)
    g = torch.Generator().manual_seed(36)
    for kk, _ in batches:
        pick = torch.randint(0, stored.numel(), (kk.numel() // 2,), generator=g).to(DEV)
        kk[::2] = stored[pick]
    tr = _trainer(N, minibatch=B, max_nnz_per_example=width, table_capacity=1 << 18)
    assert tr.localize_mode == "tpf"
    tr.load_model(pat, n0=0.5)
    sc = ModelScorer.from_text(pat, tr.bits, DEV)
    sc.score(batches[0][0], batches[0][1], width=width, margins=False)
    want_loss = sc.result()["loss"]
    tr.step(batches[0][0], batches[0][1], width=width)
    first = tr.progress()["loss"]
    print("first loss", first, "scorer", want_loss)
    assert abs(first - want_loss) <= 1e-6 * abs(want_loss)
    assert want_loss > 2.0  # (far from ln 2: the pull did see the stored weights)
    for kk, y in batches[1:]:
        tr.step(kk, y, width=width)
    ak, aw, _, _ = U.sorted_state(tr)
    z64, n_seed = U.seed_state64(w, "ftrl", "decay", 0.5)
    allk, W, _ = U.reference_steps(k, w, z64, n_seed, batches, width, "ftrl", "decay")
    assert np.array_equal(ak.view(np.int64), allk.numpy())
    torch.testing.assert_close(torch.from_numpy(aw), W, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------- 4. growth on the device
def test_growth_on_the_device(tmp_path):
    n = 50_000
    k, w = U.entries(n, 37, 0)
    o = np.argsort(k)
    U.write_model(str(tmp_path / "m_S0"), k, w)
    tr = _trainer(0, table_capacity=1024, table_growth=True)
    r = tr.load_model(str(tmp_path / "m_S.*"), chunk_bytes=1 << 16)
    assert r["seeded"] == n and r["table_capacity"] == tr.table.capacity >= 2 * n
    sk, sw, _, _ = U.sorted_state(tr)
    assert np.array_equal(sk, k[o]) and np.array_equal(sw, w[o])
    assert tr.progress()["table_grown"] > 0


# -------------------------------------------------------------------------------- 5. app
def test_app_parser_gpu_warm_start(tmp_path):
    _, warm_cpu, model = U.cold_then_warm(tmp_path, "cpu")
    conf = U.app_conf(tmp_path / "gpu.conf", tmp_path / "data", tmp_path / "gpu" / "m",
                      model_in=model)
    warm_gpu = U.run_app(conf, DEV, parser="gpu")
    assert warm_gpu["parser"] == "gpu"
    assert warm_gpu["warm_start_entries"] == warm_cpu["warm_start_entries"] > 50
    assert warm_gpu["warm_start_seeded"] == warm_cpu["warm_start_seeded"]
    ak, aw, _, _ = U.app_table(warm_gpu)
    bk, bw, _, _ = U.app_table(warm_cpu)
    assert torch.equal(ak, bk)
    torch.testing.assert_close(aw, bw, rtol=1e-4, atol=1e-5)
