"""Growing the KV table on the device (kv_rehash, csrc/hip/kv_table.hip): the kernel on
its own, the 1-GPU trainer on every route from a 1024-slot table against a table sized
large from the start, the emulated 2-peer exchanges, and the file-fed app."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
from parameter_server_amd.ops.keymix import unmix
from parameter_server_amd.ops.kv_table import InitRule, KVTable
from test_table_grow import (HOMES, SIZES, check_grown, fill_table, keys_with_home,
                             random_keys)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------- kv_rehash
@pytest.mark.parametrize("home", list(HOMES))
@pytest.mark.parametrize("fill", ["one", "half", "full"])
@pytest.mark.parametrize("cap,new", SIZES)
def test_rehash_keeps_every_slot(cap, new, fill, home):
    """Every key reachable from its new home, its 32-byte record unchanged (NaN payloads,
    -0.0, the SGD step count, both flag bits), the returned count equal to the census. (Slot
    positions are free: the CAS order is; the records are compared by key.)"""
    t = KVTable(cap, DEV, InitRule("constant", 0.25), key_range=HOMES[home])
    n = {"one": 1, "half": cap // 2, "full": cap}[fill]
    keys = random_keys(t, n + 16, seed=cap + n)
    keys, absent = keys[:n], keys[n:]
    rec = fill_table(t, keys)
    before = t.census()
    obj, init, err = t, t.init, t._err
    moved = t.grow(new)
    assert t is obj and t.capacity == new and tuple(t.slots.shape) == (new, 4)
    assert t.init is init and t._err is err
    check_grown(t, keys, rec, absent, before, moved)
    t.check_ok()
    # the grown table keeps working: a new key initialises by the carried rule
    slot, w = t.resolve(absent[:1].to(DEV), insert=True)
    assert int(slot[0]) >= 0 and float(w[0]) == 0.25 and t.census()[0] == n + 1


@pytest.mark.parametrize("home", list(HOMES))
def test_rehash_one_long_chain_that_wraps(home):
    """64 keys of ONE home slot in the completely full 64-slot table: the chain wraps past
    the last slot before the growth (home 40) and after it (home = the new table's last
    slot), where 64 lanes contend for the same run of slots."""
    for new, h_new in ((128, None), (256, 255)):
        t = KVTable(64, DEV, key_range=HOMES[home])
        keys = (keys_with_home(t, 40, 64) if h_new is None
                else keys_with_home(t, h_new, 64, cap=new))
        rec = fill_table(t, keys)
        before = t.census()
        moved = t.grow(new)
        absent = random_keys(t, 8, seed=5)
        absent = absent[~torch.isin(absent, keys)]
        check_grown(t, keys, rec, absent, before, moved)
        t.check_ok()


def test_rehash_many_blocks_matches_cpu_twin():
    """More slots than one grid pass covers (2^20 > 2048 blocks x 256), hashed and ordered:
    the same records per key as the CPU twin."""
    keys = torch.randperm(1 << 24, generator=torch.Generator().manual_seed(9))[:300000]
    absent = torch.arange(1 << 24, (1 << 24) + 64)
    for kr in (None, (0, 1 << 25)):
        g, c = KVTable(1 << 20, DEV, key_range=kr), KVTable(1 << 20, "cpu", key_range=kr)
        rec = fill_table(c, keys)
        assert torch.equal(fill_table(g, keys), rec)
        before = c.census()
        assert g.census() == before
        assert g.grow(1 << 21) == c.grow(1 << 21) == 300000
        check_grown(g, keys, rec, absent, before, 300000)
        a, b = g.slots.cpu(), c.slots
        a, b = a[a[:, 0] != -1], b[b[:, 0] != -1]
        assert torch.equal(a[torch.argsort(a[:, 0])], b[torch.argsort(b[:, 0])])


# ------------------------------------------------------------------- trainer, one GPU
B, WIDTH, STEPS, NFEAT, SPACE = 512, 10, 30, 20000, 1 << 20
RULES = {"ftrl": dict(alpha=0.05, beta=1.0, l1=0.5, l2=0.1),
         "adagrad": dict(alpha=0.05, beta=1.0, l1=0.5, l2=0.1),
         "sgd": dict(alpha=0.002, beta=1.0, l1=0.05, l2=0.1)}


@functools.lru_cache(maxsize=None)
def _batches():
    """30 minibatches of 512 rows x 10 binary features over 20,000 feature ids (a fixed
    random subset of the 2^20 hashed space), labels from a hidden sparse model; values
    for the valued route."""
    g = torch.Generator().manual_seed(1234)
    ids = torch.randperm(SPACE, generator=g)[:NFEAT]
    hidden = torch.randn(NFEAT, generator=g) * (torch.rand(NFEAT, generator=g) < 0.3)
    out = []
    for _ in range(STEPS):
        f = torch.randint(0, NFEAT, (B, WIDTH), generator=g)
        y = torch.where(hidden[f].sum(1) + 0.3 * torch.randn(B, generator=g) > 0, 1.0, -1.0)
        v = 0.5 + torch.rand(B * WIDTH, generator=g)
        out.append((ids[f].reshape(-1).to(DEV), y.to(DEV), v.to(DEV)))
    return out


def _run(tr, route, batches=None):
    bs = batches or _batches()
    if route == "ahead":  # every pull but the first issued inside the previous step
        loc = tr.localize(bs[0][0], buf=0)
        for t, (k, y, _) in enumerate(bs):
            nxt = tr.localize(bs[t + 1][0], buf=(t + 1) % 2) if t + 1 < len(bs) else None
            tr.step(k, y, width=WIDTH, loc=loc, next_loc=nxt)
            loc = nxt
        return
    for k, y, v in bs:
        if route == "flat":
            tr.step(k, y, width=WIDTH)
        elif route == "flat_csr":
            tr.step(k, y, width=WIDTH, vals=v)
        else:  # the generic step on a compact localisation (float atomics)
            tr.step(k, y, width=WIDTH, prefetch=lambda: None)


def _state(tr):
    keys, w, z, n = tr.table.occupied()
    raw = unmix(keys, tr.bits)
    o = torch.argsort(raw)
    return raw[o].cpu(), w[o].cpu(), z[o].cpu(), n[o].cpu()


def _trainer(algo, cap, growth, **kw):
    cfg = SparseLRConfig(num_features=SPACE, minibatch=B, max_nnz_per_example=WIDTH, algo=algo,
                         table_capacity=cap, table_growth=growth, **RULES[algo], **kw)
    return SparseLRTrainer(cfg, device=DEV)


@pytest.mark.parametrize("route", ["flat", "flat_csr", "ahead", "compact"])
@pytest.mark.parametrize("algo", ["ftrl", "adagrad", "sgd"])
def test_trainer_grows_from_1024_slots_like_a_large_table(algo, route):
    large = _trainer(algo, 65536, False)
    _run(large, route)
    pl = large.progress()
    tr = _trainer(algo, 1024, True)
    assert tr.localize_mode == "tpf"
    _run(tr, route)
    pg = tr.progress()  # (check_ok inside: the full flag never fired)
    assert pg["table_grown"] >= 3 and pg["table_capacity"] == tr.table.capacity >= 65536
    assert (pl["table_grown"], pl["table_capacity"]) == (0, 65536)
    assert tr.table.census()[0] <= tr.cfg.table_grow_check * tr.table.capacity
    if route != "compact":
        assert tr._compact is None  # (the flat layout ran every step)
    a, b = _state(large), _state(tr)
    assert torch.equal(a[0], b[0]) and a[0].numel() > 15000
    assert int((a[1] != 0).sum()) > 100  # trained weights, not only zeros
    if route == "compact":
        torch.testing.assert_close(b[1], a[1], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(b[2], a[2], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(b[3], a[3], rtol=1e-4, atol=1e-5)
    else:
        # fixed-point sums, and a key's update does not depend on where its slot lies
        for x, y in zip(a[1:], b[1:]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert abs(pl["loss"] - pg["loss"]) < 1e-6


def test_small_table_without_growth_is_full():
    tr = _trainer("ftrl", 1024, False)
    with pytest.raises(RuntimeError, match="KVTable full"):
        _run(tr, "flat", _batches()[:3])
        tr.progress()


def test_refused_growth_warns_once_and_then_fails_like_a_fixed_table():
    tr = _trainer("ftrl", 1024, True, max_table_bytes=32 * 2048)
    with pytest.warns(RuntimeWarning, match="max_table_bytes") as rec:
        with pytest.raises(RuntimeError, match="KVTable full"):
            _run(tr, "flat", _batches()[:3])
            tr.progress()
    assert len([w for w in rec if "table growth refused" in str(w.message)]) == 1
    assert tr.table.capacity == 1024


def test_scorer_taken_before_a_growth_scores_the_grown_table():
    tr = _trainer("ftrl", 1024, True)
    bs = _batches()
    _run(tr, "flat", bs[:2])
    sc = tr.scorer()
    cap = tr.table.capacity
    _run(tr, "flat", bs[2:])
    tr.flush()
    assert tr.table.capacity > cap and sc.table is tr.table
    k = bs[0][0]
    m = sc.predict(k, width=WIDTH)
    keys, w, _, _ = tr.table.occupied()
    from parameter_server_amd.models.scorer import ModelScorer

    ref = ModelScorer.from_pairs(keys, w, tr.bits, DEV).predict(k, width=WIDTH)
    assert float(m.abs().max()) > 0
    torch.testing.assert_close(m, ref, rtol=1e-6, atol=1e-6)


def test_state_dict_of_a_grown_trainer_loads_into_a_small_growing_one():
    src = _trainer("ftrl", 1024, True)
    _run(src, "flat")
    want = _state(src)
    tr = _trainer("ftrl", 1024, True)
    tr.load_state_dict(src.state_dict())
    assert tr.progress()["table_grown"] == 1
    assert tr.table.census()[0] <= tr.cfg.table_grow_at * tr.table.capacity
    got = _state(tr)
    for x, y in zip(want, got):
        assert torch.equal(x, y)
    _run(tr, "flat", _batches()[:2])  # and it trains on (its launch lists are fresh)
    tr.progress()
    small = _trainer("ftrl", 1024, False)
    with pytest.raises(RuntimeError, match="KVTable full"):
        small.load_state_dict(src.state_dict())


def test_prefill_counts_towards_the_bound():
    tr = _trainer("ftrl", 1024, True)
    assert tr.prefill(5000, chunk=1000) > 4900
    tr.table.check_ok()
    assert tr.table.capacity >= 8192 and tr._growth.grown >= 2


# --------------------------------------------------------------- two emulated peers
def _peer_cfg(plane, cap, growth):
    kw = dict(num_features=SPACE, minibatch=B, max_nnz_per_example=WIDTH, table_capacity=cap,
              table_growth=growth, **RULES["ftrl"])
    if plane == "merged":
        kw.update(consistency="ssp:2", exchange_merge="on")
    return SparseLRConfig(**kw)


def _peers_grow_like_large(plane, make_comm):
    outs = []
    for cap, growth in ((65536, False), (1024, True)):
        tr = SparseLRTrainer(_peer_cfg(plane, cap, growth), make_comm(), DEV)
        assert tr.padded and tr.merged == (plane == "merged")
        _run(tr, "flat", _batches()[:12])
        outs.append((tr.progress(), _state(tr), tr))
    (pl, a, _), (pg, b, tr) = outs
    assert pg["table_grown"] >= 2 and tr.table.capacity > 1024
    assert torch.equal(a[0], b[0]) and a[0].numel() > 15000
    torch.testing.assert_close(b[1], a[1], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(b[2], a[2], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(b[3], a[3], rtol=1e-4, atol=1e-4)
    assert abs(pl["loss"] - pg["loss"]) < 1e-4
    return float((a[1] - b[1]).abs().max())


@pytest.mark.parametrize("plane", ["padded", "merged"])
def test_two_emulated_peers_grow_like_a_large_table(plane):
    from parameter_server_amd.parallel.comm import LoopbackComm

    _peers_grow_like_large(plane, lambda: LoopbackComm(2, DEV))


def _nccl_loopback_main():
    """(a fresh process: a 1-rank RCCL group carries the emulated exchanges)"""
    from parameter_server_amd.parallel.comm import nccl_loopback

    dev = torch.device("cuda", 0)
    out = {p: _peers_grow_like_large(p, lambda: nccl_loopback(2, dev))
           for p in ("padded", "merged")}
    print(json.dumps(out))


def test_two_peers_over_the_rccl_loopback_grow_like_a_large_table():
    code = ("import sys; sys.path.insert(0, 'tests'); import test_table_grow_gpu as t; "
            "t._nccl_loopback_main()")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert set(out) == {"padded", "merged"}


# ------------------------------------------------------------------------------- app
def _write_libsvm(d, binary_width, nfiles=3, rows=600, nkeys=6000, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 1, nkeys) * (rng.random(nkeys) < 0.2)
    os.makedirs(d, exist_ok=True)
    for p in range(nfiles):
        with open(os.path.join(d, f"part-{p}"), "w") as f:
            for _ in range(rows):
                if binary_width:
                    k = np.sort(rng.choice(np.arange(1, nkeys), binary_width, replace=False))
                    y = 1 if w[k].sum() + 0.2 * rng.normal() > 0 else -1
                    f.write(f"{y} " + " ".join(f"{a}:1" for a in k) + "\n")
                    continue
                k = np.unique(rng.integers(1, nkeys, size=int(rng.integers(5, 40))))
                v = rng.random(k.size)
                y = 1 if (w[k] * v).sum() + 0.2 * rng.normal() > 0 else -1
                f.write(f"{y} " + " ".join(f"{a}:{b:.4f}" for a, b in zip(k, v)) + "\n")


@pytest.mark.parametrize("binary_width", [12, 0])
def test_app_grows_and_writes_the_model_of_a_large_table(tmp_path, binary_width):
    """``-table_capacity 1024 -table_growth on`` against ``-table_capacity 65536``: the same
    model file -- byte for byte on the flat route (one width, binary features), within the
    tolerances of test_app_parser_gpu_matches_parser_cpu for valued variable-width rows."""
    from parameter_server_amd.app.gpu import _flags, run_async_sgd
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    data = tmp_path / "data"
    _write_libsvm(str(data), binary_width)
    texts, res = {}, {}
    for name, extra in (("large", ["-table_capacity", "65536"]),
                        ("grown", ["-table_capacity", "1024", "-table_growth", "on"])):
        model = tmp_path / f"model_{name}" / "m"
        conf = tmp_path / f"{name}.conf"
        conf.write_text(f"""linear_method {{
training_data {{ format: TEXT text: LIBSVM file: "{data}/part.*" }}
model_output {{ format: TEXT file: "{model}" }}
loss {{ type: LOGIT }}
penalty {{ type: L1 lambda: 0.05 lambda: 0.01 }}
learning_rate {{ type: DECAY alpha: 0.5 beta: 1 }}
async_sgd {{ algo: FTRL minibatch: 200 num_data_pass: 1 max_delay: 0 report_interval: 1 }}
}}""")
        flags = _flags(["-app_file", str(conf), "-num_features", str(1 << 20), "-num_threads", "2",
                        "-device", "cuda", "-quiet", "-data_cache", "off",
                        "-max_nnz_per_example", "40"] + extra)
        dev = torch.device("cuda")
        r = res[name] = run_async_sgd(load_app_config(str(conf)).linear_method, LocalComm(dev),
                                      dev, flags)
        assert r["examples"] == 1800 and r["steps"] == 9
        with open(r["model"], "rb") as f:
            texts[name] = f.read()
    assert (res["large"]["table_grown"], res["large"]["table_capacity"]) == (0, 65536)
    assert res["grown"]["table_grown"] >= 1
    assert res["grown"]["table_capacity"] == res["grown"]["trainer"].table.capacity > 1024
    if binary_width:
        assert texts["grown"] == texts["large"] and len(texts["large"]) > 500
        return

    def model(t):
        return {int(k): float(w) for k, w in (ln.split("\t") for ln in t.decode().splitlines())}

    g, c = model(texts["grown"]), model(texts["large"])
    assert set(g) == set(c) and len(g) > 50
    keys = sorted(g)
    np.testing.assert_allclose([g[k] for k in keys], [c[k] for k in keys], rtol=1e-4, atol=1e-5)
