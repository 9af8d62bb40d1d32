"""Growing the KV table instead of failing when it fills, on the CPU: ``KVTable.grow``
(the kv_rehash twin in csrc/core/cpu_kernels.cc), the host-side growth policy
(models/sparse_lr_growth.py) on a stub table, and two gloo ranks on the padded and merged
exchanges against a run whose table was sized large from the start."""
import os
import socket
import warnings

import pytest
import torch
import torch.multiprocessing as mp

from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
from parameter_server_amd.models.sparse_lr_growth import GrowthPolicy
from parameter_server_amd.ops.kv_table import InitRule, KVTable
from parameter_server_amd.ops.synthetic import criteo_batch

U64 = (1 << 64) - 1


def _i64(x: int) -> int:
    return x - (1 << 64) if x >= (1 << 63) else x


def fill_table(t: KVTable, keys: torch.Tensor, seed: int = 0):
    """Insert ``keys`` and give every slot a payload of awkward bit patterns: w / z cycle
    through NaN payloads, -0.0, denormals and infinities, n / acc are random bits, cnt is a
    step count, flags take all four values of the touched and published-init bits.
    Returns the [n, 4] int64 records in the order of ``keys``."""
    slot, _ = t.resolve(keys.to(t.device), insert=True, with_w=False)
    if t.gpu:
        t.check_ok()
    assert bool((slot >= 0).all())
    n = keys.numel()
    g = torch.Generator().manual_seed(seed)
    special = torch.tensor([0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0x00000001,
                            0x3F800000, 0x7FA00000, 0xFF800000], dtype=torch.int64)
    rnd = lambda: torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64)  # noqa: E731
    i = torch.arange(n)
    w, z = special[i % 8], special[(i // 8 + 3) % 8]
    cnt, flags = (i * 2654435761) % (1 << 32), i % 4
    rec = torch.stack([keys.cpu(), w | (z << 32), rnd() | (rnd() << 32), cnt | (flags << 32)], 1)
    t.slots[slot] = rec.to(t.device)
    return rec


def keys_with_home(t: KVTable, home: int, n: int, cap: int | None = None) -> torch.Tensor:
    """``n`` distinct keys whose home slot in a table of ``cap`` slots (default: the
    table's) is ``home``: one long probe chain. Ordered homes: consecutive keys of the slice
    of the range that maps there; hashed homes: searched."""
    from parameter_server_amd.ops.native import core

    cap = cap or t.capacity
    lg = cap.bit_length() - 1
    out = []
    if t.home_m:
        # home = ((k - base) * m) >> (64 - lg): the first key of home h is ceil(h * 2^(64-lg) / m)
        k = t.home_base + -(-(home << (64 - lg)) // t.home_m)
        while len(out) < n:
            assert (((k - t.home_base) * t.home_m) & U64) >> (64 - lg) == home, "range too narrow"
            out.append(_i64(k))
            k += 1
    else:
        k = 1
        while len(out) < n:
            if core().fmix64(k) & (cap - 1) == home:
                out.append(k)
            k += 1
    return torch.tensor(out, dtype=torch.int64)


def random_keys(t: KVTable, n: int, seed: int) -> torch.Tensor:
    """``n`` distinct keys of the table's key range (any 62-bit key for hashed homes)."""
    lo, hi = t.key_range if t.key_range is not None else (0, 1 << 62)
    g = torch.Generator().manual_seed(seed)
    span = hi - lo
    ks = set()
    while len(ks) < n:
        r = torch.randint(0, 1 << 62, (2 * n,), generator=g, dtype=torch.int64).tolist()
        ks.update(_i64(lo + x % span) for x in r)
    return torch.tensor(sorted(ks)[:n], dtype=torch.int64)[torch.randperm(n, generator=g)]


def check_grown(t: KVTable, keys: torch.Tensor, rec: torch.Tensor, absent: torch.Tensor,
                census_before, moved: int):
    """After ``t.grow``: every key reachable, absent keys absent, records unchanged as raw
    32-byte slots sorted by key, census unchanged and equal to the returned count."""
    dev = t.device
    slot, _ = t.resolve(keys.to(dev), insert=False, with_w=False)
    assert bool((slot >= 0).all()), "a key is not reachable from its new home"
    assert torch.equal(t.slots[slot].cpu(), rec)
    miss, _ = t.resolve(absent.to(dev), insert=False, with_w=False)
    assert bool((miss == -1).all())
    sl = t.slots.cpu()
    occ = sl[sl[:, 0] != -1]
    assert torch.equal(occ[torch.argsort(occ[:, 0])], rec[torch.argsort(rec[:, 0])])
    assert t.census() == census_before
    assert moved == census_before[0] == keys.numel() == t.num_inserted


HOMES = {"hashed": None, "ordered": (0, 1 << 40), "narrow": (123456789, 123456789 + 100000)}
SIZES = [(64, 128), (64, 1024), (4096, 8192)]


@pytest.mark.parametrize("home", list(HOMES))
@pytest.mark.parametrize("fill", ["one", "half", "full"])
@pytest.mark.parametrize("cap,new", SIZES)
def test_grow_keeps_every_slot_cpu(cap, new, fill, home):
    t = KVTable(cap, "cpu", InitRule("constant", 0.25), key_range=HOMES[home])
    n = {"one": 1, "half": cap // 2, "full": cap}[fill]
    keys = random_keys(t, n + 16, seed=cap + n)
    keys, absent = keys[:n], keys[n:]
    rec = fill_table(t, keys)
    before = t.census()
    obj, init = t, t.init
    moved = t.grow(new)
    assert t is obj and t.capacity == new and tuple(t.slots.shape) == (new, 4) and t.init is init
    check_grown(t, keys, rec, absent, before, moved)


@pytest.mark.parametrize("home", list(HOMES))
def test_grow_one_long_chain_that_wraps_cpu(home):
    """64 keys of ONE home slot fill the 64-slot table: the chain wraps past the last slot,
    before the growth (home 40) and after it (the last slot of the new table)."""
    for new, h_new in ((128, None), (256, 255)):
        t = KVTable(64, "cpu", key_range=HOMES[home])
        keys = (keys_with_home(t, 40, 64) if h_new is None
                else keys_with_home(t, h_new, 64, cap=new))
        rec = fill_table(t, keys)
        before = t.census()
        moved = t.grow(new)
        absent = random_keys(t, 8, seed=5)
        absent = absent[~torch.isin(absent, keys)]
        check_grown(t, keys, rec, absent, before, moved)


def test_grow_rejects_shrinking_and_same_capacity_is_a_noop():
    t = KVTable(256)
    keys = random_keys(t, 100, seed=1)
    fill_table(t, keys)
    slots = t.slots
    with pytest.raises(ValueError, match="below the current"):
        t.grow(128)
    assert t.grow(256) == 100 and t.slots is slots
    assert t.grow(200) == 100 and t.slots is slots  # (rounds up to the current 256)


def test_remap_slots_follows_the_keys():
    t = KVTable(64)
    keys = random_keys(t, 40, seed=2)
    slot, _ = t.resolve(keys)
    old = t.slots
    t.grow(512)
    idx = torch.cat([slot, torch.tensor([-1, -1])])
    new = t.remap_slots(old, idx)
    want, _ = t.resolve(keys, insert=False)
    assert torch.equal(new[:-2], want) and new[-2:].tolist() == [-1, -1]


# ----------------------------------------------------------------------- the policy
class StubTable:
    """capacity / census / grow of a KVTable, over a Python set; full raises like one."""

    def __init__(self, cap):
        self.capacity, self.keys, self.grows = cap, set(), []

    def census(self):
        return len(self.keys), 0

    def grow(self, cap):
        assert cap > self.capacity and cap & (cap - 1) == 0
        self.grows.append((self.capacity, cap, len(self.keys)))
        self.capacity = cap
        return len(self.keys)

    def insert(self, ks):
        self.keys.update(ks)
        if len(self.keys) > self.capacity:
            raise RuntimeError("KVTable full: increase capacity")


def test_policy_bound_arithmetic():
    tb = StubTable(1024)
    p = GrowthPolicy(tb, check=0.75, at=0.5)
    for i in range(7):  # 7 x 100 <= 768: the bound only adds, nothing is counted
        p.admit(100)
        tb.insert(range(i * 60, i * 60 + 60))  # (40 of each 100 were seen before)
    assert (p.bound, p.checks, p.grown) == (700, 0, 0)
    p.admit(100)  # 800 > 768: exact count 420 <= 512 and 520 <= 768: no growth
    assert (p.bound, p.checks, p.grown, tb.capacity) == (420 + 100, 1, 0, 1024)
    tb.insert(range(420, 520))
    p.admit(300)  # 820 > 768: count 520 > 512: 2048 -> 520 > 512 = at / 2 of it -> 4096
    assert (p.checks, p.grown, tb.capacity, p.bound) == (2, 1, 4096, 520 + 300)
    assert tb.grows == [(1024, 4096, 520)]


def test_policy_sizes_for_the_incoming_keys_too():
    tb = StubTable(1024)
    p = GrowthPolicy(tb)
    p.admit(5000)  # an empty table, but one minibatch alone would overfill it
    assert tb.capacity == 8192 and 5000 <= 0.75 * 8192 and p.bound == 5000
    assert p.target(0, 0) == 8192 and p.target(4097, 0) == 32768 and p.target(4096, 2048) == 8192
    assert p.target(4096, 2049) == 16384


@pytest.mark.parametrize("batch,universe", [(37, 3000), (300, 20000), (4608, 20000)])
def test_policy_never_passes_check_and_spaces_its_checks(batch, universe):
    g = torch.Generator().manual_seed(batch)
    tb = StubTable(1024)
    p = GrowthPolicy(tb, check=0.75, at=0.5)
    since, last_cap = 0, None
    for _ in range(400):
        ks = torch.randint(0, universe, (batch,), generator=g).tolist()
        checks = p.checks
        p.admit(len(ks))
        if p.checks != checks:
            # keys submitted from the minibatch that caused the last check to this one
            if last_cap is not None:
                assert since + len(ks) > (p.check - p.at) * last_cap
            since, last_cap = 0, tb.capacity
        since += len(ks)
        tb.insert(ks)
        assert len(tb.keys) <= p.bound <= p.check * tb.capacity
    assert p.grown >= 2 and not p.refused
    assert len(tb.keys) <= p.at * tb.capacity  # (the universe is exhausted: a settled table)
    for old, new, occ in tb.grows:
        assert occ <= p.at / 2 * new


def test_policy_refuses_past_max_bytes_and_then_the_table_fills():
    tb = StubTable(1024)
    p = GrowthPolicy(tb, max_bytes=32 * 4096)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(RuntimeError, match="KVTable full"):
            for i in range(200):
                p.admit(100)
                tb.insert(range(i * 100, i * 100 + 100))
    assert p.refused and tb.capacity <= 4096
    assert len([w for w in rec if "table growth refused" in str(w.message)]) == 1


def test_policy_refuses_when_the_allocation_fails():
    tb = StubTable(1024)
    p = GrowthPolicy(tb, reserve=lambda cap: False)
    with pytest.warns(RuntimeWarning, match="could not be allocated"):
        p.admit(5000)
    assert p.refused and tb.capacity == 1024 and p.grown == 0


def test_policy_rejects_bad_fractions():
    for check, at in ((0.5, 0.5), (0.4, 0.5), (1.5, 0.5), (0.75, 0.0)):
        with pytest.raises(ValueError, match="table_grow"):
            GrowthPolicy(StubTable(64), check=check, at=at)


# ----------------------------------------------------------------------- the trainer
def _train_cpu(steps=8, **kw):
    cfg = SparseLRConfig(num_features=1 << 20, minibatch=128, l1=0.5, **kw)
    tr = SparseLRTrainer(cfg)
    for s in range(steps):
        k, lab = criteo_batch(128, seed=7, row0=s * 128, num_features=cfg.num_features,
                              cards=[300] * 26)
        tr.step(k, lab)
    p = tr.progress()
    sd = tr.state_dict()
    o = torch.argsort(sd["keys"])
    return tr, p, {k: sd[k][o] for k in ("keys", "w", "z", "n")}


def test_trainer_cpu_growth_equals_a_large_table():
    _, pl, large = _train_cpu(table_capacity=1 << 15)
    tr, pg, grown = _train_cpu(table_capacity=1024, table_growth=True)
    assert pg["table_grown"] >= 2 and pg["table_capacity"] == tr.table.capacity > 1024
    assert (pl["table_grown"], pl["table_capacity"]) == (0, 1 << 15)
    for f in large:
        assert torch.equal(large[f], grown[f]), f
    assert tr.table.census()[0] <= tr.cfg.table_grow_check * tr.table.capacity
    with pytest.raises(RuntimeError, match="KVTable full"):
        _train_cpu(table_capacity=1024)


def test_trainer_cpu_refused_growth_fails_like_a_fixed_table():
    with pytest.warns(RuntimeWarning, match="max_table_bytes"):
        with pytest.raises(RuntimeError, match="KVTable full"):
            _train_cpu(table_capacity=1024, table_growth=True, max_table_bytes=32 * 2048)


def test_trainer_cpu_state_dict_loads_into_a_small_growing_trainer():
    src, _, want = _train_cpu(table_capacity=1024, table_growth=True)
    tr = SparseLRTrainer(SparseLRConfig(num_features=1 << 20, minibatch=128, l1=0.5,
                                        table_capacity=1024, table_growth=True))
    tr.load_state_dict(src.state_dict())
    assert tr.table.capacity > 1024 and tr.progress()["table_grown"] == 1
    assert tr.table.census()[0] <= tr.cfg.table_grow_at * tr.table.capacity
    sd = tr.state_dict()
    o = torch.argsort(sd["keys"])
    for f in want:
        assert torch.equal(sd[f][o], want[f]), f
    small = SparseLRTrainer(SparseLRConfig(num_features=1 << 20, minibatch=128,
                                           table_capacity=1024))
    with pytest.raises(RuntimeError, match="KVTable full"):
        small.load_state_dict(src.state_dict())


def test_growth_is_refused_where_others_hold_the_table():
    from types import SimpleNamespace

    two = SimpleNamespace(world=2, rank=0, backend="gloo", device=torch.device("cpu"))
    cfg = SparseLRConfig(num_features=1 << 20, minibatch=128, exchange="p2p", consistency="asp",
                         table_growth=True, table_capacity=1024)
    with pytest.raises(ValueError, match="table_growth is not supported on exchange='p2p'"):
        SparseLRTrainer(cfg, two)
    tr = SparseLRTrainer(SparseLRConfig(num_features=1 << 20, minibatch=128, table_capacity=1024,
                                        table_growth=True))
    with pytest.raises(ValueError, match="caller owns the exchange pipeline"):
        tr._mx_external = True
    off = SparseLRTrainer(SparseLRConfig(num_features=1 << 20, minibatch=128, table_capacity=1024))
    off._mx_external = True  # (growth off: a caller's pipeline works as before)
    assert off._mx_external is True


# ----------------------------------------------------------------------- two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, cfg_kw, steps):
    """One rank: the same minibatches through a trainer whose table was sized large and
    through one that starts at 1024 slots and grows (one after the other, one group)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import torch.distributed as dist

    from parameter_server_amd.parallel.comm import init_from_env

    comm, dev = init_from_env("cpu")
    out = {}
    for name, kw in (("large", dict(table_capacity=1 << 15)),
                     ("grown", dict(table_capacity=1024, table_growth=True))):
        cfg = SparseLRConfig(**cfg_kw, **kw)
        tr = SparseLRTrainer(cfg, comm, dev)
        for s in range(steps):
            if rank == 1 and s == steps - 1 and cfg.exchange == "padded":
                # (this rank's data ran out: a key-less step)
                tr.idle_step()
                continue
            k, lab = criteo_batch(cfg.minibatch, seed=100 + rank, row0=s * cfg.minibatch,
                                  num_features=cfg.num_features, cards=[2000] * 26)
            tr.step(k, lab)
        out[name] = {"progress": tr.progress(), "state": tr.state_dict(),
                     "capacity": tr.table.capacity}
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("plane", ["padded", "merged", "exact"])
def test_two_ranks_grow_alike_and_match_a_large_table(tmp_path, plane):
    # (a configured row capacity: the bound then adds 2 x 1536 keys per exchange from the
    # first step on, so the table grows in several steps, also in the middle of the run)
    cfg_kw = dict(num_features=1 << 20, minibatch=64, l1=0.5, exchange_capacity=1536)
    cfg_kw.update({"padded": dict(exchange="padded"),
                   "merged": dict(exchange="padded", consistency="ssp:2", exchange_merge="on"),
                   "exact": dict(exchange="exact")}[plane])
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), cfg_kw, 8), nprocs=2, join=True)
    res = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(2)]
    assert res[0]["grown"]["capacity"] == res[1]["grown"]["capacity"] > 1024
    assert res[0]["grown"]["progress"]["table_grown"] >= 2
    assert res[0]["grown"]["progress"]["table_grown"] == res[1]["grown"]["progress"]["table_grown"]
    for r in res:
        a, b = r["large"]["state"], r["grown"]["state"]
        oa, ob = torch.argsort(a["keys"]), torch.argsort(b["keys"])
        assert torch.equal(a["keys"][oa], b["keys"][ob])
        assert a["keys"].numel() > 1000
        for f in ("w", "z", "n"):  # (the tolerance of tests/test_dist_gloo.py)
            assert float((a[f][oa] - b[f][ob]).abs().max()) < 1e-5, f
        assert abs(r["large"]["progress"]["loss"] - r["grown"]["progress"]["loss"]) < 1e-6
