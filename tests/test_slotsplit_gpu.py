"""The device split by slot (slotsplit.hip, ops/slotsplit.py) against
``SlotData.from_batch`` on the same arrays: at every boundary of the work decomposition (the
tile of features per workgroup), on every cause of deferral, behind carried rows, and
through ``SlotReader(split="device")``, ``DarlinTrainer`` and the app."""
import os

import numpy as np
import pytest
import torch

from parameter_server_amd import data
from parameter_server_amd.data import ExampleBatch
from parameter_server_amd.data.slot_reader import SlotData, SlotReader
from parameter_server_amd.ops.slotsplit import max_ids, split_by_slot, tile

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = ["SPARSE_BINARY", "SPARSE"]


def _batch(rows, valued=False, seed=0) -> ExampleBatch:
    """``rows``: per row the list of (slot id, number of keys)."""
    rng = np.random.default_rng(seed)
    rp, slots = [0], []
    for r in rows:
        for g, k in r:
            slots.append(np.full(k, g, np.int32))
        rp.append(rp[-1] + sum(k for _, k in r))
    slots = np.concatenate(slots) if slots else np.zeros(0, np.int32)
    n = slots.size
    keys = rng.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n).astype(np.uint64)
    vals = (rng.integers(1, 9, n) / 4).astype(np.float32) if valued else None
    return ExampleBatch(np.ones(len(rows), np.float32), np.array(rp, np.int64), keys, vals, slots)


def _same(got: dict, ref: dict):
    assert list(got) == sorted(ref)
    for g in ref:
        for u, v in zip(got[g], ref[g]):
            assert (u is None) == (v is None)
            if v is not None:
                assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v)


def _up(x, dt):
    if x is None:
        return None
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(DEV, dt)


def _check(b: ExampleBatch, *, cause=None, cell_cap=None):
    """Kernel result == SlotData.from_batch on ``b``; deferred exactly with ``cause``."""
    ref = SlotData.from_batch(b).groups
    got = split_by_slot(None, _up(b.row_ptr, torch.int64), _up(b.keys, torch.int64),
                        _up(b.vals, torch.float32), _up(b.slots, torch.int32), cell_cap=cell_cap)
    torch.cuda.synchronize()
    assert (got.deferred, got.cause) == (cause is not None, cause)
    assert all(x.is_cuda for t in got.groups.values() for x in t if x is not None)
    _same(got.numpy(), ref)
    return got


# ------------------------------------------------------------------ decomposition
@pytest.mark.parametrize("valued", [False, True])
def test_one_row_of_n_features_around_the_tile(valued):
    T = tile()
    for n in (0, 1, T - 1, T, T + 1, 2 * T + 1):
        # (one run per group in the row, the ids not in ascending order)
        a, c = n // 3, n // 4
        row = [(g, k) for g, k in ((11, a), (2, n - a - c), (5, c)) if k]
        got = _check(_batch([row], valued, seed=n))
        assert len(got.groups) == len(row)


def test_row_boundary_on_a_tile_edge():
    T = tile()
    # the same group ends one row and starts the next, exactly at the edge
    _check(_batch([[(1, 10), (3, T - 10)], [(3, 5), (8, T - 5)], [(8, 1)]], True))
    _check(_batch([[(1, T)], [(1, T)], [(1, 1)]]))
    # rows without features on the edge
    _check(_batch([[(4, T - 1), (6, 1)], [], [], [(6, 2)], []]))


@pytest.mark.parametrize("valued", [False, True])
def test_one_run_longer_than_two_tiles(valued):
    T = tile()
    _check(_batch([[(7, 3)], [(1, 5), (2, 2 * T + 300), (3, 7)], [(2, 4), (3, 1)]], valued))


def test_runs_that_cross_a_tile_edge_by_one_feature():
    T = tile()
    # group 9's run of 40: one feature before the edge, then one feature behind it
    for first in (T - 1, T - 39):
        _check(_batch([[(5, first), (9, 40)], [(5, 3)], [(9, 2)]], True))
        _check(_batch([[(5, first)], [(9, 40), (5, 3)], [(9, 2)]], True))
    # a run of two features, one on each side
    _check(_batch([[(1, T - 1), (4, 2), (6, 10)], [(4, 1)]]))


def test_label_only_rows():
    got = _check(_batch([[]] * 3000))
    assert got.groups == {}
    rows = [[] for _ in range(3000)]
    rows[0], rows[1234], rows[2999] = [(3, 2)], [(3, 1), (5, 2)], [(5, 1)]
    _check(_batch(rows, True))


def test_extreme_slot_ids_and_one_slot():
    top = 2 ** 31 - 1
    got = _check(_batch([[(0, 1), (7, 2), (top, 1)], [(top, 2)], [(0, 3)], [(7, 1), (top, 1)]]))
    assert list(got.groups) == [0, 7, top]
    got = _check(_batch([[(6, 1)], [(6, 3)], [], [(6, 2)]], True))
    assert list(got.groups) == [6]


def test_most_slot_ids_and_one_more():
    M = max_ids()
    assert M == 4096
    ids = np.random.default_rng(1).permutation(1 << 20)[:M + 1] * 2047 + 3
    got = _check(_batch([[(int(g), 1) for g in ids[:M]]], True))
    assert len(got.groups) == M
    _check(_batch([[(int(g), 1) for g in ids]], True), cause="ids")
    # ids the parser never produces, but an array may hold
    b = _batch([[(1, 2), (2, 2)]])
    b.slots[2] = -5
    _check(b, cause="ids")


@pytest.mark.parametrize("valued", [False, True])
def test_group_named_twice_in_a_row_defers(valued):
    T = tile()
    _check(_batch([[(4, 2), (9, 1), (4, 3)], [(9, 2)]], valued), cause="repeat")
    # the two runs in different tiles
    _check(_batch([[(1, 3)], [(4, 20), (9, T + 10), (4, 3)], [(9, 2)]], valued), cause="repeat")


def test_cell_cap():
    b = _batch([[(1, 2), (2, 1)], [(2, 3)], [(1, 1)], [(2, 1), (5, 4)]], True)
    _check(b, cell_cap=3 * 5)  # S * (R + 1) cells: fits exactly
    _check(b, cell_cap=3 * 5 - 1, cause="cells")
    _check(b, cell_cap=0, cause="cells")


# ------------------------------------------------------------------ behind the parser
def _files(tmp_path, fmt, rows=(1500, 1500)):
    from parameter_server_amd.data.synthetic import sparse_groups, write_text

    files = []
    for k, n in enumerate(rows):
        sd = sparse_groups(n, groups=5, present=3, keys_per_group=500, seed=70 + k)
        if fmt == "SPARSE":
            rng = np.random.default_rng(k)
            sd.groups = {g: (o, kk, rng.integers(1, 9, kk.size).astype(np.float32) / 4)
                         for g, (o, kk, _) in sd.groups.items()}
        files.append(str(tmp_path / f"part-{k}"))
        write_text(sd, files[-1], fmt)
    return files


@pytest.mark.parametrize("fmt", FMTS)
def test_split_behind_carried_rows(tmp_path, fmt):
    from parameter_server_amd.ops.textparse import parse_text_device
    from parameter_server_amd.ops.textparse import TextParseBuffers

    raw = open(_files(tmp_path, fmt, (700,))[0], "rb").read()
    cut = raw.index(b"\n", len(raw) // 3) + 1
    a, b = raw[:cut], raw[cut:]
    dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(DEV)  # noqa: E731
    out = TextParseBuffers(1000, 40000, DEV)
    p1 = parse_text_device(dev(a), fmt, ignore_slot=False, out=out)
    p2 = parse_text_device(dev(b), fmt, ignore_slot=False, out=out, row0=p1.rows, nnz0=p1.nnz)
    assert not p1.deferred and not p2.deferred and p1.nnz > 0 and int(p2.row_ptr[0]) == p1.nnz
    for p, text in ((p1, a), (p2, b)):
        ref = SlotData.from_batch(data.parse_text(text, fmt, ignore_slot=False)).groups
        vals = out.vals[p.keys.storage_offset():][:p.nnz] if fmt == "SPARSE" else None
        got = split_by_slot(p.labels, p.row_ptr, p.keys, vals, p.slots)
        assert not got.deferred and len(got.groups) == 5
        _same(got.numpy(), ref)


def _same_data(a: SlotData, b: SlotData):
    assert np.array_equal(a.labels, b.labels) and a.labels.dtype == b.labels.dtype
    _same({g: a.groups[g] for g in sorted(a.groups)}, b.groups)


def _host(sd: SlotData) -> SlotData:
    assert isinstance(sd.labels, np.ndarray)
    for o, k, v in sd.groups.values():
        assert o.is_cuda and o.dtype == torch.int64 and k.is_cuda and k.dtype == torch.int64
        assert v is None or (v.is_cuda and v.dtype == torch.float32)
    return SlotData(sd.labels, {g: (o.cpu().numpy(), k.cpu().numpy().view(np.uint64),
                                    None if v is None else v.cpu().numpy())
                                for g, (o, k, v) in sd.groups.items()})


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """Per format: the files, and what the host route reads from them (with its cache)."""
    out = {}
    for fmt in FMTS:
        d = tmp_path_factory.mktemp(fmt.lower())
        files = _files(d, fmt)
        hc = SlotReader(files, fmt, cache_prefix=str(d / "ch") + "/", parser="cpu")
        out[fmt] = (d, files, hc.read())
    return out


@pytest.mark.parametrize("fmt", FMTS)
def test_slot_reader_device_split_matches_host_route(routes, fmt):
    d, files, host = routes[fmt]
    r = SlotReader(files, fmt, parser="gpu", split="device", device=DEV)
    assert (r.parser, r.split, r.resident) == ("gpu", "device", False)
    got = r.read()
    # (write_text names each group once per row: a condition, not a measurement)
    assert r.split_deferred_chunks == 0 and r.deferred_chunks == 0
    assert got.rows == 3000 and len(got.groups) == 5
    assert (next(iter(got.groups.values()))[2] is None) == (fmt == "SPARSE_BINARY")
    _same_data(got, host)
    assert got.info() == host.info()
    # the device split needs the device parser; the defaults and "auto" stay on the host
    assert SlotReader(files, fmt, parser="cpu", split="device", device=DEV).split == "host"
    assert SlotReader(files, fmt, parser="auto", split="device", device=DEV).split == "host"
    assert SlotReader(files, "LIBSVM", parser="gpu", split="device", device=DEV).split == "host"
    assert SlotReader(files, fmt, parser="gpu", device=DEV).split == "host"
    assert SlotReader(files, fmt, parser="gpu", resident=True, device=DEV).resident is False
    with pytest.raises(ValueError):
        SlotReader(files, fmt, split="gpu")
    # the cache files are the host route's byte for byte; a second read hits them
    rc = SlotReader(files, fmt, cache_prefix=str(d / "cg") + "/", parser="gpu", split="device",
                    device=DEV)
    _same_data(rc.read(), host)
    assert rc.hit_cache == 0
    _same_data(rc.read(), host)
    assert rc.hit_cache == 2
    names = sorted(os.listdir(d / "ch"))
    assert names == sorted(os.listdir(d / "cg")) and len(names) > 10
    for name in names:
        assert open(d / "ch" / name, "rb").read() == open(d / "cg" / name, "rb").read(), name


@pytest.mark.parametrize("fmt", FMTS)
def test_slot_reader_resident(routes, fmt):
    d, files, host = routes[fmt]
    r = SlotReader(files, fmt, parser="gpu", split="device", resident=True, device=DEV)
    assert r.resident
    got = r.read()
    assert r.split_deferred_chunks == 0 and r.deferred_chunks == 0
    _same_data(_host(got), host)
    assert got.info() == host.info()
    # with a cache the files are written from a copy; the hit returns numpy arrays
    rc = SlotReader(files, fmt, cache_prefix=str(d / "cr") + "/", parser="gpu", split="device",
                    resident=True, device=DEV)
    _same_data(_host(rc.read()), host)
    for name in sorted(os.listdir(d / "ch")):
        assert open(d / "ch" / name, "rb").read() == open(d / "cr" / name, "rb").read(), name
    _same_data(rc.read(), host)
    assert rc.hit_cache == 2


@pytest.mark.parametrize("ignore_slot", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_slot_reader_joins_chunks_on_the_device(routes, fmt, ignore_slot, monkeypatch):
    from parameter_server_amd.data import slot_reader

    d, files, _ = routes[fmt]
    host = SlotReader(files, fmt, parser="cpu", ignore_slot=ignore_slot).read()
    monkeypatch.setattr(slot_reader, "_CHUNK", 16384)
    assert os.path.getsize(files[0]) > 3 * 16384
    for resident in (False, True):
        r = SlotReader(files, fmt, parser="gpu", split="device", resident=resident, device=DEV,
                       ignore_slot=ignore_slot)
        got = r.read()
        assert r.split_deferred_chunks == 0 and r.deferred_chunks == 0
        _same_data(_host(got) if resident else got, host)
    assert (list(host.groups) == [1]) == ignore_slot


def test_all_ones_sparse_file_is_binary(tmp_path, monkeypatch):
    from parameter_server_amd.data import slot_reader
    from parameter_server_amd.data.synthetic import sparse_groups, write_text

    sd = sparse_groups(1200, groups=4, present=2, keys_per_group=100, seed=5)
    sd.groups = {g: (o, k, np.ones(k.size, np.float32)) for g, (o, k, _) in sd.groups.items()}
    f = str(tmp_path / "part-0")
    write_text(sd, f, "SPARSE")
    host = SlotReader([f], "SPARSE", parser="cpu").read()
    for chunk in (slot_reader._CHUNK, 16384):  # one chunk; several, the ones carried along
        monkeypatch.setattr(slot_reader, "_CHUNK", chunk)
        assert os.path.getsize(f) > 2 * 16384
        got = SlotReader([f], "SPARSE", parser="gpu", split="device", device=DEV).read()
        assert all(v is None for _, _, v in got.groups.values())
        _same_data(got, host)


def test_slot_reader_counts_the_chunks_it_hands_back(tmp_path):
    f = str(tmp_path / "part-0")
    with open(f, "w") as fh:  # (the first row names group 4 twice)
        fh.write("1; 4 10 11; 9 5; 4 12\n0; 9 3\n1; 4 7; 9 8 6\n")
    host = SlotReader([f], "SPARSE_BINARY", parser="cpu").read()
    assert host.groups[4][0].tolist() == [0, 3, 3, 4]
    for resident in (False, True):
        r = SlotReader([f], "SPARSE_BINARY", parser="gpu", split="device", resident=resident,
                       device=DEV)
        got = r.read()
        assert r.split_deferred_chunks == 1 and r.deferred_chunks == 0
        _same_data(_host(got) if resident else got, host)


# ------------------------------------------------------------------ Darlin, the app
@pytest.mark.parametrize("fmt", FMTS)
def test_darlin_from_resident_data_matches_host_data(routes, fmt):
    from parameter_server_amd.models.darlin import DarlinConfig, DarlinTrainer

    _, files, host = routes[fmt]
    res = SlotReader(files, fmt, parser="gpu", split="device", resident=True, device=DEV).read()
    cfg = DarlinConfig(l1=1.0, max_pass=1, seed=0)
    th = DarlinTrainer(host, cfg, device=DEV)
    tr = DarlinTrainer(res, cfg, device=DEV)
    for name in ("col", "row", "val"):
        u, v = getattr(tr, name), getattr(th, name)
        assert (u is None) == (v is None)
        if v is not None:
            assert u.dtype == v.dtype and torch.equal(u, v), name
    assert th.col.numel() > 5000 and np.array_equal(tr.colptr, th.colptr)
    assert torch.equal(tr.y, th.y) and tr.info == th.info and tr.num_cols == th.num_cols
    assert all(np.array_equal(tr.group_keys[g], th.group_keys[g]) for g in th.group_keys)
    # Both trainers now run the same kernels on bitwise equal arrays. Those kernels add their
    # fp64 sums (G / U per column, the margins, the objective) with unordered atomics
    # (bcd.hip), so one trainer does not repeat its own objective to the last bit
    # (tests/test_darlin_gpu.py says the same of the fused row pass); what two orders of the
    # same sums can differ by is bounded instead. u = 2^-53, n = 3000 rows, terms of
    # magnitude <= 1: a column's G and U are sums of <= n terms, each off by <= n u times its
    # sum of magnitudes, so the column's step G / U-like is off by <= ~4 n u; a margin adds
    # <= 6 such steps (3 groups x 2 keys per row); the objective adds n losses with slope
    # <= 1: <= 4 n u * 6 * n = 2.4e-8 absolute, on an objective above n ln 2 / 2 > 1000 that
    # is 2.4e-11 relative in the worst case.
    oh, od = [p.objective for p in th.train()], [p.objective for p in tr.train()]
    print("objectives: host data", oh, "resident data", od)
    assert len(oh) == 1 and oh[0] > 1000
    np.testing.assert_allclose(od, oh, rtol=2.4e-11, atol=0)


def test_app_slot_split_device_matches_parser_cpu(tmp_path):
    from parameter_server_amd.app.gpu import _flags, run_darlin
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    files = _files(tmp_path, "SPARSE_BINARY", (600, 600, 600))
    models = {}
    for name, args in (("device", ["-parser", "gpu", "-slot_split", "device"]),
                       ("cpu", ["-parser", "cpu"])):
        model = tmp_path / f"model_{name}" / "m"
        conf = tmp_path / f"{name}.conf"
        conf.write_text(f"""linear_method {{
training_data {{ format: TEXT text: SPARSE_BINARY file: "{tmp_path}/part.*" }}
model_output {{ format: TEXT file: "{model}" }}
loss {{ type: LOGIT }}
penalty {{ type: L1 lambda: 1 }}
learning_rate {{ type: CONSTANT alpha: 1 }}
darlin {{ max_pass_of_data: 3 epsilon: 1e-9 feature_block_ratio: 2
  random_feature_block_order: false max_block_delay: 1 }}
}}""")
        flags = _flags(["-app_file", str(conf), "-num_threads", "2", "-device", "cuda", "-quiet"]
                       + args)
        dev = torch.device("cuda")
        res = run_darlin(load_app_config(str(conf)).linear_method, LocalComm(dev), dev, flags)
        assert res["examples"] == 1800 and res["passes"] == 3
        assert res["parser"] == ("gpu" if name == "device" else "cpu")
        assert res["slot_split"] == ("device" if name == "device" else "host")
        assert res["split_deferred_chunks"] == 0 and res["deferred_chunks"] == 0
        models[name] = open(res["model"], "rb").read()
    assert len(models["device"].splitlines()) > 20
    assert models["device"] == models["cpu"]
    assert _flags(["-app_file", "x"]).slot_split == "host"
