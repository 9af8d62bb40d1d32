"""The device model-text paths (modeltext.hip, the model lines of textparse.hip,
ops/modeltext.py) against the host code on the same data: files byte for byte what
``write_text_model`` writes -- at every boundary of the work decomposition, in unsigned key
order, with and without entries the formatter defers -- and pairs bit for bit what
``read_text_models`` yields, on plain text (which must not be deferred), around the span
edges, and on every kind of line that has to take the host rules, exceptions included."""
import os

import numpy as np
import pytest
import torch

import modeltext_corpus as corpus
from parameter_server_amd.models import ModelScorer, SparseLRConfig, SparseLRTrainer
from parameter_server_amd.ops.modeltext import (pairs_of, read_text_models_device,
                                                write_text_model_device)
from parameter_server_amd.ops.native import core, hipops
from parameter_server_amd.utils.checkpoint import read_text_models, write_text_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPAN = 16384  # bytes of text per workgroup (textparse.hip)
OK = corpus.OK


def _t(k: np.ndarray, w: np.ndarray):
    return (torch.from_numpy(k.astype(np.uint64).view(np.int64).copy()).to(DEV),
            torch.from_numpy(w.astype(np.float32).copy()).to(DEV))


def _same_file(tmp_path, k, w, **kw):
    """The device writer's file == the host writer's; returns (bytes, deferred_chunks)."""
    tag = len(os.listdir(tmp_path))
    hp, dp = str(tmp_path / f"h{tag}" / "m_S0"), str(tmp_path / f"d{tag}" / "m_S0")
    n_host = write_text_model(hp, k.astype(np.uint64), w.astype(np.float32))
    n_dev, deferred = write_text_model_device(dp, *_t(k, w), **kw)
    torch.cuda.synchronize()
    with open(hp, "rb") as f:
        want = f.read()
    with open(dp, "rb") as f:
        got = f.read()
    assert n_dev == n_host
    if got != want:
        i = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{len(got)} vs {len(want)} bytes, first difference at {i}: "
                             f"{got[max(0, i - 40):i + 40]!r} vs {want[max(0, i - 40):i + 40]!r}")
    return got, deferred


def _clean(n: int, seed: int, lo_exp: int = -20):
    """n distinct keys of every length, in-domain weights of every notation (magnitudes
    from 5 * 10^(lo_exp - 2) up)."""
    rng = np.random.default_rng(seed)
    k = corpus.keys_for(4 * n + 16)
    k = k[np.sort(np.unique(k, return_index=True)[1])][:n]
    rng.shuffle(k)
    m = rng.standard_normal(n)
    m = np.where(m < 0, -1.0, 1.0) * np.maximum(np.abs(m), 0.05)  # (|w| in [5e-22, 1e8))
    w = (m * 10.0 ** rng.integers(lo_exp, 8, n)).astype(np.float32)
    assert k.size == n and corpus.in_domain(w).all()
    return k, w


# ------------------------------------------------------------------------------ writer
def test_writer_block_boundaries(tmp_path):
    W = int(hipops().modeltext_block())
    assert W == 1024
    for n in (0, 1, W - 1, W, W + 1, 2 * W + 3):
        k, w = _clean(n, 100 + n)
        raw, deferred = _same_file(tmp_path, k, w)
        assert deferred == 0 and raw.count(b"\n") == n


def test_writer_chunk_boundaries(tmp_path):
    k, w = _clean(5000, 7)
    raw, deferred = _same_file(tmp_path, k, w, chunk_entries=2048)
    assert deferred == 0 and raw.count(b"\n") == 5000


def test_writer_unsigned_key_order(tmp_path):
    rng = np.random.default_rng(11)
    hi = np.array([1 << 63, (1 << 63) + 1, (1 << 64) - 1, (1 << 64) - 2, 3 << 62], dtype=np.uint64)
    k = np.concatenate([hi, np.arange(0, 40, dtype=np.uint64), np.array([(1 << 63) - 1], np.uint64),
                        rng.integers(1 << 62, 1 << 63, 300, dtype=np.uint64) * np.uint64(2)])
    k = np.unique(k)
    rng.shuffle(k)
    w = rng.standard_normal(k.size).astype(np.float32)
    raw, deferred = _same_file(tmp_path, k, w)
    keys = [int(x.split(b"\t")[0]) for x in raw.splitlines()]
    assert deferred == 0 and keys == sorted(keys) and keys[-1] == (1 << 64) - 1
    assert sum(x >= 1 << 63 for x in keys) > 100 and keys[0] == 0
    # dropped entries: zero, minus zero, NaN
    w[::5] = 0.0
    w[1::5] = -0.0
    w[2::5] = np.nan
    raw, _ = _same_file(tmp_path, k, w)
    assert raw.count(b"\n") == k.size - len(w[::5]) - len(w[1::5]) - len(w[2::5])


def test_writer_corpus_weights_and_deferral(tmp_path):
    w = corpus.weights()
    w = w[corpus.in_domain(w)]
    k = np.arange(w.size, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15)  # (distinct: odd)
    _, st, _ = core().textfmt_entries(k, w)
    assert np.all(st == OK) and w.size > 300_000  # the host routine defers none of them
    raw, deferred = _same_file(tmp_path, k, w, chunk_entries=1 << 17)
    assert deferred == 0 and raw.count(b"\n") == w.size
    # one out-of-domain weight in the middle chunk of three
    k2 = np.arange(1, 3 * 2048 + 1, dtype=np.uint64)
    for odd in (3e9, np.inf, 1e-30, 1e-40):
        w2 = w[:k2.size].copy()
        w2[2048 + 1000] = odd
        _, st, _ = core().textfmt_entries(k2, w2)
        assert (st != OK).sum() == 1
        raw, deferred = _same_file(tmp_path, k2, w2, chunk_entries=2048)
        assert deferred == 1 and raw.count(b"\n") == k2.size


def _train(num_features: int):
    B, width = 1000, 8
    cfg = SparseLRConfig(num_features=num_features, minibatch=B, table_capacity=1 << 14, l1=0.001,
                         alpha=0.5, beta=1.0)
    tr = SparseLRTrainer(cfg, device=DEV)
    g = torch.Generator().manual_seed(5)
    if num_features:
        pool = torch.randint(0, num_features, (3000,), generator=g, dtype=torch.int64)
    else:  # raw 64-bit keys, most of them at or above 2^63
        pool = (torch.randint(0, 1 << 32, (3000,), generator=g, dtype=torch.int64) << 32) | \
            torch.randint(0, 1 << 32, (3000,), generator=g, dtype=torch.int64)
        pool[::4] >>= 20
    for _ in range(4):
        keys = pool[torch.randint(0, pool.numel(), (B * width,), generator=g)].to(DEV)
        labels = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).float().to(DEV)
        tr.step(keys, labels, width=width)
    return tr


@pytest.mark.parametrize("num_features", [0, 1 << 20])
def test_trainer_save_and_round_trip(tmp_path, num_features):
    tr = _train(num_features)
    assert tr.bits == (64 if num_features == 0 else 20)
    dp = tr.save_model(str(tmp_path / "dev" / "m"), text_io="device")
    assert tr.last_save["deferred_chunks"] == 0
    hp = tr.save_model(str(tmp_path / "host" / "m"), text_io="host")
    ap = tr.save_model(str(tmp_path / "auto" / "m"))
    with open(dp, "rb") as f:
        raw = f.read()
    with open(hp, "rb") as f:
        assert f.read() == raw
    with open(ap, "rb") as f:
        assert f.read() == raw
    nnz = tr.table.census()[1]
    assert raw.count(b"\n") == nnz == tr.last_save["entries"] > 500
    # round trip: every non-zero weight comes back bit for bit
    keys, w, entries, deferred = read_text_models_device(dp, DEV)
    assert (entries, deferred) == (nnz, 0)
    from parameter_server_amd.ops.keymix import unmix

    mk, mw = tr.table.occupied_weights()
    keep = mw != 0
    want = dict(zip(unmix(mk[keep], tr.bits).tolist(), mw[keep].view(torch.int32).tolist()))
    assert dict(zip(keys.tolist(), w.view(torch.int32).tolist())) == want


# ------------------------------------------------------------------------------ reader
def _pairs_equal(path: str, chunk_bytes: int = 32 << 20, deferred_want=0):
    """Device reader == dict reader on the files of ``path``: the same pairs bit for bit,
    in file order."""
    rk, rw = pairs_of(read_text_models(path))
    keys, w, entries, deferred = read_text_models_device(path, DEV, chunk_bytes=chunk_bytes)
    torch.cuda.synchronize()
    assert entries == rk.numel()
    assert torch.equal(keys.cpu(), rk) and torch.equal(w.cpu().view(torch.int32),
                                                       rw.view(torch.int32))
    if deferred_want is not None:
        assert deferred == deferred_want
    return keys, w


def _plain_text(n: int, seed: int) -> bytes:
    """Lines of the writer above whose weight tokens all scan kOk: nine digits times
    10^-22 at the least is inside the scanner's exact domain (csrc/core/textnum.h)."""
    k, w = _clean(n, seed, lo_exp=-12)
    order = np.argsort(k, kind="stable")
    lines = corpus.python_lines(k[order], w[order])
    _, st = core().textnum_f32([x.split(b"\t")[1][:-1] for x in lines])
    assert np.all(st == OK)  # (the seed is picked so that no token is a deferred tie)
    return b"".join(lines)


def test_reader_plain_text_around_the_span_edge(tmp_path):
    text = _plain_text(1600, 21)
    assert len(text) > 2 * SPAN + 64
    for size in (SPAN - 1, SPAN, SPAN + 1, 2 * SPAN):
        # whole lines up to the size, then filler lines "<key>\t1\n" that end exactly there
        cut = text.rfind(b"\n", 0, size - 24) + 1
        rem, fill = size - cut, []
        while rem > 32:
            fill.append(b"%d\t1\n" % (7000000 + len(fill)))  # (10 bytes, distinct keys)
            rem -= 10
        fill += [b"600000000\t1\n", b"8" * (rem - 15) + b"\t1\n"]  # (12 and 11..20 bytes)
        raw = text[:cut] + b"".join(fill)
        assert len(raw) == size and 23 <= rem <= 32
        p = tmp_path / f"s{size}" / "m_S0"
        p.parent.mkdir()
        p.write_bytes(raw)
        _pairs_equal(str(p))
        p.write_bytes(raw[:-1])  # the final line without its newline
        _pairs_equal(str(p))


def test_reader_chunks_and_empty_lines(tmp_path):
    text = _plain_text(13000, 22)
    assert 200_000 < len(text) < 500_000
    p = tmp_path / "m_S0"
    p.write_bytes(text)
    keys, _ = _pairs_equal(str(p), chunk_bytes=65536)
    assert keys.numel() == 13000
    lines = text.splitlines(keepends=True)
    p.write_bytes(b"\n" + b"".join(x + (b"\n" if i % 7 == 0 else b"") for i, x in enumerate(lines))
                  + b"\n\n")
    _pairs_equal(str(p), chunk_bytes=65536)
    p.write_bytes(b"\n\n")
    assert _pairs_equal(str(p))[0].numel() == 0
    p.write_bytes(b"")
    assert _pairs_equal(str(p))[0].numel() == 0


FALLBACK = {
    "crlf": b"77000001\t0.5\r\n77000002\t0.25\r\n",
    "leading_space": b"77000001\t0.5\n 77000002\t0.25\n77000003\t1\n",
    "trailing_space": b"77000001\t0.5 \n77000002\t0.25\n",
    "second_tab": b"77000001\t0.5\n77000002\t0.25\t7\n",
    "plus_key": b"+77000005\t0.5\n77000006\t1\n",
    "plus_weight": b"77000005\t+0.5\n77000006\t1\n",
    "plus_minus_weight": b"77000005\t+-0.5\n",
    "nan_weight": b"77000005\tnan\n77000006\t1\n",
    "underscore": b"7700_0001\t1_0.5\n",
    "key_21_digits": b"100000000000000000000\t1\n",
    "key_2_64": b"18446744073709551616\t1\n",
    "negative_key": b"-77000005\t1\n",
    "no_weight": b"77000005\n",
    "empty_weight": b"77000005\t\n77000006\t1\n",
    "long_weight": b"77000005\t0." + b"1" * 80 + b"\n",
    "many_digits": b"77000005\t0.12345678901234567890\n",
    "repeated_key": b"77000005\t0.5\n77000006\t1\n77000005\t0.75\n",
    "bytes": b"77000005\t0.5\n\xff\xfe\t1\n",
}


@pytest.mark.parametrize("name", sorted(FALLBACK))
def test_reader_fallback_inputs(tmp_path, name):
    """The host reader's result, or its exception type, through ``from_text``."""
    head = _plain_text(40, 23)
    p = tmp_path / "m_S0"
    p.write_bytes(head + FALLBACK[name])
    pat = str(tmp_path / "m_S.*")
    try:
        want = ModelScorer.from_text(pat, 64, DEV, text_io="host")
    except Exception as e:  # noqa: BLE001 (the type is what is compared)
        with pytest.raises(type(e)):
            ModelScorer.from_text(pat, 64, DEV, text_io="device")
        return
    got = ModelScorer.from_text(pat, 64, DEV, text_io="device")
    _same_table(got, want)
    # (a repeated key parses as plain text; the occupancy check then reloads on the host)
    assert got.deferred_chunks == (0 if name == "repeated_key" else 1)


def _same_table(got: ModelScorer, want: ModelScorer):
    assert got.entries == want.entries and got.table.capacity == want.table.capacity
    (gk, gw), (wk, ww) = got.table.occupied_weights(), want.table.occupied_weights()
    go, wo = torch.argsort(gk), torch.argsort(wk)
    assert torch.equal(gk[go], wk[wo])
    assert torch.equal(gw[go].view(torch.int32), ww[wo].view(torch.int32))


def test_reader_repeated_key_across_files(tmp_path):
    (tmp_path / "m_S0").write_bytes(_plain_text(40, 24) + b"77000005\t0.5\n")
    (tmp_path / "m_S1").write_bytes(b"77000005\t0.75\n77000006\t1\n")
    pat = str(tmp_path / "m_S.*")
    want = ModelScorer.from_text(pat, 64, DEV, text_io="host")
    got = ModelScorer.from_text(pat, 64, DEV, text_io="device")
    _same_table(got, want)
    assert got.entries == 42
    m = got.predict(torch.tensor([77000005, 77000006], dtype=torch.int64, device=DEV), width=1)
    assert m.tolist() == [0.75, 1.0]


def test_from_text_device_equals_host(tmp_path):
    tr = _train(1 << 20)
    tr.save_model(str(tmp_path / "m"))
    pat = str(tmp_path / "m_S.*")
    a = ModelScorer.from_text(pat, tr.bits, DEV, text_io="device")
    b = ModelScorer.from_text(pat, tr.bits, DEV, text_io="host")
    c = ModelScorer.from_text(pat, tr.bits, DEV)
    assert a.entries == b.entries == c.entries == tr.table.census()[1]
    assert a.deferred_chunks == 0 and c.deferred_chunks == 0
    _same_table(a, b)
    # a small CSR minibatch over model keys and unknown ones
    g = torch.Generator().manual_seed(9)
    mk, _ = tr.table.occupied_weights()
    from parameter_server_amd.ops.keymix import unmix

    known = unmix(mk, tr.bits).cpu()
    widths = torch.randint(1, 12, (64,), generator=g)
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), widths.cumsum(0)]).to(DEV)
    nnz = int(widths.sum())
    keys = torch.where(torch.rand(nnz, generator=g) < 0.8,
                       known[torch.randint(0, known.numel(), (nnz,), generator=g)],
                       torch.randint(0, 1 << 20, (nnz,), generator=g)).to(DEV)
    vals = torch.randn(nnz, generator=g).to(DEV)
    ma = a.predict(keys, row_ptr=row_ptr, vals=vals)
    mb = b.predict(keys, row_ptr=row_ptr, vals=vals)
    assert torch.equal(ma.view(torch.int32), mb.view(torch.int32)) and float(ma.abs().max()) > 0
