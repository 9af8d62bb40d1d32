"""The device text parser (textparse.hip, ops/textparse.py) against the host parser on the
same bytes: labels, row offsets and keys bitwise, values bitwise or None by the host's
binary rule, bad-line and row counts -- on clean corpora (which must not be deferred to
the host), at every boundary of the work decomposition, on malformed and random bytes,
behind carried rows, through the DeviceFeeder and through the file-fed app."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from parameter_server_amd import data
from parameter_server_amd.ops.native import core
from parameter_server_amd.ops.textparse import (TextParseBuffers, parse_text_device,
                                                segments_valued, supported)
from parameter_server_amd.ops.textparse import traits as textparse_traits
from textparse_cases import _dev, check_against_host

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPAN = 16384  # bytes of text per workgroup (textparse.hip)
_check = functools.partial(check_against_host, ignore_slot=True)


# ------------------------------------------------------------------ corpora
def _value(rng) -> str:
    k = rng.randrange(4)
    if k == 0:
        return "1"
    if k == 1:  # short signed decimal
        return rng.choice(["", "-", "+"]) + f"{rng.randrange(1000)}.{rng.randrange(1000):03d}"
    if k == 2:  # d.ddde+-x inside the exact domain
        return (rng.choice(["", "-"]) + f"{rng.randrange(1, 10)}.{rng.randrange(1000):03d}"
                + rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randrange(0, 9)))
    return str(rng.randrange(1, 100000))


def _libsvm_rows(rows: int, seed: int, max_w: int = 200):
    rng = random.Random(seed)
    out = []
    for r in range(rows):
        w = 0 if rng.random() < 0.05 else rng.randint(1, max_w if rng.random() < 0.1 else 12)
        hi = (1 << 64) - 1 if rng.random() < 0.3 else 1 << 20
        idx = sorted(rng.randint(0, hi) for _ in range(w))
        if w and rng.random() < 0.05:
            idx[-1] = (1 << 64) - 1
        label = rng.choice(["1", "-1", "+1", "0", "0.5", "-2.5e-1"])
        out.append((label, [f"{i}:{_value(rng)}" for i in idx]))
    return out


def _join(rows, sep=" ", eol="\n", trailing=True) -> bytes:
    s = eol.join(sep.join([lab] + feats) for lab, feats in rows)
    return (s + (eol if trailing else "")).encode()


@pytest.fixture(scope="module")
def libsvm_rows():
    rows = _libsvm_rows(3000, 7)
    # the corpus is clean: no value or label the shared scanner would defer or reject
    toks = [lab.encode() for lab, _ in rows] + \
        [f.split(":")[1].encode() for _, feats in rows for f in feats]
    _, st = core().textnum_f32(toks)
    assert not st.any()
    assert any(not f for _, f in rows) and max(len(f) for _, f in rows) > 100
    return rows


@pytest.mark.parametrize("sep,eol", [(" ", "\n"), ("\t", "\n"), ("  ", "\n"), (" ", "\r\n")])
@pytest.mark.parametrize("hash_mod", [0, 65536, 10 ** 9])
def test_clean_libsvm_not_deferred(libsvm_rows, sep, eol, hash_mod):
    for trailing in (True, False):
        got = _check(_join(libsvm_rows, sep, eol, trailing), "LIBSVM", hash_mod)
        assert got.rows == 3000 and got.vals is not None


def test_binary_libsvm_has_no_values():
    rng = random.Random(3)
    rows = [("1", [f"{i}:1" for i in sorted(rng.sample(range(1000), 39))]) for _ in range(500)]
    got = _check(_join(rows), "LIBSVM", 0)
    assert got.vals is None and got.width == 39


# ------------------------------------------------------------------ decomposition
def _short_lines(total: int, seed: int) -> bytes:
    """Exactly ``total`` bytes of ~40-byte LIBSVM lines: whole tokens only, the rest
    filled with blanks (the last line may lack its newline)."""
    rng = random.Random(seed)
    out = bytearray()
    while True:
        idx = sorted(rng.randrange(10 ** 4, 10 ** 5) for _ in range(rng.randint(2, 4)))
        toks = ["1"] + [f" {i}:1" for i in idx] + [f" {rng.randrange(10 ** 5, 10 ** 6)}:0.25", "\n"]
        for t in toks:
            if len(out) + len(t) > total:
                return bytes(out) + b" " * (total - len(out))
            out += t.encode()


def test_empty_and_blank_buffers():
    for raw in (b"", b"\n\n\n", b"\n", b" \t \r\n\r\n", b"1 2:3 4:5", b"-1", b"1\n"):
        got = _check(raw, "LIBSVM")
        assert got.deferred is False
    assert _check(b"\n\t\t\n", "CRITEO").rows == 0
    assert _check(b"1\t5", "CRITEO").rows == 1


@pytest.mark.parametrize("spans", [1, 2])
def test_lengths_around_span_edges(spans):
    # lines shift by one byte per case: every alignment of a token start, a token end and
    # a newline against the span edge occurs
    for total in range(spans * SPAN - 4, spans * SPAN + 4):
        _check(_short_lines(total, total), "LIBSVM", 65536)
    base = _short_lines(spans * SPAN + 64, 5)
    for shift in range(48):  # (longer than a line)
        _check(b" " * shift + base, "LIBSVM")


def test_one_very_long_line_between_short_ones():
    rng = random.Random(11)
    idx = sorted(rng.sample(range(1 << 40), 20000))
    long_line = ("1 " + " ".join(f"{i}:{_value(rng)}" for i in idx) + "\n").encode()
    assert len(long_line) > 250_000
    raw = _short_lines(4000, 1) + b"\n" + long_line + _short_lines(4000, 2) + b"\n"
    got = _check(raw, "LIBSVM", 10 ** 9)
    assert int(np.diff(got.row_ptr.cpu().numpy()).max()) == 20000


# ------------------------------------------------------------------ malformed input
def test_malformed_and_deferring_lines(libsvm_rows):
    good = [" ".join([lab] + feats) for lab, feats in libsvm_rows[:500]]
    bad = ["1 5:1 3:1", "1 abc:1", "1 7", "1 123456789012345678901:1", "1 1:1e400",
           "1 " + "9" * 70 + ":1", "# a comment", "  # indented comment",
           "1 1:0.12345678901234567", "1 2:1.2345678901234567e5", "1 1:", "1 :1", "x 1:1",
           "1 1:1:1", "1 1:nan", "1 1:inf", "1 18446744073709551616:1", "1 1:--1", "1 1:1e",
           "1 4:1 4:2 4:3"]
    rng = random.Random(5)
    whole = _check(("\n".join(good + bad) + "\n").encode(), "LIBSVM", 0, clean=False)
    assert whole.deferred and whole.bad_lines > 5
    for b in bad:  # each alone among good rows
        lines = list(good[:40])
        lines.insert(rng.randrange(len(lines)), b)
        _check(("\n".join(lines) + "\n").encode(), "LIBSVM", 65536, clean=False)


@pytest.mark.parametrize("fmt", ["LIBSVM", "CRITEO"])
def test_random_printable_bytes(fmt):
    rng = random.Random(99)
    alphabet = [chr(c) for c in range(33, 127)] + [" ", "\t", "\n", ":", "1", "0", " ", "\n"] * 6
    raw = "".join(rng.choice(alphabet) for _ in range(65536)).encode()
    got = _check(raw, fmt, 65536, clean=False)
    assert got.rows <= 65536 and got.nnz <= 65536  # (inside the counted sizes)
    rp = got.row_ptr.cpu().numpy()
    assert rp[0] == 0 and rp[-1] == got.nnz and (np.diff(rp) >= 0).all()


def test_output_capacity_overflow_defers():
    rows = _libsvm_rows(400, 21, max_w=30)
    raw = _join(rows)
    ref = data.parse_text(raw, "LIBSVM", ignore_slot=True)
    out = TextParseBuffers(100, 50, DEV)  # too small for 400 rows
    got = parse_text_device(_dev(raw), "LIBSVM", 0, out=out)
    assert got.deferred and got.rows == ref.rows and got.nnz == ref.nnz
    assert np.array_equal(got.keys.cpu().numpy().view(np.uint64), ref.keys.view(np.uint64))
    # the sticky flag was cleared: the grown buffers parse on the device again
    again = parse_text_device(_dev(raw), "LIBSVM", 0, out=out)
    assert again.deferred is False and again.rows == ref.rows


# ------------------------------------------------------------------ CRITEO
def _criteo_rows(rows: int, seed: int, eol: str = "\n") -> bytes:
    rng = random.Random(seed)
    lines = []
    for _ in range(rows):
        f = [rng.choice(["0", "1", "-1", "+1", "3"])]
        nf = 39 if rng.random() < 0.7 else rng.randint(0, 38)
        for j in range(nf):
            if rng.random() < 0.2:
                f.append("")
            elif j < 13:
                v = rng.choice([0, -1, -rng.randrange(1 << 20), rng.randrange(100),
                                rng.randrange((1 << 31) - 1), (1 << 31) - 2])
                f.append(str(v))
            else:
                nd = rng.choice([1, 8, 8, 8, 16])
                f.append("".join(rng.choice("0123456789abcdefABCDEF") for _ in range(nd)))
        lines.append("\t".join(f))
    return (eol.join(lines) + eol).encode()


@pytest.mark.parametrize("hash_mod", [0, 10 ** 9])
@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_clean_criteo_not_deferred(hash_mod, eol):
    raw = _criteo_rows(2000, 13, eol)
    got = _check(raw, "CRITEO", hash_mod)
    assert got.rows == 2000 and got.vals is None
    _check(raw[:-len(eol)], "CRITEO", hash_mod)  # (no final newline)


def test_criteo_fixed_width_and_malformed():
    rng = random.Random(2)
    full = "\n".join("1\t" + "\t".join(
        [str(rng.randrange(1000)) for _ in range(13)] +
        [f"{rng.randrange(1 << 32):08x}" for _ in range(26)]) for _ in range(300)) + "\n"
    assert _check(full.encode(), "CRITEO", 1 << 22).width == 39
    for bad in ("\t5\t6", "1\t 5", "1\t5 6", "1\tx", "1" + "\t" * 14 + "xyz", "# note",
                "1\t" + str(1 << 31), "1\t99999999999999999999", "1" + "\t7" * 45, "a\t1"):
        _check((full[:2000] + bad + "\n" + full[:1200]).encode(), "CRITEO", 0, clean=False)


# ------------------------------------------------------------------ base offsets
def test_base_offsets_behind_carried_rows(libsvm_rows):
    a, b = _join(libsvm_rows[:700]), _join(libsvm_rows[700:1500], trailing=False)
    ref = data.parse_text(a + b, "LIBSVM", ignore_slot=True, hash_mod=65536)
    out = TextParseBuffers(2000, 40000, DEV)
    p1 = parse_text_device(_dev(a), "LIBSVM", 65536, out=out)
    p2 = parse_text_device(_dev(b), "LIBSVM", 65536, out=out, row0=p1.rows, nnz0=p1.nnz)
    assert not p1.deferred and not p2.deferred
    rows, nnz = p1.rows + p2.rows, p1.nnz + p2.nnz
    assert (rows, nnz) == (ref.rows, ref.nnz)
    assert np.array_equal(out.row_ptr[:rows + 1].cpu().numpy(), ref.row_ptr)
    assert np.array_equal(out.keys[:nnz].cpu().numpy().view(np.uint64), ref.keys.view(np.uint64))
    assert np.array_equal(out.labels[:rows].cpu().numpy(), ref.labels)
    assert np.array_equal(out.vals[:nnz].cpu().numpy().view(np.uint32), ref.vals.view(np.uint32))
    # a deferred second chunk lands behind the carried rows as well
    p3 = parse_text_device(_dev(b + b"\n1 9:1 3:1\n"), "LIBSVM", 65536, out=out, row0=p1.rows,
                           nnz0=p1.nnz)
    assert p3.deferred and p3.bad_lines == 1 and p3.rows == p2.rows
    assert np.array_equal(out.row_ptr[:rows + 1].cpu().numpy(), ref.row_ptr)
    assert np.array_equal(out.keys[:nnz].cpu().numpy().view(np.uint64), ref.keys.view(np.uint64))


# ------------------------------------------------------------------ the one entry
# three clean lines per format, smallest work space first: every call has to regrow what the
# format before it left behind
SIX = [("ADFEA", b"99 1 1 10:1 20:2\n7 1 0 30:1\n8 1 -3 5:6 4:2 3:1\n"),
       ("TERAFEA", b"1 55 | 18014398509481985 5\n0 56 | 7\n-2 57 | 36028797018963970 8 9\n"),
       ("LIBSVM", b"1 2:0.5 7:1\n-1 3:2\n0 4:1 9:3 11:-2e-3\n"),
       ("CRITEO", b"1\t5\t7\n0\t3\n1\t\t9\t\t12\n"),
       ("SPARSE_BINARY", b"1; 3 5 6; 7 9\n0; 2 4\n-1; 4096 1; 3 2 8\n"),
       ("SPARSE", b"1; 3 5:0.5 6:1; 7 9:-2e-3\n0; 2 4:1\n-1; 1 8:3 9:0.25\n")]
# one line shape per kernel family with 12-digit keys (~2.5 spans of them below)
LONG = {"ADFEA": "{r} 1 1 {a}:3 {b}:7 {c}:3\n", "LIBSVM": "1 {a}:0.5 {b}:1 {c}:-2.25\n",
        "SPARSE_BINARY": "1; 3 {a} {b}; 7 {c}\n"}


def _straddling(fmt: str) -> bytes:
    """40 KiB of clean ``fmt`` lines in which one key lies across byte 16384, the end of the
    first span: the first line's key lengths shift everything behind it."""
    rng = random.Random(7)
    keys = sorted(rng.randrange(10 ** 11, 10 ** 12) for _ in range(3 * 1200))
    body = "".join(LONG[fmt].format(r=r, a=keys[3 * r], b=keys[3 * r + 1], c=keys[3 * r + 2])
                   for r in range(1200))
    for d in range(2, 24):
        first = LONG[fmt].format(r=0, a="1" * (d // 2), b="2" * (d - d // 2), c=10 ** 12)
        raw = (first + body).encode()
        raw = raw[:raw.rindex(b"\n", 0, 40 * 1024) + 1]
        if raw[SPAN - 3:SPAN + 3].isdigit():
            return raw
    raise AssertionError("no key across the span edge")


def test_six_formats_share_one_set_of_buffers():
    from parameter_server_amd.ops.native import hipops

    out = TextParseBuffers(1 << 15, 1 << 15, DEV)
    family = None
    for fmt, raw in SIX:
        t = textparse_traits(fmt)
        need = hipops().textparse_work_words(len(raw), t.id)
        if t.family != family:  # (the first call of a family has to regrow the work space)
            assert out.work is None or out.work.numel() < need
        family = t.family
        got = check_against_host(raw, fmt, 1000, ignore_slot=not t.slots, out=out)
        assert got.rows == 3 and got.out is out and out.work.numel() >= need
    for fmt in LONG:  # ~2.5 spans, one format per family: a token read across the span edge
        raw = _straddling(fmt)
        assert 2 * SPAN < len(raw) <= 40 * 1024
        got = check_against_host(raw, fmt, 0, ignore_slot=not textparse_traits(fmt).slots, out=out)
        assert got.rows > 700 and got.out is out


def test_supported_formats_and_cpu_path():
    assert all(supported(f) for f in ("LIBSVM", "CRITEO", "ADFEA", "TERAFEA", "SPARSE",
                                      "SPARSE_BINARY"))
    assert not supported("DENSE") and not supported("VW")
    for fmt, line in (("DENSE", b"1 2 3\n"), ("VW", b"1 |a x:2\n")):
        with pytest.raises(ValueError):
            parse_text_device(_dev(line), fmt)
    got = parse_text_device(torch.frombuffer(bytearray(b"1 2 | 3\n"), dtype=torch.uint8), "TERAFEA")
    assert got.rows == 1 and not got.keys.is_cuda
    v = torch.tensor([1, 1, 2, 1, 1, 1, 0.5], device=DEV)
    b = torch.tensor([0, 2, 3, 6, 6, 7], device=DEV)
    assert segments_valued(v, b).tolist() == [0, 1, 0, 0, 1]


# ------------------------------------------------------------------ feeder
def _feed(files, parser, *, minibatch=1000, max_nnz=30000, cache_dir=None, passes=2, **kw):
    from parameter_server_amd.data.feeder import DeviceFeeder

    f = DeviceFeeder(files, "LIBSVM", minibatch, max_nnz, DEV, num_features=1 << 22,
                     passes=passes, shuffle=True, seed=5, parser=parser, chunk_bytes=65536,
                     cache_dir=cache_dir, **kw)
    out = []
    for b in f:
        torch.cuda.current_stream().synchronize()
        rp = b.row_ptr.cpu().numpy() if b.row_ptr is not None else None
        if rp is None:  # omitted for fixed-width minibatches: the offsets are arithmetic
            assert b.width > 0
            rp = np.arange(0, (b.rows + 1) * b.width, b.width, dtype=np.int64)
        out.append((b.rows, b.nnz, b.width, b.keys.cpu().numpy().copy(),
                    b.labels.cpu().numpy().copy(), rp,
                    None if b.vals is None else b.vals.cpu().numpy().copy()))
        f.release(b)
    return f, out


def _same_batches(a, b, width=True):
    assert [x[:3 if width else 2] for x in a] == [x[:3 if width else 2] for x in b]
    for x, y in zip(a, b):
        for u, v in zip(x[3:], y[3:]):
            assert (u is None) == (v is None)
            if u is not None:
                assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8))


def _write_rows(path, rows):
    with open(path, "wb") as f:
        f.write(_join(rows))


def test_feeder_matches_cpu_parser_binary_files(tmp_path):
    """Files of 2,500, 1 and 4,100 rows (variable widths, one file fixed width 39, all
    "k:1"), a row longer than a chunk, minibatches cut by rows and by features, two
    shuffled passes, then the cache the GPU pass left behind."""
    from parameter_server_amd.data import bincache

    rng = random.Random(17)

    def row(w):
        return (rng.choice(["1", "-1"]), [f"{i}:1" for i in sorted(rng.sample(range(1 << 30), w))])

    a = [row(rng.randint(0, 60)) for _ in range(2500)]
    a[1234] = row(9000)  # ~100 KB of text: longer than a 64 KiB chunk
    files = []
    for name, rows in (("a", a), ("b", [row(7)]), ("c", [row(39) for _ in range(4100)])):
        files.append(str(tmp_path / f"part-{name}"))
        _write_rows(files[-1], rows)
    _, ref = _feed(files, "cpu")
    f, got = _feed(files, "gpu")
    assert f.parser == "gpu" and f.text_passes == 2
    _same_batches(got, ref)
    assert sum(x[0] for x in got) == 2 * 6601
    assert any(x[0] < 1000 and x[1] > 20000 for x in got)  # cut by features
    assert any(x[2] == 39 for x in got) and any(x[2] == 0 for x in got)
    assert all(x[6] is None for x in got)
    assert f.deferred_chunks == 2  # the long row's chunk, once per pass
    assert f.text_chunks > 2 * 12 and f.bytes_text == 2 * sum(os.path.getsize(p) for p in files)
    # with a cache directory: the GPU text pass leaves valid caches, the next pass streams them
    cache = str(tmp_path / "cache")
    f2, got2 = _feed(files, "gpu", cache_dir=cache)
    assert f2.text_passes == 1 and f2.cached_passes == 1
    # (a cached pass reports one width for the whole run, 0 here: the arrays are the same)
    _same_batches(got2, ref, width=False)
    for p in files:
        cf = bincache.open_valid(p, cache, "LIBSVM", 5, 1 << 22, True)
        assert cf is not None
        cf.close()
    _, ref3 = _feed(files, "cpu", cache_dir=str(tmp_path / "cache_cpu"))
    _same_batches(got2, ref3)
    for p in files:  # the two parsers leave the same cache bytes behind
        pa = bincache.cache_path(cache, p, "LIBSVM", 1 << 22, True)
        pb = bincache.cache_path(str(tmp_path / "cache_cpu"), p, "LIBSVM", 1 << 22, True)
        assert open(pa, "rb").read() == open(pb, "rb").read()


def test_feeder_matches_cpu_parser_valued_files(tmp_path, libsvm_rows):
    files = []
    # (the one-row file holds a value other than 1: the CPU path drops the values of a
    # minibatch that joins a valued file with an all-"k:1" one)
    one = next(i for i in range(1300, 3000)
               if any(not f.endswith(":1") for f in libsvm_rows[i][1]))
    for k, rows in enumerate((libsvm_rows[:1300], libsvm_rows[one:one + 1], libsvm_rows[1301:])):
        files.append(str(tmp_path / f"part-{k}"))
        _write_rows(files[-1], rows)
    _, ref = _feed(files, "cpu", minibatch=500, max_nnz=6000)
    f, got = _feed(files, "auto", minibatch=500, max_nnz=6000)
    assert f.parser == "gpu" and f.deferred_chunks == 0
    _same_batches(got, ref)
    assert all(x[6] is not None for x in got) and any(x[0] < 500 for x in got[:-1])


def test_feeder_leftover_rows_of_one_width(tmp_path):
    """The rows left at the end of the pass all have one width while the chunk they were
    parsed in does not (their offsets still come from the chunk's row_ptr)."""
    rng = random.Random(23)

    def row(w):
        return ("1", [f"{i}:0.5" for i in sorted(rng.sample(range(1 << 20), w))])

    p = str(tmp_path / "part-0")
    _write_rows(p, [row(rng.randint(0, 6)) for _ in range(700)] + [row(3) for _ in range(300)])
    assert os.path.getsize(p) < 65536  # one chunk
    _, ref = _feed([p], "cpu", minibatch=400, passes=1)
    f, got = _feed([p], "gpu", minibatch=400, passes=1)
    assert f.text_chunks == 1 and [x[0] for x in got] == [400, 400, 200] and got[-1][2] == 3
    _same_batches(got, ref)


def test_feeder_falls_back_where_there_is_no_device_parser(tmp_path):
    from parameter_server_amd.data.feeder import DeviceFeeder

    p = tmp_path / "t"
    p.write_text("1 5 | 11 12\n0 6 | 13\n")
    f = DeviceFeeder([str(p)], "TERAFEA", 10, 100, DEV, parser="gpu")
    assert f.parser == "cpu" and sum(b.rows for b in f) == 2
    f = DeviceFeeder([str(p)], "LIBSVM", 10, 100, DEV, parser="auto", max_lines_per_file=1)
    assert f.parser == "cpu"


# ------------------------------------------------------------------ app
def _write_app_libsvm(d, nfiles=3, rows=600, seed=0, nkeys=3000):
    """The generator of tests/test_app_gpu.py's single-GPU case (valued, variable width)."""
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 1, nkeys) * (rng.random(nkeys) < 0.2)
    os.makedirs(d, exist_ok=True)
    for p in range(nfiles):
        with open(os.path.join(d, f"part-{p}"), "w") as f:
            for _ in range(rows):
                k = np.unique(rng.integers(1, nkeys, size=int(rng.integers(5, 40))))
                v = rng.random(k.size)
                y = 1 if (w[k] * v).sum() + 0.2 * rng.normal() > 0 else -1
                f.write(f"{y} " + " ".join(f"{a}:{b:.4f}" for a, b in zip(k, v)) + "\n")


def _read_model(path):
    out = {}
    with open(path) as f:
        for ln in f:
            k, w = ln.split("\t")
            out[int(k)] = float(w)
    return out


@pytest.mark.parametrize("num_features", [0, 1 << 12])
def test_app_parser_gpu_matches_parser_cpu(tmp_path, num_features):
    from parameter_server_amd.app.gpu import _flags, run_async_sgd
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    data_dir = tmp_path / "data"
    _write_app_libsvm(str(data_dir))
    models = {}
    for parser in ("gpu", "cpu"):
        model = tmp_path / f"model_{parser}" / "m"
        conf = tmp_path / f"{parser}.conf"
        conf.write_text(f"""linear_method {{
training_data {{ format: TEXT text: LIBSVM file: "{data_dir}/part.*" }}
model_output {{ format: TEXT file: "{model}" }}
loss {{ type: LOGIT }}
penalty {{ type: L1 lambda: 0.05 lambda: 0.01 }}
learning_rate {{ type: DECAY alpha: 0.5 beta: 1 }}
async_sgd {{ algo: FTRL minibatch: 200 num_data_pass: 1 max_delay: 0 report_interval: 1 }}
}}""")
        flags = _flags(["-app_file", str(conf), "-num_features", str(num_features),
                        "-num_threads", "2", "-device", "cuda", "-table_capacity", str(1 << 16),
                        "-quiet", "-parser", parser, "-data_cache", "off"])
        dev = torch.device("cuda")
        res = run_async_sgd(load_app_config(str(conf)).linear_method, LocalComm(dev), dev, flags)
        assert res["examples"] == 1800 and res["steps"] == 9
        assert res["parser"] == parser
        if parser == "gpu":
            assert res["deferred_chunks"] == 0 and res["text_chunks"] == 3
        models[parser] = _read_model(res["model"])
    g, c = models["gpu"], models["cpu"]
    assert set(g) == set(c) and len(g) > 50
    keys = sorted(g)
    np.testing.assert_allclose([g[k] for k in keys], [c[k] for k in keys], rtol=1e-4, atol=1e-5)
