"""The device parser of the slot-grouped text formats (pstext.hip, ops/textparse.py) against
the host parser on the same bytes: labels, row offsets, keys and slot ids bitwise, values
bitwise or None by the host's binary rule, bad-line and row counts -- on clean corpora
(which must not be deferred to the host), at every boundary of the work decomposition, on
every kind of line the kernels hand back, on random bytes, behind carried rows, through the
DeviceFeeder, the file-fed app and the SlotReader."""
import functools
import os
import random
import re

import numpy as np
import pytest
import torch

from parameter_server_amd import data
from parameter_server_amd.ops import textparse
from parameter_server_amd.ops.native import core
from parameter_server_amd.ops.textparse import TextParseBuffers, parse_text_device
from textparse_cases import _dev, check_against_host

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPAN = 16384  # bytes of text per workgroup (textparse.cuh)
FMTS = ["SPARSE_BINARY", "SPARSE"]
_check = functools.partial(check_against_host, ignore_slot=False)


# ------------------------------------------------------------------ corpora
def _val(rng) -> str:
    """A value inside the exact domain of csrc/core/textnum.h."""
    k = rng.randrange(5)
    if k == 0:
        return "1"
    if k == 1:
        return rng.choice(["", "-", "+"]) + f"{rng.randrange(500)}.{rng.randrange(100):02d}"
    if k == 2:
        return (rng.choice(["", "-"]) + f"{rng.randrange(1, 10)}.{rng.randrange(100):02d}"
                + rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randrange(0, 7)))
    if k == 3:
        return f"0.{rng.randrange(1, 10 ** 6):06d}"
    return str(rng.randrange(0, 30000))


def _rows(n: int, seed: int, valued: bool, ones: bool = False):
    """[(label, [(group id, [feature token, ...]), ...])]: 1-40 groups of 1-30 keys, mostly
    few and short so that the corpus stays a few hundred KB."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        ng = rng.randint(1, 40) if rng.random() < 0.04 else rng.randint(1, 4)
        groups = []
        for _ in range(ng):
            nk = rng.randint(1, 30) if rng.random() < 0.05 else rng.randint(1, 4)
            feats = []
            for _ in range(nk):
                r = rng.random()
                key = (1 << 64) - 1 if r < 0.02 else rng.randrange(1 << 64) if r < 0.3 else \
                    rng.randrange(1 << 20)
                feats.append(f"{key}:{'1' if ones else _val(rng)}" if valued else str(key))
            groups.append((rng.randrange(4096), feats))
        out.append((rng.choice(["0", "1", "-1", "+1"]), groups))
    return out


STYLES = [(" ", "; ", False, "\n"), ("\t", ";", True, "\n"), ("  ", "; ", True, "\r\n"),
          (" ", ";", False, "\r\n")]  # separator, group delimiter, trailing ';', line end


def _join(rows, sep=" ", gd="; ", trail=False, eol="\n", last_eol=True) -> bytes:
    lines = []
    for lab, groups in rows:
        s = gd.join([lab] + [sep.join([str(g)] + feats) for g, feats in groups])
        lines.append(s + (";" if trail else ""))
    return (eol.join(lines) + (eol if last_eol else "")).encode()


@pytest.fixture(scope="module")
def corpora():
    out = {}
    for fmt in FMTS:
        rows = _rows(2000, 7 if fmt == "SPARSE" else 8, fmt == "SPARSE")
        if fmt == "SPARSE":  # clean: no value the shared scanner would defer or reject
            toks = [f.split(":")[1].encode() for _, gs in rows for _, fs in gs for f in fs]
            _, st = core().textnum_f32(toks)
            assert not st.any()
        assert max(len(gs) for _, gs in rows) > 30
        assert max(len(fs) for _, gs in rows for _, fs in gs) > 25
        out[fmt] = rows
    return out


@pytest.mark.parametrize("ignore_slot", [True, False])
@pytest.mark.parametrize("hash_mod", [0, 65536, 10 ** 9])
@pytest.mark.parametrize("fmt", FMTS)
def test_clean_corpora_not_deferred(corpora, fmt, hash_mod, ignore_slot):
    for k, (sep, gd, trail, eol) in enumerate(STYLES):
        raw = _join(corpora[fmt], sep, gd, trail, eol, last_eol=k != 1)
        assert 3 * SPAN < len(raw) < 900_000
        got = _check(raw, fmt, hash_mod, ignore_slot=ignore_slot)
        assert got.rows == 2000 and (got.vals is not None) == (fmt == "SPARSE")


def test_all_ones_sparse_has_no_values():
    raw = _join(_rows(600, 3, True, ones=True))
    assert len(raw) > 2 * SPAN
    got = _check(raw, "SPARSE", 0)
    assert got.vals is None and got.valued


# ------------------------------------------------------------------ decomposition
def _short_lines(total: int, seed: int, valued: bool) -> bytes:
    """Exactly ``total`` bytes of short lines: whole tokens only, the rest filled with
    blanks (the last line may lack its newline or its last groups)."""
    rng = random.Random(seed)
    out = bytearray()
    while True:
        toks = [rng.choice(["1", "0", "-1"])]
        for _ in range(rng.randint(1, 3)):
            toks.append(rng.choice([";", "; "]) + str(rng.randrange(4096)))
            for _ in range(rng.randint(1, 3)):
                k = rng.randrange(10 ** 3, 10 ** 7)
                toks.append(f" {k}:{rng.choice(['1', '0.25', '3'])}" if valued else f" {k}")
        toks.append(rng.choice(["\n", ";\n"]))
        for t in toks:
            if len(out) + len(t) > total:
                return bytes(out) + b" " * (total - len(out))
            out += t.encode()


def test_empty_and_blank_buffers():
    for fmt in FMTS:
        for raw in (b"", b"\n\n\n", b"\n", b" \t \r\n\r\n", b"1", b"-1\n", b"1;", b"1;;\n"):
            got = _check(raw, fmt)
            assert got.nnz == 0
    assert _check(b"1; 3 4 5", "SPARSE_BINARY").nnz == 2
    assert _check(b"0;7 4:0.5", "SPARSE").rows == 1


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("spans", [1, 2])
def test_lengths_around_span_edges(fmt, spans):
    for d in range(-17, 18):
        total = spans * SPAN + d
        _check(_short_lines(total, total, fmt == "SPARSE"), fmt, 65536)
    # lines shift by one byte per case: every alignment of a token start, a token end, a
    # ';' and a newline against the span edge occurs
    base = _short_lines(spans * SPAN + 64, 5, fmt == "SPARSE")
    for shift in range(48):
        _check(b" " * shift + base, fmt, ignore_slot=bool(shift & 1))


@pytest.mark.parametrize("spans", [1, 2])
def test_each_token_class_on_both_sides_of_a_span_edge(spans):
    line = b"1; 77 123 456; 9 5\n"
    at = {"label": 0, "semicolon": 1, "head": 3, "feature": 6, "second semicolon": 13,
          "second head": 15}
    filler = _short_lines(spans * SPAN - 200, 31, False)
    filler = filler[:filler.rfind(b"\n") + 1]
    tail = _short_lines(300, 32, False)
    for name, off in at.items():
        for edge in (spans * SPAN - 1, spans * SPAN):  # the last byte of a span, the first
            pad = edge - off - len(filler)
            assert pad > 0
            raw = filler + b" " * (pad - 1) + b"\n" + line + tail
            assert raw[edge:edge + 1] == line[off:off + 1], name
            for ignore_slot in (False, True):
                _check(raw, "SPARSE_BINARY", ignore_slot=ignore_slot)


@pytest.mark.parametrize("fmt", FMTS)
def test_one_group_longer_than_two_spans(fmt):
    rng = random.Random(11)
    n = 5000
    feats = [f"{rng.randrange(1 << 40)}" + (f":{_val(rng)}" if fmt == "SPARSE" else "")
             for _ in range(n)]
    v = ":2" if fmt == "SPARSE" else ""
    long_line = (f"1; 17 4{v}; 4001 " + " ".join(feats) + f"; 5 6{v}\n").encode()
    assert len(long_line) > 2 * SPAN + 4000
    valued = fmt == "SPARSE"
    raw = _short_lines(3000, 1, valued) + b"\n" + long_line + _short_lines(3000, 2, valued) + b"\n"
    got = _check(raw, fmt, 10 ** 9)
    assert int(np.diff(got.row_ptr.cpu().numpy()).max()) == n + 2
    assert int((got.slots == 4001).sum()) == n  # the gather reached across the spans


def test_many_one_token_lines():
    got = _check(b"1\n" * 20000 + b"0\n-1", "SPARSE_BINARY")
    assert got.rows == 20002 and got.nnz == 0


# ------------------------------------------------------------------ deferring lines
DEFER_BOTH = ["1; 3 " + "9" * 70, "#c; 1 2", "  #c; 1 2", "1 2; 3 4", "1 2", "1 2 3", ";", "; 1 2",
              "  ;", "\t; 3 4; 5 6", "1x 2; 3 4"]
DEFER_BINARY = ["1; 3 4:5", "1; 3 4: 5", "1; 3 :4", "1; 3 4:"]
DEFER_SPARSE = ["1; 3 4 : 5", "1; 3 4:", "1; 3 :5", "1; 3 4:5:6", "1; 3 4", "1; 3 4:5 6",
                "1; 3 4:0.12345678901234567", "1; 3 4:1e400", "1; 3 4:nan"]
DEFER_SLOTS = ["1; x 2 3", "1; -1 2", "1; 2147483648 2", "1; 1.5 2", "1; 3:4 5"]
EXTRA = ["1;;2 3", "1; 5;", "#c; 1 2", "1.0; 1 2", "1; 1 99999999999999999999",
         "1; 1 " + "7" * 70, "1; 2 18446744073709551616", "1;", "+1;4 0", "1 ;3 4", "1\t; 3 4",
         "-0; 3 4", "1; 3 4;; ;5 6; ", "x; 1 2", "1; 3 -4"]


def _feat(s: str, fmt: str) -> str:
    """A SPARSE_BINARY line's plain keys as SPARSE features (heads and labels untouched)."""
    if fmt != "SPARSE":
        return s
    lab, *groups = s.split(";")
    out = [lab]
    for g in groups:
        t = g.split()
        out.append(" ".join(t[:1] + [f"{k}:1" if k.isdigit() else k for k in t[1:]]))
    return "; ".join(out) if len(out) > 1 else s


@pytest.mark.parametrize("fmt", FMTS)
def test_deferring_and_malformed_lines(corpora, fmt):
    good = _join(corpora[fmt][:60]).decode().splitlines()
    rng = random.Random(5)
    own = DEFER_BINARY if fmt == "SPARSE_BINARY" else DEFER_SPARSE
    cases = [(_feat(b, fmt), True, None) for b in DEFER_BOTH] + [(b, True, None) for b in own] + \
        [(_feat(b, fmt), True, False) for b in DEFER_SLOTS] + \
        [(_feat(b, fmt), False, None) for b in EXTRA]
    for bad, must_defer, slot_mode in cases:
        lines = list(good)
        lines.insert(rng.randrange(len(lines) + 1), bad)
        raw = ("\n".join(lines) + "\n").encode()
        for ignore_slot in ((True, False) if slot_mode is None else (slot_mode,)):
            got = _check(raw, fmt, 65536, ignore_slot=ignore_slot, clean=False)
            if must_defer:
                assert got.deferred is True, bad
    whole = ("\n".join(good + [c[0] for c in cases]) + "\n").encode()
    got = _check(whole, fmt, 0, clean=False)
    assert got.deferred and got.bad_lines > 5


def test_unread_group_heads():
    # without slots nobody reads the head: "x" heads a clean group; with slots it is a bad line
    raw = b"1; 7 8\n1; x 2 3\n0; 9 1\n"
    got = _check(raw, "SPARSE_BINARY", ignore_slot=True)
    assert got.deferred is False and got.keys.cpu().tolist() == [8, 2, 3, 1]
    got = _check(raw, "SPARSE_BINARY", ignore_slot=False, clean=False)
    assert got.deferred and got.bad_lines == 1 and got.rows == 2
    got = _check(b"1; 3:4 2:0.5 3:1\n", "SPARSE", ignore_slot=True)
    assert got.deferred is False and got.keys.cpu().tolist() == [2, 3]


@pytest.mark.parametrize("ignore_slot", [True, False])
@pytest.mark.parametrize("fmt", FMTS)
def test_random_bytes(fmt, ignore_slot):
    rng = random.Random(99 + ignore_slot)
    alphabet = "0123456789;: \t\r\n-+.e#"
    raw = "".join(rng.choice(alphabet) for _ in range(65536)).encode()
    got = _check(raw, fmt, 65536, ignore_slot=ignore_slot, clean=False)
    rp = got.row_ptr.cpu().numpy()
    assert rp[0] == 0 and rp[-1] == got.nnz and (np.diff(rp) >= 0).all()
    # sparser noise: mostly well-formed tokens, some lines parse
    rng = random.Random(7 + ignore_slot)
    toks = ["1", "0", "12", "345:1", "7:0.5", ";", "; ", " ", " ", "\n", "\n", "\t", "\r\n", ":",
            "#", "-1", "+1", "1e3", "6 7"]
    raw = "".join(rng.choice(toks) for _ in range(30000)).encode()
    _check(raw, fmt, 0, ignore_slot=ignore_slot, clean=False)


# ------------------------------------------------------------------ buffers
@pytest.mark.parametrize("fmt", FMTS)
def test_output_capacity_overflow_defers(corpora, fmt):
    raw = _join(corpora[fmt][:400])
    ref = data.parse_text(raw, fmt, ignore_slot=False)
    out = TextParseBuffers(100, 50, DEV)  # too small for 400 rows
    got = parse_text_device(_dev(raw), fmt, 0, ignore_slot=False, out=out)
    assert got.deferred and got.rows == ref.rows and got.nnz == ref.nnz
    assert np.array_equal(got.keys.cpu().numpy().view(np.uint64), ref.keys.view(np.uint64))
    assert np.array_equal(got.slots.cpu().numpy(), ref.slots)
    # the sticky flag was cleared: the grown buffers parse on the device again
    again = parse_text_device(_dev(raw), fmt, 0, ignore_slot=False, out=out)
    assert again.deferred is False and again.rows == ref.rows
    assert np.array_equal(again.slots.cpu().numpy(), ref.slots)


@pytest.mark.parametrize("fmt", FMTS)
def test_base_offsets_behind_carried_rows(corpora, fmt):
    rows = corpora[fmt]
    a, b = _join(rows[:300]), _join(rows[300:700], last_eol=False)
    ref = data.parse_text(a + b, fmt, ignore_slot=False, hash_mod=65536)
    out = TextParseBuffers(1000, 40000, DEV)
    p1 = parse_text_device(_dev(a), fmt, 65536, ignore_slot=False, out=out)
    p2 = parse_text_device(_dev(b), fmt, 65536, ignore_slot=False, out=out, row0=p1.rows,
                              nnz0=p1.nnz)
    assert not p1.deferred and not p2.deferred
    n_rows, nnz = p1.rows + p2.rows, p1.nnz + p2.nnz
    assert (n_rows, nnz) == (ref.rows, ref.nnz)

    def same():
        assert np.array_equal(out.row_ptr[:n_rows + 1].cpu().numpy(), ref.row_ptr)
        assert np.array_equal(out.keys[:nnz].cpu().numpy().view(np.uint64),
                              ref.keys.view(np.uint64))
        assert np.array_equal(out.labels[:n_rows].cpu().numpy(), ref.labels)
        assert np.array_equal(out.slots[:nnz].cpu().numpy(), ref.slots)
        if fmt == "SPARSE":
            assert np.array_equal(out.vals[:nnz].cpu().numpy().view(np.uint32),
                                  ref.vals.view(np.uint32))

    same()
    # a deferred second chunk lands behind the carried rows as well
    p3 = parse_text_device(_dev(b + b"\n; 9 3\n"), fmt, 65536, ignore_slot=False, out=out,
                              row0=p1.rows, nnz0=p1.nnz)
    assert p3.deferred and p3.bad_lines == 1 and p3.rows == p2.rows
    same()


def test_supported_formats():
    names = ("DENSE", "SPARSE", "SPARSE_BINARY", "ADFEA", "LIBSVM", "TERAFEA", "VW", "CRITEO")
    for k, f in enumerate(names, 1):
        on = f not in ("DENSE", "VW")
        assert textparse.supported(f) == textparse.supported(k) == on
        assert (textparse.traits(f) is not None) == on
        if on:
            t = textparse.traits(f)
            assert t == textparse.traits(k) and t.id == k == data.TEXT_FORMATS[f]
            assert t.valued == (f in ("LIBSVM", "SPARSE"))
            assert t.slots == (f in ("SPARSE", "SPARSE_BINARY", "ADFEA", "TERAFEA"))
        assert textparse.produces_slots(f) == textparse.produces_slots(k) == \
            (f in ("SPARSE", "SPARSE_BINARY", "ADFEA", "TERAFEA"))
    with pytest.raises(ValueError):
        parse_text_device(_dev(b"1 2:3\n"), "LIBSVM", ignore_slot=False)
    with pytest.raises(ValueError):
        parse_text_device(_dev(b"1\t2\t3\n"), "CRITEO", ignore_slot=False)
    with pytest.raises(KeyError):
        parse_text_device(_dev(b"1; 2 3\n"), "NOPE")


# ------------------------------------------------------------------ feeder
def _slot_data(fmt, rows, seed):
    from parameter_server_amd.data.synthetic import sparse_classification

    return sparse_classification(rows, groups=(1, 2, 3, 4, 5), keys_per_group=3000,
                                 nnz_per_row=(1, 3, 5, 2, 4), binary=fmt == "SPARSE_BINARY",
                                 seed=seed)


def _feed(files, fmt, parser, *, cache_dir=None, passes=2):
    from parameter_server_amd.data.feeder import DeviceFeeder

    f = DeviceFeeder(files, fmt, 500, 6000, DEV, num_features=1 << 22, passes=passes,
                     shuffle=True, seed=5, parser=parser, chunk_bytes=16384, cache_dir=cache_dir)
    out = []
    for b in f:
        torch.cuda.current_stream().synchronize()
        rp = b.row_ptr.cpu().numpy() if b.row_ptr is not None else \
            np.arange(0, (b.rows + 1) * b.width, b.width, dtype=np.int64)
        out.append((b.rows, b.nnz, b.keys.cpu().numpy().copy(), b.labels.cpu().numpy().copy(), rp,
                    None if b.vals is None else b.vals.cpu().numpy().copy()))
        f.release(b)
    return f, out


def _same_batches(a, b):
    assert [x[:2] for x in a] == [x[:2] for x in b]
    for x, y in zip(a, b):
        for u, v in zip(x[2:], y[2:]):
            assert (u is None) == (v is None)
            if u is not None:
                assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8))


@pytest.mark.parametrize("fmt", FMTS)
def test_feeder_matches_cpu_parser(tmp_path, fmt):
    from parameter_server_amd.data.synthetic import write_text

    files = []
    for k, rows in enumerate((1300, 1, 900)):
        files.append(str(tmp_path / f"part-{k}"))
        write_text(_slot_data(fmt, rows, 40 + k), files[-1], fmt)
    assert os.path.getsize(files[0]) > 4 * 16384  # several chunks per file
    _, ref = _feed(files, fmt, "cpu")
    f, got = _feed(files, fmt, "gpu")
    assert f.parser == "gpu" and f.text_passes == 2 and f.deferred_chunks == 0
    assert f.text_chunks > 2 * 6
    assert sum(x[0] for x in got) == 2 * 2201
    _same_batches(got, ref)
    assert all((x[5] is None) == (fmt == "SPARSE_BINARY") for x in got)
    # with a cache directory the second pass streams the cache the GPU text pass left behind
    f2, got2 = _feed(files, fmt, "gpu", cache_dir=str(tmp_path / "cache"))
    assert f2.parser == "gpu" and f2.text_passes == 1 and f2.cached_passes == 1
    assert f2.deferred_chunks == 0
    _, ref2 = _feed(files, fmt, "cpu", cache_dir=str(tmp_path / "cache_cpu"))
    _same_batches(got2, ref2)
    _same_batches(got2[:len(ref) // 2], ref[:len(ref) // 2])


# ------------------------------------------------------------------ app
def test_app_parser_gpu_matches_parser_cpu_on_a_ctr_conf(tmp_path):
    from parameter_server_amd.app.gpu import _flags, run_async_sgd
    from parameter_server_amd.data.synthetic import write_text
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    data_dir = tmp_path / "data"
    os.makedirs(data_dir)
    for p in range(3):
        write_text(_slot_data("SPARSE_BINARY", 600, 60 + p), str(data_dir / f"part-{p}"))
    golden = open(os.path.join(os.path.dirname(__file__), "golden", "confs",
                               "online_ftrl.conf")).read()
    models = {}
    for parser in ("gpu", "cpu"):
        model = tmp_path / f"model_{parser}" / "m"
        conf = tmp_path / f"{parser}.conf"
        text = re.sub(r"training_data \{.*?\}", lambda m: "training_data { format: TEXT text: "
                      f'SPARSE_BINARY file: "{data_dir}/part.*" }}', golden, flags=re.S)
        text = text.replace('"out/online_ftrl"', f'"{model}"')
        assert "SPARSE_BINARY" in text and str(model) in text
        conf.write_text(text)
        flags = _flags(["-app_file", str(conf), "-num_features", str(1 << 20), "-num_threads", "2",
                        "-device", "cuda", "-table_capacity", str(1 << 16), "-quiet",
                        "-parser", parser, "-data_cache", "off"])
        dev = torch.device("cuda")
        res = run_async_sgd(load_app_config(str(conf)).linear_method, LocalComm(dev), dev, flags)
        assert res["examples"] == 2 * 1800 and res["text_passes"] == 2
        assert res["parser"] == parser
        if parser == "gpu":
            assert res["deferred_chunks"] == 0 and res["text_chunks"] == 6
        models[parser] = open(res["model"], "rb").read()
    assert len(models["gpu"].splitlines()) > 20
    assert models["gpu"] == models["cpu"]


# ------------------------------------------------------------------ SlotReader
@pytest.mark.parametrize("fmt", FMTS)
def test_slot_reader_device_route_matches_host_route(tmp_path, fmt):
    from parameter_server_amd.data.slot_reader import SlotReader
    from parameter_server_amd.data.synthetic import sparse_groups, write_text
    from parameter_server_amd.models.darlin import DarlinConfig, DarlinTrainer

    files = []
    for k in range(2):
        sd = sparse_groups(1500, groups=5, present=3, keys_per_group=500, seed=70 + k)
        if fmt == "SPARSE":
            rng = np.random.default_rng(k)
            sd.groups = {g: (o, kk, rng.integers(1, 9, kk.size).astype(np.float32) / 4)
                         for g, (o, kk, _) in sd.groups.items()}
        assert len(sd.groups) == 5 and any((np.diff(o) == 0).any() for o, _, _ in sd.groups.values())
        files.append(str(tmp_path / f"part-{k}"))
        write_text(sd, files[-1], fmt)

    def same(a, b):
        assert np.array_equal(a.labels, b.labels) and sorted(a.groups) == sorted(b.groups)
        for g in a.groups:
            for u, v in zip(a.groups[g], b.groups[g]):
                assert (u is None) == (v is None)
                if u is not None:
                    assert u.dtype == v.dtype and np.array_equal(u, v)

    host = SlotReader(files, fmt, parser="cpu").read()
    r = SlotReader(files, fmt, parser="gpu", device=DEV)
    assert r.parser == "gpu"
    dev = r.read()
    assert r.deferred_chunks == 0 and dev.rows == 3000 and len(dev.groups) == 5
    same(dev, host)
    assert SlotReader(files, "LIBSVM", parser="gpu", device=DEV).parser == "cpu"
    # (measured no faster than the host route: "auto" does not choose it)
    assert SlotReader(files, fmt, parser="auto", device=DEV).parser == "cpu"
    # with a cache: the device route stores what the host route stores; a second read hits it
    rc = SlotReader(files, fmt, cache_prefix=str(tmp_path / "cg") + "/", parser="gpu", device=DEV)
    same(rc.read(), host)
    assert rc.hit_cache == 0
    same(rc.read(), host)
    assert rc.hit_cache == 2
    hc = SlotReader(files, fmt, cache_prefix=str(tmp_path / "ch") + "/", parser="cpu")
    hc.read()
    for name in sorted(os.listdir(tmp_path / "ch")):
        if name.endswith(".npy"):
            assert open(tmp_path / "ch" / name, "rb").read() == \
                open(tmp_path / "cg" / name, "rb").read(), name
    # one Darlin pass from each route
    cfg = DarlinConfig(l1=1.0, max_pass=1, seed=0)
    ph = DarlinTrainer(host, cfg).train()
    pd = DarlinTrainer(dev, cfg).train()
    assert [p.objective for p in pd] == [p.objective for p in ph]
