"""The device parser of the CTR log formats ADFEA / TERAFEA (adtext.hip, ops/textparse.py)
against the host parser on the same bytes: labels, row offsets, keys and slot ids bitwise,
bad-line and row counts -- on clean corpora (which must not be deferred to the host), at
every boundary of the work decomposition, on every kind of line the kernels hand back, on
random bytes, behind carried rows, through the DeviceFeeder, the SlotReader and the app."""
import functools
import os
import random
import re

import numpy as np
import pytest
import torch

from parameter_server_amd import data
from parameter_server_amd.ops.textparse import TextParseBuffers, parse_text_device
from textparse_cases import _dev, check_against_host

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPAN = 16384  # bytes of text per workgroup (textparse.cuh)
FMTS = ["ADFEA", "TERAFEA"]
_check = functools.partial(check_against_host, ignore_slot=False)


def _on_defer_list(raw: bytes, fmt: str, ignore_slot: bool) -> bool:
    """Whether ``raw`` holds anything the device parser hands back (the list of adtext.hip),
    decided here on the CPU, token by token."""
    seps = " :\t\r" if fmt == "ADFEA" else " \t\r"
    for line in raw.decode("latin-1").split("\n"):
        toks = re.split("[" + seps + "]+", line.strip(seps))
        toks = [t for t in toks if t]
        if not toks:
            if line.strip(" \t\r"):
                return True  # (ADFEA: colons only)
            continue
        if fmt == "ADFEA" and line.lstrip(" \t\r").startswith(":"):
            return True
        if any(len(t) > 64 for t in toks) or toks[0].startswith("#") or len(toks) < 3:
            return True
        if fmt == "ADFEA" and len(toks) % 2 == 0:
            return True
        label = toks[2] if fmt == "ADFEA" else toks[0]
        if not re.fullmatch(r"\+?-?\d+", label) or not -(1 << 63) <= int(label) < (1 << 63):
            return True
        rest = toks[3:]
        keys = rest[0::2] if fmt == "ADFEA" else rest
        if any(not re.fullmatch(r"\d+", k) or int(k) >= 1 << 64 for k in keys):
            return True
        if fmt == "ADFEA" and not ignore_slot:
            if any(not re.fullmatch(r"\+?\d+", g) or int(g) >= 1 << 31 for g in rest[1::2]):
                return True
    return False


# ------------------------------------------------------------------ corpora
def _rows(n: int, seed: int, fmt: str):
    """[(label, [(key, group), ...])]: 0-40 entries, mostly few; keys up to 2^64 - 1 (for
    TERAFEA the group is the key's top 10 bits)."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        r = rng.random()
        w = 0 if r < 0.1 else rng.randint(20, 40) if r < 0.15 else rng.randint(1, 6)
        ents = []
        for _ in range(w):
            r = rng.random()
            key = (1 << 64) - 1 if r < 0.02 else rng.randrange(1 << 64) if r < 0.4 else \
                rng.randrange(1 << 20)
            grp = rng.choice([0, (1 << 31) - 1, rng.randrange(4096)]) if fmt == "ADFEA" else key >> 54
            ents.append((key, grp))
        out.append((rng.choice(["0", "1", "-1", "+1", "7"]), ents))
    return out


# separator, ADFEA key/group joint, line end
STYLES = [(" ", ":", "\n"), ("\t", ":", "\n"), ("  ", ":", "\r\n"), (" ", "\t", "\r\n")]


def _join(rows, fmt, sep=" ", joint=":", eol="\n", last_eol=True, first_id=0) -> bytes:
    lines = []
    for i, (lab, ents) in enumerate(rows, first_id):
        if fmt == "ADFEA":
            toks = [str(i), "1", lab] + [f"{k}{joint}{g}" for k, g in ents]
        else:
            toks = [lab, str(i), "|"] + [str(k) for k, _ in ents]
        lines.append(sep.join(toks))
    return (eol.join(lines) + (eol if last_eol else "")).encode()


@pytest.fixture(scope="module")
def corpora():
    out = {}
    for fmt in FMTS:
        rows = _rows(2000, 7 if fmt == "ADFEA" else 8, fmt)
        assert any(not e for _, e in rows) and max(len(e) for _, e in rows) > 30
        assert any(k == (1 << 64) - 1 for _, e in rows for k, _ in e)
        if fmt == "TERAFEA":
            assert len({g for _, e in rows for _, g in e}) > 100
        out[fmt] = rows
    return out


@pytest.mark.parametrize("ignore_slot", [True, False])
@pytest.mark.parametrize("hash_mod", [0, 65536, 10 ** 9])
@pytest.mark.parametrize("fmt", FMTS)
def test_clean_corpora_not_deferred(corpora, fmt, hash_mod, ignore_slot):
    for k, (sep, joint, eol) in enumerate(STYLES):
        raw = _join(corpora[fmt], fmt, sep, joint, eol, last_eol=k != 1)
        assert 3 * SPAN < len(raw) < 900_000
        assert not _on_defer_list(raw, fmt, ignore_slot)  # (so nothing may be deferred)
        got = _check(raw, fmt, hash_mod, ignore_slot=ignore_slot)
        assert got.rows == 2000


# ------------------------------------------------------------------ decomposition
def _short_lines(total: int, seed: int, fmt: str) -> bytes:
    """Exactly ``total`` bytes of short whole lines, the rest filled with blanks."""
    rng = random.Random(seed)
    out = bytearray()
    while True:
        lab = rng.choice(["1", "0", "-1"])
        n = rng.randint(0, 3)
        if fmt == "ADFEA":
            toks = [str(rng.randrange(1000)), "1", lab] + \
                [f"{rng.randrange(10 ** 3, 10 ** 7)}:{rng.randrange(50)}" for _ in range(n)]
        else:
            toks = [lab, str(rng.randrange(1000)), "|"] + \
                [str((rng.randrange(1, 20) << 54) + rng.randrange(10 ** 6)) for _ in range(n)]
        line = (" ".join(toks) + "\n").encode()
        if len(out) + len(line) > total:
            return bytes(out) + b" " * (total - len(out))
        out += line


def test_empty_and_blank_buffers():
    for fmt in FMTS:
        for raw in (b"", b"\n\n\n", b"\n", b" \t \r\n\r\n", b"  "):
            got = _check(raw, fmt)
            assert got.rows == 0 and got.nnz == 0
    # no trailing newline, tabs, CRLF
    assert _check(b"5 1 1 3:4 5:6", "ADFEA").nnz == 2
    assert _check(b"5\t1\t0\t3\t4\r\n\r\n6 1 1\r\n", "ADFEA").rows == 2
    assert _check(b"1 5 | 18014398509481985 7", "TERAFEA").nnz == 2
    assert _check(b"0\t5\t|\t9\r\n\r\n1 6 |\r\n", "TERAFEA").rows == 2


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("spans", [1, 2])
def test_lengths_around_span_edges(fmt, spans):
    for d in range(-17, 18):
        total = spans * SPAN + d
        _check(_short_lines(total, total, fmt), fmt, 65536)
    # lines shift by one byte per case: every alignment of a token start, a token end and a
    # newline against the span edge occurs
    base = _short_lines(spans * SPAN + 64, 5, fmt)
    for shift in range(48):
        _check(b" " * shift + base, fmt, ignore_slot=bool(shift & 1))


CLASS_AT = {
    "ADFEA": (b"77 1 1 123:45 678:9\n",
              {"skipped id": 0, "label": 5, "key": 7, "colon": 10, "group": 11, "second key": 14}),
    "TERAFEA": (b"1 77 | 123 456\n", {"label": 0, "skipped": 2, "bar": 5, "key": 7,
                                      "second key": 11}),
}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("spans", [1, 2])
def test_each_token_class_on_both_sides_of_a_span_edge(fmt, spans):
    line, at = CLASS_AT[fmt]
    filler = _short_lines(spans * SPAN - 200, 31, fmt)
    filler = filler[:filler.rfind(b"\n") + 1]
    tail = _short_lines(300, 32, fmt)
    for name, off in at.items():
        for edge in (spans * SPAN - 1, spans * SPAN):  # the last byte of a span, the first
            pad = edge - off - len(filler)
            assert pad > 0
            raw = filler + b" " * (pad - 1) + b"\n" + line + tail
            assert raw[edge:edge + 1] == line[off:off + 1], name
            for ignore_slot in (False, True):
                _check(raw, fmt, ignore_slot=ignore_slot)


def _tokens_before(raw: bytes, at: int, fmt: str) -> int:
    """Tokens of the line holding byte ``at`` that start before it."""
    a = raw.rfind(b"\n", 0, at) + 1
    return len([t for t in re.split(rb"[ :\t\r]+" if fmt == "ADFEA" else rb"[ \t\r]+", raw[a:at])
                if t])


@pytest.mark.parametrize("fmt", FMTS)
def test_one_line_longer_than_two_spans(fmt):
    rng = random.Random(11)
    n = 4000
    ents = [(rng.randrange(1 << rng.choice((8, 30, 64))), rng.randrange(300)) for _ in range(n)]
    if fmt == "TERAFEA":
        ents = [(k, k >> 54) for k, _ in ents]
    long_line = _join([("1", ents)], fmt)
    assert len(long_line) > 2 * SPAN + 4000
    parities = set()
    for shift in range(0, 24, 3):
        raw = _short_lines(3000 + shift, 1, fmt) + long_line + _short_lines(3000, 2, fmt)
        # the carry into the spans that start inside the long line, which has no newline there
        carries = [_tokens_before(raw, e, fmt) for e in (SPAN, 2 * SPAN)]
        assert all(c > 100 for c in carries)
        parities |= {c & 1 for c in carries}
        got = _check(raw, fmt, 10 ** 9, ignore_slot=bool(shift & 1))
        assert int(np.diff(got.row_ptr.cpu().numpy()).max()) == n
    assert parities == {0, 1}


@pytest.mark.parametrize("fmt", FMTS)
def test_many_short_lines(fmt):
    rng = random.Random(3)
    if fmt == "ADFEA":
        kinds = ["1 1 1\n", "2 1 0\n", "3 1 1 7:2\n"]
    else:
        kinds = ["1 1 |\n", "0 2 |\n", "1 3 | 7\n"]
    raw = "".join(rng.choice(kinds[:2] if rng.random() < 0.95 else kinds[2:])
                  for _ in range(9000)).encode()
    got = _check(raw, fmt, ignore_slot=False)
    # (6-byte lines, one in twenty 8 or 10 bytes: more than 2500 rows per span)
    assert got.rows == 9000 and got.rows * SPAN / len(raw) > 2500


@pytest.mark.parametrize("fmt", FMTS)
def test_label_only_lines_between_normal_ones(corpora, fmt):
    rows = []
    for k, r in enumerate(corpora[fmt][:900]):
        rows.append(r)
        if k % 3 == 0:
            rows.append(("1", []))
    raw = _join(rows, fmt)
    assert len(raw) > SPAN
    got = _check(raw, fmt, ignore_slot=False)
    assert got.rows == 1200 and int((np.diff(got.row_ptr.cpu().numpy()) == 0).sum()) >= 300


# ------------------------------------------------------------------ deferring lines
DEFER = {
    "ADFEA": ["5 1 1 " + "9" * 65 + ":3", "5 1 1 999999999999999999999:3",
              "5 1 x 3:4", "5 1", "5", "5 1 1 3:4 5", "5 1 1 3", "#5 1 1 3:4", "  #c 1 1 3:4",
              ": 5 1 1 3:4", " :", "5 1 1.0 3:4", "5 1 1 3x:4", "5 1 1 18446744073709551616:4"],
    "TERAFEA": ["1 5 | " + "9" * 65, "1 5 | 999999999999999999999", "x 5 | 3", "1 5", "1",
                "#1 5 | 3", "  #c 5 | 3", "1.0 5 | 3", "1 5 | 3x", "1 5 | 3:4", "1 5 | -3",
                "1 5 | 18446744073709551616"],
}
DEFER_SLOTS = ["5 1 1 3:-1", "5 1 1 3:2147483648", "5 1 1 3:x", "5 1 1 3:1.5",
               "5 1 1 3:99999999999999999999"]  # ADFEA, with slots kept
# lines the host takes and the kernels must take too
TAKEN = {
    "ADFEA": ["5# 1 1 3:4", "5 x -0 3:4", "x y +1 3:4", "5 1 1 3:2147483647",
              "5 1 1 :3:4", "5 1 1 3::4 : 5 : 6 ", "5:1:1:3:4", "5 1 -9223372036854775808"],
    "TERAFEA": ["+1 # | 3", "0 x y 3", "1 5 | 18446744073709551615", "-0 5 |", "1 5 3"],
}


@pytest.mark.parametrize("fmt", FMTS)
def test_deferring_and_malformed_lines(corpora, fmt):
    good = _join(corpora[fmt][:60], fmt).decode().splitlines()
    rng = random.Random(5)
    cases = [(b, True, None) for b in DEFER[fmt]] + [(b, False, None) for b in TAKEN[fmt]]
    if fmt == "ADFEA":
        cases += [(b, True, False) for b in DEFER_SLOTS]
    for bad, must_defer, slot_mode in cases:
        lines = list(good)
        lines.insert(rng.randrange(len(lines) + 1), bad)
        raw = ("\n".join(lines) + "\n").encode()
        for ignore_slot in ((True, False) if slot_mode is None else (slot_mode,)):
            assert _on_defer_list(raw, fmt, ignore_slot) == must_defer, bad
            got = _check(raw, fmt, 65536, ignore_slot=ignore_slot, clean=False)
            assert got.deferred is must_defer, bad
    whole = ("\n".join(good + [c[0] for c in cases]) + "\n").encode()
    got = _check(whole, fmt, 0, clean=False)
    assert got.deferred and got.bad_lines > 5


def test_unread_group_tokens():
    # without slots nobody reads the group: junk there is a clean entry unless the host
    # rejects it (it does not); with slots kept the chunk is the host's
    raw = b"5 1 1 7:x 8:-1 9:2147483648 10:1.5\n6 1 0 11:3\n"
    assert not _on_defer_list(raw, "ADFEA", True)
    got = _check(raw, "ADFEA", ignore_slot=True)
    assert got.deferred is False and got.keys.cpu().tolist() == [7, 8, 9, 10, 11]
    got = _check(raw, "ADFEA", ignore_slot=False, clean=False)
    assert got.deferred and got.bad_lines == 1 and got.rows == 1


@pytest.mark.parametrize("ignore_slot", [True, False])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("fmt", FMTS)
def test_random_bytes(fmt, seed, ignore_slot):
    rng = random.Random(99 + seed)
    alphabet = "0123456789" * 2 + " \t\r:|-\n\n"
    raw = "".join(rng.choice(alphabet) for _ in range(8192)).encode()
    got = _check(raw, fmt, 65536, ignore_slot=ignore_slot, clean=False)
    rp = got.row_ptr.cpu().numpy()
    assert rp[0] == 0 and rp[-1] == got.nnz and (np.diff(rp) >= 0).all()
    # sparser noise: mostly well-formed tokens, many lines parse
    toks = ["1", "0", "12", "345:1", "7", " | ", " ", " ", " ", "\n", "\n", "\t", "\r\n", ":",
            "-1", "+1", "6 7", "18446744073709551615", "1 1 1 "]
    raw = "".join(rng.choice(toks) for _ in range(4000)).encode()
    _check(raw, fmt, 0, ignore_slot=ignore_slot, clean=False)


# ------------------------------------------------------------------ buffers
@pytest.mark.parametrize("fmt", FMTS)
def test_output_capacity_overflow_defers(corpora, fmt):
    raw = _join(corpora[fmt][:400], fmt)
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
    assert np.array_equal(again.keys.cpu().numpy().view(np.uint64), ref.keys.view(np.uint64))


@pytest.mark.parametrize("fmt", FMTS)
def test_base_offsets_behind_carried_rows(corpora, fmt):
    rows = corpora[fmt]
    a, b = _join(rows[:300], fmt), _join(rows[300:700], fmt, last_eol=False, first_id=300)
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

    same()
    # a deferred second chunk lands behind the carried rows as well
    p3 = parse_text_device(_dev(b + b"\nx 1 y 3:4\n"), fmt, 65536, ignore_slot=False, out=out,
                              row0=p1.rows, nnz0=p1.nnz)
    assert p3.deferred and p3.bad_lines == 1 and p3.rows == p2.rows
    same()


# ------------------------------------------------------------------ feeder
def _slot_data(rows, seed):
    from parameter_server_amd.data.synthetic import sparse_classification

    return sparse_classification(rows, groups=(1, 2, 3, 4, 5), keys_per_group=3000,
                                 nnz_per_row=(1, 3, 5, 2, 4), binary=True, seed=seed)


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


def test_feeder_matches_cpu_parser(tmp_path):
    from parameter_server_amd.data.feeder import DeviceFeeder
    from parameter_server_amd.data.synthetic import write_text

    files = []
    for k, rows in enumerate((1300, 1, 900)):
        files.append(str(tmp_path / f"part-{k}"))
        write_text(_slot_data(rows, 40 + k), files[-1], "ADFEA")
    assert os.path.getsize(files[0]) > 4 * 16384  # several chunks per file
    _, ref = _feed(files, "ADFEA", "cpu")
    f, got = _feed(files, "ADFEA", "gpu")
    assert f.parser == "gpu" and f.text_passes == 2 and f.deferred_chunks == 0
    assert f.text_chunks > 2 * 6
    assert sum(x[0] for x in got) == 2 * 2201
    _same_batches(got, ref)
    assert all(x[5] is None for x in got)
    # with a cache directory the second pass streams the cache the GPU text pass left behind
    f2, got2 = _feed(files, "ADFEA", "gpu", cache_dir=str(tmp_path / "cache"))
    assert f2.parser == "gpu" and f2.text_passes == 1 and f2.cached_passes == 1
    assert f2.deferred_chunks == 0
    _, ref2 = _feed(files, "ADFEA", "cpu", cache_dir=str(tmp_path / "cache_cpu"))
    _same_batches(got2, ref2)
    _same_batches(got2[:len(ref) // 2], ref[:len(ref) // 2])
    assert DeviceFeeder(files, "ADFEA", 500, 6000, DEV, parser="auto").parser == "gpu"
    # TERAFEA keeps the CPU parser in the feeder
    assert DeviceFeeder(files, "TERAFEA", 500, 6000, DEV, parser="gpu").parser == "cpu"


# ------------------------------------------------------------------ SlotReader
def _same_slot_data(a, b):
    assert np.array_equal(a.labels, b.labels) and sorted(a.groups) == sorted(b.groups)
    for g in a.groups:
        for u, v in zip(a.groups[g], b.groups[g]):
            assert (u is None) == (v is None)
            if u is not None:
                assert u.dtype == v.dtype and np.array_equal(u, v)
    assert a.info() == b.info()


def _slot_reader_routes(files, fmt, host):
    """Every device route of the SlotReader against the host route's ``host``; returns the
    chunks the device split handed back, per route."""
    from parameter_server_amd.data.slot_reader import SlotReader, _to_host

    deferred = {}
    for name, kw in (("host", {}), ("device", {"split": "device"}),
                     ("resident", {"split": "device", "resident": True})):
        r = SlotReader(files, fmt, parser="gpu", device=DEV, **kw)
        assert r.parser == "gpu" and r.split == ("host" if name == "host" else "device")
        sd = r.read()
        assert r.deferred_chunks == 0
        if name == "resident":
            assert all(t[1].is_cuda for t in sd.groups.values())
            assert sd.info() == host.info()
            sd = _to_host(sd)
        _same_slot_data(sd, host)
        deferred[name] = r.split_deferred_chunks
    assert SlotReader(files, fmt, parser="auto", device=DEV).parser == "cpu"
    return deferred


@pytest.mark.parametrize("fmt", FMTS)
def test_slot_reader_device_routes_match_host_route(tmp_path, fmt):
    from parameter_server_amd.data.slot_reader import SlotReader
    from parameter_server_amd.data.synthetic import sparse_groups, write_text

    files = []
    for k in range(2):
        sd = sparse_groups(1500, groups=5, present=3, keys_per_group=500, seed=70 + k)
        assert len(sd.groups) == 5 and any((np.diff(o) == 0).any() for o, _, _ in sd.groups.values())
        files.append(str(tmp_path / f"part-{k}"))
        write_text(sd, files[-1], fmt)  # (every row's groups contiguous)
    host = SlotReader(files, fmt, parser="cpu").read()
    assert host.rows == 3000 and len(host.groups) == 5
    deferred = _slot_reader_routes(files, fmt, host)
    assert deferred == {"host": 0, "device": 0, "resident": 0}


def test_slot_reader_terafea_with_a_group_repeated_in_a_row(tmp_path):
    from parameter_server_amd.data.slot_reader import SlotReader

    rng = random.Random(4)
    lines = []
    for i in range(800):
        ks = [(g << 54) | rng.randrange(1 << 30) for g in (3, 9, 3, 1)[:rng.randint(1, 4)]]
        lines.append(" ".join([str(i & 1), str(i), "|"] + [str(k) for k in ks]))
    p = tmp_path / "part-0"
    p.write_bytes(("\n".join(lines) + "\n").encode())
    host = SlotReader([str(p)], "TERAFEA", parser="cpu").read()
    assert sorted(host.groups) == [1, 3, 9]
    deferred = _slot_reader_routes([str(p)], "TERAFEA", host)
    assert deferred["host"] == 0 and deferred["device"] > 0 and deferred["resident"] > 0


# ------------------------------------------------------------------ app
def test_app_parser_gpu_matches_parser_cpu_on_an_adfea_conf(tmp_path):
    from parameter_server_amd.app.gpu import _flags, run_async_sgd
    from parameter_server_amd.data.synthetic import write_text
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    data_dir = tmp_path / "data"
    os.makedirs(data_dir)
    for p in range(3):
        write_text(_slot_data(600, 60 + p), str(data_dir / f"part-{p}"), "ADFEA")
    golden = open(os.path.join(os.path.dirname(__file__), "golden", "confs",
                               "online_ftrl.conf")).read()
    models = {}
    for parser in ("gpu", "cpu"):
        model = tmp_path / f"model_{parser}" / "m"
        conf = tmp_path / f"{parser}.conf"
        text = re.sub(r"training_data \{.*?\}", lambda m: "training_data { format: TEXT text: "
                      f'ADFEA file: "{data_dir}/part.*" }}', golden, flags=re.S)
        text = text.replace('"out/online_ftrl"', f'"{model}"')
        assert "ADFEA" in text and str(model) in text
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


@pytest.mark.parametrize("fmt", FMTS)
def test_app_slot_split_device_matches_parser_cpu(tmp_path, fmt):
    from parameter_server_amd.app.gpu import _flags, run_darlin
    from parameter_server_amd.data.synthetic import sparse_groups, write_text
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    for k in range(3):
        write_text(sparse_groups(600, groups=5, present=3, keys_per_group=300, seed=80 + k),
                   str(tmp_path / f"part-{k}"), fmt)
    models, objective = {}, {}
    for name, args in (("device", ["-parser", "gpu", "-slot_split", "device"]),
                       ("cpu", ["-parser", "cpu"])):
        model = tmp_path / f"model_{name}" / "m"
        conf = tmp_path / f"{name}.conf"
        conf.write_text(f"""linear_method {{
training_data {{ format: TEXT text: {fmt} file: "{tmp_path}/part.*" }}
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
        objective[name] = res["progress"].objective
    assert len(models["device"].splitlines()) > 20
    assert models["device"] == models["cpu"]
    # Darlin's column sums add rows by atomics, so two runs need not agree to the last bit;
    # the bound is the one derived in tests/test_slotsplit_gpu.py for n = 3000 rows of this
    # shape (4 n u * 6 n absolute on an objective above n ln 2 / 2), which n = 1800 is under
    np.testing.assert_allclose(objective["device"], objective["cpu"], rtol=2.4e-11, atol=0)
