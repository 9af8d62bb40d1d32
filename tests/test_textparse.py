"""CPU checks of the GPU text parser's host-side parts: the number scanners it shares
with the device (csrc/core/textnum.h, built into ``_pscore`` for this purpose) against
the host parser and Python, the feeder's parser selection, and a sanitizer build of the
scanners fed random bytes."""
import os
import random
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from parameter_server_amd import data
from parameter_server_amd.ops.native import core

OK, BAD, DEFER = 0, 1, 2
ROOT = Path(__file__).resolve().parents[1]
SEED = 20240611


def _rand_decimal(rng):
    """(string, significant digits, written exponent)."""
    nd = rng.randint(1, 17)
    digs = [rng.choice("123456789")] + [rng.choice("0123456789") for _ in range(nd - 1)]
    digs = "".join(digs)
    form = rng.randrange(4)
    if form == 0:    # d.ddd
        s = digs[0] + "." + digs[1:] if nd > 1 else digs + ".0"
    elif form == 1:  # .ddd
        s = "." + digs
    elif form == 2:  # ddd.
        s = digs + "."
    else:            # dE+-x
        s = digs
    ex = 0
    if form == 3 or rng.random() < 0.5:
        ex = rng.randint(-30, 30)
        s += rng.choice("eE") + rng.choice(["", "+"] if ex >= 0 else [""]) + str(ex)
    sign = rng.choice(["", "-", "+"])
    return sign + s, len(digs.rstrip("0")), ex


def _cpu_values(strings):
    """{index: float32} of the strings the host parser accepts as a LIBSVM value."""
    text = "".join(f"0 {i}:{s}\n" for i, s in enumerate(strings)).encode()
    b = data.parse_text(text, "LIBSVM", ignore_slot=True, nthreads=4)
    vals = np.ones(b.keys.size, np.float32) if b.vals is None else b.vals
    return dict(zip(b.keys.tolist(), vals.tolist())), b.info["bad_lines"]


def test_f32_scanner_matches_host_parser():
    rng = random.Random(SEED)
    gen = [_rand_decimal(rng) for _ in range(1_000_000)]
    hand = ["0", "-0", "1", "0.1", "16777217", "1e-45", "3.4028235e38", "3.4028236e38", "1e39",
            "inf", "nan", "1e", "1e+", "--1", "1.2.3"]
    strings = [g[0] for g in gen] + hand
    vals, st = core().textnum_f32([s.encode() for s in strings])
    assert vals.dtype == np.float32 and len(vals) == len(strings)
    ref, bad_lines = _cpu_values(strings)
    assert bad_lines == len(strings) - len(ref)
    is_val = st == OK
    # every value is the host parser's value, bit for bit, and numpy's
    idx = np.flatnonzero(is_val)
    assert all(i in ref for i in idx.tolist())
    want = np.array([ref[i] for i in idx.tolist()], np.float32)
    assert np.array_equal(vals[idx].view(np.uint32), want.view(np.uint32))
    npv = np.array([np.float32(strings[i]) for i in idx.tolist()], np.float32)
    assert np.array_equal(vals[idx].view(np.uint32), npv.view(np.uint32))
    # every string reported bad is one the host parser rejects
    assert all(i not in ref for i in np.flatnonzero(st == BAD).tolist())
    # the hand list: values where the routine must decide, bad where the text is malformed
    h0 = len(gen)
    got = {s: (int(st[h0 + k]), float(vals[h0 + k])) for k, s in enumerate(hand)}
    assert got["0"] == (OK, 0.0) and got["1"] == (OK, 1.0)
    assert got["-0"][0] == OK and np.signbit(np.float32(vals[h0 + 1]))
    assert got["0.1"] == (OK, float(np.float32(0.1)))
    assert got["16777217"] == (OK, 16777216.0)
    for s in ("1e", "1e+", "--1", "1.2.3"):
        assert got[s][0] == BAD, s
    for s in ("1e39", "3.4028236e38", "1e-45", "inf", "nan"):
        assert got[s][0] != OK, s  # (outside the exact domain: bad or deferred)
    # short decimals never defer (a condition on SEED: an inexact float tie has
    # probability 2^-29 per string)
    short = np.array([g[1] <= 9 and abs(g[2]) <= 10 for g in gen])
    assert int(np.count_nonzero(st[:h0][short] == DEFER)) == 0
    assert int(np.count_nonzero(short)) > 100_000


def test_integer_scanners_match_python():
    rng = random.Random(SEED + 1)
    dec = ["".join(rng.choice("0123456789") for _ in range(rng.randint(1, 21)))
           for _ in range(200_000)]
    dec += ["18446744073709551615", "18446744073709551616", "9223372036854775807",
            "9223372036854775808", "0", "00000000000000000000001", "", "+1", "-1", "1 ", "1a"]
    v, st = core().textnum_u64([s.encode() for s in dec])
    for s, x, c in zip(dec, v.tolist(), st.tolist()):
        ok = s.isdigit() and s.isascii() and int(s) < 1 << 64
        assert (c == OK) == ok, s
        assert c in (OK, BAD)
        if ok:
            assert x == int(s), s
    sdec = [rng.choice(["", "-", "+", "+-"]) + s for s in dec[:100_000]] + \
        ["-9223372036854775808", "-9223372036854775809", "9223372036854775807",
         "9223372036854775808", "-", "+", "", "--1", "-+1", "++1"]
    v, st = core().textnum_i64([s.encode() for s in sdec])
    for s, x, c in zip(sdec, v.tolist(), st.tolist()):
        body = s[1:] if s.startswith("+") else s
        mag = body[1:] if body.startswith("-") else body
        ok = mag.isdigit() and mag.isascii() and -(1 << 63) <= int(body) < 1 << 63
        assert (c == OK) == ok, s
        if ok:
            assert x == int(body), s
    hexs = ["".join(rng.choice("0123456789abcdefABCDEF") for _ in range(rng.randint(1, 17)))
            for _ in range(200_000)]
    hexs += ["ffffffffffffffff", "10000000000000000", "00000000000000000ff", "0x1f", "g", "", "-1"]
    v, st = core().textnum_hex([s.encode() for s in hexs])
    for s, x, c in zip(hexs, v.tolist(), st.tolist()):
        ok = s != "" and all(ch in "0123456789abcdefABCDEF" for ch in s) and int(s, 16) < 1 << 64
        assert (c == OK) == ok, s
        if ok:
            assert x == int(s, 16), s


def test_token_length_bound_defers():
    long_tok = b"0" * 64 + b"1"
    for fn in ("textnum_f32", "textnum_u64", "textnum_i64", "textnum_hex"):
        _, st = getattr(core(), fn)([long_tok[:64], long_tok])
        assert st.tolist() == [OK, DEFER], fn


def test_criteo_bucket_matches_double_log2():
    def ref(v):
        return np.floor(2.0 * np.log2(1.0 + v.astype(np.float64))).astype(np.uint64)

    v = np.arange(0, 1 << 24, dtype=np.int64)
    ids, st = core().textnum_criteo_bucket(v)
    assert not st.any() and np.array_equal(ids, ref(v))
    rng = np.random.default_rng(SEED)
    v = rng.integers(1 << 24, 1 << 31, size=1_000_000, dtype=np.int64)
    v[:3] = [(1 << 31) - 1, (1 << 31) - 2, 1 << 24]
    ids, st = core().textnum_criteo_bucket(v)
    assert not st.any() and np.array_equal(ids, ref(v))
    ids, st = core().textnum_criteo_bucket(np.array([-5, 0, 1 << 31, 1 << 40, (1 << 63) - 1],
                                                    dtype=np.int64))
    assert st.tolist() == [OK, OK, DEFER, DEFER, DEFER] and ids[:2].tolist() == [0, 0]


# ----------------------------------------------------------------- feeder fallback
def _write_libsvm(path, rows, seed):
    rng = random.Random(seed)
    with open(path, "w") as f:
        for _ in range(rows):
            w = rng.randint(0, 12)
            idx = sorted(rng.randrange(1, 1 << 40) for _ in range(w))
            f.write(rng.choice(["1", "-1", "+1"]) + "".join(
                f" {k}:{rng.choice(['1', '0.5', '-2.25', '3e-2'])}" for k in idx) + "\n")


def _batches(feeder):
    out = []
    for b in feeder:
        out.append((b.rows, b.nnz, b.width, b.keys.numpy().copy(), b.labels.numpy().copy(),
                    None if b.row_ptr is None else b.row_ptr.numpy().copy(),
                    None if b.vals is None else b.vals.numpy().copy()))
        feeder.release(b)
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[:3] == y[:3]
        for u, v in zip(x[3:], y[3:]):
            assert (u is None) == (v is None)
            if u is not None:
                assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8))


def test_feeder_parser_choice_on_cpu(tmp_path):
    from parameter_server_amd.data.feeder import DeviceFeeder

    files = []
    for i, rows in enumerate((700, 1, 450)):
        p = tmp_path / f"part-{i}.libsvm"
        _write_libsvm(p, rows, SEED + i)
        files.append(str(p))
    kw = dict(num_features=1 << 20, passes=2, shuffle=True, seed=3)
    ref = _batches(DeviceFeeder(files, "LIBSVM", 256, 2000, "cpu", parser="cpu", **kw))
    assert sum(b[0] for b in ref) == 2 * 1151
    for parser in ("gpu", "auto"):
        f = DeviceFeeder(files, "LIBSVM", 256, 2000, "cpu", parser=parser, **kw)
        _same(_batches(f), ref)
        assert f.parser == "cpu" and f.text_chunks == 0 and f.deferred_chunks == 0
    with pytest.raises(ValueError):
        DeviceFeeder(files, "LIBSVM", 256, 2000, "cpu", parser="fpga")


# ----------------------------------------------------------------- sanitizer program
def test_textnum_fuzz_under_asan_ubsan(tmp_path):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler with sanitizer runtimes")
    exe = tmp_path / "textnum_fuzz"
    inc = ROOT / "parameter_server_amd" / "csrc" / "core"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        f"-I{inc}", str(ROOT / "tests" / "native" / "textnum_fuzz.cc"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1 halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1 halt_on_error=1"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "textnum_fuzz OK" in r.stdout
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in out, out[-6000:]
