"""CPU checks of the model-text paths' host-side parts: the number formatter the device
writer shares with the host (csrc/core/textfmt.h, built into ``_pscore`` for this purpose)
against Python's own formatting, the model-file discovery both readers use, the CPU routes
of the device entry points, and a sanitizer build of the formatter."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import modeltext_corpus as corpus
from parameter_server_amd.ops.native import core
from parameter_server_amd.utils import checkpoint

ROOT = Path(__file__).resolve().parents[1]
OK, DEFER, SKIP = corpus.OK, corpus.DEFER, corpus.SKIP


def _split(text: bytes, lens: np.ndarray) -> list[bytes]:
    ends = np.cumsum(lens)
    return [text[e - l:e] for e, l in zip(ends.tolist(), lens.tolist())]


def test_formatter_matches_python():
    """Every entry the formatter writes is Python's line; it writes every in-domain one.
    f32(999999999) is 1e9 itself (Python: ``1e+09``, the carry into the exponent): on the
    deferred side of the domain's upper edge, as 3e9 is."""
    w = corpus.weights()
    k = corpus.keys_for(w.size)
    assert w.size >= 1_000_000
    text, st, lens = core().textfmt_entries(k, w)
    dom = corpus.in_domain(w)
    assert dom.sum() > 300_000
    zero = w == 0
    assert np.array_equal(st == SKIP, zero) and np.array_equal(st == OK, dom)
    assert np.all(st[~dom & ~zero] == DEFER) and np.all(lens[st != OK] == 0)
    want = corpus.python_lines(k[dom], w[dom])
    if text != b"".join(want):  # (locate the first difference)
        got = _split(text, lens[dom])
        bad = [(i, g, x) for i, (g, x) in enumerate(zip(got, want)) if g != x][:5]
        raise AssertionError(f"{bad}")
    assert max(map(len, want)) <= 37
    # what the corpus is meant to hold
    lines = set(want)
    for s in (b"9\t1000000.12\n", b"9\t1000000.38\n"):
        assert any(x.endswith(s[1:]) for x in lines)
    assert f"{float(np.float32(999999999)):.9g}" == "1e+09"
    for e in range(-22, 9):
        p = np.float32(10.0 ** e)
        assert corpus.in_domain(np.array([p]))[0] == (float(p) >= 1e-22)
    notation = {x.split(b"\t")[1] for x in lines}
    assert b"0.000100000005\n" in notation and b"-0.000100000005\n" in notation  # f32(1e-4)
    assert b"9.99999975e-05\n" in notation and b"999999936\n" in notation  # (the floats below)
    assert b"100000000\n" in notation and b"0.5\n" in notation


def test_formatter_keys():
    k = np.array(corpus.KEYS, dtype=np.uint64)
    text, st, lens = core().textfmt_entries(k, np.full(k.size, -0.5, np.float32))
    assert np.all(st == OK)
    assert _split(text, lens) == [f"{int(x)}\t-0.5\n".encode() for x in corpus.KEYS]


def test_out_of_domain_defers():
    w = np.array([np.inf, -np.inf, 1e-30, 3e9, -3e9, 1e-40, 1.4e-45, 1e9, 9.9e-23, 3.4e38],
                 dtype=np.float32)
    text, st, lens = core().textfmt_entries(np.arange(w.size, dtype=np.uint64), w)
    assert np.all(st == DEFER) and text == b"" and not lens.any()
    text, st, lens = core().textfmt_entries(np.zeros(3, np.uint64),
                                            np.array([0.0, -0.0, np.nan], np.float32))
    assert st.tolist() == [SKIP, SKIP, DEFER] and text == b""


def test_find_model_files_and_readers_agree(tmp_path):
    d = tmp_path / "out"
    for i, name in enumerate(["m_S0", "m_S1", "m_S10", "other_S0", "m_S2.bak"]):
        checkpoint.write_text_model(str(d / name), np.array([i + 1], np.uint64),
                                    np.array([float(i + 1)], np.float32))
    glob_pat, regex_pat = str(d / "m_S*"), str(d / "m_S[0-9]+")
    assert checkpoint.find_model_files(glob_pat) == \
        [str(d / n) for n in ("m_S0", "m_S1", "m_S10", "m_S2.bak")]
    # (no glob match: the last component is a regex, matched from the start of the name)
    assert checkpoint.find_model_files(regex_pat) == \
        [str(d / n) for n in ("m_S0", "m_S1", "m_S10", "m_S2.bak")]
    assert checkpoint.find_model_files(str(d / "m_S1$")) == [str(d / "m_S1")]
    assert checkpoint.find_model_files(str(d / "nothing.*")) == []
    assert checkpoint.read_text_models(glob_pat) == {1: 1.0, 2: 2.0, 3: 3.0, 5: 5.0}
    assert checkpoint.read_text_models(str(d / "m_S1$")) == {2: 2.0}
    with pytest.raises(FileNotFoundError):
        checkpoint.find_model_files(str(tmp_path / "missing" / "m.*"))


def test_cpu_tensors_take_the_host_code(tmp_path):
    from parameter_server_amd.models import ModelScorer
    from parameter_server_amd.ops.modeltext import (read_text_models_device,
                                                    write_text_model_device)

    k = torch.tensor([5, -1, 1 << 40, 7, 3], dtype=torch.int64)  # (-1: 2^64 - 1, sorts last)
    w = torch.tensor([0.25, -2.0, 1e-30, 0.0, float("nan")])
    n, deferred = write_text_model_device(str(tmp_path / "a" / "m_S0"), k, w)
    checkpoint.write_text_model(str(tmp_path / "b_S0"), k, w)
    assert (n, deferred) == (3, 0)
    raw = (tmp_path / "a" / "m_S0").read_bytes()
    assert raw == (tmp_path / "b_S0").read_bytes()
    assert raw == b"5\t0.25\n1099511627776\t1e-30\n18446744073709551615\t-2\n"
    n, _ = write_text_model_device(str(tmp_path / "e" / "m_S0"), k[:0], w[:0])
    assert n == 0 and (tmp_path / "e" / "m_S0").read_bytes() == b""
    keys, ww, entries, deferred = read_text_models_device(str(tmp_path / "a" / "m_S.*"), "cpu")
    assert (entries, deferred) == (3, 0)
    assert keys.tolist() == [5, 1 << 40, -1] and ww.tolist() == w[[0, 2, 1]].tolist()
    for mode in ("auto", "host"):
        sc = ModelScorer.from_text(str(tmp_path / "a" / "m_S.*"), 64, "cpu", text_io=mode)
        assert sc.entries == 3 and sc.deferred_chunks == 0
    with pytest.raises(ValueError):
        ModelScorer.from_text(str(tmp_path / "a" / "m_S.*"), 64, "cpu", text_io="device")
    with pytest.raises(ValueError):
        ModelScorer.from_text(str(tmp_path / "a" / "m_S.*"), 64, "cpu", text_io="gpu")


def test_trainer_save_model_text_io_cpu(tmp_path):
    from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
    from parameter_server_amd.ops.synthetic import criteo_batch

    N, B = 1 << 20, 200
    tr = SparseLRTrainer(SparseLRConfig(num_features=N, minibatch=B, table_capacity=1 << 15,
                                        l1=0.01, alpha=0.5, beta=1.0), device="cpu")
    for s in range(3):
        k, l = criteo_batch(B, seed=7, row0=s * B, num_features=N, cards=[200] * 26)
        tr.step(k, l, width=39)
    a = Path(tr.save_model(str(tmp_path / "a"), text_io="auto")).read_bytes()
    b = Path(tr.save_model(str(tmp_path / "b"), text_io="host")).read_bytes()
    assert a == b and a.count(b"\n") == tr.table.census()[1] == tr.last_save["entries"] > 50
    assert tr.last_save["deferred_chunks"] == 0
    kk, ww = tr.table.occupied_weights()
    ko, wo, _, _ = tr.table.occupied()
    assert torch.equal(kk, ko) and torch.equal(ww, wo)
    with pytest.raises(ValueError):
        tr.save_model(str(tmp_path / "c"), text_io="device")


# ----------------------------------------------------------------- sanitizer program
def test_textfmt_fuzz_under_asan_ubsan(tmp_path):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler with sanitizer runtimes")
    exe = tmp_path / "textfmt_fuzz"
    inc = ROOT / "parameter_server_amd" / "csrc" / "core"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        f"-I{inc}", str(ROOT / "tests" / "native" / "textfmt_fuzz.cc"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1 halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1 halt_on_error=1"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "textfmt_fuzz OK" in r.stdout
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in out, out[-6000:]
