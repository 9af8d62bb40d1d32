"""Per-example prediction files (ops/scoretext.py, ``ModelScorer.evaluate(predictions=)``,
the app's ``-predict_output``) on the CPU: the bare-score formatter the device kernels share
with the host (csrc/core/textfmt.h ``put_score``, built into ``_pscore``) against Python's
own ``"%.9g"``, a sanitizer build of it, the writer's host route and the app's routes. The
oracle everywhere is the plain Python loop. The corpus and file helpers below are run again
on the device by tests/test_predict_output_gpu.py."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import modeltext_corpus as corpus
from test_app_eval import ROWS, _eval_conf, _flags, _port, _write

from parameter_server_amd.ops.keymix import key_bits_for
from parameter_server_amd.ops.native import core

ROOT = Path(__file__).resolve().parents[1]
OK, DEFER = corpus.OK, corpus.DEFER
SHORTEST, LONGEST = np.float32(0.0), np.float32(-1.23456787e-22)  # "0", "-1.23456782e-22"


# ---------------------------------------------------------------- corpus
def score_domain(x: np.ndarray) -> np.ndarray:
    """The score formatter's exact domain: the model formatter's, and +-0."""
    return corpus.in_domain(x) | ((x.view(np.uint32) & np.uint32(0x7fffffff)) == 0)


def domain_bits(n: int, seed: int) -> np.ndarray:
    """``n`` random f32 bit patterns inside the domain (both signs, every binade of it),
    as float32."""
    rng = np.random.default_rng(seed)
    out, have = [], 0
    while have < n:
        r = rng.integers(0, 1 << 32, n + n // 8 + 64, dtype=np.uint64).astype(np.uint32)
        be = (53 + rng.integers(0, 104, r.size)).astype(np.uint32)  # 2^-74 .. 2^29
        x = ((r & np.uint32(0x807fffff)) | (be << np.uint32(23))).view(np.float32)
        x = x[corpus.in_domain(x)]
        out.append(x)
        have += x.size
    return np.concatenate(out)[:n]


def boundary_values() -> np.ndarray:
    """float32, inside the domain or not: +-0, the neighbours of 1e-22 and 1e9 on both
    sides, the neighbours of every power of ten (where a nine-digit rounding can carry into
    a tenth digit), powers of ten, the notation switches, the shortest and the longest outputs."""
    v = [0.0, 1.0, 0.5, 0.1, 7.0, 1000000.125, 1000000.375, 123456789.0, 999999999.0,
         float(LONGEST), 1.23456787e-05, 0.000123456784, 123456.789]
    v += [10.0 ** e for e in range(-22, 10)]
    h = np.array(v, dtype=np.float32)
    for pivot in (1e-22, 1e9, 1e-4, 1e-5, 1e8, 1.0, 10.0, 1e-10):
        p = np.float32(pivot)
        for _ in range(3):  # three floats below, the pivot, three above
            p = np.nextafter(p, np.float32(0))
        for _ in range(7):
            h = np.append(h, p)
            p = np.nextafter(p, np.float32(np.inf))
    # the floats next to every power of ten: where nine nines and a tenth digit >= 5 would
    # carry (9.99999999x -> 10.0000000)
    for e in range(-20, 9):
        p = np.float32(10.0 ** e)
        h = np.append(h, [np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(np.inf))])
    h = h.astype(np.float32)
    return np.concatenate([h, -h])


def python_scores(x: np.ndarray) -> list[bytes]:
    return [("%.9g" % float(v)).encode() for v in x]


def _split(text: bytes, lens: np.ndarray) -> list[bytes]:
    ends = np.cumsum(lens)
    return [text[e - l:e] for e, l in zip(ends.tolist(), lens.tolist())]


def _check_formatter(x: np.ndarray):
    text, st, lens = core().textfmt_scores(np.ascontiguousarray(x).view(np.uint32))
    dom = score_domain(x)
    assert np.array_equal(st == OK, dom) and np.all(st[~dom] == DEFER)
    assert np.all(lens[~dom] == 0)
    want = python_scores(x[dom])
    if text != b"".join(want):  # (locate the first difference)
        got = _split(text, lens[dom])
        raise AssertionError([(g, w) for g, w in zip(got, want) if g != w][:5])
    return want


# ---------------------------------------------------------------- formatter
def test_score_formatter_matches_python_on_random_bits():
    x = domain_bits(1_000_000, corpus.SEED + 7)
    assert x.size == 1_000_000 and score_domain(x).all()
    want = _check_formatter(x)
    assert min(map(len, want)) >= 1 and max(map(len, want)) == 15


def test_score_formatter_boundaries():
    x = boundary_values()
    want = set(_check_formatter(x))
    for s in (b"0", b"-0", b"1", b"-1", b"1.00000003e-22", b"100000000", b"999999936",
              b"9.99999975e-06", b"-0.000100000005", b"-1.23456782e-22", b"1000000.12",
              b"1000000.38", b"10", b"0.5"):
        assert s in want, s
    # f32(999999999) is 1e9 itself: on the deferred side, like the floats above 1e9
    dom = score_domain(x)
    assert not dom[x == np.float32(1e9)].any() and dom[x == np.nextafter(
        np.float32(1e9), np.float32(0))].all()
    lo = np.float32(1e-22)  # 1.00000003e-22, the smallest float of the domain
    assert float(lo) >= 1e-22 and dom[x == lo].all()
    assert not dom[x == np.nextafter(lo, np.float32(0))].any()
    # (f32 is too coarse for a carry next to 1: the float below it keeps its eight digits)
    assert ("%.9g" % float(np.nextafter(np.float32(1.0), np.float32(0)))) == "0.99999994"
    assert len(python_scores(np.array([SHORTEST]))[0]) == 1
    assert len(python_scores(np.array([LONGEST]))[0]) == 15
    # the whole random corpus of the model-text tests too (all of f32: most of it defers)
    _check_formatter(corpus.weights(200_000))


def test_score_formatter_defers_out_of_domain():
    w = np.array([np.inf, -np.inf, np.nan, 1e-30, 3e9, -3e9, 1e-40, 1.4e-45, -1.4e-45, 1e9,
                  9.9e-23, 3.4e38, 1.1754942e-38], dtype=np.float32)
    text, st, lens = core().textfmt_scores(w.view(np.uint32))
    assert np.all(st == DEFER) and text == b"" and not lens.any()
    text, st, lens = core().textfmt_scores(np.array([0, 0x80000000], np.uint32))
    assert st.tolist() == [OK, OK] and text == b"0-0" and lens.tolist() == [1, 2]


# ---------------------------------------------------------------- sanitizer program
def test_scorefmt_fuzz_under_asan_ubsan(tmp_path):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler with sanitizer runtimes")
    exe = tmp_path / "scorefmt_fuzz"
    inc = ROOT / "parameter_server_amd" / "csrc" / "core"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        f"-I{inc}", str(ROOT / "tests" / "native" / "scorefmt_fuzz.cc"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1 halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1 halt_on_error=1"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "scorefmt_fuzz OK" in r.stdout
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in out, out[-6000:]


# ---------------------------------------------------------------- writer, host route
def python_lines(score, label=None) -> bytes:
    """The oracle: one ``%.9g`` per column."""
    s = [float(np.float32(v)) for v in np.asarray(score, dtype=np.float32)]
    if label is None:
        return "".join("%.9g\n" % v for v in s).encode()
    y = [float(np.float32(v)) for v in np.asarray(label, dtype=np.float32)]
    return "".join("%.9g\t%.9g\n" % (a, b) for a, b in zip(y, s)).encode()


def append_unevenly(w, margins, labels, seed=5):
    """All rows, in pieces of uneven sizes (0 among them); some from longer tensors with
    ``rows=``."""
    rng = np.random.default_rng(seed)
    n, a = margins.numel(), 0
    w.append(margins[:0], None if labels is None else labels[:0], rows=0)
    while a < n:
        k = min(n - a, int(rng.integers(0, max(2, n // 5))))
        if k % 2:
            w.append(margins[a:a + k], None if labels is None else labels[a:a + k])
        else:  # (a longer tensor, as a feeder's label buffer is)
            w.append(margins[a:], None if labels is None else labels[a:], rows=k)
        a += k


@pytest.mark.parametrize("value", ["margin", "prob"])
@pytest.mark.parametrize("columns", [("score",), ("label", "score")])
def test_writer_cpu_equals_python_loop(tmp_path, columns, value):
    from parameter_server_amd.ops.scoretext import PredictionWriter

    n, chunk = 1037, 250  # four whole chunks and a partial one
    x = np.concatenate([domain_bits(n - 40, 3), boundary_values()[:40]])
    m = torch.from_numpy(x.copy())
    m[::11] = torch.tensor(-60.0)  # (a probability under 1e-22)
    y = torch.where(torch.arange(n) % 3 == 0, 1.0, -1.0)
    two = len(columns) == 2
    path = tmp_path / "deep" / "dir" / "pred"
    with PredictionWriter(str(path), "cpu", columns=columns, value=value, chunk_rows=chunk) as w:
        append_unevenly(w, m, y if two else None)
        out = w.close()
    s = torch.sigmoid(m) if value == "prob" else m
    want = python_lines(s.numpy(), y.numpy() if two else None)
    assert path.read_bytes() == want
    assert out == {"rows": n, "bytes": len(want), "chunks": 5, "deferred_chunks": 0}
    assert w.close() == out  # (idempotent)


def test_writer_cpu_empty_and_arguments(tmp_path):
    from parameter_server_amd.ops.scoretext import (PredictionWriter, format_scores,
                                                    format_scores_host)

    with PredictionWriter(str(tmp_path / "none"), "cpu") as w:
        pass
    assert (tmp_path / "none").read_bytes() == b"" and w.close()["rows"] == 0
    with PredictionWriter(str(tmp_path / "zero"), "cpu", columns=("label", "score")) as w:
        for _ in range(3):
            w.append(torch.ones(4), torch.ones(4), rows=0)
    assert (tmp_path / "zero").read_bytes() == b""
    assert w.close() == {"rows": 0, "bytes": 0, "chunks": 0, "deferred_chunks": 0}
    with pytest.raises(ValueError):
        w.append(torch.ones(1), torch.ones(1))  # closed
    with pytest.raises(ValueError):
        PredictionWriter(str(tmp_path / "x"), "cpu", text_io="device")
    for kw in (dict(text_io="gpu"), dict(value="logit"), dict(columns=("score", "label")),
               dict(chunk_rows=0)):
        with pytest.raises(ValueError):
            PredictionWriter(str(tmp_path / "x"), "cpu", **kw)
    with PredictionWriter(str(tmp_path / "y"), "cpu", columns=("label", "score")) as w:
        with pytest.raises(ValueError):
            w.append(torch.ones(2))  # no labels
        with pytest.raises(ValueError):
            w.append(torch.ones(2), torch.ones(2), rows=3)
    x = torch.tensor([0.0, -0.0, 1.5, float("inf"), float("nan"), 1e-30, -2e9])
    assert format_scores(x) == format_scores_host(x) == b"0\n-0\n1.5\ninf\nnan\n1e-30\n-2e+09\n"
    assert format_scores(x[:3], x[:3]) == b"0\t0\n-0\t-0\n1.5\t1.5\n"
    assert format_scores(x[:0]) == b""


# ---------------------------------------------------------------- scorer and app
def make_feeder(files, text, device, minibatch=256, num_features=0):
    """The feeder ``app/gpu._score_files`` builds for these files."""
    from parameter_server_amd.data.feeder import DeviceFeeder

    return DeviceFeeder(list(files), text, minibatch, minibatch * 128, torch.device(device),
                        num_features=num_features, passes=1, shuffle=False, nthreads=2,
                        ignore_slot=True, cache_dir=None)


def predict_files(scorer, files, text, device, minibatch=256, num_features=0):
    """(margins, labels) of ``ModelScorer.predict`` over the files, in the feeder's order."""
    feeder = make_feeder(files, text, device, minibatch, num_features)
    ms, ys = [], []
    for b in feeder.iter_pass(0):
        kw = dict(row_ptr=b.row_ptr[:b.rows + 1]) if b.row_ptr is not None else \
            dict(width=b.width)
        ms.append(scorer.predict(b.keys[:b.nnz], vals=b.vals, **kw).clone())
        ys.append(b.labels[:b.rows].clone())
        feeder.release(b)
    return torch.cat(ms).cpu(), torch.cat(ys).cpu()


def read_predictions(path, ncols=1):
    """The file's columns parsed back as float32 (``%.9g`` round-trips an f32), one row a
    line."""
    rows = [ln.split("\t") for ln in Path(path).read_text().splitlines()]
    assert all(len(r) == ncols for r in rows)
    return np.array([[float(v) for v in r] for r in rows], dtype=np.float64).astype(
        np.float32).reshape(len(rows), ncols)


def same_bits(a, b) -> bool:
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


FIGURES = ("examples", "loss", "accuracy", "auc", "auc_tie_bound")


def eval_with_predictions(tmp_path, device, **flags):
    """The evaluation route on the files of test_app_eval, with and without
    ``-predict_output``: (result with, result without, scorer over the same model, files)."""
    from parameter_server_amd.app.gpu import run_model_evaluation
    from parameter_server_amd.models import ModelScorer
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    data, pattern = tmp_path / "data", str(tmp_path / "model" / "m_S.*")
    if not data.exists():
        _write(str(data), model=str(tmp_path / "model" / "m_S0"))
    lm = load_app_config(str(_eval_conf(tmp_path, data, pattern))).linear_method
    dev = torch.device(device)
    plain = run_model_evaluation(lm, LocalComm(dev), dev, _flags(device=device))
    res = run_model_evaluation(lm, LocalComm(dev), dev, _flags(device=device, **flags))
    sc = ModelScorer.from_text(pattern, key_bits_for(0), dev)
    return res, plain, sc, [str(data / f"part-{p}") for p in range(3)]


def test_app_flags_parse():
    from parameter_server_amd.app.gpu import _flags as parse

    f = parse(["-app_file", "x"])
    assert (f.predict_output, f.predict_value, f.predict_columns) == ("", "margin", "score")
    f = parse(["-predict_output", "out/p", "-predict_value", "prob", "-predict_columns",
               "label,score"])
    assert (f.predict_output, f.predict_value, f.predict_columns) == \
        ("out/p", "prob", "label,score")
    with pytest.raises(SystemExit):
        parse(["-predict_value", "logit"])


def test_app_eval_conf_writes_predictions_cpu(tmp_path):
    out = tmp_path / "pred" / "sub" / "p"
    res, plain, sc, files = eval_with_predictions(tmp_path, "cpu", predict_output=str(out),
                                                  predict_columns="label,score")
    assert [res[k] for k in FIGURES] == [plain[k] for k in FIGURES]
    assert "prediction_file" not in plain
    assert res["prediction_file"] == str(out) + "_W0" and res["prediction_sources"] == files
    assert res["prediction_rows"] == res["rank_examples"] == 3 * ROWS
    assert res["prediction_bytes"] == os.path.getsize(res["prediction_file"])
    assert res["prediction_deferred_chunks"] == 0
    got = read_predictions(res["prediction_file"], 2)
    m, y = predict_files(sc, files, "LIBSVM", "cpu")
    assert same_bits(got[:, 1], m.numpy()) and same_bits(got[:, 0], y.numpy())
    assert Path(res["prediction_file"]).read_bytes() == python_lines(m.numpy(), y.numpy())
    # probabilities, one column
    res_p, _, _, _ = eval_with_predictions(tmp_path, "cpu", predict_output=str(tmp_path / "q"),
                                           predict_value="prob")
    assert same_bits(read_predictions(res_p["prediction_file"])[:, 0], torch.sigmoid(m).numpy())


def test_app_training_conf_writes_validation_predictions_cpu(tmp_path):
    from parameter_server_amd.app.gpu import _result_line, run_async_sgd
    from parameter_server_amd.models import ModelScorer
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    train, val, model = tmp_path / "train", tmp_path / "val", tmp_path / "model" / "m"
    _write(str(train), seed=1)
    _write(str(val), seed=2)
    c = tmp_path / "train.conf"
    c.write_text(f"""linear_method {{
training_data {{ format: TEXT text: LIBSVM file: "{train}/part.*" }}
validation_data {{ format: TEXT text: LIBSVM file: "{val}/part.*" }}
model_output {{ format: TEXT file: "{model}" }}
loss {{ type: LOGIT }}
penalty {{ type: L1 lambda: 0.05 lambda: 0.01 }}
learning_rate {{ type: DECAY alpha: 0.5 beta: 1 }}
async_sgd {{ algo: FTRL minibatch: 200 num_data_pass: 1 report_interval: 100000 }}
}}""")
    lm = load_app_config(str(c)).linear_method
    dev = torch.device("cpu")
    outs = [run_async_sgd(lm, LocalComm(dev), dev, _flags(table_capacity=1 << 16, **kw))
            for kw in ({}, dict(predict_output=str(tmp_path / "vp")))]
    v0, v = outs[0]["validation"], outs[1]["validation"]
    assert [v[k] for k in FIGURES] == [v0[k] for k in FIGURES]
    assert v["prediction_file"] == str(tmp_path / "vp_W0")
    assert v["prediction_rows"] == v["rank_examples"] == 3 * ROWS
    assert f"predictions {v['prediction_file']} ({3 * ROWS} rows)" in _result_line(v)
    files = [str(val / f"part-{p}") for p in range(3)]
    sc = ModelScorer.from_text(f"{model}_S.*", key_bits_for(0), dev)
    m, _ = predict_files(sc, files, "LIBSVM", "cpu", minibatch=200)
    assert same_bits(read_predictions(v["prediction_file"])[:, 0], m.numpy())
    assert float(m.abs().max()) > 0


def _two_rank_worker(rank, world, port, conf, out_dir):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from parameter_server_amd.app.gpu import run_model_evaluation
    from parameter_server_amd.parallel.comm import DistComm
    from parameter_server_amd.utils.config import load_app_config

    lm = load_app_config(conf).linear_method
    res = run_model_evaluation(lm, DistComm("cpu"), torch.device("cpu"),
                               _flags(predict_output=os.path.join(out_dir, "two", "p")))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_app_two_ranks_write_their_own_files(tmp_path):
    import torch.multiprocessing as mp

    res, _, sc, files = eval_with_predictions(tmp_path, "cpu",
                                              predict_output=str(tmp_path / "one"))
    mp.spawn(_two_rank_worker, args=(2, _port(), str(tmp_path / "eval.conf"), str(tmp_path)),
             nprocs=2, join=True)
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=False) for i in range(2)]
    assert [x["prediction_file"] for x in r] == [str(tmp_path / "two" / f"p_W{i}")
                                                 for i in range(2)]
    assert sum(x["prediction_rows"] for x in r) == res["prediction_rows"] == 3 * ROWS
    assert sorted(r[0]["prediction_sources"] + r[1]["prediction_sources"]) == files
    for x in r:
        assert x["prediction_rows"] == x["rank_examples"] == ROWS * len(x["prediction_sources"])
        m, _ = predict_files(sc, x["prediction_sources"], "LIBSVM", "cpu")
        assert same_bits(read_predictions(x["prediction_file"])[:, 0], m.numpy())
        assert x["examples"] == res["examples"] and x["auc"] == res["auc"]
