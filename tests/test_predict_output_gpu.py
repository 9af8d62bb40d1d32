"""Per-example prediction files on the device (scoretext.hip, ops/scoretext.py,
``ModelScorer.evaluate(predictions=)``, the app's ``-predict_output``) against the plain
Python loop on the same floats: the kernels byte for byte at every boundary of the work
decomposition and every alignment of a block's first byte, the capacity check, deferral of a
chunk that holds a value outside the formatter's domain, the streaming writer against its
host route, and the scorer and app routes against ``ModelScorer.predict``.

Unless a test says otherwise its inputs are inside the formatter's domain (filtered with
the host formatter's status, checked below), so the device may defer none of them."""
import os

import numpy as np
import pytest
import torch

from test_app_eval import NKEYS, ROWS, _reference
from test_predict_output import (FIGURES, append_unevenly, boundary_values, domain_bits,
                                 eval_with_predictions, make_feeder, predict_files,
                                 python_lines, read_predictions, same_bits, score_domain)

from parameter_server_amd.ops.native import core, hipops
from parameter_server_amd.ops.scoretext import PredictionWriter, format_scores

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 1024  # rows per workgroup (scoretext.hip)
CANARY = 0xA5


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)


def _host_ok(x: np.ndarray) -> bool:
    st = core().textfmt_scores(np.ascontiguousarray(x, np.float32).view(np.uint32))[1]
    return bool(np.all(st == 0))


_CORPORA = {}


def corpus_of(kind: str) -> np.ndarray:
    """2E + 1 float32 values: "short" every line ``0``, "long" every value 15 characters,
    "mixed" random in-domain bits, the in-domain boundary values and zeros of both signs."""
    if kind not in _CORPORA:
        n = 2 * E + 1
        if kind == "short":
            x = np.zeros(n, np.float32)
        elif kind == "long":
            x = domain_bits(40 * n, 17)
            x = x[np.array([len("%.9g" % float(v)) == 15 for v in x])][:n]
        else:
            b = boundary_values()
            b = b[score_domain(b)]
            x = np.concatenate([domain_bits(n - b.size - 64, 19), b,
                                np.tile(np.array([0.0, -0.0], np.float32), 32)])
            np.random.default_rng(23).shuffle(x)
        assert x.size == n and x.dtype == np.float32 and score_domain(x).all() and _host_ok(x)
        _CORPORA[kind] = x
    return _CORPORA[kind]


def run_kernels(score, label, cap=None, tail=64, skew=0):
    """One ``scoretext_format`` call into a canary-filled buffer whose first byte sits
    ``skew`` bytes past a 16-byte boundary: (header, the whole buffer)."""
    ops = hipops()
    n = score.shape[0]
    want_len = len(python_lines(score, label))
    cap = want_len if cap is None else cap
    buf = torch.full((16 + max(cap, want_len) + tail,), CANARY, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[skew:]
    hdr = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    work = torch.empty(int(ops.scoretext_work_bytes(n)), dtype=torch.uint8, device=DEV)
    a, b = (_dev(score), None) if label is None else (_dev(label), _dev(score))
    ops.scoretext_format(a, b, out, hdr, work, cap)
    torch.cuda.synchronize()
    return hdr.cpu().tolist(), out.cpu().numpy()


def check_kernels(score, label, skew=0):
    """The text equals the oracle with the capacity exactly the text's size, and nothing
    past it is written."""
    want = python_lines(score, label)
    (nbytes, ndefer, over), out = run_kernels(score, label, skew=skew)
    assert (nbytes, ndefer, over) == (len(want), 0, 0)
    got = out[:nbytes].tobytes()
    if got != want:
        i = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), -1)
        raise AssertionError(f"n={len(score)} skew={skew}: first difference at {i}: "
                             f"{got[max(0, i - 40):i + 40]!r} vs {want[max(0, i - 40):i + 40]!r}")
    assert np.all(out[nbytes:] == CANARY)


def test_block_size_and_line_bounds():
    ops = hipops()
    assert int(ops.scoretext_block()) == E
    assert int(ops.scoretext_max_line(1)) == 16 and int(ops.scoretext_max_line(2)) == 32
    assert len(python_lines(corpus_of("long")[:1])) == 16


@pytest.mark.parametrize("kind", ["short", "long", "mixed"])
@pytest.mark.parametrize("two", [False, True], ids=["score", "label_score"])
def test_kernels_equal_python_loop(kind, two):
    x = corpus_of(kind)
    y = x[::-1].copy() if kind != "mixed" else np.where(np.arange(x.size) % 3 == 0, 1.0,
                                                         -1.0).astype(np.float32)
    for n in (0, 1, 2, E - 1, E, E + 1, 2 * E + 1):
        check_kernels(x[:n], y[:n] if two else None)
    # 0..15 one-character-score lines first, the buffer itself starting p bytes past a
    # 16-byte boundary: the first block boundary on every residue mod 16
    for p in range(16):
        one = np.full(p, 7.0, np.float32)
        for n in (E - 1, E + 1, 2 * E + 1):
            check_kernels(np.concatenate([one, x[:n]]),
                          np.concatenate([one, y[:n]]) if two else None, skew=p)


@pytest.mark.parametrize("two", [False, True], ids=["score", "label_score"])
def test_capacity_one_byte_short_writes_nothing(two):
    x = corpus_of("mixed")
    y = corpus_of("long") if two else None
    want = python_lines(x, y)
    (nbytes, ndefer, over), out = run_kernels(x, y, cap=len(want) - 1)
    assert (nbytes, ndefer, over) == (len(want), 0, 1)
    assert np.all(out == CANARY)  # (nothing at all, the canary past the size included)
    (nbytes, ndefer, over), out = run_kernels(x, y, cap=len(want))
    assert over == 0 and out[:nbytes].tobytes() == want and np.all(out[nbytes:] == CANARY)


ODD = {"inf": np.inf, "nan": np.nan, "1e9": 1e9, "subnormal": 1e-40}


@pytest.mark.parametrize("odd", sorted(ODD))
def test_one_out_of_domain_value_defers_its_chunk(tmp_path, odd):
    x = corpus_of("mixed")[:3 * 512].copy()
    y = np.where(np.arange(x.size) % 2 == 0, 1.0, -1.0).astype(np.float32)
    x[512 + 300] = ODD[odd]  # the middle chunk of three
    assert not _host_ok(x) and _host_ok(np.delete(x, 512 + 300))
    (nbytes, ndefer, over), _ = run_kernels(x[512:1024], None)
    assert ndefer == 1 and over == 0
    (_, ndefer, _), _ = run_kernels(x[512:1024], y[512:1024])  # (in the second column)
    assert ndefer == 1
    for two in (False, True):
        path = tmp_path / f"p{int(two)}"
        with PredictionWriter(str(path), DEV, columns=("label", "score") if two else ("score",),
                              text_io="device", chunk_rows=512) as w:
            w.append(_dev(x), _dev(y))
        assert path.read_bytes() == python_lines(x, y if two else None)
        assert w.close()["deferred_chunks"] == 1 and w.close()["chunks"] == 3
    assert format_scores(_dev(x)) == python_lines(x)


@pytest.mark.parametrize("value", ["margin", "prob"])
@pytest.mark.parametrize("two", [False, True], ids=["score", "label_score"])
def test_device_writer_equals_host_writer(tmp_path, two, value):
    n = 9 * E + 3
    x = np.concatenate([corpus_of("mixed")] * 5)[:n].copy()
    if value == "prob":  # margins whose probability stays inside the domain
        x = np.clip(x, -40.0, 40.0)
    y = np.where(np.arange(n) % 3 == 0, 1.0, -1.0).astype(np.float32)
    m, lab = _dev(x), _dev(y)
    cols = ("label", "score") if two else ("score",)
    outs = {}
    for io in ("device", "host"):
        path = tmp_path / io
        with PredictionWriter(str(path), DEV, columns=cols, value=value, text_io=io,
                              chunk_rows=2 * E) as w:
            append_unevenly(w, m, lab if two else None)
        outs[io] = (path.read_bytes(), w.close())
    assert outs["device"][0] == outs["host"][0]
    want = python_lines(torch.sigmoid(m).cpu().numpy() if value == "prob" else x,
                        y if two else None)
    assert outs["host"][0] == want
    assert outs["device"][1] == outs["host"][1] == \
        {"rows": n, "bytes": len(want), "chunks": 5, "deferred_chunks": 0}
    assert format_scores(m[:E + 5], lab[:E + 5] if two else None) == \
        python_lines(x[:E + 5], y[:E + 5] if two else None)


def test_prob_below_the_domain_defers_but_matches(tmp_path):
    """sigmoid(-60) < 1e-22: the chunk is the host loop's, the file the same."""
    m = torch.linspace(-70.0, 30.0, 3 * 256, device=DEV)
    with PredictionWriter(str(tmp_path / "p"), DEV, value="prob", chunk_rows=256) as w:
        w.append(m)
    assert (tmp_path / "p").read_bytes() == python_lines(torch.sigmoid(m).cpu().numpy())
    assert w.close()["deferred_chunks"] == 1


# ---------------------------------------------------------------- scorer
def _small_files(d):
    """A model of the keys below NKEYS; two valued LIBSVM files and two binary files of a
    few hundred rows, some of them without any key of the model (and one without keys)."""
    from parameter_server_amd.utils.checkpoint import write_text_model

    rng = np.random.default_rng(31)
    w = rng.normal(0, 1, NKEYS).astype(np.float32)
    os.makedirs(d / "model", exist_ok=True)
    write_text_model(str(d / "model" / "m_S0"), np.arange(NKEYS, dtype=np.uint64), w)
    files = {"LIBSVM": [], "SPARSE_BINARY": []}
    for text in files:
        for p in range(2):
            path = d / f"{text.lower()}-{p}"
            with open(path, "w") as f:
                for r in range(150 + 37 * p):
                    lo, hi = (1, NKEYS) if r % 9 else (NKEYS + 100, NKEYS + 5000)  # unknown
                    k = np.unique(rng.integers(lo, hi, size=int(rng.integers(1, 30))))
                    y = int(rng.integers(0, 2))
                    if text == "LIBSVM":
                        f.write(f"{2 * y - 1} " + " ".join(
                            f"{a}:{b:.4f}" for a, b in zip(k, rng.random(k.size))) + "\n")
                    elif r == 77:
                        f.write(f"{y}\n")
                    else:
                        f.write(f"{y}; 1 " + " ".join(map(str, k)) + "\n")
            files[text].append(str(path))
    return files


@pytest.mark.parametrize("text", ["LIBSVM", "SPARSE_BINARY"])
def test_scorer_evaluate_with_writer(tmp_path, text):
    from parameter_server_amd.models import ModelScorer
    from parameter_server_amd.ops.keymix import key_bits_for

    files = _small_files(tmp_path)[text]
    pattern, bits = str(tmp_path / "model" / "m_S.*"), key_bits_for(0)
    # (8 rows a minibatch: one wave of the probe kernel holds them all, so the f64 sums are
    # added in one order and "exactly" is a property of the code, not of the scheduling)
    B = 8
    plain = ModelScorer.from_text(pattern, bits, DEV).evaluate(make_feeder(files, text, DEV, B))
    sc = ModelScorer.from_text(pattern, bits, DEV)
    with PredictionWriter(str(tmp_path / "pred"), DEV, columns=("label", "score"),
                          text_io="device", chunk_rows=100) as w:
        sc.evaluate(make_feeder(files, text, DEV, B), predictions=w)
    torch.cuda.synchronize()
    m, y = predict_files(sc, files, text, DEV, B)
    got = read_predictions(tmp_path / "pred", 2)
    assert m.numel() == 2 * 150 + 37 == w.close()["rows"] and w.close()["deferred_chunks"] == 0
    assert same_bits(got[:, 1], m.numpy()) and same_bits(got[:, 0], y.numpy())
    assert int((m == 0).sum()) >= 2 * 150 // 9 and float(m.abs().max()) > 0
    assert sc.result() == plain.result()
    (sa, ca), (sb, cb) = sc.totals(), plain.totals()
    assert torch.equal(sa, sb) and torch.equal(ca, cb)


# ---------------------------------------------------------------- app
def test_app_predict_output_gpu_against_cpu_route(tmp_path):
    """The same number of lines as the CPU route, every margin within the row bounds of
    tests/test_score_gpu.py (each route within the bound of the fp64 reference, so within
    twice it of the other), and ``-predict_value prob`` = torch.sigmoid of the margin
    file's values on the device."""
    (tmp_path / "c").mkdir()
    res_c, _, _, _ = eval_with_predictions(tmp_path, "cpu", predict_output=str(tmp_path / "c/p"))
    res_g, plain_g, sc, files = eval_with_predictions(tmp_path, DEV,
                                                      predict_output=str(tmp_path / "g/p"))
    exact = [k for k in FIGURES if k != "loss"]  # (the loss: f64 atomics in any order)
    assert [res_g[k] for k in exact] == [plain_g[k] for k in exact]
    assert abs(res_g["loss"] - plain_g["loss"]) <= 1e-12 * plain_g["loss"]
    assert res_g["prediction_rows"] == res_c["prediction_rows"] == 3 * ROWS
    assert res_g["prediction_deferred_chunks"] == 0
    mc = read_predictions(res_c["prediction_file"])[:, 0].astype(np.float64)
    mg = read_predictions(res_g["prediction_file"])[:, 0]
    _, m_ref, bound, _ = _reference(tmp_path / "data", str(tmp_path / "model" / "m_S.*"))
    m_ref, bound = m_ref.numpy(), bound.numpy()
    assert np.all(np.abs(mg.astype(np.float64) - m_ref) <= bound)
    assert np.all(np.abs(mc - m_ref) <= bound)
    assert np.all(np.abs(mg.astype(np.float64) - mc) <= 2 * bound)
    m, _ = predict_files(sc, files, "LIBSVM", DEV)
    assert same_bits(mg, m.numpy())
    res_p, _, _, _ = eval_with_predictions(tmp_path, DEV, predict_output=str(tmp_path / "g/q"),
                                           predict_value="prob", predict_columns="label,score")
    got = read_predictions(res_p["prediction_file"], 2)
    assert same_bits(got[:, 1], torch.sigmoid(torch.from_numpy(mg).to(DEV)).cpu().numpy())
    assert set(np.unique(got[:, 0]).tolist()) == {-1.0, 1.0}
