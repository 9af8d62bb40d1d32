"""The GPU app's evaluation route (app/gpu.py run_model_evaluation): a conf with
``validation_data`` + ``model_input`` scores the stored ``key\\tweight`` model on LIBSVM
files through DeviceFeeder + ModelScorer, against the CPU evaluator
(app/linear_method/model_evaluation.py evaluate_model: fp64 margins, exact AUC)."""
import os
import socket
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NKEYS, ROWS, SEED = 3000, 400, 0


def _write(d, seed=SEED, nfiles=3, rows=ROWS, model=None):
    """Three LIBSVM files of valued rows (5..40 keys below NKEYS, so ``-num_features 4096``
    hashes them onto themselves) and a text model holding ~90 % of the keys."""
    from parameter_server_amd.utils.checkpoint import write_text_model

    rng, wrng = np.random.default_rng(seed), np.random.default_rng(1234)  # one planted model
    w = (wrng.normal(0, 1, NKEYS) * (wrng.random(NKEYS) < 0.9)).astype(np.float32)
    os.makedirs(d, exist_ok=True)
    for p in range(nfiles):
        with open(os.path.join(d, f"part-{p}"), "w") as f:
            for _ in range(rows):
                k = np.unique(rng.integers(1, NKEYS, size=int(rng.integers(5, 40))))
                v = rng.random(k.size)
                y = 1 if (w[k] * v).sum() + 0.5 * rng.normal() > 0 else -1
                f.write(f"{y} " + " ".join(f"{a}:{b:.4f}" for a, b in zip(k, v)) + "\n")
    if model is not None:
        write_text_model(model, np.arange(NKEYS, dtype=np.uint64), w)


def _eval_conf(tmp_path, data, model_pattern, name="eval.conf"):
    c = tmp_path / name
    c.write_text(f"""linear_method {{
validation_data {{ format: TEXT text: LIBSVM file: "{data}/part.*" }}
model_input {{ format: TEXT file: "{model_pattern}" }}
loss {{ type: LOGIT }}
}}""")
    return c


def _flags(**kw):
    d = dict(app_file=None, app_conf=None, num_features=0, max_nnz_per_example=128,
             num_threads=2, device="cpu", seed=0, table_capacity=0, quiet=True, minibatch=256)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _reference(data, model_pattern):
    """evaluate_model's figures, and per row the fp64 margin and the derived f32 bound
    (ops/score.row_bound) from the same files and model."""
    from parameter_server_amd.app.linear_method.model_evaluation import evaluate_model
    from parameter_server_amd.data import ExampleBatch, parse_text, read_file
    from parameter_server_amd.ops.score import row_bound
    from parameter_server_amd.utils.checkpoint import read_text_models

    files = [str(data / f"part-{p}") for p in range(3)]
    model = read_text_models(model_pattern)
    ref = evaluate_model(model, files, "LIBSVM")
    b = ExampleBatch.concat([parse_text(read_file(f), "LIBSVM", ignore_slot=True) for f in files])
    m_ref, bound = row_bound(torch.from_numpy(b.keys.view(np.int64).copy()), model,
                             torch.from_numpy(b.vals.astype(np.float32)),
                             torch.from_numpy(b.row_ptr.astype(np.int64)))
    return ref, m_ref, bound, torch.from_numpy(b.labels.astype(np.float32))


def _check_against_cpu_evaluator(res, data, pattern):
    ref, m_ref, bound, labels = _reference(data, pattern)
    assert res["examples"] == ref["examples"] == 3 * ROWS
    assert abs(res["auc"] - ref["auc"]) <= res["auc_tie_bound"] + 1e-6
    # accuracy: exact once the rows whose sign f32 rounding could flip are set aside
    aside = m_ref.abs() <= bound
    assert int(aside.sum()) <= 0.01 * m_ref.numel()
    sure = int((((labels > 0) == (m_ref > 0)) & ~aside).sum())
    for correct in (round(res["accuracy"] * res["examples"]),
                    round(ref["accuracy"] * ref["examples"])):
        assert sure <= correct <= sure + int(aside.sum())
    assert 0 < res["loss"] < 0.6 and res["auc"] > 0.8


def test_reference_alone_sets_aside_under_one_percent(tmp_path):
    """The seed's property the accuracy check relies on, from the fp64 reference alone."""
    _write(str(tmp_path / "data"), model=str(tmp_path / "model" / "m_S0"))
    _, m_ref, bound, _ = _reference(tmp_path / "data", str(tmp_path / "model" / "m_S.*"))
    assert int((m_ref.abs() <= bound).sum()) <= 0.01 * m_ref.numel()


def _eval_route(tmp_path, device, num_features):
    from parameter_server_amd.app.gpu import route, run_model_evaluation
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    data, pattern = tmp_path / "data", str(tmp_path / "model" / "m_S.*")
    _write(str(data), model=str(tmp_path / "model" / "m_S0"))
    lm = load_app_config(str(_eval_conf(tmp_path, data, pattern))).linear_method
    assert route(lm) is run_model_evaluation
    dev = torch.device(device)
    res = run_model_evaluation(lm, LocalComm(dev), dev,
                               _flags(device=device, num_features=num_features))
    _check_against_cpu_evaluator(res, data, pattern)
    return res


@pytest.mark.parametrize("num_features", [0, 4096])
def test_eval_route_cpu_matches_cpu_evaluator(tmp_path, num_features):
    _eval_route(tmp_path, "cpu", num_features)


@pytest.mark.gpu
@pytest.mark.parametrize("num_features", [0, 4096])
def test_eval_route_gpu_matches_cpu_evaluator(tmp_path, num_features):
    res = _eval_route(tmp_path, "cuda", num_features)
    assert res["h2d_bytes"] > 0


def test_golden_eval_conf_routes_to_model_evaluation(monkeypatch):
    """tests/golden/confs/eval_model.conf (no solver block) parses and ``main`` hands it
    to run_model_evaluation; the files it names do not exist, so the function is a stub."""
    from parameter_server_amd.app import gpu
    from parameter_server_amd.utils.config import load_app_config

    conf = os.path.join(ROOT, "tests", "golden", "confs", "eval_model.conf")
    lm = load_app_config(conf).linear_method
    assert lm.model_input.file[0] == "out/online_ftrl_S.*"
    assert gpu.route(lm) is gpu.run_model_evaluation
    seen = []

    def stub(lm, comm, device, flags):
        seen.append((lm.validation_data.text, comm.world, device.type, flags.minibatch))
        return {"examples": 0, "seconds": 1.0}

    monkeypatch.setattr(gpu, "run_model_evaluation", stub)
    assert gpu.main(["-app_file", conf, "-device", "cpu", "-quiet"]) == 0
    assert seen == [("SPARSE_BINARY", 1, "cpu", 65536)]


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, conf, out_dir):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from parameter_server_amd.app.gpu import run_model_evaluation
    from parameter_server_amd.parallel.comm import DistComm
    from parameter_server_amd.utils.config import load_app_config

    lm = load_app_config(conf).linear_method
    res = run_model_evaluation(lm, DistComm("cpu"), torch.device("cpu"), _flags())
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


FIGURES = ("examples", "accuracy", "auc", "auc_tie_bound")


def test_eval_route_two_ranks_equal_one(tmp_path):
    """3 files over 2 gloo ranks (2 + 1): the all-reduced figures are the 1-rank run's."""
    import torch.multiprocessing as mp

    one = _eval_route(tmp_path, "cpu", 0)
    conf = str(tmp_path / "eval.conf")
    mp.spawn(_two_rank_worker, args=(2, _port(), conf, str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=False) for i in range(2)]
    assert sorted(x["rank_examples"] for x in r) == [ROWS, 2 * ROWS]
    for x in r:
        assert [x[k] for k in FIGURES] == [one[k] for k in FIGURES]
        assert abs(x["loss"] - one["loss"]) <= 1e-12 * one["loss"]


def test_darlin_model_scored_through_the_eval_route(tmp_path):
    """A model trained by run_darlin (SPARSE_BINARY files) is scored from its text file
    like any other: same examples as evaluate_model, AUC within the tie bound."""
    from test_app_gpu import _darlin_files
    from test_app_gpu import _flags as train_flags

    from parameter_server_amd.app.gpu import run_darlin, run_model_evaluation
    from parameter_server_amd.app.linear_method.model_evaluation import evaluate_model
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.checkpoint import read_text_models
    from parameter_server_amd.utils.config import load_app_config

    data, model, conf = _darlin_files(tmp_path)
    dev = torch.device("cpu")
    run_darlin(load_app_config(str(conf)).linear_method, LocalComm(dev), dev, train_flags())
    c = tmp_path / "eval.conf"
    c.write_text(f"""linear_method {{
validation_data {{ format: TEXT text: SPARSE_BINARY file: "{data}/part.*" }}
model_input {{ format: TEXT file: "{model}_S.*" }}
}}""")
    res = run_model_evaluation(load_app_config(str(c)).linear_method, LocalComm(dev), dev,
                               _flags())
    ref = evaluate_model(read_text_models(f"{model}_S.*"),
                         sorted(str(p) for p in data.iterdir()), "SPARSE_BINARY")
    assert res["examples"] == ref["examples"] == 1800 and res["model_entries"] > 10
    assert abs(res["auc"] - ref["auc"]) <= res["auc_tie_bound"] + 1e-6 and res["auc"] > 0.7


def test_training_conf_with_validation_data_scores_after_training(tmp_path):
    """A training conf that also has validation_data: ``out["validation"]`` (scored from
    the trainer's own table) equals a separate evaluation run on the saved model."""
    from parameter_server_amd.app.gpu import run_async_sgd, run_model_evaluation
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
    out = run_async_sgd(lm, LocalComm(dev), dev, _flags(table_capacity=1 << 16))
    v = out["validation"]
    assert v["examples"] == 3 * ROWS and v["auc"] > 0.6
    lm_e = load_app_config(str(_eval_conf(tmp_path, val, f"{model}_S.*"))).linear_method
    e = run_model_evaluation(lm_e, LocalComm(dev), dev, _flags())
    assert [v[k] for k in FIGURES] == [e[k] for k in FIGURES]
    assert abs(v["loss"] - e["loss"]) <= 1e-12 * e["loss"]
