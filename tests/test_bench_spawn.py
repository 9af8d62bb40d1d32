"""bench.py contract: ``python bench.py --gpus N`` fans out N ranks by itself
(no torchrun in front) and rank 0 prints one JSON line for the whole job."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu", *args],
                         capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_self_spawns_ranks():
    B = 1024
    r = _run("--gpus", "3", "--steps", "2", "--warmup", "1", "--minibatch", str(B),
             "--num-features", "1e6")
    assert r["n_gpus"] == 3
    assert r["config"]["global_batch"] == 3 * B
    assert r["config"]["parallelism"] == "dp3+kvshard3"
    assert r["value"] > 0 and r["steps"] == 2


def test_bench_single_rank_unchanged():
    B = 1024
    r = _run("--gpus", "1", "--steps", "2", "--warmup", "1", "--minibatch", str(B),
             "--num-features", "1e6")
    assert r["n_gpus"] == 1 and r["config"]["global_batch"] == B
    for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data"):
        assert k in r


def test_bench_dump_outputs_and_full(tmp_path, monkeypatch):
    """``--dump-outputs DIR`` writes the trained state and the progress behind the line's
    train block as float32 / float64 ``.npy``; a second run with the same arguments (here
    with ``--full``, which adds nothing to the line's headline fields) writes the same
    arrays: the inputs do not change from run to run, and the CPU path applies them in one
    order."""
    import numpy as np

    monkeypatch.setenv("PSAMD_PRE_TIMING_ITERS", "2")  # (bench.py's default, pinned here)
    a = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--minibatch", "512",
         "--num-features", "1e5")
    r1 = _run(*a, "--dump-outputs", str(tmp_path / "a"))
    r2 = _run(*a, "--full", "--dump-outputs", str(tmp_path / "b"))
    for r in (r1, r2):
        assert r["steps"] == 3 and r["ms_per_step"] > 0
        assert abs(r["value"] * r["ms_per_step"] * 1e-3 - 512) < 1e-6 * 512
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["keys.npy", "n.npy", "progress.npy", "w.npy", "z.npy"]
    out = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 64 << 20
    k = out["keys.npy"]
    assert k.size == r1["train"]["table_occupied_rank0"] > 0 and np.all(np.diff(k) > 0)
    assert out["w.npy"].shape == out["z.npy"].shape == out["n.npy"].shape == k.shape
    # examples: the 3 timed steps and the 2 untimed iterations right before them
    assert out["progress.npy"][0] == (3 + 2) * 512
    assert abs(out["progress.npy"][1] - r1["train"]["loss"]) < 1e-12
    for n in names:
        assert np.array_equal(out[n], np.load(tmp_path / "b" / n)), n


def test_dump_outputs_samples_large_state(tmp_path):
    """More rows than ``max_rows``: exactly ``max_rows`` are written, still sorted by key
    with each key's own w / z / n (also from bf16 state), and the same rows whatever
    order the table handed them over in."""
    import importlib.util

    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location("psamd_bench_dump",
                                                  os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.DUMP_MAX_ROWS * (8 + 3 * 4) + 6 * 8 + 5 * 128 <= 64 << 20  # (.npy headers)
    n, cap = 1000, 64
    g = torch.Generator().manual_seed(5)
    keys = torch.randperm(10 ** 6, generator=g)[:n]
    sd = {"keys": keys, "w": (keys % 251).float() / 8, "z": -(keys % 127).float(),
          "n": (keys % 63).to(torch.bfloat16)}  # (all exact in bf16 / fp32)
    prog = dict(examples=1.0, loss=0.5, accuracy=0.75, auc=0.7, nnz_w=3.0, updt_ratio=0.1)
    bench.dump_outputs(str(tmp_path / "a"), sd, prog, max_rows=cap)
    perm = torch.randperm(n, generator=g)
    bench.dump_outputs(str(tmp_path / "b"), {k: v[perm] for k, v in sd.items()}, prog,
                       max_rows=cap)
    a = {x: np.load(tmp_path / "a" / (x + ".npy")) for x in ("keys", "w", "z", "n", "progress")}
    k = a["keys"].astype(np.int64)
    assert k.shape == (cap,) and np.all(np.diff(k) > 0) and np.isin(k, keys.numpy()).all()
    assert a["w"].dtype == a["z"].dtype == a["n"].dtype == np.float32
    assert np.array_equal(a["w"], (k % 251) / 8) and np.array_equal(a["z"], -(k % 127.0))
    assert np.array_equal(a["n"], k % 63)
    assert a["progress"].tolist() == [1.0, 0.5, 0.75, 0.7, 3.0, 0.1]
    for x in a:
        assert np.array_equal(a[x], np.load(tmp_path / "b" / (x + ".npy"))), x
    bench.dump_outputs(str(tmp_path / "c"), sd, prog, max_rows=n)  # (at the cap: every row)
    assert np.array_equal(np.load(tmp_path / "c" / "keys.npy"), np.sort(keys.numpy()))


def test_bench_stalled_rank_fails_fast():
    """A rank that stops joining collectives (injected sleep at timed step 1) makes the
    job exit non-zero within the collective timeout, and the surviving ranks name
    their rank, phase, step and last collective (no silent hang)."""
    import time

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(PSAMD_COMM_TIMEOUT="8", PSAMD_INJECT_STALL="1:1:600")
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu", "--gpus", "3",
                          "--steps", "4", "--warmup", "1", "--minibatch", "1024",
                          "--num-features", "1e6"],
                         capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    dt = time.time() - t0
    assert out.returncode != 0
    assert dt < 120, dt
    assert "[psamd] FAILED rank 0: phase timed" in out.stderr or \
        "[psamd] FAILED rank 2: phase timed" in out.stderr, out.stderr[-3000:]
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]


def test_bench_failed_captured_attempt_reruns_eagerly():
    """Multi-rank runs go through per-rank supervisors: when the first attempt (the
    collectives captured in the step graphs) fails on the ranks, every supervisor re-runs
    the job in fresh processes with eager collectives, and rank 0 still prints exactly
    one JSON line, which records the fallback."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(PSAMD_INJECT_CAPTURE_FAIL="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu", "--gpus", "3",
                          "--steps", "2", "--warmup", "1", "--minibatch", "1024",
                          "--num-features", "1e6"],
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "re-running in fresh processes with eager collectives" in out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 3 and r["comm"]["fallback"] == 3 and r["comm"]["captured"] is False


def _spawn_env(**extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra)
    return env


def test_bench_post_timing_rank_failure_is_reported():
    """A rank that exits non-zero AFTER the timed region (rank 2, injected) does not void
    the measurement, but the JSON line records which rank failed with what code."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu", "--gpus", "3",
                          "--steps", "2", "--warmup", "1", "--minibatch", "1024",
                          "--num-features", "1e6"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT,
                         env=_spawn_env(PSAMD_INJECT_POST_EXIT="2:7"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["comm"]["post_timing_failures"] == [2]
    assert r["comm"]["rank_exit_codes"][2] == 7
    assert "re-running" not in out.stderr  # a complete measurement is not re-run


def test_bench_teardown_hang_is_capped():
    """A rank hanging after the timed region is killed PSAMD_TEARDOWN_TIMEOUT seconds
    after it passed the timed region, not at the attempt limit."""
    import time

    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu", "--gpus", "2",
                          "--steps", "2", "--warmup", "1", "--minibatch", "1024",
                          "--num-features", "1e6"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT,
                         env=_spawn_env(PSAMD_INJECT_TEARDOWN_HANG="1:600",
                                        PSAMD_TEARDOWN_TIMEOUT="5"))
    assert out.returncode == 0, out.stderr[-3000:]
    assert time.time() - t0 < 150
    r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert r["comm"]["post_timing_failures"] == [1]
    assert r["comm"]["rank_exit_codes"][1] == 125
