"""Shared by test_warm_start.py and test_warm_start_gpu.py: model files, the float64 state
formulas, the plain fp32 PyTorch loop of ``apply_update`` (kv_slot.cuh) and the app conf of
a warm-started run."""
import os
import types

import numpy as np
import torch

# the headline penalties and learning rate (SparseLRConfig defaults)
L1, L2, ALPHA, BETA = 10.0, 1.0, 0.01, 10.0


def entries(n: int, seed: int, num_features: int = 0):
    """n distinct raw keys (uint64; num_features = 0: raw 64-bit keys, half of them with the
    top bit set) and weights of both signs with magnitudes 1e-6 .. 1e3."""
    rng = np.random.default_rng(seed)
    if num_features:
        k = rng.choice(num_features, n, replace=False).astype(np.uint64)
    else:
        k = np.unique(rng.integers(0, 1 << 63, 2 * n, dtype=np.uint64))[:n]
        rng.shuffle(k)
        k[::2] |= np.uint64(1 << 63)
    w = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
    assert np.unique(k).size == n and (w != 0).all()
    return k, w


def write_model(path: str, k: np.ndarray, w: np.ndarray) -> str:
    from parameter_server_amd.utils.checkpoint import write_text_model

    write_text_model(path, k.astype(np.uint64), w.astype(np.float32))
    return path


def eta0_of(lr_type: str, n0: float, alpha=ALPHA, beta=BETA) -> float:
    return alpha if lr_type == "constant" else alpha / (n0 + beta)


def seed_state64(w: np.ndarray, algo: str, lr_type: str, n0: float, alpha=ALPHA, beta=BETA,
                 l1=L1, l2=L2):
    """(z, n) that reproduce ``w``, in float64 (n: the exact float32 the table holds)."""
    w = w.astype(np.float64)
    if algo == "ftrl":
        inv_eta0 = 1.0 / alpha if lr_type == "constant" else (n0 + beta) / alpha
        return -(w * (inv_eta0 + l2) + np.copysign(l1, w)), np.float32(n0)
    if algo == "adagrad":
        return np.zeros_like(w), np.float32(n0) * np.float32(n0)
    return np.zeros_like(w), np.float32(0.0)


def prox32(zz, eta, l1, l2):
    """soft_threshold_prox (kv_slot.cuh) in numpy float32."""
    zz, eta, l1, l2 = (np.float32(v) for v in (zz, eta, l1, l2))
    leta = l1 * eta
    out = np.where(zz > 0, zz - leta, zz + leta) / (np.float32(1) + l2 * eta)
    return np.where(np.abs(zz) <= leta, np.float32(0), out).astype(np.float32)


def sorted_state(tr):
    """state_dict of a trainer ordered by raw key (unsigned): (keys u64, w, z, n) numpy."""
    sd = tr.state_dict()
    k = sd["keys"].numpy().view(np.uint64)
    o = np.argsort(k)
    return k[o], sd["w"].numpy()[o], sd["z"].numpy()[o], sd["n"].numpy()[o]


def minibatches(steps: int, B: int, width: int, num_features: int, seed: int, device="cpu"):
    """Fixed minibatches of binary rows: [(keys int64 [B * width], labels float32 [B])]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        k = torch.randint(0, num_features, (B * width,), generator=g, dtype=torch.int64)
        y = (torch.rand(B, generator=g) < 0.4).float() * 2 - 1
        out.append((k.to(device), y.to(device)))
    return out


def reference_steps(keys_u64, w, z, n, batches, width: int, algo: str, lr_type: str,
                    alpha=ALPHA, beta=BETA, l1=L1, l2=L2):
    """apply_update's arithmetic (kv_slot.cuh) as a plain fp32 PyTorch loop over binary
    minibatches, one update per key and minibatch, started from the state (w, z, n) of the
    raw keys ``keys_u64``; a key the state does not hold starts at zero. Returns (sorted raw
    keys as int64 bit patterns in signed order of the values used here, W, first loss):
    keys are < 2^63 in these tests."""
    mb_keys = torch.cat([k.cpu() for k, _ in batches])
    allk = torch.unique(torch.cat([mb_keys, torch.from_numpy(keys_u64.astype(np.int64))]))
    K = allk.numel()
    W, Z, N, C = torch.zeros(K), torch.zeros(K), torch.zeros(K), torch.zeros(K)
    at = torch.searchsorted(allk, torch.from_numpy(keys_u64.astype(np.int64)))
    W[at], Z[at] = torch.from_numpy(w.astype(np.float32)), torch.from_numpy(z.astype(np.float32))
    N[at] = torch.full((at.numel(),), float(n))
    first_loss = None
    for k, y in batches:
        k, y = k.cpu(), y.cpu()
        B = y.numel()
        idx = torch.searchsorted(allk, k)
        row = torch.arange(B).repeat_interleave(width)
        m = torch.zeros(B, dtype=torch.float64).index_add_(0, row, W[idx].double()).float()
        if first_loss is None:
            first_loss = float(torch.nn.functional.softplus(-y.double() * m.double()).mean())
        coef = -y * torch.sigmoid(-y * m)
        g = torch.zeros(K, dtype=torch.float64).index_add_(0, idx, coef[row].double()).float()
        u = torch.unique(idx)
        gu, w_old = g[u], W[u]
        if algo == "ftrl":
            n_new = torch.sqrt(N[u] * N[u] + gu * gu)
            Z[u] = Z[u] + gu - (n_new - N[u]) / alpha * w_old
            N[u] = n_new
            eta = torch.full_like(gu, alpha) if lr_type == "constant" else alpha / (n_new + beta)
            zz = -Z[u] * eta
        elif algo == "adagrad":
            N[u] = N[u] + gu * gu
            eta = alpha / (beta + torch.sqrt(N[u]))
            zz = w_old - eta * gu
        else:
            C[u] = C[u] + 1
            eta = torch.full_like(gu, alpha) if lr_type == "constant" else \
                alpha / (beta + torch.sqrt(C[u]))
            zz = w_old - eta * gu
        leta = l1 * eta
        W[u] = torch.where(zz.abs() <= leta, torch.zeros_like(zz),
                           (zz - torch.sign(zz) * leta) / (1 + l2 * eta))
    return allk, W, first_loss


def run_steps(tr, batches, width: int):
    for k, y in batches:
        tr.step(k, y, width=width)
    tr.flush()


# ------------------------------------------------------------------------------ the app
def write_libsvm(d: str, nfiles=3, rows=300, seed=0, nkeys=2000):
    rng = np.random.default_rng(seed)
    wt = rng.normal(0, 1, nkeys) * (rng.random(nkeys) < 0.2)
    os.makedirs(d, exist_ok=True)
    for p in range(nfiles):
        with open(os.path.join(d, f"part-{p}"), "w") as f:
            for _ in range(rows):
                k = np.unique(rng.integers(1, nkeys, size=int(rng.integers(5, 30))))
                v = rng.random(k.size)
                y = 1 if (wt[k] * v).sum() + 0.2 * rng.normal() > 0 else -1
                f.write(f"{y} " + " ".join(f"{a}:{b:.4f}" for a, b in zip(k, v)) + "\n")


def app_conf(path, data, model_out, model_in=None, minibatch=100):
    warm = f'model_input {{ format: TEXT file: "{model_in}_S.*" }}\n' if model_in else ""
    with open(path, "w") as f:
        f.write(f"""linear_method {{
training_data {{ format: TEXT text: LIBSVM file: "{data}/part.*" }}
{warm}model_output {{ format: TEXT file: "{model_out}" }}
loss {{ type: LOGIT }}
penalty {{ type: L1 lambda: 0.05 lambda: 0.01 }}
learning_rate {{ type: DECAY alpha: 0.5 beta: 1 }}
async_sgd {{ algo: FTRL minibatch: {minibatch} num_data_pass: 1 max_delay: 0 report_interval: 1 }}
}}""")
    return str(path)


def app_flags(**kw):
    d = dict(app_file=None, app_conf=None, num_features=0, max_nnz_per_example=64,
             num_threads=2, device="cpu", seed=0, table_capacity=1 << 14, quiet=True)
    d.update(kw)
    return types.SimpleNamespace(**d)


def run_app(conf_path: str, device: str, **flags):
    from parameter_server_amd.app.gpu import route
    from parameter_server_amd.parallel.comm import LocalComm
    from parameter_server_amd.utils.config import load_app_config

    lm = load_app_config(conf_path).linear_method
    dev = torch.device(device)
    fn = route(lm)
    assert fn.__name__ == "run_async_sgd"
    return fn(lm, LocalComm(dev), dev, app_flags(device=device, **flags))


def cold_then_warm(tmp_path, device: str, **flags):
    """A cold app run that writes yesterday's model, then the warm-started run of the same
    conf + ``model_input``: (cold result, warm result, model prefix)."""
    data, cold_m, warm_m = tmp_path / "data", tmp_path / "cold" / "m", tmp_path / "warm" / "m"
    if not data.exists():
        write_libsvm(str(data))
    cold = run_app(app_conf(tmp_path / "cold.conf", data, cold_m), device, **flags)
    warm = run_app(app_conf(tmp_path / "warm.conf", data, warm_m, model_in=cold_m), device,
                   **flags)
    return cold, warm, str(cold_m)


def app_table(res):
    """(raw keys, w, z, n) of an app result's trainer table, ordered by raw key (host)."""
    from parameter_server_amd.ops.keymix import unmix

    tr = res["trainer"]
    tr.flush()
    k, w, z, n = tr.table.occupied()
    raw = unmix(k, tr.bits).cpu()
    o = torch.argsort(raw)
    return raw[o], w.cpu()[o], z.cpu()[o], n.cpu()[o]
