"""Scoring a stored model (ops/score.py, models/scorer.py): the CPU path, and the case
builders / checks that tests/test_score_gpu.py runs again on the fused probe kernel
(csrc/hip/predict.hip).

Reference for margins: an fp64 dictionary loop over the RAW keys (``row_bound``: no
mixing, no table). Bound per row, derived not measured: (n_r + 2) 2^-23 sum |w x| over the
row's n_r occurrences (every product rounded once, at most n_r - 1 f32 additions in any
order, 2^-24 each, doubled)."""
import math
import os
import socket

import pytest
import torch

from parameter_server_amd.ops.keymix import mix, unmix
from parameter_server_amd.ops.kv_table import KVTable
from parameter_server_amd.ops.linear import AUC_BINS, exact_auc
from parameter_server_amd.ops.score import ScoreAccum, auc_from_counts, row_bound, score


# ---------------------------------------------------------------- case builders
def _raw_keys(g, bits, n):
    """n distinct raw keys of a ``bits``-bit key space (64: half with the top bit set)."""
    if bits == 64:
        k = torch.randint(0, 1 << 62, (2 * n,), generator=g, dtype=torch.int64)
        k[::2] |= -(1 << 63)  # top bit
    else:
        k = torch.randint(0, 1 << bits, (3 * n,), generator=g, dtype=torch.int64)
    k = torch.unique(k)
    return k[torch.randperm(k.numel(), generator=g)][:n]


class Case:
    """A model (table + the raw-key dictionary of the same weights) and one minibatch."""

    def __init__(self, device, *, bits=34, lens=(39,) * 257, fixed=False, vals=False, seed=0,
                 universe=600, model_keys=None, capacity=None, key_range=None, lanes=0,
                 model_raw=None):
        g = torch.Generator().manual_seed(seed)
        self.device, self.bits, self.lanes = torch.device(device), bits, lanes
        uni = _raw_keys(g, bits, universe)
        nm = universe // 2 if model_keys is None else model_keys  # ~half of the probes absent
        raw_m = uni[:nm] if model_raw is None else model_raw
        w = torch.randn(raw_m.numel(), generator=g)
        self.w_of = dict(zip(raw_m.tolist(), w.double().tolist()))
        self.table = KVTable(capacity or max(64, 2 * raw_m.numel()), self.device,
                             key_range=key_range)
        if raw_m.numel():
            self.table.load(mix(raw_m.to(self.device), bits), w)
        lens = torch.tensor(lens, dtype=torch.int64)
        self.B = lens.numel()
        nnz = int(lens.sum())
        self.keys = uni[torch.randint(0, uni.numel(), (nnz,), generator=g)]
        self.row_ptr = None if fixed else torch.cat([torch.zeros(1, dtype=torch.int64),
                                                     torch.cumsum(lens, 0)])
        self.width = int(lens[0]) if fixed else None
        self.vals = torch.rand(nnz, generator=g) + 0.5 if vals else None
        self.labels = torch.where(torch.rand(self.B, generator=g) < 0.4, 1.0, -1.0)

    def dev(self, t):
        return None if t is None else t.to(self.device)

    def run(self, acc=None, labels=True):
        return score(self.table, self.dev(self.keys), self.bits, row_ptr=self.dev(self.row_ptr),
                     width=self.width, vals=self.dev(self.vals),
                     labels=self.dev(self.labels) if labels else None, acc=acc, B=self.B,
                     lanes=self.lanes)


def check_case(c: Case):
    """Margins within the derived row bound of the fp64 dictionary loop; the table's bytes
    untouched; two runs bitwise equal; every metric consistent with the returned margins."""
    before = c.table.slots.clone()
    acc = ScoreAccum(c.device)
    m = c.run(acc)
    m2 = c.run(ScoreAccum(c.device))
    assert torch.equal(c.table.slots, before)
    assert torch.equal(m, m2)
    assert torch.equal(m, c.run(labels=False))  # margins-only launch
    m = m.cpu()
    m_ref, bound = row_bound(c.keys, c.w_of, c.vals, c.row_ptr, c.width)
    err = (m.double() - m_ref).abs()
    assert bool((err <= bound).all()), (float((err - bound).max()), int((err > bound).sum()))
    check_metrics(acc, m, c.labels)
    return m


def check_metrics(acc: ScoreAccum, m: torch.Tensor, labels: torch.Tensor):
    sums, counts = acc.sums().cpu().tolist(), acc.counts().cpu()
    B = m.numel()
    pos = int((labels > 0).sum())
    assert sums[2] == B
    assert int(counts[:AUC_BINS].sum()) == B - pos and int(counts[AUC_BINS:].sum()) == pos
    assert sums[1] == int(((labels > 0) == (m > 0)).sum())
    y = torch.where(labels > 0, 1.0, -1.0).double()
    loss_ref = float(torch.nn.functional.softplus(-y * m.double()).sum())
    assert abs(sums[0] - loss_ref) <= 1e-6 * loss_ref
    auc, tie = auc_from_counts(counts)
    if pos and B - pos:
        # (1e-12: the two quotients' own f64 rounding when the distance equals the bound)
        assert abs(auc - exact_auc(m, labels)) <= tie + 1e-12, (auc, exact_auc(m, labels), tie)


def ordered_wrap_case(device):
    """An ordered-home table (``key_range`` given) of 64 slots whose highest mixed keys
    all have home slot 63: their chain wraps past the end of the table."""
    bits = 12
    hi = torch.arange(4096 - 6, 4096, dtype=torch.int64)          # home 63, chain 63, 0..4
    rest = torch.arange(5, 4000, 137, dtype=torch.int64)          # 30 more, spread out
    raw, raw_rest = unmix(hi, bits), unmix(rest, bits)
    c = Case(device, bits=bits, lens=(7,) * 70, universe=400, capacity=64,
             key_range=(0, 4096), model_raw=raw, seed=5)
    g = torch.Generator().manual_seed(6)
    # (the rest in a second load, so the six take slots 63, 0..4 on the GPU's concurrent
    # inserts too)
    w_rest = torch.randn(rest.numel(), generator=g)
    c.table.load(mix(raw_rest.to(c.device), bits), w_rest)
    c.w_of.update(zip(raw_rest.tolist(), w_rest.double().tolist()))
    # probe the wrapped keys themselves in every row
    c.keys[::7] = raw[torch.randint(0, 6, (70,), generator=g)]
    slot, _ = c.table.resolve(mix(raw.to(c.device), bits), insert=False, with_w=False)
    assert sorted(slot.cpu().tolist()) == [0, 1, 2, 3, 4, 63]  # the chain did wrap
    return c


LONG = (5, 20000, 3, 0, 12)

CASES = {
    "one_key": dict(lens=(1,), universe=4, model_keys=4),
    "empty_middle_row": dict(lens=(4, 0, 9)),
    "w39_fixed_257": dict(lens=(39,) * 257, fixed=True),
    "w39_csr_vals_257": dict(lens=(39,) * 257, vals=True),
    "long_row_8": dict(lens=LONG, lanes=8, vals=True),
    "long_row_64": dict(lens=LONG, lanes=64, vals=True),
    "bits12": dict(bits=12, lens=(17,) * 70, vals=True),
    "bits32": dict(bits=32, lens=(17,) * 70),
    "bits34": dict(bits=34, lens=(17,) * 70),
    "bits64_top_bit": dict(bits=64, lens=(17,) * 70, vals=True),
    "rcv1_rows_auto_64": dict(lens=tuple(range(40, 140)), vals=True),
    "chains_load_075": dict(lens=(9,) * 90, universe=96, model_keys=48, capacity=64),
}


# ---------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("name", sorted(CASES))
def test_score_cpu_cases(name):
    check_case(Case("cpu", **CASES[name]))


def test_score_cpu_ordered_home_chain_wraps():
    check_case(ordered_wrap_case("cpu"))


def test_score_cpu_full_table_absent_keys_end():
    """64 keys in 64 slots: an absent key's chain meets no empty slot and ends on the
    trip bound. (CPU path only: on the GPU a missing bound would hang the machine; there
    the bound is read at the loop, predict.hip probe_on.)"""
    c = Case("cpu", lens=(9,) * 40, universe=128, model_keys=64, capacity=64)
    assert c.table.census()[0] == 64
    check_case(c)


def check_empty_model(device):
    c = Case(device, lens=(11,) * 50, model_keys=0)
    acc = ScoreAccum(c.device)
    m = c.run(acc)
    assert torch.equal(m.cpu(), torch.zeros(50))
    s = acc.sums().cpu().tolist()
    assert s[2] == 50 and abs(s[0] / 50 - math.log(2)) <= 1e-6 * math.log(2)


def test_score_cpu_empty_model():
    check_empty_model("cpu")


def check_accumulation(device):
    """Three minibatches into one accumulator == their concatenation scored once."""
    c = Case(device, lens=(39,) * 277, fixed=True, seed=3)
    keys, labels = c.dev(c.keys), c.dev(c.labels)
    one = ScoreAccum(device)
    ms = [score(c.table, keys[a * 39:b * 39], c.bits, width=39, labels=labels[a:b], acc=one)
          for a, b in ((0, 100), (100, 157), (157, 277))]
    cat = ScoreAccum(device)
    m = c.run(cat)
    assert torch.equal(torch.cat(ms), m)
    a, b = one.sums().cpu().tolist(), cat.sums().cpu().tolist()
    assert a[1:] == b[1:] and torch.equal(one.counts(), cat.counts())
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0])


def test_score_cpu_accumulates_over_minibatches():
    check_accumulation("cpu")


def test_auc_from_counts_small():
    h = torch.zeros(2 * AUC_BINS, dtype=torch.int64)
    h[3], h[10] = 2, 1                      # negatives in bins 3 (x2) and 10
    h[AUC_BINS + 3], h[AUC_BINS + 20] = 1, 1  # positives in bins 3 and 20
    auc, tie = auc_from_counts(h)
    # pairs: (p3: ties 2 negs -> 1, below 0) + (p20: 3 below) = 4 of 6
    assert auc == 4 / 6 and tie == 2 / 12
    assert math.isnan(auc_from_counts(torch.zeros(2 * AUC_BINS, dtype=torch.int64))[0])


# ---------------------------------------------------------------- trainer
def train_and_score(device, tmp_path):
    """5 steps of B = 200, then the same fresh minibatch through ``tr.scorer()`` (the
    trainer's own ordered-home table, zero weights included) and through ``from_text`` on
    ``tr.save_model()`` (hashed homes, non-zero weights; 9 significant digits round-trip
    f32): equal margins bit for bit, equal counts and histogram."""
    from parameter_server_amd.models import ModelScorer, SparseLRConfig, SparseLRTrainer
    from parameter_server_amd.ops.synthetic import criteo_batch

    N, B = 1 << 20, 200
    cfg = SparseLRConfig(num_features=N, minibatch=B, table_capacity=1 << 15, l1=0.01,
                         alpha=0.5, beta=1.0)
    tr = SparseLRTrainer(cfg, device=device)
    for s in range(5):
        k, l = criteo_batch(B, seed=7, row0=s * B, num_features=N, cards=[200] * 26,
                            device=device)
        tr.step(k, l, width=39)
    k, l = criteo_batch(B, seed=7, row0=5 * B, num_features=N, cards=[200] * 26, device=device)
    a = tr.scorer()
    assert a.table is tr.table
    path = tr.save_model(str(tmp_path / "m"))
    b = ModelScorer.from_text(str(tmp_path / "m_S.*"), tr.bits, device)
    assert b.entries == tr.table.census()[1] > 50
    ma, mb = a.score(k, l, width=39), b.score(k, l, width=39)
    assert torch.equal(ma, mb) and float(ma.abs().max()) > 0
    (sa, ca), (sb, cb) = a.totals(), b.totals()
    assert torch.equal(sa, sb) and torch.equal(ca, cb)
    assert torch.equal(tr.predict(k, width=39), ma)
    r = a.result()
    assert r["examples"] == B and 0 < r["loss"] < math.log(2) and r["auc"] > 0.5
    return path


def test_trainer_scorer_equals_saved_model_cpu(tmp_path):
    train_and_score("cpu", tmp_path)


def test_from_text_fails_loudly_when_the_table_is_too_small(tmp_path):
    from parameter_server_amd.models import ModelScorer
    from parameter_server_amd.utils.checkpoint import write_text_model

    write_text_model(str(tmp_path / "m_S0"), torch.arange(1, 101), torch.ones(100))
    with pytest.raises(RuntimeError, match="KVTable full"):
        ModelScorer.from_text(str(tmp_path / "m_S.*"), 20, "cpu", capacity=64)
    sc = ModelScorer.from_text(str(tmp_path / "m_S.*"), 20, "cpu")
    assert sc.entries == 100 and sc.table.capacity == 256 and sc.table.census() == (100, 100)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _val_batch(B):
    from parameter_server_amd.ops.synthetic import criteo_batch

    return criteo_batch(B, seed=99, row0=0, num_features=1 << 20, cards=[200] * 26)


def _replica_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from parameter_server_amd.models import SparseLRConfig, SparseLRTrainer
    from parameter_server_amd.ops.synthetic import criteo_batch
    from parameter_server_amd.parallel.comm import DistComm

    comm = DistComm("cpu")
    cfg = SparseLRConfig(num_features=1 << 20, minibatch=200, table_capacity=1 << 15, l1=0.01,
                         alpha=0.5, beta=1.0)
    tr = SparseLRTrainer(cfg, comm, "cpu")
    for s in range(5):
        k, l = criteo_batch(200, seed=100 + rank, row0=s * 200, num_features=1 << 20,
                            cards=[200] * 26)
        tr.step(k, l, width=39)
    sc = tr.scorer()  # the replica: every rank holds both shards' non-zero weights
    assert sc.table is not tr.table
    k, l = _val_batch(301)
    a, b = (0, 120) if rank == 0 else (120, 301)  # the rows split unevenly
    sc.score(k[a * 39:b * 39], l[a:b], width=39)
    sums, counts = sc.totals(comm)
    tr.save_model(os.path.join(out_dir, "m"))
    torch.save({"sums": sums, "counts": counts, "result": sc.result(comm)},
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_replica_equals_saved_files(tmp_path):
    import torch.multiprocessing as mp

    from parameter_server_amd.models import ModelScorer

    mp.spawn(_replica_worker, args=(2, _port(), str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=False) for i in range(2)]
    one = ModelScorer.from_text(str(tmp_path / "m_S.*"), 20, "cpu")
    k, l = _val_batch(301)
    one.score(k, l, width=39)
    sums, counts = one.totals()
    for x in r:
        assert x["sums"].tolist()[1:] == sums.tolist()[1:] and float(sums[2]) == 301.0
        assert torch.equal(x["counts"], counts)
        assert abs(float(x["sums"][0]) - float(sums[0])) <= 1e-12 * float(sums[0])
        assert x["result"]["examples"] == 301
        assert x["result"]["auc"] == one.result()["auc"]
