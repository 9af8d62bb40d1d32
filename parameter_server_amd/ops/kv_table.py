"""HBM-resident open-addressing KV table for scalar linear models.

Python handle over the ``kv_*`` kernels (csrc/hip/kv_table.hip) with an
identical C++ host implementation (csrc/core/cpu_kernels.cc) for CPU tensors.
It is the MI355X-native replacement of the reference's per-server
``KVStore<Key, V, Entry, SGDState>`` (src/parameter/kv_store.h:28-80), whose
hash-map entries carry the optimizer (src/app/linear_method/async_sgd.h:71-124).

Slots are 32 bytes ``{u64 key | f32 w, z, n, acc | u32 cnt, flags}`` stored as an
``int64 [capacity, 4]`` tensor; keys are stored in the *mixed* key space.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .native import core, hipops, is_gpu, ptr

EMPTY_KEY = -1  # 0xFFFF_FFFF_FFFF_FFFF as int64

ALGOS = {"sgd": 0, "standard": 0, "adagrad": 1, "ftrl": 2}
LR_TYPES = {"constant": 1, "decay": 2}
INIT_TYPES = {"zero": 0, "constant": 1, "gaussian": 2, "uniform": 3}


@dataclass
class UpdateRule:
    """Server-side per-key update (SGD / AdaGrad / FTRL-proximal with L1+L2).

    Mirrors reference LearningRate (learning_rate.h:15-22: CONSTANT=alpha,
    DECAY=alpha/(x+beta)) and ElasticNet::proximal (penalty.h:38-43).
    """

    algo: str = "ftrl"
    lr_type: str = "decay"
    alpha: float = 0.01
    beta: float = 10.0
    l1: float = 0.0
    l2: float = 0.0
    grad_scale: float = 1.0
    max_delta: float = 0.0

    def args(self):
        return (ALGOS[self.algo.lower()], LR_TYPES[self.lr_type.lower()], float(self.alpha),
                float(self.beta), float(self.l1), float(self.l2), float(self.grad_scale),
                float(self.max_delta))


@dataclass
class InitRule:
    """Reference ParameterInitConfig {ZERO, CONSTANT, GAUSSIAN, ...} (param.proto)."""

    type: str = "zero"
    value: float = 0.0
    std: float = 0.0
    seed: int = 0

    def args(self):
        return INIT_TYPES[self.type.lower()], float(self.value), float(self.std), int(self.seed) & ((1 << 64) - 1)


def next_pow2(x: int) -> int:
    return 1 << max(0, int(x - 1).bit_length())


class KVTable:
    def __init__(self, capacity: int, device="cpu", init: InitRule | None = None,
                 key_range: tuple[int, int] | None = None):
        """``key_range = (lo, hi)``: the (mixed) key range this shard owns; keys then get
        ORDERED home slots (see kv_table.hip home_slot) instead of hashed ones."""
        cap = next_pow2(max(64, int(capacity)))
        self.home_base, self.home_m = 0, 0
        self.key_range = (int(key_range[0]), int(key_range[1])) if key_range is not None else None
        if key_range is not None:
            lo, hi = int(key_range[0]), int(key_range[1])
            if hi > lo:
                self.home_base = lo
                self.home_m = ((1 << 64) - 1) // (hi - lo)
        self.capacity = cap
        self.device = torch.device(device)
        self.init = init or InitRule()
        self.slots = torch.empty((cap, 4), dtype=torch.int64, device=self.device)
        self.gpu = self.device.type == "cuda"
        if self.gpu:
            self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
            # no per-wave insert counter on the hot path: one device atomic per wave on a
            # single address serialises (measured ~50 us of a 55 us resolve at 234k
            # keys); the occupancy comes from census() when it is needed
            self._inserted = None
            hipops().kv_init(self.slots)
        else:
            core().kv_init(ptr(self.slots), cap)
        self.num_inserted = 0  # host-side count (CPU path exact; GPU path lazily synced)

    # ------------------------------------------------------------------ pull
    def resolve_args(self) -> tuple:
        """The trailing arguments every native lookup-or-insert of this table takes (GPU):
        the init rule, the error word, the insert counter and the ordered-home mapping."""
        return (*self.init.args(), self._err, self._inserted, self.home_base, self.home_m)

    def resolve(self, keys: torch.Tensor, insert: bool = True, with_w: bool = True,
                n_dev: torch.Tensor | None = None):
        """Lookup-or-insert mixed keys; returns (slot_idx int64, w float32 | None)."""
        keys = keys.contiguous()
        n = keys.numel()
        slot = torch.empty(n, dtype=torch.int64, device=keys.device)
        w = torch.empty(n, dtype=torch.float32, device=keys.device) if with_w else None
        if self.gpu:
            hipops().kv_resolve(self.slots, keys, n_dev, slot, w, insert, *self.resolve_args())
        else:
            it, iv, isd, seed = self.init.args()
            ins, full = core().kv_resolve(ptr(self.slots), self.capacity, ptr(keys), n, ptr(slot),
                                          ptr(w), insert, it, iv, isd, seed, self.home_base,
                                          self.home_m)
            self.num_inserted += ins
            if full:
                raise RuntimeError("KVTable full: increase capacity")
        return slot, w

    def gather(self, slot_idx: torch.Tensor, field: int = 0, n_dev=None, out=None):
        n = slot_idx.numel()
        out = torch.empty(n, dtype=torch.float32, device=slot_idx.device) if out is None else out
        if self.gpu:
            hipops().kv_gather(self.slots, slot_idx, n_dev, out, field)
        else:
            core().kv_gather(ptr(self.slots), ptr(slot_idx), n, ptr(out), field)
        return out

    def set(self, slot_idx, w=None, z=None, n=None):
        if self.gpu:
            hipops().kv_set(self.slots, slot_idx, w, z, n)
        else:
            core().kv_set(ptr(self.slots), ptr(slot_idx), slot_idx.numel(), ptr(w), ptr(z), ptr(n))

    # ------------------------------------------------------------------ push
    def update(self, slot_idx: torch.Tensor, grad: torch.Tensor, rule: UpdateRule,
               stats: torch.Tensor | None = None, n_dev=None):
        """Apply one optimizer step per (unique-in-call) slot; stats += [dnnz, sum w^2, sum dw^2]."""
        if self.gpu:
            hipops().kv_update(self.slots, slot_idx, grad.contiguous(), n_dev, *rule.args(), stats)
        else:
            assert n_dev is None
            core().kv_update(ptr(self.slots), ptr(slot_idx), ptr(grad.contiguous()),
                             slot_idx.numel(), *rule.args(), ptr(stats))

    # ------------------------------------------------------------- inspection
    def census(self):
        """(occupied slots, nonzero weights)."""
        if self.gpu:
            c = hipops().kv_census(self.slots).cpu()
            return int(c[0]), int(c[1])
        return core().kv_census(ptr(self.slots), self.capacity)

    def check_ok(self):
        if self.gpu and int(self._err.item()) != 0:
            raise RuntimeError("KVTable full: increase capacity")

    def occupied(self, chunk: int = 1 << 27):
        """(mixed keys, w, z, n) of every occupied slot (device tensors). Scanned in
        chunks of slots: boolean-mask indexing over more than 2^31 elements overflows in
        torch, and a whole-table copy of a 2^31-slot table would take 32 GiB."""
        parts = []
        for a in range(0, self.capacity, chunk):
            sl = self.slots[a:a + chunk]
            keys = sl[:, 0]
            mask = keys != EMPTY_KEY
            vals = sl[:, 1:3].contiguous().view(torch.float32)  # w,z,n,acc
            parts.append((keys[mask], vals[mask, 0], vals[mask, 1], vals[mask, 2]))
        if len(parts) == 1:
            return parts[0]
        return tuple(torch.cat([p[i] for p in parts]) for i in range(4))

    def occupied_weights(self, chunk: int = 1 << 27):
        """(mixed keys, w) of every occupied slot (device tensors): ``occupied`` without
        the copies of z and n, for a model save."""
        parts = []
        for a in range(0, self.capacity, chunk):
            sl = self.slots[a:a + chunk]
            keys = sl[:, 0]
            mask = keys != EMPTY_KEY
            w = sl[:, 1].contiguous().view(torch.float32)[0::2]  # (the low word of w | z)
            parts.append((keys[mask], w[mask]))
        if len(parts) == 1:
            return parts[0]
        return tuple(torch.cat([p[i] for p in parts]) for i in range(2))

    def load(self, keys_mixed: torch.Tensor, w, z=None, n=None):
        slot, _ = self.resolve(keys_mixed.to(self.device), insert=True, with_w=False)
        self.set(slot, w.to(self.device).float().contiguous(),
                 None if z is None else z.to(self.device).float().contiguous(),
                 None if n is None else n.to(self.device).float().contiguous())
        self.check_ok()
        return slot

    # ------------------------------------------------------------- warm start
    SEED_COUNTS = ("seeded", "overwritten", "foreign", "out_of_range", "skipped")

    def clear(self):
        """Every slot empty again (capacity, init rule and home mapping stay)."""
        if self.gpu:
            hipops().kv_init(self.slots)
        else:
            core().kv_init(ptr(self.slots), self.capacity)
        self.num_inserted = 0

    def new_seed_counts(self) -> torch.Tensor:
        """The striped counters ``seed(..., counts=)`` adds to over several calls."""
        return torch.zeros(64 * 16, dtype=torch.int64, device=self.device)

    def seed_counts(self, counts: torch.Tensor) -> dict:
        """``counts`` as {"seeded", "overwritten", "foreign", "out_of_range", "skipped"}
        (GPU: the one host sync of a seeded load)."""
        tot = counts.view(-1, 16).sum(0)[:len(self.SEED_COUNTS)].tolist()
        return dict(zip(self.SEED_COUNTS, (int(v) for v in tot)))

    def seed(self, raw_keys: torch.Tensor, w: torch.Tensor, bits: int, lo: int, hi: int,
             rule: UpdateRule, n0: float = 0.0, stats: torch.Tensor | None = None,
             counts: torch.Tensor | None = None):
        """Warm start: (raw key, weight) pairs of a stored model into this table, with the
        optimizer state of ``rule`` that REPRODUCES each weight (kv_table.hip kv_seed; a
        table loaded with w and z = n = 0 forgets w at a key's first FTRL update).

        ``raw_keys``: int64 bit patterns; a key outside [0, 2^bits) (bits < 64) is counted
        as ``out_of_range``. Kept: keys whose mixed value lies in [lo, hi) (others:
        ``foreign``) with a weight that is neither 0 nor NaN (others: ``skipped``). Each is
        looked up or inserted (``seeded`` / ``overwritten``) and its whole slot written: w
        the given bits, acc = cnt = 0, the published-init flag, and with ``n0 >= 0`` a prior
        gradient norm, inv_eta0 = 1 / alpha (constant) or (n0 + beta) / alpha (decay):
        FTRL n = n0, z = -(w (inv_eta0 + l2) + copysign(l1, w)); AdaGrad z = 0, n = n0^2;
        SGD z = n = 0. ``stats[0]`` gains the change of the non-zero weight count.

        Returns the counts as a dict; with ``counts`` (``new_seed_counts``) they are added
        there instead and nothing is read back (``seed_counts`` at the end). Nothing else
        may be using the table. A repeated key within or across calls is ``overwritten``
        with no promise which weight stays."""
        algo, lr_type, alpha, beta, l1, l2 = rule.args()[:6]
        n0 = float(n0)
        if n0 < 0 or alpha <= 0:
            raise ValueError("KVTable.seed: n0 >= 0 and alpha > 0")
        lo, hi = int(lo), int(hi)
        if hi <= lo:
            raise ValueError(f"KVTable.seed: empty key range [{lo}, {hi})")
        raw_keys = raw_keys.to(self.device).contiguous()
        w = w.to(self.device, torch.float32).contiguous()
        if raw_keys.dtype != torch.int64 or raw_keys.shape != w.shape or raw_keys.dim() != 1:
            raise ValueError("KVTable.seed: int64 key bit patterns and weights of one 1-d shape")
        own = counts if counts is not None else self.new_seed_counts()
        if self.gpu:
            if raw_keys.numel():
                hipops().kv_seed(self.slots, raw_keys, w, bits, lo, hi - 1, algo, lr_type, alpha,
                                 beta, l1, l2, n0, own, stats, self._err, self.home_base,
                                 self.home_m)
        elif raw_keys.numel():
            self._seed_host(raw_keys, w, bits, lo, hi, (algo, lr_type, alpha, beta, l1, l2), n0,
                            stats, own)
        return self.seed_counts(own) if counts is None else None

    def _seed_host(self, raw, w, bits, lo, hi, rule, n0, stats, counts):
        """The PyTorch reference of kv_seed: mix, range mask, resolve(insert), whole-slot
        write with z in float32 in the kernel's operation order."""
        from .keymix import mix, to_unsigned_order

        algo, lr_type, alpha, beta, l1, l2 = rule
        in_bits = torch.ones_like(raw, dtype=torch.bool) if bits == 64 else \
            (raw >= 0) & (raw < (1 << bits))
        h = mix(raw, bits)
        hu = to_unsigned_order(h)  # (signed order == unsigned order)
        owned = (hu >= lo - (1 << 63)) & (hu <= hi - 1 - (1 << 63))
        keep = (w != 0) & ~torch.isnan(w)
        act = in_bits & owned & keep
        hk, wk = h[act].contiguous(), w[act]
        pre, w_pre = self.resolve(hk, insert=False)
        before = self.num_inserted
        slot, _ = self.resolve(hk, insert=True, with_w=False)  # (a full table raises here)
        fresh = self.num_inserted - before
        # non-zero weights gained: every inserted key, and present ones that held 0
        dnnz = fresh + int(((pre >= 0) & (w_pre == 0)).sum())
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
        inv_eta0 = 1.0 / f32(alpha) if lr_type == LR_TYPES["constant"] else \
            (f32(n0) + f32(beta)) / f32(alpha)
        if algo == ALGOS["ftrl"]:
            z = -(wk * (inv_eta0 + f32(l2)) + torch.copysign(f32(l1), wk))
            n = f32(n0)
        else:
            z = torch.zeros_like(wk)
            n = f32(n0) * f32(n0) if algo == ALGOS["adagrad"] else f32(0.0)
        fl = self.slots.view(torch.float32)   # [cap, 8]: key | w z | n acc | cnt flags
        it = self.slots.view(torch.int32)
        fl[slot, 2], fl[slot, 3], fl[slot, 4], fl[slot, 5] = wk, z, n.expand_as(wk), 0.0
        it[slot, 6], it[slot, 7] = 0, 2  # cnt, flags = kSlotInit (kv_slot.cuh)
        c = counts.view(-1, 16)[0]
        c[0] += fresh
        c[1] += int(act.sum()) - fresh
        c[2] += int((in_bits & ~owned).sum())
        c[3] += int((~in_bits).sum())
        c[4] += int((in_bits & owned & ~keep).sum())
        if stats is not None:
            stats.view(-1)[0] += float(dnnz)

    # ---------------------------------------------------------------- growth
    def grow(self, capacity: int) -> int:
        """Rehash every occupied slot, as the whole 32-byte record, into a table of
        ``capacity`` slots (rounded up to a power of two), in place: this object stays,
        ``slots`` and ``capacity`` are replaced. Returns the occupied count (also left
        in ``num_inserted``). The error word, the init rule and the home mapping carry
        over. Slot indices and launch lists taken before the call are stale after it."""
        cap = next_pow2(max(64, int(capacity)))
        if cap < self.capacity:
            raise ValueError(f"KVTable.grow: capacity {cap} is below the current {self.capacity}")
        if cap == self.capacity:
            self.num_inserted = self.census()[0]
            return self.num_inserted
        old = self.slots
        new = torch.empty((cap, 4), dtype=torch.int64, device=self.device)
        if self.gpu:
            hipops().kv_init(new)
            moved = hipops().kv_rehash(old, new, self.home_base, self.home_m, self._err)
            # the caching allocator hands the old block out again only to work queued
            # behind the rehash on this stream
            old.record_stream(torch.cuda.current_stream(self.device))
            moved = int(moved.item())
        else:
            core().kv_init(ptr(new), cap)
            moved, full = core().kv_rehash(ptr(old), self.capacity, ptr(new), cap,
                                           self.home_base, self.home_m)
            if full:
                raise RuntimeError("KVTable full: increase capacity")
        self.slots, self.capacity = new, cap
        self.num_inserted = int(moved)
        return self.num_inserted

    def remap_slots(self, old_slots: torch.Tensor, slot_idx: torch.Tensor) -> torch.Tensor:
        """Slot indices into ``old_slots`` (this table's slots before a ``grow``) as the
        indices of the same keys in the table now; -1 (absent) stays -1."""
        cap = old_slots.shape[0]
        ok = (slot_idx >= 0) & (slot_idx < cap)
        keys = old_slots[:, 0][slot_idx.clamp(0, cap - 1)]
        ok &= keys != EMPTY_KEY
        new, _ = self.resolve(keys.contiguous(), insert=False, with_w=False)
        return torch.where(ok, new, torch.full_like(new, -1))

    def nbytes(self) -> int:
        return self.capacity * 32
