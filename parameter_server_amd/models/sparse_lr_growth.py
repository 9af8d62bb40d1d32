"""SparseLRTrainer's table growth (``SparseLRConfig.table_growth``): the host-side policy
that decides when the KV table is rehashed into a larger one (``KVTable.grow``), and the
trainer mixin that feeds it and repairs what a growth leaves stale.

The reference's ``KVStore`` grows its hash map with every new key
(src/parameter/kv_store.h:37-57); a fixed open-addressing table can only be sized in
advance. With growth on, the trainer keeps an UPPER BOUND of the occupied slots -- the
last exact count plus every key handed to the table since -- without ever reading the
device for it, and takes the exact count only when that bound says the table might pass
``table_grow_check`` of its capacity."""
from __future__ import annotations

import warnings

import torch


class GrowthPolicy:
    """When to grow ``table`` (anything with ``capacity``, ``census()`` and ``grow(cap)``).

    ``admit(incoming)`` is called before ``incoming`` keys are handed to the table. While
    ``bound + incoming <= check x capacity`` it only adds to the bound. Otherwise it takes
    the exact occupancy (``prepare()`` first: whatever must finish before the table is
    read or replaced; ``reduce_max``: the largest count over all ranks, so every rank
    decides alike) and grows when the table is more than ``at`` full, or when the incoming
    keys could carry it past ``check``: the capacity doubles until the occupancy is at
    most ``at / 2`` of it and occupancy + incoming at most ``check`` of it. Then the bound
    restarts from the exact count. So checks are at least ``(check - at) x capacity``
    admitted keys apart, and while growth is possible the occupancy never passes
    ``check x capacity``: the table's sticky full flag cannot fire.

    A growth past ``max_bytes`` (32 bytes per slot), or one whose allocation fails
    (``reserve(cap)`` false on any rank), is refused: one warning, no further checks, and
    the table fails as loudly as a fixed one if it does fill."""

    def __init__(self, table, *, check: float = 0.75, at: float = 0.5, max_bytes: int = 1 << 62,
                 prepare=None, reduce_max=None, reserve=None, changed=None):
        if not 0.0 < at < check <= 1.0:
            raise ValueError(f"table growth needs 0 < table_grow_at ({at}) < table_grow_check "
                             f"({check}) <= 1")
        self.table = table
        self.check, self.at, self.max_bytes = float(check), float(at), int(max_bytes)
        self.prepare, self.reduce_max, self.reserve, self.changed = (prepare, reduce_max, reserve,
                                                                     changed)
        self.bound = 0       # upper bound of the occupied slots
        self.grown = 0       # growths so far
        self.checks = 0      # exact counts taken so far
        self.refused = False

    def target(self, occ: int, incoming: int = 0) -> int:
        """The capacity for ``occ`` occupied slots about to receive ``incoming`` keys."""
        cap = int(self.table.capacity)
        if occ <= self.at * cap and occ + incoming <= self.check * cap:
            return cap
        while occ > self.at / 2 * cap or occ + incoming > self.check * cap:
            cap *= 2
        return cap

    def admit(self, incoming: int) -> None:
        incoming = int(incoming)
        if not self.refused and self.bound + incoming > self.check * self.table.capacity:
            self.recount(incoming)
        self.bound += incoming

    def recount(self, incoming: int = 0) -> int:
        """Take the exact occupancy, grow if it calls for it, restart the bound."""
        if self.prepare is not None:
            self.prepare()
        occ = int(self.table.census()[0])
        if self.reduce_max is not None:
            occ = int(self.reduce_max(occ))
        self.checks += 1
        cap = self.target(occ, incoming)
        if cap > self.table.capacity:
            self._grow(cap)
        self.bound = occ
        return occ

    def _grow(self, cap: int) -> None:
        if cap * 32 > self.max_bytes:
            return self._refuse(f"{cap} slots ({cap * 32} bytes) would pass max_table_bytes "
                                f"{self.max_bytes}")
        if self.reserve is not None and not self.reserve(cap):
            return self._refuse(f"{cap} slots ({cap * 32} bytes) could not be allocated")
        old = self.table.slots if hasattr(self.table, "slots") else None
        self.table.grow(cap)
        self.grown += 1
        if self.changed is not None:
            self.changed(old)

    def _refuse(self, why: str) -> None:
        self.refused = True
        warnings.warn(f"table growth refused: {why}; the table stays at "
                      f"{self.table.capacity} slots and the run fails with 'KVTable full' "
                      f"if it fills", RuntimeWarning, stacklevel=4)


class TableGrowth:
    """Mixin of SparseLRTrainer (models/sparse_lr.py): feeds ``GrowthPolicy``."""

    _growth: GrowthPolicy | None = None
    _grow_seen = None  # (id, generation) of a localisation whose keys were counted ahead

    def _growth_setup(self):
        cfg = self.cfg
        if not cfg.table_growth:
            return
        # (a policy with bad fractions raises here, before the first step)
        self._growth = GrowthPolicy(
            self.table, check=cfg.table_grow_check, at=cfg.table_grow_at,
            max_bytes=cfg.max_table_bytes, prepare=self._growth_prepare,
            reduce_max=self._growth_max if self.G > 1 and not self._loopback else None,
            reserve=self._growth_reserve, changed=self._table_changed)

    @staticmethod
    def _growth_supported(cfg, G: int):
        """Raise for the data planes a growth cannot serve (before anything is allocated)."""
        if cfg.table_growth and G > 1 and cfg.exchange == "p2p":
            raise ValueError("table_growth is not supported on exchange='p2p': the peers map "
                             "this rank's table over IPC and would keep the old one")

    # bench.py's pipelines issue the exchanges themselves (trainer._mx_external = True) and
    # hold captured graphs over the table: no growth there
    @property
    def _mx_external(self) -> bool:
        return self.__dict__.get("_mx_external", False)

    @_mx_external.setter
    def _mx_external(self, v: bool):
        if v and self._growth is not None:
            raise ValueError("table_growth is not supported when the caller owns the exchange "
                             "pipeline (its launch lists and graphs hold the table)")
        self.__dict__["_mx_external"] = bool(v)

    # ---------------------------------------------------------------- the bound
    def _growth_step(self, keys, loc, next_loc):
        """Before a step is issued: admit the keys it hands to the table. One rank: this
        minibatch's occurrences, unless they were admitted when an earlier step pulled
        them ahead (``next_loc``), plus those of this step's ``next_loc``. G ranks: the G
        rows of C keys one exchange can bring this owner -- the same on every rank."""
        g = self._growth
        if self.G > 1:
            return g.admit(self.G * self._growth_row_capacity())
        n = 0
        if loc is None:
            n = int(keys.numel())
        elif (id(loc), getattr(loc, "gen", None)) != self._grow_seen:
            n = int(getattr(loc, "nnz", 0) or (keys.numel() if keys is not None else 0))
        self._grow_seen = None
        if next_loc is not None and next_loc is not loc:
            n += int(getattr(next_loc, "nnz", 0))
            seen = (id(next_loc), getattr(next_loc, "gen", None))
        else:
            seen = None
        g.admit(n)
        self._grow_seen = seen

    def _growth_row_capacity(self) -> int:
        """Upper bound of the keys one source sends this owner in one exchange."""
        if self.xc is not None:
            return int(self.xc.C)
        # before the rows exist (and on the exact exchange): what _agree_capacity can agree
        # on at most -- the configured capacity, or a whole minibatch
        C = int(self.cfg.exchange_capacity) if self.padded else 0
        top = max(64, int(self.max_nnz))
        return min(max(64, (C + 63) // 64 * 64), top) if C > 0 else top

    # ------------------------------------------------------- the policy's callbacks
    def _growth_prepare(self):
        """Everything issued so far reads or writes the table that is about to be counted
        and replaced: wait for it (also on the exchange's own streams)."""
        if self.gpu:
            torch.cuda.synchronize(self.device)

    def _growth_max(self, occ: int) -> int:
        t = self.comm.all_reduce_(self._to_comm(torch.tensor([float(occ)], dtype=torch.float64)),
                                  op="max")
        return int(t.item())

    def _growth_reserve(self, cap: int) -> bool:
        """Whether ``cap`` slots can be allocated -- on every rank, so all grow or none.
        (The block returns to the allocator's cache, where ``KVTable.grow`` finds it.)"""
        ok = 1.0
        try:
            torch.empty((cap, 4), dtype=torch.int64, device=self.device)
        except (RuntimeError, MemoryError):  # (torch's out-of-memory error is a RuntimeError)
            ok = 0.0
        if self.G > 1 and not self._loopback:
            ok = float(self.comm.all_reduce_(
                self._to_comm(torch.tensor([-ok], dtype=torch.float64)), op="max").item()) * -1.0
        return ok > 0.0

    def _table_changed(self, old_slots=None):
        """The table changed under the trainer: its contents were rewritten in place
        (``load_state_dict``: ``old_slots`` None) or its slots were replaced by a growth
        (``old_slots``: the tensor before it). Drops what holds the slots tensor or
        weights read from it: the launch lists and a pull issued ahead are rebuilt by the
        next step. After a growth the slot indices that still have gradients on the way
        -- the exchange rings' resolved pulls, the exact exchange's deferred push -- are
        translated through their keys (``KVTable.remap_slots``), so a growth changes
        neither which pushes are applied nor the step they are applied in."""
        self._plans.clear()
        self._pre = None
        self._grow_seen = None
        if old_slots is None:
            return
        held = list(self.xc.slots) if self.xc is not None else []
        if self.pending is not None:
            held += list(self.pending[0])
        for idx in held:
            idx.copy_(self.table.remap_slots(old_slots, idx))

    def _growth_load(self, own: torch.Tensor):
        """``load_state_dict`` with growth on: make room for the keys this rank owns (the
        true entries of ``own``) first."""
        if self._growth is not None:
            self._growth_room(int(own.sum()))

    def _growth_room(self, incoming: int, exact: bool = True):
        """Make room for ``incoming`` keys about to be loaded into the table (collective
        when G > 1: every rank calls it with the same sequence of ``exact`` / bounds).
        ``exact=False`` (``load_model``, once per chunk with the chunk's entry count --
        the same on every rank): the occupancy is counted only when the host's upper
        bound says the load could pass ``table_grow_at``."""
        g = self._growth
        if g is None or g.refused:
            return
        cap = self.table.capacity
        if not exact and g.bound + incoming <= g.at * cap:
            g.bound += incoming
            return
        self._growth_prepare()
        need = int(self.table.census()[0]) + int(incoming)
        if g.reduce_max is not None:  # (the fullest shard decides: equal capacities)
            need = g.reduce_max(need)
        if need > g.at * cap:
            while need > g.at / 2 * cap:
                cap *= 2
            g._grow(cap)
        g.bound = need
