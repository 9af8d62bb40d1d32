"""One parsed chunk of examples split by feature group (slot): what
``SlotData.from_batch`` makes of a CSR batch with per-feature slot ids, on the device
(``slotsplit.hip``) for GPU tensors and by a stable sort for CPU tensors.

The device path is a strict fast path with the contract of ops/textparse.py: a chunk the
kernels decide is split entirely by them; a chunk that names more than ``max_ids()``
groups or a group id outside [0, 2^31) (cause ``"ids"``), whose
``S * (R + 1)`` cells exceed the cell cap (``"cells"``) or in which a row names a group
twice (``"repeat"``: the stable order of two runs cannot be had from unordered atomics) is
copied back, split by ``SlotData.from_batch`` and uploaded -- the caller sees the same
arrays and ``deferred=True``. One small header (group count, flags, group ids and totals)
is read back per call, a stream synchronisation: call it per chunk of text.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .native import hipops, is_gpu

SS_S, SS_FLAGS, SS_NCELLS, SS_TOTAL, SS_IDS = 0, 1, 2, 3, 8  # header words (slotsplit.h)
F_IDS, F_REPEAT, F_CELLS, F_INPUT = 1, 2, 4, 8


def tile() -> int:
    """Features per workgroup of the per-feature kernels."""
    return int(hipops().slotsplit_tile())


def max_ids() -> int:
    """Most distinct group ids of a chunk the device path takes (the reference's kSlotIDmax)."""
    return int(hipops().slotsplit_max_ids())


def default_cell_cap() -> int:
    return int(hipops().slotsplit_default_cell_cap())


@dataclass
class SlotSplit:
    """``groups[g] = (offset int64[rows + 1], keys int64[nnz_g] (raw uint64 bits), vals
    f32[nnz_g] | None)`` for every distinct slot id ``g``, ascending; the groups are views
    into slot-major arrays on the inputs' device."""

    groups: dict
    deferred: bool = False
    cause: str | None = None  # "ids" | "repeat" | "cells" when deferred

    def numpy(self) -> dict:
        """The groups as ``SlotData.from_batch`` has them: int64 / uint64 / float32 arrays."""
        return {g: (o.cpu().numpy(), k.cpu().numpy().view(np.uint64),
                    None if v is None else v.cpu().numpy())
                for g, (o, k, v) in self.groups.items()}


def _tensor(x, dtype):
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        if x.dtype == np.uint64:
            x = x.view(np.int64)
        x = torch.from_numpy(x)
    return x.to(dtype).contiguous()


def _split_cpu(row_ptr, keys, vals, slots) -> dict:
    R, n = row_ptr.numel() - 1, keys.numel()
    if n == 0:
        return {}
    ids, sidx = torch.unique(slots, sorted=True, return_inverse=True)
    order = torch.argsort(sidx, stable=True)  # slot-major, the original order inside a slot
    bounds = [0] + torch.cumsum(torch.bincount(sidx, minlength=ids.numel()), 0).tolist()
    row_of = torch.repeat_interleave(torch.arange(R, dtype=torch.int64),
                                     row_ptr[1:] - row_ptr[:-1])[order]
    keys_s = keys[order]
    vals_s = None if vals is None else vals[order]
    first = torch.arange(R + 1, dtype=torch.int64)
    out = {}
    for s, g in enumerate(ids.tolist()):
        a, b = bounds[s], bounds[s + 1]
        off = torch.searchsorted(row_of[a:b].contiguous(), first).to(torch.int64)
        out[int(g)] = (off, keys_s[a:b], None if vals_s is None else vals_s[a:b])
    return out


def _split_host(row_ptr, keys, vals, slots, device) -> dict:
    """The deferred chunk: copied back, split by ``SlotData.from_batch``, uploaded."""
    from ..data import ExampleBatch
    from ..data.slot_reader import SlotData

    rp = row_ptr.cpu().numpy()
    b = ExampleBatch(np.zeros(rp.size - 1, np.float32), rp, keys.cpu().numpy().view(np.uint64),
                     None if vals is None else vals.cpu().numpy(), slots.cpu().numpy())
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)  # noqa: E731
    return {g: (up(o), up(k.view(np.int64)), None if v is None else up(v))
            for g, (o, k, v) in SlotData.from_batch(b).groups.items()}


def split_by_slot(labels, row_ptr, keys, vals, slots, *, cell_cap: int | None = None) -> SlotSplit:
    """Split the examples ``row_ptr`` int64[R + 1] (any base) / ``keys`` int64[N] (uint64
    bit patterns; a uint64 array is taken as such) / ``vals`` f32[N] or None / ``slots``
    int32[N] by slot. ``labels`` (f32[R] or None) only fixes the row count. GPU tensors take
    the kernels (on the current stream), CPU tensors and arrays the PyTorch path.
    ``cell_cap``: the most ``S * (R + 1)`` cells the device path takes (default
    ``default_cell_cap()``, at most 2^30)."""
    row_ptr = _tensor(row_ptr, torch.int64)
    keys = _tensor(keys, torch.int64)
    slots = _tensor(slots, torch.int32)
    vals = None if vals is None else _tensor(vals, torch.float32)
    R, n = row_ptr.numel() - 1, keys.numel()
    if R < 0 or slots.numel() != n or (vals is not None and vals.numel() != n):
        raise ValueError("split_by_slot: row_ptr [R + 1], keys / vals / slots [N]")
    if labels is not None and len(labels) != R:
        raise ValueError("split_by_slot: one label per row")
    if not is_gpu(keys):
        if n and (R < 1 or int(row_ptr[-1] - row_ptr[0]) != n):
            raise ValueError("split_by_slot: row_ptr does not cover the features")
        return SlotSplit(_split_cpu(row_ptr, keys, vals, slots))
    if not (is_gpu(row_ptr) and is_gpu(slots) and (vals is None or is_gpu(vals))):
        raise ValueError("split_by_slot: all arrays on one device")
    if n == 0:
        return SlotSplit({})
    if R < 1:
        raise ValueError("split_by_slot: features without a row")
    H = hipops()
    dev = keys.device
    cap = default_cell_cap() if cell_cap is None else int(cell_cap)
    if not 0 <= cap <= 1 << 30:
        raise ValueError("split_by_slot: cell_cap in [0, 2^30]")
    # (S <= max_ids: a chunk of few rows needs a small work space whatever the cap)
    cells = max(1, min(cap, max_ids() * (R + 1)))
    with torch.cuda.device(dev):
        hdr = torch.empty(H.slotsplit_hdr_words(), dtype=torch.int32, device=dev)
        work = torch.empty(H.slotsplit_work_words(n, cells), dtype=torch.int32, device=dev)
        keys_out = torch.empty_like(keys)
        vals_out = None if vals is None else torch.empty_like(vals)
        H.slotsplit(row_ptr, keys, vals, slots, min(cap, cells), cells, keys_out, vals_out, hdr,
                    work)
        h = hdr.cpu()  # (the one read-back of the call)
        flags = int(h[SS_FLAGS])
        if flags & F_INPUT and not flags & (F_IDS | F_CELLS):
            raise ValueError("split_by_slot: row_ptr does not cover the features")
        if flags:
            cause = "ids" if flags & F_IDS else "cells" if flags & F_CELLS else "repeat"
            return SlotSplit(_split_host(row_ptr, keys, vals, slots, dev), True, cause)
        S, m = int(h[SS_S]), max_ids()
        ids = h[SS_IDS:SS_IDS + S].tolist()
        totals = h[SS_IDS + m:SS_IDS + m + S].tolist()
        off = torch.empty((S, R + 1), dtype=torch.int64, device=dev)
        H.slotsplit_offsets(work, n, cells, R, S, off)
    groups, a = {}, 0
    for s, g in enumerate(ids):
        b = a + totals[s]
        groups[int(g)] = (off[s], keys_out[a:b], None if vals_out is None else vals_out[a:b])
        a = b
    return SlotSplit(groups)
