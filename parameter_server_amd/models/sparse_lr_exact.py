"""SparseLRTrainer's generic pull / push: one shard, and G > 1 with exchange="exact"
(count exchange + sized all-to-all-v, one host sync per step; fused into two
all-to-alls where nothing filters or quantises). A mixin of models/sparse_lr.py."""
from __future__ import annotations

import torch

from ..ops import fixing_float as ff
from ..ops.native import hipops


class ExactExchange:
    # ------------------------------------------------------- fused exchange (G > 1)
    def _exchange_fused(self, loc):
        """One step of the multi-GPU data plane with 2 all-to-alls instead of 3:

        A: per peer [keys(t) | grads(t-1)] packed as int32 words (keys are u32 when
           the mixed key space has <= 32 bits, else 2 words) -> the owner first
           applies the pushes of step t-1 (one optimizer step per source, rank
           order), THEN resolves the pulls of step t, so every pull sees all pushes
           up to t-1 (same order of operations as the unfused path: BSP results);
        B: weights back.
        The per-peer counts of both directions come from ONE all-gather of the
        G x G count matrix (the only host synchronisation of the step)."""
        uniq, n_uniq = loc.uniq, loc.n_uniq
        G, dev = self.G, uniq.device
        kw = 1 if self.bits <= 32 else 2
        off = self.part.split_sorted(uniq, n_uniq)
        send_t = (off[1:] - off[:-1]).to(torch.int64)
        M_dev = self.comm.all_gather_counts(send_t, to_host=False)
        if self._prefetch is not None:  # overlap the next minibatch with this sync
            self._prefetch()
            self._prefetch = None
        M = M_dev.cpu()                                  # [G src, G dst], host
        send_t = M[self.rank].tolist()
        recv_t = M[:, self.rank].tolist()
        U = int(sum(send_t))
        if self.pending is not None:
            slot_p, send_p, recv_p, g_p = self.pending
        else:
            slot_p, send_p, recv_p, g_p = None, [0] * G, [0] * G, None
        keys = uniq[:U]
        k32 = keys.to(torch.int32) if kw == 1 else keys.contiguous().view(torch.int32)
        g32 = g_p.view(torch.int32) if g_p is not None else None
        pieces, ks, gs = [], 0, 0
        for p in range(G):
            pieces.append(k32[ks * kw:(ks + send_t[p]) * kw])
            ks += send_t[p]
            if g32 is not None:
                pieces.append(g32[gs:gs + send_p[p]])
                gs += send_p[p]
        sendbuf = torch.cat(pieces) if pieces else torch.empty(0, dtype=torch.int32, device=dev)
        ssz = [kw * send_t[p] + send_p[p] for p in range(G)]
        rsz = [kw * recv_t[s] + recv_p[s] for s in range(G)]
        recv = self.comm.all_to_all_v(sendbuf, ssz, rsz)
        kparts, gparts, a = [], [], 0
        for s in range(G):
            kparts.append(recv[a:a + kw * recv_t[s]])
            a += kw * recv_t[s]
            n = recv_p[s]
            if n and slot_p is not None:
                gparts.append((slot_p[s], recv[a:a + n].view(torch.float32)))
            a += n
        self._apply_pushes(gparts)  # pushes of step t-1 first ...
        rk = torch.cat(kparts)
        if kw == 1:
            req = rk.to(torch.int64) & 0xFFFFFFFF
        else:
            req = rk.view(torch.int64)
        slot, w = self.table.resolve(req, insert=True)  # ... then the pulls of step t
        slots_by_src, a = [], 0
        for s in range(G):
            slots_by_src.append(slot[a:a + recv_t[s]])
            a += recv_t[s]
        w_back = self.comm.all_to_all_v(w, recv_t, send_t)
        return w_back, ("fused", slots_by_src, send_t, recv_t, U)

    def _fused_flush(self):
        """Exchange and apply the gradients the last fused step deferred (``flush``)."""
        slot_p, send_p, recv_p, g_p = self.pending
        self.pending = None
        g_in = self.comm.all_to_all_v(g_p, send_p, recv_p)
        parts, a = [], 0
        for s in range(self.G):
            n = recv_p[s]
            if n:
                parts.append((slot_p[s], g_in[a:a + n]))
            a += n
        self._apply_pushes(parts)

    def _apply_pushes(self, parts):
        """parts: [(slots, grads)] per source in rank order."""
        if not parts:
            return
        if self.cfg.push_mode == "aggregate":
            self._apply_aggregated(torch.cat([p[0] for p in parts]),
                                   torch.cat([p[1] for p in parts]).contiguous())
            return
        for slot, g in parts:  # one optimizer step per push message, in rank order
            self.table.update(slot, g.contiguous(), self.rule, self.stats)

    # ---------------------------------------------------------------- pull/push
    def _pull(self, uniq: torch.Tensor, n_uniq: torch.Tensor):
        """Pull weights of sorted unique mixed keys; returns (w_local, push handle)."""
        if self.G == 1:
            U = int(n_uniq.item())
            keys = uniq[:U]
            slot, w = self.table.resolve(keys, insert=True)
            return w, ("local", slot, None)
        off = self.part.split_sorted(uniq, n_uniq).cpu()
        U = int(off[-1])
        send_counts = (off[1:] - off[:-1])
        recv_counts = self.comm.exchange_counts(send_counts).cpu()
        req = self.comm.all_to_all_v(uniq[:U], send_counts.tolist(), recv_counts.tolist())
        slot, w = self.table.resolve(req, insert=True)
        w_back = self.comm.all_to_all_v(w, recv_counts.tolist(), send_counts.tolist())
        return w_back, ("dist", slot, send_counts, recv_counts, U)

    def _pull_filtered(self, loc):
        """Tail-feature filter on the generic paths (reference MinibatchReader::read,
        sgd.h:140-148): insert per-key counts into the worker's CountMin, pull only keys
        whose estimated count > tail_feature_freq; filtered keys get w = 0, no push. (The
        flat layout filters inside its bucket kernel instead, tpf_filter_unit.) GPU, one
        shard: device-side compaction and counts, no host sync."""
        if not (self.gpu and self.G == 1):
            U = loc.num_unique()
            uniq = loc.uniq[:U]
            cnt = (loc.seg_start[1:U + 1] - loc.seg_start[:U]).clamp(max=255).to(torch.uint8)
            self.filter.insert(uniq, cnt)
            keep, _ = self.filter.query(uniq, self.cfg.tail_feature_freq)
            kept_idx = torch.nonzero(keep, as_tuple=False).flatten()
            w_kept, push = self._pull(uniq[kept_idx].contiguous(),
                                      torch.tensor([kept_idx.numel()], dtype=torch.int32,
                                                   device=uniq.device))
            w_local = torch.zeros(loc.grad.numel(), dtype=torch.float32, device=uniq.device)
            w_local[kept_idx] = w_kept
            return w_local, ("filtered", kept_idx, push)
        U = loc.uniq.numel()  # (workspace length; the live count stays on the device)
        pf = self._pf
        if pf is None or pf["w"].numel() < U + 1:
            pf = self._pf = {"w": torch.empty(U + 1, dtype=torch.float32, device=self.device),
                             "wk": torch.empty(U, dtype=torch.float32, device=self.device)}
        kk, ki, nk = self._tail_filter(loc, 0)  # kept keys, kept -> unique id, kept count
        ki[:U].masked_fill_(torch.arange(U, device=self.device) >= nk.long(), U)  # tail -> dummy
        slot, wk = self.slot_buf, pf["wk"][:U]
        hipops().kv_resolve(self.table.slots, kk, nk, slot, wk, True, *self.table.resolve_args())
        w_local = pf["w"][:U + 1]
        w_local.zero_()
        w_local.index_copy_(0, ki[:U].long(), wk)  # (kept tail past nk lands on the dummy U)
        return w_local[:U], ("filtered_dev", ki[:U], slot, nk)

    def _push(self, grad: torch.Tensor, push, fold_auc: bool = False) -> bool:
        """Apply a push; True when the step's AUC epilogue rode along (``fold_auc``: the
        1-GPU KV update's block 0 turns the histogram into metrics, one launch less)."""
        kind = push[0]
        if kind == "filtered_dev":  # gradients of the kept keys, in kept order (no host sync)
            _, ki, slot, nk = push
            g = torch.cat([grad[:ki.numel()], grad.new_zeros(1)])[ki.long()]
            return self._kv_update(slot, g, nk, fold_auc)
        if kind == "filtered":
            kept_idx, inner = push[1], push[2]
            g = grad[kept_idx].contiguous()
            return self._push(g, inner)
        if kind == "local":
            slot, n_dev = push[1], push[2]
            if n_dev is not None:  # (the slot workspace is sized for the largest batch)
                slot = slot[:grad.numel()]
            if n_dev is None:
                self.table.update(slot, grad[:slot.numel()], self.rule, self.stats)
                return False
            return self._kv_update(slot, grad, n_dev, fold_auc)
        _, slot, send_counts, recv_counts, U = push
        g = grad[:U].contiguous()
        nb = self.cfg.fixing_float_bytes
        if nb:
            code, mm = ff.encode(g, nb, seed=self.cfg.seed * 7919 + self.step_count)
            mm_all = self.comm.all_to_all_v(mm.repeat(self.G), [2] * self.G, [2] * self.G)
            code_in = self.comm.all_to_all_v(code, (send_counts * nb).tolist(),
                                             (recv_counts * nb).tolist())
            parts, a = [], 0
            for s in range(self.G):
                n = int(recv_counts[s])
                parts.append(ff.decode(code_in[a * nb:(a + n) * nb], nb, mm_all[2 * s:2 * s + 2], n))
                a += n
            g_in = torch.cat(parts) if parts else torch.empty(0, device=g.device)
        else:
            g_in = self.comm.all_to_all_v(g, send_counts.tolist(), recv_counts.tolist())
        if self.cfg.push_mode == "aggregate":
            self._apply_aggregated(slot, g_in)
            return False
        a = 0
        for s in range(self.G):  # one optimizer step per push message, in rank order
            n = int(recv_counts[s])
            if n:
                self.table.update(slot[a:a + n], g_in[a:a + n], self.rule, self.stats)
            a += n
        return False

    def _kv_update(self, slot, grad, n_dev, fold_auc: bool) -> bool:
        """The 1-GPU KV update of ``n_dev`` (device count) slots; ``fold_auc``: with the
        step's AUC epilogue in its block 0. Returns ``fold_auc``."""
        auc = (dict(hist=self.hist, metrics=self.metrics, step_counter=self.step_dev)
               if fold_auc else {})
        hipops().kv_update(self.table.slots, slot, grad, n_dev, *self.rule.args(), self.stats,
                           **auc)
        return fold_auc

    def _apply_aggregated(self, slot: torch.Tensor, g_in: torch.Tensor):
        if self.gpu:
            if self.touched is None or self.touched.numel() < slot.numel():
                self.touched = torch.empty(max(slot.numel(), 1024), dtype=torch.int64,
                                           device=self.device)
                self.n_touched = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.n_touched.zero_()
            H = hipops()
            H.kv_accumulate(self.table.slots, slot, g_in, None, self.touched, self.n_touched)
            H.kv_apply_accumulated(self.table.slots, self.touched[:slot.numel()], self.n_touched,
                                   *self.rule.args(), self.stats)
            return
        valid = slot >= 0
        s, inv = torch.unique(slot[valid], return_inverse=True)
        g = torch.zeros(s.numel(), dtype=torch.float32).index_add_(0, inv, g_in[valid])
        self.table.update(s, g, self.rule, self.stats)
