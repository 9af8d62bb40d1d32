"""SparseLRTrainer's one-sided peer exchange (G > 1, exchange="p2p": parallel/p2p.py).
A mixin of models/sparse_lr.py."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from ..ops.kv_table import next_pow2
from ..ops.linear import auc_from_hist, linear_fwd_bwd
from ..ops.native import hipops
from ..parallel.p2p import PeerExchange


class P2PExchange:
    def _p2p_setup(self, loc):
        """Row geometry (C keys per owner row: slack x the largest per-owner count of the
        first minibatch over all ranks, like the padded exchange) and the IPC mappings."""
        cfg, G, dev = self.cfg, self.G, self.device
        off = torch.empty(G + 1, dtype=torch.int64, device=dev)
        hipops().owner_split(loc.uniq, loc.n_uniq, self.part.bounds_on(dev), off)
        C = self._agree_capacity(lambda: (off[1:] - off[:-1]).max())
        kw, nb, _, H = self._row_geometry(C)  # (FixingFloat pushes: the padded layout)
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
        self.xc = SimpleNamespace(
            C=C, kw=kw, H=H, nb=nb, w0=None, off=off,
            send=i32(G * H),
            gstage=torch.zeros(G * C, dtype=torch.float32, device=dev) if nb else None,
            wout=torch.zeros(G * C, dtype=torch.float32, device=dev),
            slot=torch.full((G * C,), -1, dtype=torch.int64, device=dev),
            w_local=torch.zeros(self.max_nnz, dtype=torch.float32, device=dev),
            a_slot=torch.full((G * C,), -1, dtype=torch.int64, device=dev),
            a_w=torch.zeros(G * C, dtype=torch.float32, device=dev),
            link=torch.empty(next_pow2(2 * G * C), dtype=torch.int64, device=dev),
            nxt=torch.empty(G * C, dtype=torch.int32, device=dev), ovf=i32(1),
            ovf_host=torch.zeros(1, dtype=torch.int32, pin_memory=True))
        self.px = PeerExchange(self.comm, self.table, C, kw, H, dev, Q=cfg.p2p_queue, nb=nb)

    def _p2p_step(self, loc, labels, width, prefetch=None):
        """One asynchronous step: pack this minibatch's keys per owner, pull them
        one-sided (own row: lookup-or-insert), forward + backward, pack the gradients
        next to the keys, apply the own row locally, post the peer rows into the
        owners' inboxes, and apply whatever the peers have posted here so far."""
        if self.xc is None:
            self._p2p_setup(loc)
        xc, hh, G, r = self.xc, hipops(), self.G, self.rank
        C, kw, H = xc.C, xc.kw, xc.H
        B = labels.numel()
        width = width or self.cfg.max_nnz_per_example
        self.px.wait_own()  # (the previous own-row update has read send / slot / gstage)
        hh.owner_split(loc.uniq, loc.n_uniq, self.part.bounds_on(self.device), xc.off)
        hh.xchg_pack_keys(loc.uniq, loc.n_uniq, xc.off, C, kw, H, xc.send, xc.ovf)
        if xc.nb:  # (FixingFloat: no pack_grads launch to publish the overflow flag)
            hh.xchg_publish(xc.ovf, xc.ovf_host)
        self.px.lookup(xc.send, xc.wout, xc.slot)
        if prefetch is not None:  # the next minibatch's preparation overlaps this step
            prefetch()
        U = loc.uniq.numel()
        w_local = xc.w_local[:U]
        hh.xchg_unpack_w(xc.wout, None, loc.n_uniq, xc.off, C, w_local)
        _, grad = linear_fwd_bwd(loc, w_local, labels, B=B, width=width, loss=self.cfg.loss,
                                 coef=self.coef[:B], metrics=self.metrics, hist=self.hist)
        if xc.nb:
            # FixingFloat codes for the peers (reference async_sgd.h:273-277); the own row
            # is decoded from its codes too, as the padded exchange decodes every recv row
            # (the reference quantises every push through its filter)
            hh.xchg_ff_pack_grads(grad[:U], None, loc.n_uniq, xc.off, C, kw, H, xc.nb,
                                  self._ff_seed, self.step_dev, xc.send, xc.gstage)
            g_own = xc.gstage[r * C:(r + 1) * C]
            hh.xchg_ff_decode(xc.send[r * H:(r + 1) * H], C, kw, H, xc.nb, g_own)
            auc_from_hist(self.hist, self.metrics, self.step_dev)
        else:
            hh.xchg_pack_grads(grad[:U], None, loc.n_uniq, xc.off, C, kw, H, xc.send,
                               hist=self.hist, metrics=self.metrics, step_counter=self.step_dev,
                               ovf=xc.ovf, ovf_host=xc.ovf_host)
            g_own = xc.send.view(torch.float32)[r * H + 4 + C * kw:r * H + 4 + C * kw + C]
        self.px.own_update(xc.slot[r * C:(r + 1) * C], g_own, xc.send[r * H + 1:r * H + 2],
                           self.rule, self.stats)
        self.px.post(xc.send)
        self.px.check_fatal()
        self.px.apply(self.rule, self.stats, xc.a_slot, xc.a_w, xc.link, xc.nxt,
                      rounds=self.cfg.p2p_rounds)
        self.step_count += 1
        self.examples += B
        if int(xc.ovf_host[0]):
            raise self._overflow_error("p2p exchange", "some", C)
