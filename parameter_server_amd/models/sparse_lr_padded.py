"""SparseLRTrainer's padded exchange (G > 1, default): fixed-capacity rows per peer with
device-side counts, as two collectives per step (``step_segments``) or merged into one
(``mx_*``, lag >= 1). A mixin: it reads the trainer's state (models/sparse_lr.py)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from ..ops import fixing_float as ff
from ..ops.kv_table import next_pow2
from ..ops.linear import AUC_BINS, auc_from_hist, linear_fwd_bwd, loss_id
from ..ops.native import hipops


def _same_workspace(a, b) -> bool:
    """Two localisations share device workspaces (the same Localizer buffer set)."""
    if a is b:
        return True
    ua, ub = getattr(a, "uniq", None), getattr(b, "uniq", None)
    return (isinstance(ua, torch.Tensor) and isinstance(ub, torch.Tensor) and ua.numel() > 0
            and ua.device == ub.device and ua.data_ptr() == ub.data_ptr())


class PaddedExchange:
    # ------------------------------------- two collectives per step (and idle steps)
    def idle_step(self):
        """A key-less step (multi-rank file-fed runs, app/gpu.py): a rank whose data ran
        out still joins the exchanges -- it owns a key range, so it resolves its peers'
        pulls, applies their pushes and ships its own last pushes -- without pulling,
        computing or pushing anything itself. Collective on the padded exchange; a no-op
        on one rank."""
        if self.G == 1:
            return
        if not self.padded:
            raise NotImplementedError("key-less steps need the padded exchange")
        if self._growth is not None:  # (this owner still receives its peers' keys)
            self._growth_step(None, None, None)
        if self.merged:
            return self._mx_step(None, None, idle=True)
        for _, fn in self.step_segments(None, None, idle=True):
            fn()

    def step_segments(self, keys: torch.Tensor, labels: torch.Tensor, *, width=None,
                      row_ptr=None, vals=None, rows=None, loc=None, step=None, next_loc=None,
                      idle: bool = False):
        """The step as an ordered list of ``(kind, fn)``: ``"compute"`` segments are
        pure device work on fixed buffers (capturable in a HIP graph per localisation
        buffer and ring position), ``"comm"`` segments are the two equal-split RCCL
        all-to-alls, ``"async"`` (ASP only) is the owner's push apply that pulls do
        not wait for, and ``"host"`` is the host bookkeeping. No segment reads anything
        back to the host, so a step is enqueued without waiting for the GPU.

          compute  owner-split the unique keys, pack [keys(t)] next to [grads(t-1-lag)]
          comm     all-to-all A
          compute  owner: apply the pushes of t-1-lag (one optimizer step per source,
                   rank order, all sources in one launch), then lookup-or-insert of
                   the pulled keys of t -> weights       [ASP / SSP post: resolve only]
          async    [ASP: apply the pushes of t-1-lag; the next pulls do not wait]
          comm     all-to-all B (weights back)
          post     [SSP post (lag >= 1): apply the pushes of t-lag carried by this
                   exchange; the worker does not wait for it, the next exchange does]
          compute  unpack weights, forward, backward, pack grads(t), AUC
          host     counters, overflow check

        Everything before the last compute segment is the exchange half, the rest the
        worker half (``EXCHANGE_SEGMENTS``); with lag >= 1 the exchange half of step
        t+1 may run while the worker half of step t computes (bench.py issues them on
        different streams). Buffers live in rings of ``self.R`` entries indexed by the
        absolute step ``step`` (default: the next step to compute); only ``step %
        self.R`` matters, so a graph captured for ring position j replays for every
        step t with t % R == j.
        """
        if not self.padded:
            return [("compute", lambda: self.step(keys, labels, width=width, row_ptr=row_ptr,
                                                  vals=vals, rows=rows, loc=loc,
                                                  next_loc=next_loc))]
        t = self._xt if step is None or idle else int(step)
        r = self.sched.ring(t)        # ring position of step t
        gb = self.sched.grad_ring(t)  # grads(t-1-lag) live here; keys(t) join them
        if idle:
            # a key-less step: the same exchange half with no keys packed (the carried
            # gradients still travel) and, for the worker half, no gradients of this step
            if self.xc is None:
                self._xc_setup(None)
            xc = self.xc
            return ([("compute", lambda: self._x_clear(xc.sends[gb], keys=True))]
                    + self._x_owner_half(r, gb)
                    + [("compute", lambda: self._x_clear(xc.sends[r], grads=True)),
                       ("host", lambda: self._x_done(0))])
        if loc is None:
            loc = self.localizer(keys)
        B = labels.numel()
        width = self._width(width, row_ptr)
        how = self._route(B, width, loc.nnz, row_ptr, rows, vals, loc)
        if how == "compact" and getattr(loc, "flat", False):
            # not expressible on the flat layout: the same keys, localised compactly
            loc = self._compact_localizer()(keys)
        csr = None
        if how == "flat_csr":
            csr = self._csr_operands(B, width, loc.nnz, row_ptr, rows, vals)
        elif how == "compact":
            rows = self._compact_rows(row_ptr, rows, keys.numel())
        if self.xc is None:
            self._xc_setup(loc)

        finish = self._x_worker_half(loc, labels, B, width, row_ptr, vals, rows, csr, r)
        pack = (lambda: self._x_pack_keys(loc, gb, r)) if how == "compact" else \
            (lambda: self._x_pack_keys_flat(loc, gb, r))
        return ([("compute", pack)] + self._x_owner_half(r, gb)
                + [("compute", finish), ("host", lambda: self._x_done(B))])

    def _x_worker_half(self, loc, labels, B, width, row_ptr, vals, rows, csr, r: int, **dst):
        """The worker half of a step on ring entry ``r`` as one callable (``dst``: where
        the merged exchange reads its weights and packs its gradients). The row of every
        occurrence is derived from ``row_ptr`` at replay time, inside the segment."""
        if getattr(loc, "flat", False):
            def fin():
                if csr is not None:  # (row_ptr, rows, vals); rows: scratch, refilled here
                    hipops().csr_rows(csr[0], csr[1])
                self._x_finish_flat(loc, labels, B, width, r, csr=csr, **dst)
        else:
            def fin():
                if row_ptr is not None and self.gpu:
                    hipops().csr_rows(row_ptr, rows)
                self._x_finish(loc, labels, B, width, row_ptr, vals, rows, r, **dst)
        return fin

    def _x_owner_half(self, r: int, gb: int):
        """The segments between a step's key pack and its worker half: all-to-all A, the
        owner's resolve of the pulls and apply of the carried pushes (asp: the apply on
        its own; ssp post: after the weights went back; else before the resolve),
        all-to-all B and the count of issued exchanges."""
        comm, xc = self.comm, self.xc

        def exchanged():
            self._xx += 1

        segs = [("comm", lambda: comm.all_to_all_fixed(xc.sends[gb], xc.recvs[r]))]
        if self.asp:
            segs += [("compute", lambda: self._x_resolve(r)),
                     ("async", lambda: self._x_apply(r, gb))]
        elif self.sched.post:
            segs += [("compute", lambda: self._x_resolve(r))]
        else:
            segs += [("compute", lambda: (self._x_apply(r, gb), self._x_resolve(r)))]
        segs += [("comm", lambda: comm.all_to_all_fixed(xc.wsend, xc.wrecvs[r])),
                 ("host", exchanged)]
        if self.sched.post:  # the carried pushes, after the weights went back
            segs += [("post", lambda: self._x_apply(r, gb))]
        return segs

    def _x_done(self, B: int):
        """Host bookkeeping of one worker step on the padded exchange (``B`` = 0: idle)."""
        self.step_count += 1
        self._xt += 1
        self.examples += B
        self._x_poll_overflow()

    def _x_clear(self, buf, keys: bool = False, grads: bool = False):
        """Zero the key and / or gradient count of every row of a send buffer."""
        if self.gpu:
            hipops().xchg_clear_counts(buf, self.xc.H, keys, grads)
            return
        for p in range(self.G):
            if keys:
                buf[p * self.xc.H] = 0
            if grads:
                buf[p * self.xc.H + 1] = 0

    # ------------------------------ merged exchange (one all-to-all per step, lag >= 1)
    def mx_exchange(self, s: int, next_loc=None, *, prepare=True):
        """The parts of merged exchange ``s`` (parallel/consistency.MergedSchedule) as a
        dict of callables, for a caller that orders them against other streams
        (bench.py) -- or run in order by ``_mx_step``:

          pack     keys(s+1) of ``next_loc`` into the send rows of exchange s (None: no
                   keys -- a drain or an idle rank)
          comm     the all-to-all (send rows hold grads(s-d) packed by worker s-d and the
                   weights resolved after exchange s-1)
          resolve  owner: lookup-or-insert keys(s+1) -> slots of pull step s+1, their
                   weights into the send rows of exchange s+1
          apply    owner: the pushes of step s-d (``post``: after resolve, else before)

        Everything is fixed device buffers (ring entries), so each part replays from a
        HIP graph captured for ring position s % R. ``prepare``: allocate the exchange
        rows on the first call (collective: agrees on the row capacity)."""
        if self.xc is None and prepare:
            self._xc_setup(next_loc)
        xc, ms, comm = self.xc, self.msched, self.comm
        R, d = ms.R, ms.d
        b, bn = s % R, (s + 1) % R
        send, recv = xc.sends[b], xc.recvs[b]
        flat = next_loc is not None and getattr(next_loc, "flat", False)

        def pack():
            if next_loc is None:
                self._x_clear(send, keys=True)
            elif flat:
                self._x_pack_keys_flat(next_loc, b, bn)
            else:
                self._x_pack_keys(next_loc, b, bn)

        def resolve():
            self._x_resolve(b, bn, wout=self._mx_wview(xc.sends[bn]), wstride=xc.H)

        def apply():
            if s - d >= 0:
                self._x_apply(b, (s - d) % R)

        return {"pack": pack, "comm": lambda: comm.all_to_all_fixed(send, recv),
                "resolve": resolve, "apply": apply, "post": ms.post}

    def mx_worker(self, u: int, loc, labels, *, width=None, row_ptr=None, vals=None, rows=None):
        """Worker half of step ``u`` on the merged exchange: weights read in place from
        the rows of exchange u, forward + backward, gradients into the send rows of
        exchange u+d (+ AUC epilogue). ``loc=None``: an idle step (no minibatch): only
        clears its gradient rows."""
        xc, ms = self.xc, self.msched
        R = ms.R
        b, bg = u % R, ms.grad_ring(u)
        if loc is None:
            return lambda: self._x_clear(xc.sends[bg], grads=True)
        B = labels.numel()
        width = self._width(width, row_ptr)
        csr = None
        if getattr(loc, "flat", False) and (row_ptr is not None or vals is not None):
            csr = self._csr_operands(B, width, loc.nnz, row_ptr, rows, vals)
        return self._x_worker_half(loc, labels, B, width, row_ptr, vals, rows, csr, b,
                                   send=xc.sends[bg], wsrc=self._mx_wview(xc.recvs[b]),
                                   wstride=xc.H)

    mx_done = _x_done  # host bookkeeping of one merged worker step

    def _mx_wview(self, buf: torch.Tensor) -> torch.Tensor:
        """The weight words of a row buffer, as floats from row 0's weight offset (row
        stride H)."""
        return buf.view(torch.float32)[self.xc.w0:]

    def _mx_run_exchange(self, s: int, next_loc):
        parts = self.mx_exchange(s, next_loc)
        parts["pack"]()
        parts["comm"]()
        if parts["post"]:
            parts["resolve"]()
            parts["apply"]()
        else:
            parts["apply"]()
            parts["resolve"]()
        self._mx_next = s + 1

    def _mx_step(self, keys, labels, *, width=None, row_ptr=None, vals=None, rows=None,
                 loc=None, prefetch=None, idle: bool = False):
        """Sequential API on the merged exchange: step(u) issues exchange u-1, which
        carries keys(u), and then runs the worker half of step u-1 (its weights came
        with that exchange). So a call trains the PREVIOUS minibatch; ``flush()`` (and
        ``progress()``) trains the last one and applies every outstanding push. The
        minibatch tensors are captured (labels / row_ptr / vals copied).

        A caller-supplied ``loc`` lives in a workspace the caller refills (``localize(k,
        buf=...)``): the pending minibatch keeps a copy of its keys, and when the caller's
        localisation of this minibatch reused the pending one's workspace, the pending
        minibatch is localised again into a private workspace before its worker half.
        ``prefetch`` runs after that worker half is enqueued (it may refill the pending
        minibatch's workspace)."""
        cur = None
        pend = self._mx_pend
        if not idle:
            B = labels.numel()
            width = self._width(width, row_ptr)
            buf = self._xt + (pend is not None)  # step index of this minibatch
            flat_ok = self._route(B, width, keys.numel(), row_ptr, rows, vals, None) != "compact"
            own = loc is None
            if own:
                loc = (self.localize(keys, buf=buf % 2) if flat_ok
                       else self._compact_localizer(buf % 2)(keys))
            if not getattr(loc, "flat", False):
                rows = self._compact_rows(row_ptr, rows, keys.numel())
            cur = dict(loc=loc, labels=labels.clone(), width=width,
                       row_ptr=None if row_ptr is None else row_ptr.clone(),
                       vals=None if vals is None else vals.clone(), rows=rows, B=B,
                       keys=None if own else keys.clone(), flat=flat_ok)
            if pend is not None and not pend.get("idle") and pend.get("keys") is not None \
                    and _same_workspace(pend["loc"], loc):
                # the caller localised this minibatch over the pending one's workspace:
                # localise the pending keys again, into a workspace the caller never sees
                if self.filter is not None:  # (a second localisation would count twice)
                    raise ValueError(
                        "merged exchange + tail filter: the caller's localisation of this "
                        "minibatch reused the pending minibatch's workspace; use "
                        "localize(keys, buf=t % 2) or pass keys without loc")
                pend["loc"] = self._mx_private_loc(pend["keys"], pend["flat"])
        u = self._xt + (pend is not None)
        self._mx_run_exchange(u - 1, None if cur is None else cur["loc"])
        self._mx_finish_pending()
        self._mx_pend = cur if cur is not None else {"idle": True}
        if prefetch is not None:
            prefetch()

    def _mx_private_loc(self, keys, flat: bool):
        """Merged sequential API: a localisation in a workspace of the trainer's own (not
        reachable through ``localize``), for a pending minibatch whose caller-supplied
        workspace was refilled."""
        lz = self._mx_own.get(flat)
        if lz is None:
            lz = self._mx_own[flat] = self._new_localizer(
                self.localize_mode if flat else self._compact_mode())
        return lz(keys)

    def _mx_finish_pending(self):
        p, self._mx_pend = self._mx_pend, None
        if p is None:
            return
        if p.get("idle"):  # (only clears its gradient rows; counts no examples)
            self.mx_worker(self._xt, None, None)()
        else:
            self.mx_worker(self._xt, p["loc"], p["labels"], width=p["width"],
                           row_ptr=p["row_ptr"], vals=p["vals"], rows=p["rows"])()
        self.mx_done(p.get("B", 0))

    def mx_drain(self):
        """Apply every computed push that no issued exchange has carried yet: key-less
        exchanges for the remaining ring entries (collective; synchronises the device).
        Leaves the exchange ready for a fresh bootstrap."""
        if self.xc is None:
            return
        ms = self.msched
        if self.gpu:
            torch.cuda.synchronize(self.device)
        last = self._xt - 1  # last worker step whose gradients were packed
        s = self._mx_next if self._mx_next is not None else last + 1
        while s - ms.d <= last:
            self._x_keyless_exchange(s % ms.R, (s - ms.d) % ms.R if s - ms.d >= 0 else None)
            s += 1
        # exchanges s' < s that a new bootstrap may reuse carry no gradients any more
        for j in range(ms.R):
            self._x_clear(self.xc.sends[j], keys=True, grads=True)
        self._mx_next = None
        if self.gpu:
            torch.cuda.synchronize(self.device)

    @property
    def EXCHANGE_SEGMENTS(self) -> int:  # step_segments()[:n] = exchange half
        return 6 if self.asp or self.sched.post else 5

    # ------------------------------------------------- exchange rows and their kernels
    def _xc_setup(self, loc):
        """Allocate the fixed exchange rows. Capacity C (keys per peer per step) is the
        same on every rank: configured, or slack x the max per-peer count of the first
        minibatch over all ranks (collective; hashed keys split ~Binomial(U, 1/G),
        so the margin is many standard deviations)."""
        cfg, G, dev, R = self.cfg, self.G, self.device, self.R

        def count():  # this rank's largest per-owner key count of the first minibatch
            if loc is None:  # a key-less first step (idle_step): join with count 0
                return torch.zeros(1)
            if getattr(loc, "flat", False):
                # the owner's buckets' unit counts (buckets [p * B/G, ...))
                g = hipops().tpf_groups(loc.nnz, loc.bits)
                # (tail filter: the unfiltered counts -- later minibatches keep more keys)
                cc = loc.cnt_pre if getattr(loc, "cnt_pre", None) is not None else loc.cnt
                c = cc[:4 * g].view(G, g // G, 4).to(torch.float64)
                return (c[:, :, 0] + c[:, :, 2]).sum(1).max()
            _, _, off, _ = self._owner_order(loc)
            return (off[1:] - off[:-1]).max()

        C = self._agree_capacity(count)
        kw, nb, w0, H = self._row_geometry(C, self.merged)
        # the partitioned apply needs rows sorted by key and an ordered home (key range
        # -> partition)
        part_apply = self.gpu and cfg.push_mode != "aggregate" and self.table.home_m != 0
        # ~G*C/512 partitions (~1-2 entries per thread of a 256-thread workgroup, rows
        # are ~2/3 full): a few workgroups per CU hide the chain of dependent loads each
        # one runs; many more (tiny ones) pay per-workgroup setup and stats atomics
        # (profiles/r2_owner_apply.log: 8 x 45120 entries, 2^9 -> 21 us, link pair 58 us)
        lgP = max(0, min(16, math.floor(math.log2(max(1, G * C // 512))))) if part_apply else -1
        z32 = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
        self.xc = SimpleNamespace(
            C=C, kw=kw, H=H, nb=nb, w0=w0,
            # (+ the flat pack's per-workgroup min / max partials: 2 per bucket group)
            gstage=z32(G * C + 2 * 2048, torch.float32) if nb else None,
            gins=[z32(G * C, torch.float32) for _ in range(R)] if nb else None,
            # rings of R entries indexed by step: sends[j] holds grads(j) then keys(j+1+lag);
            # recvs[j] what exchange j received; slots[j] the owner's resolved slots of
            # pull step j (its push arrives lag+1 exchanges later)
            sends=[z32(G * H, torch.int32) for _ in range(R)],
            recvs=[z32(G * H, torch.int32) for _ in range(R)],
            slots=[torch.full((G * C,), -1, dtype=torch.int64, device=dev) for _ in range(R)],
            wsend=z32(G * C, torch.float32), wrecvs=[z32(G * C, torch.float32) for _ in range(R)],
            w_local=z32(self.max_nnz, torch.float32), ovf=z32(1, torch.int32),
            offs=[z32(G + 1, torch.int64) for _ in range(R)], curs=[None] * R,
            # the key count the worker half reads, per ring entry (compact layout: allocated
            # by the first _owner_order)
            nkr=None,
            touched=torch.empty(G * C, dtype=torch.int64, device=dev) if self.gpu else None,
            n_touched=z32(1, torch.int32),
            # per-exchange chain scratch of the one-launch sequential push apply
            link=(torch.empty(next_pow2(2 * G * C), dtype=torch.int64, device=dev)
                  if self.gpu and lgP < 0 else None),
            nxt=torch.empty(G * C, dtype=torch.int32, device=dev) if self.gpu and lgP < 0 else None,
            # partitioned one-launch apply (kv_apply_part): the pull's keys and the
            # per-row bounds of 2^lgP key-range partitions, per ring entry
            lgP=lgP, pkeys=([torch.empty(G * C, dtype=torch.int64, device=dev) for _ in range(R)]
                            if lgP >= 0 else None),
            bnd=([torch.zeros(G * ((1 << lgP) + 1), dtype=torch.int32, device=dev)
                  for _ in range(R)] if lgP >= 0 else None),
            ovf_host=(torch.zeros(1, dtype=torch.int32, pin_memory=True) if self.gpu else None),
            ovf_np=None)
        if self.gpu:
            # a numpy view of the pinned word: ~0.1 us to read, vs a few us for a tensor
            # index, on the per-step host path of the pipelines (_x_poll_overflow)
            self.xc.ovf_np = self.xc.ovf_host.numpy()

    def _tail_filter(self, loc, ring: int):
        """Tail-feature filter on the padded exchange (reference MinibatchReader::read,
        src/learner/sgd.h:131-150): insert this minibatch's per-key occurrence counts
        into the worker's CountMin, keep the keys whose estimate > tail_feature_freq.
        Returns (kept keys in sorted order, kept -> unique id, device kept count);
        device-side compaction, no host sync, so the step stays graph-capturable.
        Filtered keys are neither pulled (w = 0) nor pushed."""
        U = loc.uniq.numel()
        freq = self.cfg.tail_feature_freq
        if not self.gpu:
            n = int(loc.n_uniq.reshape(-1)[0])
            self.filter.insert_segments(loc.uniq, loc.seg_start, loc.n_uniq)
            keep, _ = self.filter.query(loc.uniq[:n], freq)
            idx = torch.nonzero(keep, as_tuple=False).flatten().to(torch.int32)
            return (loc.uniq[:n][idx.long()].contiguous(), idx,
                    torch.tensor([idx.numel()], dtype=torch.int32))
        tf = self._tf
        if tf is None or tf["keep"].numel() < U:
            i32 = lambda k: torch.empty(k, dtype=torch.int32, device=self.device)  # noqa: E731
            tf = self._tf = {"keep": i32(U), "incl": i32(U),
                             "keys": [torch.empty(U, dtype=torch.int64, device=self.device)
                                      for _ in range(self.R)],
                             "idx": [i32(U) for _ in range(self.R)],
                             "n": [torch.zeros(1, dtype=torch.int32, device=self.device)
                                   for _ in range(self.R)]}
        keep, incl = tf["keep"][:U], tf["incl"][:U]
        self.filter.insert_segments(loc.uniq, loc.seg_start, loc.n_uniq)
        hh = hipops()
        keep.zero_()
        hh.cm_query(self.filter.cells.view(torch.int32), self.filter.k, self.filter.vmax,
                    loc.uniq, loc.n_uniq, freq, keep, None)
        torch.cumsum(keep, 0, dtype=torch.int32, out=incl)
        kk, ki, nk = tf["keys"][ring], tf["idx"][ring], tf["n"][ring]
        hh.compact_kept(keep, incl, loc.n_uniq, ki, nk, None, loc.uniq, kk)
        return kk, ki, nk

    def _owner_order(self, loc, ring: int = 0):
        """(keys in owner order, perm owner-order -> unique id | None, off[G+1], count)."""
        if self.filter is not None and self.xc is not None:
            kk, ki, nk = self._tail_filter(loc, ring)
            off = self.xc.offs[ring]
            if self.gpu:
                hipops().owner_split(kk, nk, self.part.bounds_on(self.device), off)
            else:
                off = self.part.split_sorted(kk, nk)
            return kk, ki, off, nk
        if self.gpu:
            off = self.xc.offs[ring] if self.xc is not None else torch.empty(
                self.G + 1, dtype=torch.int64, device=self.device)
            hipops().owner_split(loc.uniq, loc.n_uniq, self.part.bounds_on(self.device), off)
            if self.xc is None:
                return loc.uniq, None, off, loc.n_uniq
            # the count the worker half reads later lives in the ring, not in the
            # localiser (a caller may refill that workspace before the worker half runs)
            if self.xc.nkr is None:
                self.xc.nkr = [torch.zeros(1, dtype=torch.int32, device=self.device)
                               for _ in range(self.R)]
            nk = self.xc.nkr[ring]
            nk.copy_(loc.n_uniq.reshape(-1)[:1])
            return loc.uniq, None, off, nk
        return loc.uniq, None, self.part.split_sorted(loc.uniq, loc.n_uniq), loc.n_uniq

    def _x_pack_keys(self, loc, gb: int, r: int):
        xc = self.xc
        ukeys, perm, off, nkeys = self._owner_order(loc, r)
        xc.curs[r] = (perm, off, nkeys)
        send = xc.sends[gb]
        if self.gpu:
            hh = hipops()
            hh.xchg_pack_keys(ukeys, nkeys, off, xc.C, xc.kw, xc.H, send, xc.ovf)
            if xc.nb:  # (FixingFloat push: no pack_grads launch to carry the flag)
                hh.xchg_publish(xc.ovf, xc.ovf_host)
            return
        H, C, kw = xc.H, xc.C, xc.kw
        for p in range(self.G):
            a, cnt = int(off[p]), int(off[p + 1] - off[p])
            c = min(cnt, C)
            send[p * H] = c
            xc.ovf += cnt - c
            k = ukeys[a:a + c]
            k32 = k.to(torch.int32) if kw == 1 else k.contiguous().view(torch.int32)
            send[p * H + 4:p * H + 4 + c * kw] = k32

    def _x_pack_keys_flat(self, loc, gb: int, r: int):
        """Flat layout: every bucket's (rank-sorted) keys straight into its owner's row."""
        xc = self.xc
        xc.curs[r] = None
        hh = hipops()
        hh.tpf_pack_keys(loc.nnz, loc.bits, self.G, loc.cnt, loc.uniqf, xc.C, xc.kw, xc.H,
                         xc.sends[gb], xc.ovf)
        # (the overflow flag reaches the host through tpf_pack_grads' extra workgroup,
        # fixing-float or not)

    def _x_finish_flat(self, loc, labels, B: int, width: int, r: int, send=None, wsrc=None,
                       wstride: int = 0, csr=None):
        """Flat layout, worker half: the pulled weights into tile-entry order, the flat
        fused forward + tile backward, every key's gradient (per-bucket fixed-point sums)
        into its owner's row of the next exchange [+ FixingFloat codes], AUC epilogue.
        (merged exchange: weights read in place from the received rows ``wsrc`` with row
        stride ``wstride``, gradients into ``send``.)"""
        xc, hh = self.xc, hipops()
        n, bits, G = loc.nnz, loc.bits, self.G
        send = xc.sends[r] if send is None else send
        hh.tpf_unpack_w(n, bits, G, loc.cnt, loc.ent_pos, loc.ent_j, xc.C,
                        xc.wrecvs[r] if wsrc is None else wsrc, loc.w_ent, wstride)
        coef = self._coef(B)
        if csr is not None:  # (row_ptr, rows, vals): valued / variable-width rows
            hh.tp_fwd_bwd_csr(loc.rep, loc.dcnt, None, n, *csr, loc.w_ent, labels, B,
                              loss_id(self.cfg.loss), coef, self.metrics, self.hist, AUC_BINS,
                              loc.psum, None, None, None, None, False)
        else:
            hh.tp_fwd_bwd(loc.rep, loc.dcnt, None, n, width, None, loc.w_ent, labels, B,
                          loss_id(self.cfg.loss), coef, self.metrics, self.hist, AUC_BINS,
                          loc.psum, None, None, None, None, False)
        hh.tpf_pack_grads(n, bits, G, loc.cnt, loc.ent_pos, loc.ent_j, xc.C, xc.kw, xc.H,
                          loc.psum, send, xc.gstage if xc.nb else None, self.hist, self.metrics,
                          self.step_dev, xc.ovf, xc.ovf_host)
        if xc.nb:
            hh.xchg_ff_encode(xc.gstage, xc.C, xc.kw, xc.H, xc.nb, self._ff_seed, self.step_dev,
                              send,
                              per=hh.tpf_groups(n, bits) // G)  # (the pack's partials)

    def _x_poll_overflow(self):
        """Raise at the first step whose exchange dropped keys (the device counter is
        published into pinned host memory by the pack kernel: no stream sync; on the
        GPU the check sees a pack that has completed, at most the pipeline depth
        behind). Dropped keys would have been pulled as 0 and their pushes lost."""
        xc = self.xc
        ovf = int(xc.ovf_np[0]) if xc.ovf_np is not None else int(xc.ovf.item())
        if ovf:
            raise self._overflow_error("padded exchange", ovf, xc.C)

    def _x_grads(self, r: int):
        """Gradient source of the pushes received by exchange ``r``: (tensor, row stride)."""
        xc = self.xc
        if xc.nb:  # FixingFloat codes -> f32, one launch for all source rows
            self._x_ff_decode(r)
            return xc.gins[r], xc.C
        g0 = 4 + xc.C * xc.kw
        return xc.recvs[r].view(torch.float32)[g0:], xc.H

    def _x_apply(self, r: int, gb: int):
        """Owner: the pushes carried by exchange ``r`` (gradients of the pull step
        whose resolved slots are ``slots[gb]``), every source row in ONE launch pair
        with per-push semantics (source-rank order per key) or summed per key
        (``push_mode='aggregate'``)."""
        xc, G, H, C = self.xc, self.G, self.xc.H, self.xc.C
        pslot, recv = xc.slots[gb], xc.recvs[r]
        if self.gpu:
            hh = hipops()
            if xc.nb and self.cfg.push_mode != "aggregate" and xc.bnd is not None:
                # FixingFloat codes decoded inside the apply (no decode launch)
                hh.kv_apply_part(self.table.slots, pslot, xc.pkeys[gb], xc.gins[r], C, recv, H,
                                 C, xc.bnd[gb], xc.lgP, *self.rule.args(), self.stats,
                                 ff_nb=xc.nb, kw=xc.kw)
                return
            gsrc, gstride = self._x_grads(r)
            if self.cfg.push_mode == "aggregate":
                xc.n_touched.zero_()
                hh.kv_accumulate_rows(self.table.slots, pslot, gsrc, gstride, recv, H, C,
                                      xc.touched, xc.n_touched)
                hh.kv_apply_accumulated(self.table.slots, xc.touched, xc.n_touched,
                                        *self.rule.args(), self.stats)
            elif xc.bnd is not None:
                hh.kv_apply_part(self.table.slots, pslot, xc.pkeys[gb], gsrc, gstride, recv, H, C,
                                 xc.bnd[gb], xc.lgP, *self.rule.args(), self.stats)
            else:
                hh.kv_update_rows(self.table.slots, pslot, gsrc, gstride, recv, H, C, xc.link,
                                  xc.nxt, *self.rule.args(), self.stats)
            return
        rows = [recv[s * H:(s + 1) * H] for s in range(G)]
        if xc.nb:
            self._x_ff_decode(r)
            grads = [xc.gins[r][s * C:(s + 1) * C] for s in range(G)]
        else:
            g0 = 4 + C * xc.kw
            grads = [rows[s][g0:g0 + C].view(torch.float32) for s in range(G)]
        parts = []
        for s in range(G):
            ng = int(rows[s][1])
            if ng:
                parts.append((pslot[s * C:s * C + ng], grads[s][:ng]))
        self._apply_pushes(parts)

    def _x_resolve(self, r: int, rs: int | None = None, wout=None, wstride: int = 0):
        """Owner: lookup-or-insert the keys pulled by exchange ``r`` -> slots[rs] (default
        rs = r) and their weights -> ``wout`` (default wsend; row stride ``wstride``, 0 =
        C: the merged exchange writes them into the next send rows)."""
        xc, G, H, C, kw = self.xc, self.G, self.xc.H, self.xc.C, self.xc.kw
        recv = xc.recvs[r]
        rs = r if rs is None else rs
        wout = xc.wsend if wout is None else wout
        ws = wstride or C
        if self.gpu:
            hipops().kv_resolve_rows(self.table.slots, recv, H, C, kw, xc.slots[rs], wout,
                                     True, *self.table.resolve_args(),
                                     xc.pkeys[rs] if xc.bnd is not None else None,
                                     xc.bnd[rs] if xc.bnd is not None else None, max(xc.lgP, 0),
                                     wstride=ws)
            return
        for s in range(G):
            row = recv[s * H:(s + 1) * H]
            nk = int(row[0])
            if not nk:
                continue
            if kw == 1:
                req = row[4:4 + nk].to(torch.int64) & 0xFFFFFFFF
            else:
                req = row[4:4 + 2 * nk].contiguous().view(torch.int64)
            slot, w = self.table.resolve(req, insert=True)
            xc.slots[rs][s * C:s * C + nk] = slot
            wout[s * ws:s * ws + nk] = w

    def _x_finish(self, loc, labels, B, width, row_ptr, vals, rows, r: int, send=None,
                  wsrc=None, wstride: int = 0):
        xc = self.xc
        perm, off, n_uniq = xc.curs[r]
        wrecv = xc.wrecvs[r] if wsrc is None else wsrc
        send = xc.sends[r] if send is None else send  # grads(t) -> sends[t % R]
        ws = wstride or xc.C
        if self.gpu:
            w_local = xc.w_local[:loc.uniq.numel()]
            if self.filter is not None:
                w_local.zero_()  # filtered keys: w = 0
            hipops().xchg_unpack_w(wrecv, perm, n_uniq, off, xc.C, w_local, wstride=ws)
        else:
            w_local = torch.zeros(max(int(loc.n_uniq.reshape(-1)[0]), 1), dtype=torch.float32)
            for p in range(self.G):
                a, c = int(off[p]), min(int(off[p + 1] - off[p]), xc.C)
                dst = perm[a:a + c].long() if perm is not None else slice(a, a + c)
                w_local[dst] = wrecv[p * ws:p * ws + c]
        coef, grad = linear_fwd_bwd(loc, w_local, labels, B=B, width=width or 0, row_ptr=row_ptr,
                                    rows=rows, vals=vals, loss=self.cfg.loss, coef=self.coef[:B],
                                    metrics=self.metrics, hist=self.hist)
        H, C, kw = xc.H, xc.C, xc.kw
        if xc.nb:
            self._x_ff_pack(grad[:loc.uniq.numel()], perm, n_uniq, off, send)
        elif self.gpu:  # (+ the step's AUC epilogue in block 0: one launch less)
            hipops().xchg_pack_grads(grad[:loc.uniq.numel()], perm, n_uniq, off, C, kw, H, send,
                                     hist=self.hist, metrics=self.metrics,
                                     step_counter=self.step_dev, ovf=xc.ovf,
                                     ovf_host=xc.ovf_host)
            return
        else:
            for p in range(self.G):
                a, c = int(off[p]), min(int(off[p + 1] - off[p]), C)
                send[p * H + 1] = c
                g0 = p * H + 4 + C * kw
                g = grad[perm[a:a + c].long()] if perm is not None else grad[a:a + c]
                send[g0:g0 + c] = g.contiguous().view(torch.int32)
        auc_from_hist(self.hist, self.metrics, self.step_dev)

    def _x_ff_pack(self, grad, perm, n_uniq, off, send):
        """FixingFloat push (reference fixing_float.h:44-95): per owner row min/max,
        nb-byte stochastic-rounded codes; the device step clock varies the rounding
        bits across graph replays."""
        xc, H, C, kw, nb = self.xc, self.xc.H, self.xc.C, self.xc.kw, self.xc.nb
        seed = self._ff_seed
        if self.gpu:
            hipops().xchg_ff_pack_grads(grad, perm, n_uniq, off, C, kw, H, nb, seed,
                                        self.step_dev, send, xc.gstage)
            return
        for p in range(self.G):
            a, c = int(off[p]), min(int(off[p + 1] - off[p]), C)
            send[p * H + 1] = c
            g = grad[perm[a:a + c].long()] if perm is not None else grad[a:a + c]
            code, mm = ff.encode(g, nb, seed=seed + 1000003 * self.step_count + p)
            send[p * H + 2:p * H + 4] = mm.view(torch.int32)
            g0 = p * H + 4 + C * kw
            words = send[g0:g0 + (C * nb + 3) // 4].view(torch.uint8)
            words[:code.numel()] = code

    def _x_ff_decode(self, r: int):
        xc, H, C, kw, nb = self.xc, self.xc.H, self.xc.C, self.xc.kw, self.xc.nb
        recv, gin = xc.recvs[r], xc.gins[r]
        if self.gpu:
            hipops().xchg_ff_decode(recv, C, kw, H, nb, gin)
            return
        for s in range(self.G):
            row = recv[s * H:(s + 1) * H]
            n = int(row[1])
            if n:
                g0 = 4 + C * kw
                code = row[g0:g0 + (C * nb + 3) // 4].view(torch.uint8)[:n * nb]
                gin[s * C:s * C + n] = ff.decode(code, nb, row[2:4].view(torch.float32), n)

    def _x_flush(self):
        """Apply the gradients that no issued exchange has carried yet (keys-free
        exchanges, oldest first), so the shards hold every push issued so far.
        Collective."""
        if self.gpu:  # exchange halves / async applies may still run on other streams
            torch.cuda.synchronize(self.device)
        # exchange s carried grads(s - 1 - lag); steps computed whose grads no issued
        # exchange has carried yet, oldest first
        for s in self.sched.pending(self._xx, self._xt):
            b = self.sched.ring(s)
            self._x_keyless_exchange(b, b)
        if self.gpu:
            torch.cuda.synchronize(self.device)
        self._x_check_overflow()

    def _x_keyless_exchange(self, b: int, gb: int | None):
        """Ship the gradients waiting in send rows ``b`` without any keys; the owner
        applies them to the slots of pull step ``gb`` (None: nothing carried yet)."""
        send = self.xc.sends[b]
        self._x_clear(send, keys=True)
        self.comm.all_to_all_fixed(send, self.xc.recvs[b])
        if gb is not None:
            self._x_apply(b, gb)
        self._x_clear(send, grads=True)

    def _x_check_overflow(self):
        xc = self.xc
        if xc is None:
            return
        ovf = int(xc.ovf.item())
        if ovf:
            raise self._overflow_error("padded exchange", ovf, xc.C)
