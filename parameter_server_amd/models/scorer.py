"""Score a stored sparse linear model on data it was not trained on.

The GPU counterpart of the reference's ModelEvaluation
(src/app/linear_method/model_evaluation.h:9-74: load every ``key\\tweight`` file into a hash
map, Xw by lookup, AUC and accuracy). The model sits in a ``KVTable`` -- loaded from text
files (``from_text``) or a live trainer's own table (``from_table``, zero copy) -- and every
minibatch is one launch of the fused probe kernel (ops/score.py, csrc/hip/predict.hip).
Loss, correct and count sums and the AUC histogram accumulate over any number of
minibatches and ranks; ``result`` turns them into the figures.
"""
from __future__ import annotations

import torch

from ..ops.embedding import EmbeddingShard
from ..ops.keymix import mix
from ..ops.kv_table import KVTable, next_pow2
from ..ops.score import (ScoreAccum, auc_from_counts, ffm_score, fm_score, fwfm_score,
                         score)


class ModelScorer:
    def __init__(self, table: KVTable, bits: int, loss="logit"):
        self.table, self.bits, self.loss = table, int(bits), loss
        self.device = table.device
        self.acc = ScoreAccum(self.device)

    # ------------------------------------------------------------ constructors
    @classmethod
    def from_table(cls, table: KVTable, bits: int, loss="logit") -> "ModelScorer":
        """Alias an existing table (no copy); its ordered-home mapping is the table's own.
        The caller has flushed whatever writes to it (``SparseLRTrainer.scorer``)."""
        return cls(table, bits, loss)

    @classmethod
    def from_pairs(cls, keys_mixed: torch.Tensor, w: torch.Tensor, bits: int, device,
                   capacity: int | None = None, loss="logit") -> "ModelScorer":
        """A hashed-home table of the (mixed key, weight) pairs at load <= 0.5 (32 B per
        slot); an explicit ``capacity`` too small for them raises 'KVTable full'."""
        n = keys_mixed.numel()
        table = KVTable(capacity or next_pow2(max(64, 2 * n)), device)
        if n:
            table.load(keys_mixed, w)  # (check_ok inside: a full table raises)
        return cls(table, bits, loss)

    @classmethod
    def from_text(cls, pattern: str, bits: int, device, capacity: int | None = None,
                  loss="logit", text_io: str = "auto") -> "ModelScorer":
        """Every ``key\\tweight`` file matching ``pattern`` (regex or glob,
        utils/checkpoint.read_text_models). ``bits`` must be the key width the model was
        trained with (``key_bits_for(num_features)``). ``text_io``: "device" parses the
        text on the GPU (ops/modeltext.py; the same weights), "host" is the dict reader,
        "auto" the device path when ``device`` is a GPU. ``deferred_chunks`` counts the
        chunks of text the device parser left to the host rules."""
        from ..ops.modeltext import pairs_of, read_text_models_device
        from ..utils.checkpoint import read_text_models

        if text_io not in ("auto", "host", "device"):
            raise ValueError(f"from_text: text_io must be auto, host or device, not {text_io!r}")
        dev = torch.device(device)
        if text_io == "device" and dev.type != "cuda":
            raise ValueError("from_text: text_io='device' needs a GPU device")
        if text_io != "host" and dev.type == "cuda":
            raw, w, entries, deferred = read_text_models_device(pattern, dev)
            sc = cls.from_pairs(mix(raw, bits), w, bits, dev, capacity, loss)
            # a repeated key: the dict reader lets the later line win, scattered writes
            # promise no order, so the whole load goes through the dict reader
            if entries == 0 or sc.table.census()[0] == entries:
                sc.entries, sc.deferred_chunks = entries, deferred
                return sc
            del sc
        raw, w = pairs_of(read_text_models(pattern))
        sc = cls.from_pairs(mix(raw.to(dev), bits), w, bits, dev, capacity, loss)
        sc.entries, sc.deferred_chunks = raw.numel(), 0
        return sc

    # ------------------------------------------------------------ scoring
    def _score(self, keys, **kw):
        """The op behind every method below (``FMScorer`` puts its own here)."""
        return score(self.table, keys, self.bits, **kw)

    def predict(self, keys: torch.Tensor, *, row_ptr=None, width=None, vals=None,
                lanes: int = 0) -> torch.Tensor:
        """Margins only (nothing accumulated)."""
        return self._score(keys, row_ptr=row_ptr, width=width, vals=vals, lanes=lanes)

    def score(self, keys, labels, *, row_ptr=None, width=None, vals=None, margins=True,
              lanes: int = 0):
        """Margins of one labelled minibatch; its sums and bins go into the accumulator."""
        B = row_ptr.numel() - 1 if row_ptr is not None else keys.numel() // int(width)
        return self._score(keys, row_ptr=row_ptr, width=width, vals=vals, labels=labels,
                           margins=margins, acc=self.acc, loss=self.loss, B=B, lanes=lanes)

    def score_batch(self, b, margins: bool = False):
        """One ``DeviceBatch`` of a ``DeviceFeeder``."""
        keys = b.keys[:b.nnz]
        if b.row_ptr is not None:
            kw = dict(row_ptr=b.row_ptr[:b.rows + 1])
        else:
            kw = dict(width=b.width)
        return self._score(keys, vals=b.vals, labels=b.labels, margins=margins, acc=self.acc,
                           loss=self.loss, B=b.rows, **kw)

    def evaluate(self, feeder, pass_index: int = 0, predictions=None) -> "ModelScorer":
        """Drain one pass of a ``DeviceFeeder`` (each batch released behind its launch).
        ``predictions``: a ``PredictionWriter`` (ops/scoretext.py) that takes every batch's
        margins and labels, in the feeder's row order, before the batch is released; the
        sums and the histogram are the same with and without one."""
        if predictions is None:
            for b in feeder.iter_pass(pass_index):
                self.score_batch(b)
                feeder.release(b)
            return self
        for b in feeder.iter_pass(pass_index):
            m = self.score_batch(b, margins=True)
            predictions.append(m, b.labels, rows=b.rows)
            feeder.release(b)
        return self

    def totals(self, comm=None) -> tuple[torch.Tensor, torch.Tensor]:
        """(float64 [3] loss sum / correct / count, int64 [2 * AUC_BINS] histogram) on the
        host; with a ``comm`` of world > 1 summed over all ranks (collective)."""
        sums, counts = self.acc.sums(), self.acc.counts()
        if comm is not None and comm.world > 1 and getattr(comm, "backend", "") != "loopback":
            on = (lambda t: t.to(comm.device)) if getattr(comm, "backend", "") == "nccl" \
                else (lambda t: t.cpu())
            sums = comm.all_reduce_(on(sums))
            counts = comm.all_reduce_(on(counts))
        return sums.cpu(), counts.cpu()

    def result(self, comm=None) -> dict:
        """{"examples", "loss", "accuracy", "auc", "auc_tie_bound"} of everything scored so
        far; with a ``comm`` of world > 1 over all ranks (collective: the three sums and the
        histogram are sum-all-reduced). ``accuracy`` is correct / examples, not folded to
        max(acc, 1 - acc): ``evaluate_model``'s meaning (a margin of exactly 0 counts for the
        negative label here, ``(label > 0) == (m > 0)``, and for neither there). ``auc`` is
        the bucketed AUC over ``AUC_BINS`` bins of sigmoid(margin), within ``auc_tie_bound``
        of the exact one."""
        sums, counts = self.totals(comm)
        sums = sums.tolist()
        n = sums[2]
        auc, tie = auc_from_counts(counts)
        return {"examples": int(n), "loss": sums[0] / n if n else float("nan"),
                "accuracy": sums[1] / n if n else float("nan"), "auc": auc,
                "auc_tie_bound": tie}


class FMScorer(ModelScorer):
    """``ModelScorer`` for a factorization machine (models/fm.py): the model is an
    ``EmbeddingShard`` -- the KV table with the wide weights and the bf16 factor rows at the
    same slot index -- and every minibatch is one launch of the fused probe + factor kernel
    (ops/score.py ``fm_score``, csrc/hip/fm_predict.hip), for rows of any width and every
    ``embedding_dim`` the trainer accepts (multiples of 8 up to 128). ``predict``, ``score``,
    ``score_batch``, ``evaluate``, ``totals`` and ``result`` are ``ModelScorer``'s."""

    def __init__(self, shard: EmbeddingShard, bits: int, loss="logit"):
        super().__init__(shard.table, bits, loss)
        self.shard = shard

    @classmethod
    def from_shard(cls, shard: EmbeddingShard, bits: int, loss="logit") -> "FMScorer":
        """Alias an existing shard (no copy). The caller orders its own updates before the
        scoring launches (``FMTrainer.scorer``: the same stream)."""
        return cls(shard, bits, loss)

    @classmethod
    def from_state_dict(cls, sd: dict, device, capacity: int | None = None) -> "FMScorer":
        """A snapshot of ``FMTrainer.state_dict`` (or ``merge_state_dicts`` of the ranks'
        snapshots: the keys are raw ids, so any world size wrote it) in a shard of its own
        at load <= 0.5; key width and factor dimension come from the snapshot."""
        if str(sd.get("model")) != "FMTrainer":
            raise ValueError(f"snapshot of a {sd.get('model')}, not an FMTrainer")
        bits, dim = int(sd["bits"]), int(sd["dim"])
        n = sd["keys"].numel()
        shard = EmbeddingShard(capacity or next_pow2(max(64, 2 * n)), dim, device)
        if n:  # (check_ok inside: a capacity too small raises 'KVTable full')
            mk = mix(sd["keys"].cpu().contiguous(), bits)
            shard.load_state(mk, sd["w"], sd["z"], sd["n"], sd["rows"], sd["acc"],
                             cnt=sd.get("cnt"))
        return cls(shard, bits)

    def _score(self, keys, **kw):
        return fm_score(self.shard, keys, self.bits, **kw)


class FFMScorer(ModelScorer):
    """``ModelScorer`` for a field-aware factorization machine (models/ffm.py): the model is an
    ``EmbeddingShard`` whose rows hold ``num_fields`` vectors of ``k`` bf16, and every
    minibatch is one launch of the fused probe + field-sum kernel (ops/score.py ``ffm_score``,
    csrc/hip/ffm_predict.hip), for rows of any width and every geometry ``FFMConfig`` accepts.
    ``fields``: the position -> field map of fixed-width rows (None: identity), uploaded once.
    CSR rows bring ``fields=`` [nnz] int32, the field of every occurrence, with each call.
    ``evaluate``, ``totals`` and ``result`` are ``ModelScorer``'s."""

    def __init__(self, shard: EmbeddingShard, bits: int, num_fields: int, k: int, fields=None,
                 loss="logit"):
        super().__init__(shard.table, bits, loss)
        self.shard, self.F, self.k = shard, int(num_fields), int(k)
        if self.k not in (2, 4, 8) or self.F < 1 or self.F * self.k > shard.dim:
            raise ValueError(f"{self.F} fields of k = {self.k} (2, 4 or 8) do not fit rows of "
                             f"{shard.dim} columns")
        self.fields = None if fields is None else [int(f) for f in fields]
        if self.fields and not 0 <= min(self.fields) <= max(self.fields) < self.F:
            raise ValueError(f"every field must lie in [0, {self.F})")
        self._field_of = None if self.fields is None else \
            torch.tensor(self.fields, dtype=torch.int32, device=self.device)

    @classmethod
    def from_shard(cls, shard: EmbeddingShard, bits: int, num_fields: int, k: int, fields=None,
                   loss="logit") -> "FFMScorer":
        """Alias an existing shard (no copy). The caller orders its own updates before the
        scoring launches (``FFMTrainer.scorer``: the same stream)."""
        return cls(shard, bits, num_fields, k, fields, loss)

    @classmethod
    def from_state_dict(cls, sd: dict, device, num_fields: int, k: int,
                        capacity: int | None = None) -> "FFMScorer":
        """A snapshot of ``FFMTrainer.state_dict`` (or ``merge_state_dicts`` of the ranks'
        snapshots) in a shard of its own at load <= 0.5; key width and row width come from
        the snapshot, which does not record the fields: ``num_fields`` and ``k`` are the
        trainer's, and must fit the rows."""
        if str(sd.get("model")) != "FFMTrainer":
            raise ValueError(f"snapshot of a {sd.get('model')}, not an FFMTrainer")
        bits, dim = int(sd["bits"]), int(sd["dim"])
        if dim < int(num_fields) * int(k):
            raise ValueError(f"snapshot rows of {dim} columns hold no {num_fields} fields of "
                             f"k = {k}")
        n = sd["keys"].numel()
        shard = EmbeddingShard(capacity or next_pow2(max(64, 2 * n)), dim, device)
        if n:  # (check_ok inside: a capacity too small raises 'KVTable full')
            mk = mix(sd["keys"].cpu().contiguous(), bits)
            shard.load_state(mk, sd["w"], sd["z"], sd["n"], sd["rows"], sd["acc"],
                             cnt=sd.get("cnt"))
        return cls(shard, bits, num_fields, k)

    def _score(self, keys, fields=None, **kw):
        if kw.get("row_ptr") is None:
            if fields is not None:
                raise ValueError("fixed-width rows use the scorer's position -> field map; "
                                 "fields= is the field of every occurrence of CSR rows")
            fields = self._field_of
        return ffm_score(self.shard, keys, self.bits, num_fields=self.F, k=self.k, fields=fields,
                         **kw)

    def predict(self, keys: torch.Tensor, *, row_ptr=None, width=None, vals=None,
                fields=None) -> torch.Tensor:
        """Margins only (nothing accumulated)."""
        return self._score(keys, fields, row_ptr=row_ptr, width=width, vals=vals)

    def score(self, keys, labels, *, row_ptr=None, width=None, vals=None, fields=None,
              margins=True):
        """Margins of one labelled minibatch; its sums and bins go into the accumulator."""
        B = row_ptr.numel() - 1 if row_ptr is not None else keys.numel() // int(width)
        return self._score(keys, fields, row_ptr=row_ptr, width=width, vals=vals, labels=labels,
                           margins=margins, acc=self.acc, loss=self.loss, B=B)

    def score_batch(self, b, margins: bool = False):
        """One fixed-width ``DeviceBatch`` of a ``DeviceFeeder``, through the position map."""
        if b.row_ptr is not None:
            raise ValueError("FFMScorer.score_batch: a CSR DeviceBatch carries no field ids; "
                             "score CSR rows with score(keys, labels, row_ptr=, fields=)")
        return super().score_batch(b, margins)


class FwFMScorer(ModelScorer):
    """``ModelScorer`` for a field-weighted factorization machine (models/fwfm.py): the model
    is an ``EmbeddingShard`` with one vector of 8, 16 or 32 bf16 per key and ``R``, the float32
    [F, F] field-pair strengths, held by reference (a trainer's live R stays visible, nothing is
    copied per call). Every minibatch is one launch of the fused probe + Gram-tile kernel
    (ops/score.py ``fwfm_score``, csrc/hip/fwfm_predict.hip), for rows of any width.
    ``fields``: the position -> field map of fixed-width rows (None: identity), uploaded once.
    CSR rows bring ``fields=`` [nnz] int32, the field of every occurrence, with each call.
    ``evaluate``, ``totals`` and ``result`` are ``ModelScorer``'s."""

    def __init__(self, shard: EmbeddingShard, bits: int, num_fields: int, R: torch.Tensor,
                 fields=None, loss="logit"):
        super().__init__(shard.table, bits, loss)
        self.shard, self.F, self.R = shard, int(num_fields), R
        if not 1 <= self.F <= 64 or shard.dim not in (8, 16, 32):
            raise ValueError(f"{self.F} fields (1..64) on rows of {shard.dim} columns (8, 16 or "
                             "32) are outside the FwFM's geometry")
        if not isinstance(R, torch.Tensor) or R.dtype != torch.float32 or \
                tuple(R.shape) != (self.F, self.F) or R.device.type != self.device.type:
            raise ValueError(f"R must be a float32 [{self.F}, {self.F}] tensor on {self.device}")
        self.fields = None if fields is None else [int(f) for f in fields]
        if self.fields and not 0 <= min(self.fields) <= max(self.fields) < self.F:
            raise ValueError(f"every field must lie in [0, {self.F})")
        self._field_of = None if self.fields is None else \
            torch.tensor(self.fields, dtype=torch.int32, device=self.device)

    @classmethod
    def from_shard(cls, shard: EmbeddingShard, bits: int, num_fields: int, R: torch.Tensor,
                   fields=None, loss="logit") -> "FwFMScorer":
        """Alias an existing shard and R (no copy). The caller orders its own updates before
        the scoring launches (``FwFMTrainer.scorer``: the same stream)."""
        return cls(shard, bits, num_fields, R, fields, loss)

    @classmethod
    def from_state_dict(cls, sd: dict, device, fields=None,
                        capacity: int | None = None) -> "FwFMScorer":
        """A snapshot of ``FwFMTrainer.state_dict`` (or ``merge_state_dicts`` of the ranks'
        snapshots: R is replicated, the keys are raw ids) in a shard of its own at load <= 0.5;
        F and R come from ``sd["R"]``, key width and factor dimension from the snapshot, which
        does not record the position -> field map: ``fields`` is the trainer's."""
        if str(sd.get("model")) != "FwFMTrainer":
            raise ValueError(f"snapshot of a {sd.get('model')}, not an FwFMTrainer")
        bits, dim = int(sd["bits"]), int(sd["dim"])
        R = sd["R"].to(device=device, dtype=torch.float32).contiguous()
        n = sd["keys"].numel()
        shard = EmbeddingShard(capacity or next_pow2(max(64, 2 * n)), dim, device)
        if n:  # (check_ok inside: a capacity too small raises 'KVTable full')
            mk = mix(sd["keys"].cpu().contiguous(), bits)
            shard.load_state(mk, sd["w"], sd["z"], sd["n"], sd["rows"], sd["acc"],
                             cnt=sd.get("cnt"))
        return cls(shard, bits, R.shape[0], R, fields)

    def _score(self, keys, fields=None, **kw):
        if kw.get("row_ptr") is None:
            if fields is not None:
                raise ValueError("fixed-width rows use the scorer's position -> field map; "
                                 "fields= is the field of every occurrence of CSR rows")
            fields = self._field_of
        return fwfm_score(self.shard, keys, self.bits, num_fields=self.F, R=self.R,
                          fields=fields, **kw)

    def predict(self, keys: torch.Tensor, *, row_ptr=None, width=None, vals=None,
                fields=None) -> torch.Tensor:
        """Margins only (nothing accumulated)."""
        return self._score(keys, fields, row_ptr=row_ptr, width=width, vals=vals)

    def score(self, keys, labels, *, row_ptr=None, width=None, vals=None, fields=None,
              margins=True):
        """Margins of one labelled minibatch; its sums and bins go into the accumulator."""
        B = row_ptr.numel() - 1 if row_ptr is not None else keys.numel() // int(width)
        return self._score(keys, fields, row_ptr=row_ptr, width=width, vals=vals, labels=labels,
                           margins=margins, acc=self.acc, loss=self.loss, B=B)

    def score_batch(self, b, margins: bool = False):
        """One fixed-width ``DeviceBatch`` of a ``DeviceFeeder``, through the position map."""
        if b.row_ptr is not None:
            raise ValueError("FwFMScorer.score_batch: a CSR DeviceBatch carries no field ids; "
                             "score CSR rows with score(keys, labels, row_ptr=, fields=)")
        return super().score_batch(b, margins)
