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

from ..ops.keymix import mix
from ..ops.kv_table import KVTable, next_pow2
from ..ops.score import ScoreAccum, auc_from_counts, score


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
    def predict(self, keys: torch.Tensor, *, row_ptr=None, width=None, vals=None,
                lanes: int = 0) -> torch.Tensor:
        """Margins only (nothing accumulated)."""
        return score(self.table, keys, self.bits, row_ptr=row_ptr, width=width, vals=vals,
                     lanes=lanes)

    def score(self, keys, labels, *, row_ptr=None, width=None, vals=None, margins=True,
              lanes: int = 0):
        """Margins of one labelled minibatch; its sums and bins go into the accumulator."""
        B = row_ptr.numel() - 1 if row_ptr is not None else keys.numel() // int(width)
        return score(self.table, keys, self.bits, row_ptr=row_ptr, width=width, vals=vals,
                     labels=labels, margins=margins, acc=self.acc, loss=self.loss, B=B,
                     lanes=lanes)

    def score_batch(self, b, margins: bool = False):
        """One ``DeviceBatch`` of a ``DeviceFeeder``."""
        keys = b.keys[:b.nnz]
        if b.row_ptr is not None:
            kw = dict(row_ptr=b.row_ptr[:b.rows + 1])
        else:
            kw = dict(width=b.width)
        return score(self.table, keys, self.bits, vals=b.vals, labels=b.labels, margins=margins,
                     acc=self.acc, loss=self.loss, B=b.rows, **kw)

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
