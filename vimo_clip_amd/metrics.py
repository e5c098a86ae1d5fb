"""Micro-averaged multilabel average precision with torchmetrics' semantics (K16, a14).

Mirrors ``MultilabelAveragePrecision(num_labels=C, average="micro")`` as used by
TFAM/train_and_eval.py:49,87,94,122-124: ``update(preds, target)`` applies a sigmoid to that batch iff any
value lies outside [0, 1]; ``compute()`` flattens everything over labels and integrates the distinct-threshold
precision-recall curve, AP = sum_k (R_k - R_{k-1}) P_k.  Scores are kept on the device they arrive on and
sorted there (torch.sort -> rocPRIM radix sort, a library primitive); under data
parallelism the per-rank score/target rows are all-gathered first (parallel.all_gather_rows).

``DeviceMetricLog`` keeps what the two metric classes and the running loss need in device buffers that a kernel appends to
(vmc_metric_append, include/vmc.h K18): the training loops then log inside the captured step and read once per epoch.
"""
from __future__ import annotations

import ctypes
import warnings

import torch

from . import parallel


class MultilabelAveragePrecision:
    def __init__(self, num_labels: int, average: str = "micro"):
        if average != "micro":
            raise NotImplementedError("only average='micro' is used by the reference path")
        self.num_labels = num_labels
        self.reset()

    def to(self, device):
        return self

    def reset(self):
        self._scores, self._targets = [], []

    def update(self, preds: torch.Tensor, target: torch.Tensor):
        p = preds.detach().float()
        if bool(((p < 0) | (p > 1)).any()):
            p = torch.sigmoid(p)
        self._scores.append(p.reshape(-1, self.num_labels))
        self._targets.append(target.detach().reshape(-1, self.num_labels).to(torch.int64))

    def compute(self, distributed: bool = False) -> torch.Tensor:
        if not self._scores:
            return torch.tensor(float("nan"))
        s = torch.cat(self._scores, dim=0)
        y = torch.cat(self._targets, dim=0)
        if distributed:
            s, y = parallel.all_gather_rows(s), parallel.all_gather_rows(y)
        return micro_average_precision(s, y)

    __call__ = update


class Accuracy:
    """Top-1 accuracy for the single-label MammalNet variants (TFAM/train_and_eval_frame_diff_MN.py:49,87,94:
    ``Accuracy(num_classes=C)``; ``update(logits [N,C], labels.int() [N,C])``).  The reference hands the metric one-hot
    integer rows; torchmetrics is not installed here and its legacy ``Accuracy(num_classes=...)`` call form no longer
    exists in the version SURVEY.md pins (1.7.1 requires ``task=``), so the intended statistic — fraction of rows whose
    arg-max logit is the labelled class — is what is computed ("parity unpinned")."""

    def __init__(self, num_classes: int, **unused):
        self.num_classes = num_classes
        self.reset()

    def to(self, device):
        return self

    def reset(self):
        self._correct = self._total = None

    def update(self, preds: torch.Tensor, target: torch.Tensor):
        p = preds.detach().reshape(-1, self.num_classes).argmax(dim=1)
        t = target.detach()
        t = t.reshape(-1, self.num_classes).argmax(dim=1) if t.dim() >= 2 or t.numel() != p.numel() else t.reshape(-1).to(torch.int64)
        c = (p == t).sum().to(torch.float64).reshape(1)
        n = torch.tensor([float(p.numel())], dtype=torch.float64, device=c.device)
        self._correct = c if self._correct is None else self._correct + c
        self._total = n if self._total is None else self._total + n

    def compute(self, distributed: bool = False) -> torch.Tensor:
        if self._total is None:
            return torch.tensor(float("nan"))
        c, n = self._correct, self._total
        if distributed:
            c, n = parallel.all_gather_rows(c.reshape(1, 1)).sum().reshape(1), parallel.all_gather_rows(n.reshape(1, 1)).sum().reshape(1)
        return (c / n).to(torch.float32).reshape(())

    __call__ = update


def micro_average_precision(scores: torch.Tensor, targets: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """scores in [0,1] [N,C], targets {0,1} [N,C] -> scalar AP (float64 accumulation, returned as ``out_dtype``)."""
    s = scores.reshape(-1)
    y = targets.reshape(-1).to(torch.float64)
    s, order = torch.sort(s, descending=True, stable=True)
    y = y[order]
    tp = torch.cumsum(y, 0)
    fp = torch.cumsum(1.0 - y, 0)
    last = torch.ones_like(s, dtype=torch.bool)
    last[:-1] = s[1:] != s[:-1]                      # last element of every run of equal scores
    tp, fp = tp[last], fp[last]
    npos = y.sum()
    precision = tp / (tp + fp)
    recall = tp / npos
    prev = torch.cat([torch.zeros(1, dtype=recall.dtype, device=recall.device), recall[:-1]])
    return ((recall - prev) * precision).sum().to(out_dtype)


def log_scores(values: torch.Tensor, squash: torch.Tensor) -> torch.Tensor:
    """The scores MultilabelAveragePrecision.update would have kept: the sigmoid of the rows whose update call had a value outside
    [0, 1] (``squash`` non-zero), the other rows as they are."""
    return torch.where(squash.reshape(-1, 1) != 0, torch.sigmoid(values), values)


def evaluate_log(values: torch.Tensor, targets: torch.Tensor, squash: torch.Tensor, task: str, out_dtype=torch.float32) -> torch.Tensor:
    """The epoch metric from logged rows, with the arithmetic of the classes above; a pure function of its arguments (any device).
    values [N, C] fp32 as handed to the updates, targets [N, C] integer labels, squash [N] non-zero where the row's update call
    had a value outside [0, 1].  "multilabel": sigmoid of the squashed rows, the others as they are, then
    micro_average_precision (MultilabelAveragePrecision); "singlelabel": fraction of rows whose arg-max value is the arg-max
    label (Accuracy).  N = 0: NaN, as the classes.  The arithmetic is float64 and the result is rounded to ``out_dtype``."""
    if task not in ("multilabel", "singlelabel"):
        raise ValueError(f"Unsupported task '{task}'. Choose 'multilabel' or 'singlelabel'.")
    if values.shape[0] == 0:
        return torch.full((), float("nan"), dtype=out_dtype, device=values.device)
    if task == "multilabel":
        return micro_average_precision(log_scores(values, squash), targets.to(torch.int64), out_dtype=out_dtype)
    c = (values.argmax(dim=1) == targets.argmax(dim=1)).sum().to(torch.float64)
    return (c / float(values.shape[0])).to(out_dtype).reshape(())


class MetricLogStruct(ctypes.Structure):
    """ctypes mirror of ``vmc_metric_log`` (include/vmc.h): same fields in the same order."""
    _fields_ = [("values", ctypes.c_void_p), ("targets", ctypes.c_void_p), ("squash", ctypes.c_void_p), ("state", ctypes.c_void_p),
                ("loss_sum", ctypes.c_void_p), ("capacity", ctypes.c_int), ("C", ctypes.c_int)]


class DeviceMetricLog:
    """Epoch log in device memory: ``values`` [capacity, C] fp32, ``targets`` [capacity, C] uint8, ``squash`` [capacity] uint8,
    ``state`` [4] int32 (rows, steps, status, reserved) and ``loss_sum`` [1] fp32.  ``append`` only enqueues one kernel on the current
    stream (safe inside a captured step); ``read`` is the one call that synchronises.  ``capacity`` is the number of rows the caller
    will append between two ``reset`` calls: an append that does not fit is refused on the device (status bit 1) and ``read``
    raises.  ``state`` and ``loss_sum`` share one allocation, so ``read`` is one copy."""

    FULL, BAD_LABEL = 1, 2

    def __init__(self, capacity: int, num_labels: int, task: str = "multilabel", device="cuda"):
        if capacity < 1 or num_labels < 1:
            raise ValueError("DeviceMetricLog: capacity and num_labels must be positive")
        if task not in ("multilabel", "singlelabel"):
            raise ValueError(f"Unsupported task '{task}'. Choose 'multilabel' or 'singlelabel'.")
        self.capacity, self.num_labels, self.task, self.device = int(capacity), int(num_labels), task, torch.device(device)
        self.values = torch.zeros(self.capacity, self.num_labels, dtype=torch.float32, device=self.device)
        self.targets = torch.zeros(self.capacity, self.num_labels, dtype=torch.uint8, device=self.device)
        self.squash = torch.zeros(self.capacity, dtype=torch.uint8, device=self.device)
        self._small = torch.zeros(8, dtype=torch.int32, device=self.device)
        self.state, self.loss_sum = self._small[:4], self._small[4:5].view(torch.float32)
        self._struct = None

    def _c_log(self):
        if self._struct is None:
            from . import _lib
            self._struct = MetricLogStruct(_lib.ptr(self.values), _lib.ptr(self.targets), _lib.ptr(self.squash), _lib.ptr(self.state),
                                           _lib.ptr(self.loss_sum), self.capacity, self.num_labels)
        return ctypes.addressof(self._struct)

    def append(self, logits: torch.Tensor, labels: torch.Tensor, loss: torch.Tensor | None = None):
        """Log one update call: ``logits`` [B, C] (or probabilities), ``labels`` [B, C], ``loss`` a one-element device tensor that is
        added to ``loss_sum``.  Enqueue only."""
        from . import _lib
        x = logits.detach().reshape(-1, self.num_labels).contiguous().float()
        y = labels.detach().reshape(-1, self.num_labels).contiguous().float()
        if x.shape != y.shape:
            raise ValueError(f"DeviceMetricLog.append: labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}")
        if loss is not None:
            loss = loss.detach().float()
            if loss.numel() != 1:
                raise ValueError("DeviceMetricLog.append: loss must have one element")
        _lib.check(_lib.lib.vmc_metric_append(self._c_log(), _lib.ptr(x), _lib.ptr(y), _lib.ptr(loss), int(x.shape[0]), _lib.stream()),
                   "metric_append")

    def reset(self):
        self._small.zero_()

    def state_tensors(self):
        """What a capture's warm-up run must leave as it found it (graphs.GraphedTrainStep(extra_live=...)): the cursor, the
        counters, the status word and the loss sum.  Rows behind the cursor are overwritten by the next append."""
        return (self._small,)

    def read(self):
        """(rows, steps, status, loss_sum) -- synchronises: once per epoch, or whenever a running figure is wanted.  Raises when an
        append was refused (status bit 1: the capacity arithmetic of the caller is wrong); warns on a label outside {0, 1}."""
        h = self._small.cpu()
        rows, steps, status = (int(v) for v in h[:3])
        loss_sum = float(h[4:5].view(torch.float32))
        if status & self.FULL:
            raise RuntimeError(f"DeviceMetricLog: an append was refused, the log holds {rows} of {self.capacity} rows after {steps} calls: "
                               "capacity is smaller than the rows appended between two resets")
        if status & self.BAD_LABEL:
            warnings.warn("DeviceMetricLog: a label outside {0, 1} was logged (stored truncated, clamped into 0..255)", RuntimeWarning)
        return rows, steps, status, loss_sum

    def compute(self, distributed: bool = False, rows: int | None = None) -> torch.Tensor:
        """The metric of the logged rows (``evaluate_log``); ``rows``: the count a ``read()`` just returned, otherwise read here.
        Under data parallelism every rank's rows, targets and flags are all-gathered first, in rank order."""
        if rows is None:
            rows = self.read()[0]
        v, t, s = self.values[:rows], self.targets[:rows], self.squash[:rows]
        if distributed:
            v, t, s = parallel.all_gather_rows(v), parallel.all_gather_rows(t), parallel.all_gather_rows(s)
        return evaluate_log(v, t, s, self.task)
