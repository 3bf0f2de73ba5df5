"""The epoch-boundary controller of ``GATResTrainer.fit`` in plain Python: what the device kernel ``gatres_epoch_control``
(csrc/k_epoch.hip) computes, over Python floats (fp64) and ``numpy.float32`` -- the reference's ``internal_train`` after its
validation pass (train.py:426-511): best-loss bookkeeping, ``EarlyStopping(mode="min")`` and
``ReduceLROnPlateau(mode="min")`` with torch's defaults.  The tests hold it against torch's scheduler, against recorded
traces of the reference's ``EarlyStopping`` and against the kernel; a hand-written loop can drive ``set_lr`` with it.

Number formats: early stopping compares in fp32 (the reference hands it ``torch.tensor(val_loss)``, a float32 tensor, so
``best - min_delta`` is an fp32 subtraction of ``float32(min_delta)``); everything else is fp64.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np

STATE, RECORD = 10, 16               # GATRES_EPOCH_STATE, GATRES_EPOCH_RECORD of include/gatres.h
STATE_FIELDS = ("epoch", "best_loss", "best_epoch", "es_has_best", "es_best", "es_bad", "sched_best", "sched_bad",
                "improved", "stopped")                                               # GATRES_EPOCH_S_*
RECORD_FIELDS = ("epoch", "tr_loss", "val_loss", "lr_used", "lr_after", "improved", "best_loss", "best_epoch", "es_bad",
                 "stop", "sched_bad", "sched_best", "es_best", "val_graphs")        # GATRES_EPOCH_R_* ([14..15] are 0)


def weighted_mean(values: Sequence[float], graphs: Sequence[int]) -> float:
    """``sum_b v_b * g_b / n`` accumulated batch by batch in fp64: ``evaluation.metrics_from_moments``' arithmetic."""
    acc, n = 0.0, 0
    for v, g in zip(values, graphs):
        acc += float(v) * int(g)
        n += int(g)
    return acc / n if n else math.nan


class EpochController:
    def __init__(self, lr: float, *, patience: int = 100, min_delta: float = 1e-4, scheduler: bool = True,
                 scheduler_patience: int = 2, factor: float = 0.1, threshold: float = 1e-4, min_lr: float = 0.0,
                 eps: float = 1e-8):
        self.lr = float(lr)
        self.patience, self.min_delta = int(patience), float(min_delta)
        self.scheduler, self.scheduler_patience = bool(scheduler), int(scheduler_patience)
        self.factor, self.threshold, self.min_lr, self.eps = float(factor), float(threshold), float(min_lr), float(eps)
        self.epoch, self.best_loss, self.best_epoch = 0, math.inf, 0
        self.es_best: Optional[np.float32] = None
        self.es_bad = 0
        self.sched_best, self.sched_bad = math.inf, 0
        self.improved = self.stopped = False
        self.history = []

    def _early_stop(self, val_loss: float) -> bool:
        if self.patience == 0:
            return False
        m = np.float32(val_loss)
        if self.es_best is None:              # the first epoch only stores its metric
            self.es_best = m
            return False
        if np.isnan(m):
            return True
        if m < np.float32(self.es_best - np.float32(self.min_delta)):
            self.es_bad, self.es_best = 0, m
        else:
            self.es_bad += 1
        return self.es_bad >= self.patience

    def _schedule(self, val_loss: float) -> None:
        if val_loss < self.sched_best * (1.0 - self.threshold):
            self.sched_best, self.sched_bad = val_loss, 0
        else:
            self.sched_bad += 1
        if self.sched_bad > self.scheduler_patience:
            new_lr = max(self.lr * self.factor, self.min_lr)
            if self.lr - new_lr > self.eps:
                self.lr = new_lr
            self.sched_bad = 0

    def step(self, tr_loss: float, val_loss: float, val_graphs: float = 0.0) -> Dict[str, float]:
        """One epoch's decision; returns its history record (``RECORD_FIELDS``).  ``self.lr`` is the rate to train the next
        epoch with, ``self.stopped`` says whether there is one."""
        tr_loss, val_loss = float(tr_loss), float(val_loss)
        self.epoch += 1
        self.improved = val_loss < self.best_loss
        if self.improved:
            self.best_loss, self.best_epoch = val_loss, self.epoch
        lr_used = self.lr
        with np.errstate(all="ignore"):
            self.stopped = self._early_stop(val_loss)
        if not self.stopped and self.scheduler:
            self._schedule(val_loss)
        rec = dict(epoch=self.epoch, tr_loss=tr_loss, val_loss=val_loss, lr_used=lr_used, lr_after=self.lr,
                   improved=float(self.improved), best_loss=self.best_loss, best_epoch=self.best_epoch, es_bad=self.es_bad,
                   stop=float(self.stopped), sched_bad=self.sched_bad, sched_best=self.sched_best,
                   es_best=0.0 if self.es_best is None else float(self.es_best), val_graphs=float(val_graphs))
        self.history.append(rec)
        return rec

    @staticmethod
    def record_vector(rec: Dict[str, float]) -> np.ndarray:
        out = np.zeros(RECORD, dtype=np.float64)
        out[:len(RECORD_FIELDS)] = [float(rec[k]) for k in RECORD_FIELDS]
        return out

    def state_vector(self) -> np.ndarray:
        """The device controller's state after the same epochs (``STATE_FIELDS``)."""
        return np.array([self.epoch, self.best_loss, self.best_epoch, 0.0 if self.es_best is None else 1.0,
                         0.0 if self.es_best is None else float(self.es_best), self.es_bad, self.sched_best, self.sched_bad,
                         float(self.improved), float(self.stopped)], dtype=np.float64)
