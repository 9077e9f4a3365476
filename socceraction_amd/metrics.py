"""Model scores: the Brier score, log loss and AUROC the reference's notebook 3 ends with.

``public-notebooks/3-estimate-scoring-and-conceding-probabilities.ipynb`` evaluates each fitted
model with ``brier_score_loss``, ``log_loss`` and ``roc_auc_score`` and relates the first two to
the scores of the base-rate prediction.  :func:`binary_scores` computes all of them from one
label column and one probability column on the device (``ops.binary_metrics``) as functions of
the multiset of rows: Brier and log-loss terms are added as fixed-point integers and rounded
once, and the AUROC is the integer pair count ``U2`` over ``2 * n_pos * n_neg``, so the dict is
the same bit for bit from run to run and under any permutation of the rows.

Without a ROCm device the same definitions run in numpy (:func:`binary_scores_host`), so the
module can be used and tested on a CPU-only machine.  There the Brier score is bit-identical to
the device's; the log loss differs by the last bits of ``log``.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import _native, ops

KEYS = ('brier', 'log_loss', 'auroc', 'brier_baseline', 'log_loss_baseline', 'n', 'n_pos')


def _limb_sums(v: np.ndarray, scale_exp: int) -> Tuple[int, int, int]:
    """``sa_fx_quantize`` (csrc/sa_fixed.h) of every element of the non-negative float64 array
    ``v`` (each below ``2 ** scale_exp``) and the three limb sums, as Python integers."""
    v = np.ascontiguousarray(v, np.float64)
    if (v < 0).any():
        raise ValueError('score terms are non-negative')
    b = v.view(np.uint64) & np.uint64((1 << 63) - 1)  # -0.0 adds nothing
    e = (b >> np.uint64(52)).astype(np.int64)
    frac = b & np.uint64((1 << 52) - 1)
    if (e - 1022 > scale_exp).any():
        raise ValueError('a score term reaches 2 ** scale_exp')
    M = np.where(e > 0, frac | np.uint64(1 << 52), frac)
    sh = np.where(e > 0, e, 1) - 1075 + 95 - scale_exp  # Q = M * 2^sh truncated; sh <= 42
    left = np.clip(sh, 0, 63).astype(np.uint64)
    right = np.clip(-sh, 0, 63).astype(np.uint64)
    carry = np.clip(64 - sh, 1, 63).astype(np.uint64)  # sh in 1..42: the bits shifted out of `lo`
    lo = np.where(sh >= 0, M << left, np.where(sh > -64, M >> right, np.uint64(0)))
    hi = np.where(sh > 0, M >> carry, np.uint64(0))
    mask = np.uint64(0xFFFFFFFF)
    return (int((lo & mask).sum(dtype=np.uint64)), int((lo >> np.uint64(32)).sum(dtype=np.uint64)),
            int(hi.sum(dtype=np.uint64)))


def _host_columns(y, p) -> Tuple[np.ndarray, np.ndarray]:
    """uint8 labels (255 stands for a value that is neither 0 nor 1) and float32 / float64
    probabilities of array-likes."""
    y = np.asarray(y)
    p = np.asarray(p)
    if y.ndim != 1 or p.ndim != 1 or len(y) != len(p):
        raise ValueError('one label per probability, both 1-D')
    if y.dtype != np.bool_:
        ok = (y == 0) | (y == 1)
        y = np.where(ok, y, 0).astype(np.uint8) | np.where(ok, 0, 255).astype(np.uint8)
    else:
        y = y.astype(np.uint8)
    if p.dtype not in (np.float32, np.float64):
        p = p.astype(np.float64)
    return np.ascontiguousarray(y), np.ascontiguousarray(p)


def binary_scores_host(y, p) -> dict:
    """:func:`binary_scores` in numpy, by the definitions of ``sa_metric_sums`` /
    ``sa_auc_count``."""
    y, p = _host_columns(y, p)
    err = 0
    if np.isnan(p).any():
        err |= _native.SA_METRIC_ERR_NAN
    if (~np.isnan(p) & ~((p >= 0) & (p <= 1))).any():
        err |= _native.SA_METRIC_ERR_RANGE
    if (y > 1).any():
        err |= _native.SA_METRIC_ERR_LABEL
    ops.BinaryMetrics.raise_errors(err)
    n, pos = len(y), y == 1
    n_pos = int(pos.sum())
    if n == 0:
        raise ValueError('binary scores need at least one row')
    if n >= ops.GROUP_MAX_ROWS:
        raise ValueError('binary scores take fewer than 2**30 rows')
    if n_pos == 0 or n_pos == n:
        raise ValueError('Only one class present in y. The AUROC is not defined in that case.')
    eps = np.finfo(p.dtype).eps
    one = p.dtype.type(1)
    q = np.clip(np.where(pos, p, one - p), eps, one - eps)  # in p's dtype, as sklearn's log_loss
    d = p.astype(np.float64) - pos
    brier = _limb_sums(d * d, _native.SA_METRIC_BRIER_EXP)
    logl = _limb_sums(-np.log(q.astype(np.float64)), _native.SA_METRIC_LOGLOSS_EXP)
    # U2: every majority row against the sorted minority probabilities (+0.0 == -0.0 as floats)
    minority_pos = n_pos <= n - n_pos
    keys = np.sort(p[pos if minority_pos else ~pos])
    x = p[~pos if minority_pos else pos]
    lower = np.searchsorted(keys, x, 'left').astype(np.int64)
    upper = np.searchsorted(keys, x, 'right').astype(np.int64)
    twice = (len(keys) - upper) if minority_pos else lower
    u2 = int((2 * twice + (upper - lower)).sum(dtype=np.int64))
    return ops.scores_from_sums(n, n_pos, brier, logl, u2)


def binary_scores(y, p) -> dict:
    """``{'brier', 'log_loss', 'auroc', 'brier_baseline', 'log_loss_baseline', 'n', 'n_pos'}``
    of the 0 / 1 labels ``y`` against the probabilities ``p`` of the positive class, equal to
    ``brier_score_loss``, ``log_loss`` and ``roc_auc_score`` of scikit-learn up to rounding
    (float32 probabilities: of the widened column, the log-loss clip taken in float32).  The
    baselines are the Brier score and log loss of the constant prediction ``n_pos / n``.

    ``y`` and ``p`` are device tensors (uint8 / bool and float32 / float64), or numpy arrays /
    pandas Series, which are uploaded when a ROCm device is present and scored in numpy
    otherwise.  ValueError, as scikit-learn raises it: a NaN probability, a probability outside
    [0, 1], a label other than 0 / 1, a single class present (the AUROC is undefined), no rows.
    """
    if isinstance(y, torch.Tensor) and isinstance(p, torch.Tensor) and p.is_cuda:
        yd, pd_ = y, p
    elif not torch.cuda.is_available():
        if isinstance(y, torch.Tensor):
            y = y.cpu().numpy()
        if isinstance(p, torch.Tensor):
            p = p.cpu().numpy()
        return binary_scores_host(y, p)
    else:
        from .batch import device
        dev = device()
        yh, ph = _host_columns(y.cpu().numpy() if isinstance(y, torch.Tensor) else y,
                               p.cpu().numpy() if isinstance(p, torch.Tensor) else p)
        yd, pd_ = torch.from_numpy(yh).to(dev), torch.from_numpy(ph).to(dev)
    if yd.numel() == 0:
        raise ValueError('binary scores need at least one row')
    res = ops.binary_metrics(yd, pd_).finalize()
    if res['auroc'] is None:
        raise ValueError('Only one class present in y. The AUROC is not defined in that case.')
    return res
