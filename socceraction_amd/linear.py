"""Logistic regression on the device: an exact, reproducible Newton fit.

The expected-goals notebook's first model is ``LogisticRegression().fit(X, y)``.  Its objective,
``sum(loss) + ||w||^2 / (2 C)`` with an unpenalised intercept, is strictly convex: it has one
minimiser, and Newton's method reaches it in a few steps whatever the features' scale.  Here one
``sa_logit_moments`` launch per iterate turns the coefficient vector and the feature blocks into
the gradient, the Hessian and the loss as fixed-point limb sums (``csrc/sa_fixed.h``) added as
integers; the host rounds every total to float64 once, adds the penalty and solves the
``(d + 1) x (d + 1)`` system in float64.  Every decision of the loop -- the step, the Armijo test,
the stop -- hangs on those integer sums, so a fit is the same bit for bit from run to run, for
any row order and for any launch grid.  ``sa_logit_predict`` is the predictor.

What is exact: the sums over the rows (no rounding depends on their order) and, at ``beta = 0``,
every term.  What is not: a row's ``exp`` / ``log1p`` are the device library's, a few ulp from
another library's, so the sums match a host evaluation to about 1e-15 relative, not bit for bit.
"""
from __future__ import annotations

import ctypes
import math
import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .catalog import FeaturePlan

KIND_CODE = {'b': 0, 'f': 1, 'i': 2}
# Measurement hook (scripts/logit_time.py): a list that receives one (start, end) pair of timing
# events around every native sa_logit_moments call -- its two memsets and two kernels, nothing else.
LAUNCH_EVENTS: Optional[list] = None
ARMIJO = 1e-4        # sufficient-decrease constant of the step halving
MIN_STEP = 2.0 ** -30


def n_items(d: int) -> int:
    """Sums of one ``sa_logit_moments`` launch over ``d`` columns: the triangle of the ``D = d + 1``
    design columns, the ``D`` gradient terms and the loss."""
    D = d + 1
    return D * (D + 1) // 2 + D + 1


def item_grid(d: int) -> Tuple[int, int]:
    """``(blocks of rows, blocks of columns)`` of the item table of ``d`` columns: its ``D + 2`` rows
    in blocks of ``SA_LOGIT_BLOCK_J``, its ``D`` columns in blocks of ``SA_LOGIT_BLOCK_K``."""
    D = d + 1
    return -(-(D + 2) // _native.SA_LOGIT_BLOCK_J), -(-D // _native.SA_LOGIT_BLOCK_K)


def item_splits(d: int) -> int:
    """Workgroups along the launch's second grid dimension: one per block of the item table."""
    jb, kb = item_grid(d)
    return jb * kb


def item_exps(col_exp: Sequence[int], loss_exp: int) -> List[int]:
    """The scale exponent of every item, in item order."""
    D = len(col_exp)
    out = [col_exp[j] + col_exp[k] - 2 for j in range(D) for k in range(j, D)]
    return out + [int(e) for e in col_exp] + [int(loss_exp)]


def limb_total(l0: int, l1: int, l2: int) -> int:
    return int(l0) + (int(l1) << 32) + (int(l2) << 64)


def fixed_value(total: int, scale_exp: int) -> float:
    """``total * 2^(scale_exp - 95)`` rounded once to the nearest double (``sa_fx_finalize``)."""
    sh = 95 - scale_exp
    return total / (1 << sh) if sh >= 0 else float(total << -sh)


def loss_exponent(beta: np.ndarray, col_exp: Sequence[int]) -> int:
    """A scale exponent for the loss terms: a row's loss is at most ``|z| + log 2``, and ``|z| <=
    sum |beta_j| 2^E_j + |b|``."""
    bound = float(sum(abs(float(b)) * 2.0 ** e for b, e in zip(beta[:-1], col_exp[:-1])) + abs(float(beta[-1])) + 1.0)
    if not math.isfinite(bound):
        raise ValueError('logistic regression: the coefficients overflow')
    return min(900, max(1, math.frexp(bound)[1]))


def model_slots(blocks, columns: Optional[Sequence[str]] = None) -> Tuple[List[str], List[Tuple[str, int]]]:
    """``(names, [(kind, column)])`` of the model's columns in model order (default: every feature
    of the blocks' plan).  An unknown or repeated name, more than ``SA_LOGIT_MAX_COLS`` columns or
    a bool column of blocks that are not in bitmap form is a ``ValueError``; no device work."""
    from .boost import plan_columns
    order = list(blocks.plan.order)
    if columns is not None:
        order = [order[j] for j in plan_columns(blocks.plan, columns)]
    if len(order) > _native.SA_LOGIT_MAX_COLS:
        raise ValueError(f'logistic regression takes at most {_native.SA_LOGIT_MAX_COLS} columns: got {len(order)}')
    if any(kind == 'b' for _, kind, _ in order) and blocks.bool_bits is None:
        raise ValueError('the bool features must come as bitmaps (ops.features(..., bool_bits=True))')
    return [name for name, _, _ in order], [(kind, col) for _, kind, col in order]


def column_exps(blocks, kc: Sequence[Tuple[str, int]], mask: Optional[torch.Tensor] = None) -> List[int]:
    """Scale exponents of the ``d + 1`` design columns: ``|x_j| < 2^E_j`` over the rows of the mask
    (non-finite values aside: the kernel flags those).  A per-column abs-max in torch (one
    ``amax`` per numeric block, one read back); a bool column and the intercept column have 1."""
    exps = {}
    for kind in 'fi':
        cols = sorted({c for k, c in kc if k == kind})
        if not cols:
            continue
        if blocks.n == 0:
            exps.update({(kind, c): 0 for c in cols})
            continue
        t = blocks._blk(kind)[:, cols, :]  # the model's columns of every tile, before any copy of rows
        a = t.permute(1, 0, 2).reshape(len(cols), -1)[:, :blocks.n].to(torch.float64).abs()
        a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
        if mask is not None:
            a = torch.where(mask.bool().unsqueeze(0), a, torch.zeros_like(a))
        for c, e in zip(cols, torch.frexp(a.amax(dim=1))[1].tolist()):
            exps[(kind, c)] = min(_native.SA_LOGIT_EXP_MAX, max(_native.SA_LOGIT_EXP_MIN, int(e)))
    return [1 if k == 'b' else exps[(k, c)] for k, c in kc] + [1]


def _descriptors(blocks, kc):
    fb, ib = blocks.sa_blocks()[-2:]
    bits = blocks.bool_bits
    slots = (ctypes.c_int32 * max(len(kc), 1))(*[(KIND_CODE[k] << 24) | c for k, c in kc])
    return (ctypes.byref(fb), ctypes.byref(ib), int(blocks.num32), None if bits is None else bits.data_ptr(),
            0 if bits is None else bits.shape[1], blocks.plan.n_bool if bits is not None else 0, slots, len(kc)), (fb, ib)


def moments_limbs(blocks, kc, beta, y: torch.Tensor, mask: Optional[torch.Tensor], col_exp: Sequence[int],
                  loss_exp: int, grid_x: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``sa_logit_moments`` launch: ``(limbs [T, 3] int64, err [1] int32)`` on the device.
    ``beta``: ``d + 1`` float64 values (host), the intercept last.  ``grid_x``: the workgroups
    along the rows (0: the library's choice); the limbs do not depend on it."""
    from .batch import stream_handle
    dev = blocks.device
    d = len(kc)
    if len(beta) != d + 1 or len(col_exp) != d + 1:
        raise ValueError('beta and col_exp hold one value per column and one for the intercept')
    if y.dtype != torch.uint8 or y.numel() < blocks.n or not y.is_contiguous():
        raise ValueError('y must be a contiguous uint8 device column of one label per row')
    if mask is not None and (mask.dtype != torch.uint8 or mask.numel() < blocks.n or not mask.is_contiguous()):
        raise ValueError('the row mask must be a contiguous uint8 device column of one byte per row')
    bdev = torch.from_numpy(np.ascontiguousarray(beta, np.float64)).to(dev)
    limbs = torch.empty((n_items(d), 3), dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    rowbuf = torch.empty(4 * max(blocks.n, 1), dtype=torch.float64, device=dev)  # the kernels' scratch
    args, keep = _descriptors(blocks, kc)
    exps = (ctypes.c_int32 * (d + 1))(*[int(e) for e in col_exp])
    events = None
    if LAUNCH_EVENTS is not None:
        events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        events[0].record()
    _native.check(_native.lib().sa_logit_moments(
        *args, bdev.data_ptr(), exps, int(loss_exp), y.data_ptr() if y.numel() else None,
        None if mask is None else mask.data_ptr(), blocks.n, int(grid_x), rowbuf.data_ptr(), limbs.data_ptr(),
        err.data_ptr(), stream_handle()))
    if events is not None:
        events[1].record()
        LAUNCH_EVENTS.append(events)
    del keep
    return limbs, err


def raise_errors(err: int) -> None:
    if err & (_native.SA_LOGIT_ERR_NAN | _native.SA_LOGIT_ERR_NONFINITE):
        raise ValueError('Input X contains NaN or infinity.')
    if err & _native.SA_LOGIT_ERR_RANGE:
        raise ValueError('logistic regression: a term is beyond its scale exponent (a feature is too large)')


def finalize(limbs: np.ndarray, col_exp: Sequence[int], loss_exp: int):
    """``(gradient [D], Hessian [D, D], loss)`` in float64 from the host copy of the limbs: every
    total rounded once."""
    D = len(col_exp)
    vals = [fixed_value(limb_total(*row), e) for row, e in zip(limbs.tolist(), item_exps(col_exp, loss_exp))]
    H = np.zeros((D, D))
    iu = np.triu_indices(D)
    H[iu] = vals[:len(iu[0])]
    H = H + np.triu(H, 1).T
    g = np.array(vals[len(iu[0]):len(iu[0]) + D])
    return g, H, vals[-1]


def host_blocks(X, device=None, names: Optional[Sequence[str]] = None):
    """A host frame or 2-D array as bitmap-form feature blocks, uploaded the way ``boost.bin_host``
    does it: bool columns as bitmaps, float and integer columns as one-tile float64 / int64 blocks.
    ``names``: the columns a frame must provide, in that order (an array is taken by position)."""
    from . import boost, ops
    have, cols = boost._host_columns(X)
    if names is not None and hasattr(X, 'columns'):
        missing = [c for c in names if c not in have]
        if missing:
            raise ValueError(f'{" and ".join(missing)} are not available in the features')
        cols = [cols[have.index(c)] for c in names]
        have = list(names)
    n = len(cols[0]) if cols else (len(X) if hasattr(X, '__len__') else 0)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    order, per = [], {'b': [], 'f': [], 'i': []}
    for name, c in zip(have, cols):
        k = boost._kind(c)
        order.append((name, k, len(per[k])))
        per[k].append(c)
    ld, words = ops._ld(n), max(1, (n + 63) // 64)
    hb = np.zeros((max(len(per['b']), 1), words * 8), np.uint8)
    for r, c in enumerate(per['b']):
        pk = np.packbits(c.astype(bool), bitorder='little')
        hb[r, :len(pk)] = pk
    hf = boost._padded_block(per['f'], n, ld, np.float64)
    hi = boost._padded_block(per['i'], n, ld, np.int64)
    plan = FeaturePlan((), 1, False, len(per['b']), len(per['f']), len(per['i']), order, None)
    return ops.FeatureBlocks(plan, n, 1024, ld, None, torch.from_numpy(hf).to(dev), torch.from_numpy(hi).to(dev),
                             torch.from_numpy(hb.view(np.int64)).to(dev))


def check_params(C, tol, max_iter) -> None:
    if not (isinstance(C, (int, float)) and C > 0):
        raise ValueError(f'C must be positive: got {C!r}')
    if not tol > 0:
        raise ValueError(f'tol must be positive: got {tol!r}')
    if int(max_iter) < 1:
        raise ValueError(f'max_iter must be at least 1: got {max_iter!r}')


def newton(evaluate, D: int, lam: np.ndarray, tol: float, max_iter: int):
    """Newton's method with step halving from ``beta = 0`` on ``sum(loss) + 0.5 sum(lam beta^2)``.
    ``evaluate(beta) -> (gradient, Hessian, loss)`` of the unpenalised sums.  A step is taken at the
    first ``t = 1, 1/2, ...`` with ``f(beta - t s) <= f(beta) - 1e-4 t g.s`` (Armijo), or -- once the
    loss no longer resolves the decrease -- with a change of the loss within its rounding and a
    smaller gradient.  Stops at ``max|g| <= tol max(1, max|g(0)|)``.
    Returns ``(beta, iterations, converged)``."""
    def full(b):
        g, H, f = evaluate(b)
        return g + lam * b, H + np.diag(lam), f + 0.5 * float(np.sum(lam * b * b))

    beta = np.zeros(D)
    g, H, f = full(beta)
    g0 = float(np.abs(g).max())
    for it in range(max_iter):
        if float(np.abs(g).max()) <= tol * max(1.0, g0):
            return beta, it, True
        step = np.linalg.solve(H, g)
        dec = float(g @ step)
        t = 1.0
        while True:
            cand = beta - t * step
            g2, H2, f2 = full(cand)
            if f2 <= f - ARMIJO * t * dec:
                break
            if abs(f2 - f) <= 16 * np.finfo(float).eps * abs(f) and np.abs(g2).max() < np.abs(g).max():
                break
            t *= 0.5
            if t < MIN_STEP:
                return beta, it, False
        beta, g, H, f = cand, g2, H2, f2
    return beta, max_iter, bool(np.abs(g).max() <= tol * max(1.0, g0))


class DeviceLogisticRegression:
    """sklearn's ``LogisticRegression`` objective for two classes (``C sum(loss) + ||w||^2 / 2``,
    the intercept unpenalised), fitted to its optimum by Newton's method on device sums.

    Parameters
    ----------
    C : float, default=1.0
        Inverse regularisation strength.
    fit_intercept : bool, default=True
    tol : float, default=1e-10
        Stop at ``max|gradient| <= tol * max(1, max|gradient at 0|)``.
    max_iter : int, default=100
        Newton iterations; reaching it raises sklearn's ``ConvergenceWarning``.
    """

    def __init__(self, C: float = 1.0, fit_intercept: bool = True, tol: float = 1e-10, max_iter: int = 100) -> None:
        self.C, self.fit_intercept, self.tol, self.max_iter = C, fit_intercept, tol, max_iter

    def get_params(self, deep: bool = True):
        return dict(C=self.C, fit_intercept=self.fit_intercept, tol=self.tol, max_iter=self.max_iter)

    # ---------------------------------------------------------------- fitting
    def fit_blocks(self, blocks, y: torch.Tensor, rows=None, columns: Optional[Sequence[str]] = None):
        """Fit on bitmap-form feature blocks (``ops.features(..., bool_bits=True)`` or
        ``ops.select_rows``), ``y`` a device uint8 column of one label per row, over ``columns``
        (default: every feature, plan order).  ``rows``: the row numbers that take part (an index
        tensor, as in ``DeviceGBTClassifier.fit_binned``); they become the kernel's row mask."""
        check_params(self.C, self.tol, self.max_iter)
        names, kc = model_slots(blocks, columns)
        dev, n = blocks.device, blocks.n
        y = torch.as_tensor(y, device=dev)
        if y.dtype != torch.uint8 or y.dim() != 1 or y.numel() != n:
            raise ValueError('y must be a uint8 device column of one label per row')
        y = y.contiguous()
        mask = None
        if rows is not None:
            rows = torch.as_tensor(rows, device=dev).reshape(-1).to(torch.int64)
            if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
                raise ValueError(f'rows must be inside [0, {n})')
            mask = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
            mask[rows] = 1
        n_fit = n if mask is None else int(mask.sum())
        n_pos = int((y != 0).sum()) if mask is None else int(((y != 0) & (mask[:n] != 0)).sum())
        if n_fit == 0 or n_pos == 0 or n_pos == n_fit:
            raise ValueError('This solver needs samples of 2 classes in the data, but the data contains only one class')
        col_exp = column_exps(blocks, kc, mask)
        d = len(kc)

        def evaluate(beta):
            b = beta if self.fit_intercept else np.append(beta, 0.0)
            le = loss_exponent(b, col_exp)
            limbs, err = moments_limbs(blocks, kc, b, y, mask, col_exp, le)
            host = torch.cat([limbs.reshape(-1), err.to(torch.int64)]).cpu().numpy()  # one copy back
            raise_errors(int(host[-1]))
            g, H, f = finalize(host[:-1].reshape(-1, 3), col_exp, le)
            if not self.fit_intercept:
                g, H = g[:d], H[:d, :d]
            return g, H, f

        D = d + 1 if self.fit_intercept else d
        lam = np.full(D, 1.0 / float(self.C))
        if self.fit_intercept:
            lam[-1] = 0.0
        beta, n_iter, converged = newton(evaluate, D, lam, float(self.tol), int(self.max_iter))
        if not converged:
            from sklearn.exceptions import ConvergenceWarning
            warnings.warn(f'Newton solver did not converge in {n_iter} iterations: increase max_iter or tol.',
                          ConvergenceWarning)
        self.coef_ = beta[:d].reshape(1, d).copy()
        self.intercept_ = np.array([beta[d] if self.fit_intercept else 0.0])
        self.n_iter_ = np.array([n_iter], dtype=np.int32)
        self.classes_ = np.array([0, 1])
        self.feature_names_in_ = np.array(names, dtype=object)
        self.n_features_in_ = d
        return self

    def fit(self, X, y):
        """Fit on a host frame or 2-D array, uploaded the way ``boost.bin_host`` does it."""
        check_params(self.C, self.tol, self.max_iter)
        y = np.asarray(y).reshape(-1)
        classes = np.unique(y)
        if len(classes) < 2:
            raise ValueError('This solver needs samples of 2 classes in the data, but the data contains only one '
                             f'class: {classes[0] if len(classes) else None!r}')
        if len(classes) > 2:
            raise ValueError('DeviceLogisticRegression fits two classes')
        from .boost import _host_columns
        have, cols = _host_columns(X)
        if len(set(have)) != len(have):
            raise ValueError(f'repeated feature names: {sorted({c for c in have if have.count(c) > 1})}')
        if cols and len(cols[0]) != len(y):
            raise ValueError('X and y hold different numbers of rows')
        if len(have) > _native.SA_LOGIT_MAX_COLS:
            raise ValueError(f'logistic regression takes at most {_native.SA_LOGIT_MAX_COLS} columns: got {len(have)}')
        blocks = host_blocks(X)
        yd = torch.from_numpy((y == classes[1]).astype(np.uint8)).to(blocks.device)
        self.fit_blocks(blocks, yd)
        self.classes_ = classes
        return self

    # ---------------------------------------------------------------- prediction
    def _fitted(self) -> None:
        if not hasattr(self, 'coef_'):
            from sklearn.exceptions import NotFittedError
            raise NotFittedError('This DeviceLogisticRegression instance is not fitted yet.')

    def predict_blocks(self, blocks, dtype=torch.float64) -> torch.Tensor:
        """P(class 1) of every row of bitmap-form feature blocks that hold the model's columns
        (found by name), as a device tensor of ``dtype`` (float64 or float32)."""
        from .batch import stream_handle
        self._fitted()
        if dtype not in (torch.float64, torch.float32):
            raise ValueError('dtype must be torch.float64 or torch.float32')
        _, kc = model_slots(blocks, [str(c) for c in self.feature_names_in_])
        beta = np.concatenate([self.coef_[0], self.intercept_]).astype(np.float64)
        bdev = torch.from_numpy(beta).to(blocks.device)
        out = torch.empty(blocks.n, dtype=dtype, device=blocks.device)
        args, keep = _descriptors(blocks, kc)
        _native.check(_native.lib().sa_logit_predict(*args, bdev.data_ptr(), blocks.n, int(dtype == torch.float32),
                                                     out.data_ptr() if blocks.n else None, stream_handle()))
        del keep
        return out

    def predict_proba(self, X) -> np.ndarray:
        """``[n, 2]`` float64 class probabilities of a host frame or 2-D array."""
        self._fitted()
        names = [str(c) for c in self.feature_names_in_]
        blocks = host_blocks(X, names=names)
        if blocks.plan.n_bool + blocks.plan.n_f64 + blocks.plan.n_i64 != len(names):
            raise ValueError(f'X has {len(blocks.plan.order)} features, the model was fitted on {len(names)}')
        blocks.plan.order[:] = [(nm, k, c) for nm, (_, k, c) in zip(names, blocks.plan.order)]
        p = self.predict_blocks(blocks).cpu().numpy()
        return np.column_stack([1.0 - p, p])

    def predict(self, X) -> np.ndarray:
        return self.classes_[(self.predict_proba(X)[:, 1] > 0.5).astype(np.intp)]
