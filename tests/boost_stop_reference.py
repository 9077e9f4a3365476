"""Numpy restatement of items 9-12 of the boosted-tree trainer's arithmetic contract (DESIGN.md §3
"Boosted-tree training": evaluation rows, applying a tree, the integer metric of a round, the
stopping rule); TEST INFRASTRUCTURE ONLY.  Written from the contract, not from the kernels or
``socceraction_amd.boost``; items 1-8 come from ``boost_reference``.

Everything works on a host bin matrix ``B [F, n]`` uint8 (a bool feature's bin is its bit, its
only cut has index 0, so "bit set" is ``bin > cut``).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import boost_reference as br

LOGLOSS_EXP = 6  # SA_METRIC_LOGLOSS_EXP: the log-loss terms are fixed-point at 2^(6 - 95)


# --------------------------------------------------------------------------- item 10
def walk(tab, B, rows, max_depth):
    """The leaf every listed row reaches in one node table: from the root, at most ``max_depth``
    steps, right iff ``bin > cut`` (the missing bin 255 goes right), ending at ``feature < 0``."""
    rows = np.asarray(rows, np.int64)
    node = np.zeros(len(rows), np.int64)
    for _ in range(int(max_depth)):
        f = tab['feature'][node]
        live = np.flatnonzero(f >= 0)
        if not len(live):
            break
        right = B[f[live], rows[live]].astype(np.int64) > tab['cut'][node[live]]
        node[live] = 2 * node[live] + 1 + right
    return node


def apply_tree(tab, B, rows, em, max_depth):
    """``em[i] + value of row rows[i]'s leaf`` in float32 (a new array)."""
    em = np.asarray(em, np.float32)
    return (em + tab['value'][walk(tab, B, rows, max_depth)]).astype(np.float32)


# --------------------------------------------------------------------------- item 11
def u2_of(y, p):
    """The AUROC's integer by brute force: over (positive, negative) pairs, 2 where the
    positive's probability is larger, 1 where they are equal."""
    y = np.asarray(y).astype(bool)
    p = np.asarray(p)
    pos, neg = p[y][:, None], p[~y][None, :]
    return int(2 * (pos > neg).sum() + (pos == neg).sum())


def logloss_terms(y, p):
    """float64 ``-log(q)``: q the float32 probability of the true class (the complement taken in
    float32), clipped to [eps, 1 - eps] of float32 -- scikit-learn's ``log_loss`` on a float32
    column."""
    y = np.asarray(y).astype(bool)
    p = np.asarray(p, np.float32)
    eps = np.finfo(np.float32).eps
    q = np.clip(np.where(y, p, (np.float32(1.0) - p).astype(np.float32)), eps, np.float32(1.0) - eps)
    return -np.log(q.astype(np.float64))


def logloss_integer(y, p):
    """``l0 + (l1 << 32) + (l2 << 64)`` of the limb sums: every term truncated to a multiple of
    2^(LOGLOSS_EXP - 95), the truncated terms added as integers."""
    scale = 1 << (95 - LOGLOSS_EXP)
    return sum(int(Fraction(float(v)) * scale) for v in logloss_terms(y, p))


def metric_integer(y, p, metric):
    return u2_of(y, p) if metric == 'auc' else logloss_integer(y, p)


def metric_score(value, metric, y):
    y = np.asarray(y).astype(bool)
    if metric == 'auc':
        return value / (2 * int(y.sum()) * int((~y).sum()))
    return (value / (1 << (95 - LOGLOSS_EXP))) / len(y)


# --------------------------------------------------------------------------- item 12
def stopping(series, rounds, maximize):
    """``(best_iteration, rounds_run)`` of an integer series: the first round holding the best
    score, and the round count after which the counter of not strictly better rounds reaches
    ``rounds`` (None: never, every round runs)."""
    best_t, since = 0, 0
    for t, v in enumerate(series):
        if t == 0:
            continue
        improved = v > series[best_t] if maximize else v < series[best_t]
        since = 0 if improved else since + 1
        if improved:
            best_t = t
        elif rounds is not None and since == rounds:
            return best_t, t + 1
    return best_t, len(series)


# --------------------------------------------------------------------------- the trainer with held-out rows
def fit(B, y, cuts, train, eval_rows, metric='auc', early_stopping_rounds=None, **params):
    """Items 1-12 end to end with numpy's own ``exp``: rows where ``train`` is set take part in
    training, ``eval_rows`` are scored after every round, and training ends by the stopping
    rule.  Returns a dict: ``tables`` (every round run), ``series`` (the integers), ``eval_p``
    (per round), ``best_iteration``, ``rounds_run``, and ``kept`` = tables ``0..best_iteration``
    under early stopping, else all."""
    p = {**br.DEFAULTS, **params}
    D = int(p['max_depth'])
    n = B.shape[1]
    train = np.asarray(train, bool)
    eval_rows = np.asarray(eval_rows, np.int64)
    ye = np.asarray(y)[eval_rows]
    m = np.full(n, br.base_margin(p['base_score']), np.float32)
    em = np.full(len(eval_rows), br.base_margin(p['base_score']), np.float32)
    tabs, series, eps = [], [], []
    best = since = 0
    for t in range(int(p['n_estimators'])):
        gq, hq = br.quantise(br.probability(m), y)
        tab, node = br.build_tree(B, gq, hq, cuts, p, active=train)
        m = br.update_margin(m, tab, node)
        em = apply_tree(tab, B, eval_rows, em, D)
        ep = br.probability(em)
        tabs.append(tab)
        eps.append(ep)
        series.append(metric_integer(ye, ep, metric))
        if t > 0:
            improved = series[t] > series[best] if metric == 'auc' else series[t] < series[best]
            best, since = (t, 0) if improved else (best, since + 1)
        if early_stopping_rounds is not None and since == early_stopping_rounds:
            break
    assert (best, len(series)) == stopping(series, early_stopping_rounds, metric == 'auc')
    return {'tables': tabs, 'series': series, 'eval_p': eps, 'best_iteration': best, 'rounds_run': len(series),
            'kept': tabs[:best + 1] if early_stopping_rounds is not None else tabs}
