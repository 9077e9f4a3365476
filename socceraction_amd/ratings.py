"""Player and team rating tables: the grouped sums the reference's notebooks end with.

``public-notebooks/4-compute-vaep-values-and-top-players.ipynb`` (and its atomic twin) sum the
action values per player -- ``A.groupby('player_id')[values].sum()`` with a ``count = 1`` column
-- merge the minutes played and rank.  :func:`group_sums` is that group-by on the device, with
sums that do not depend on summation order (``ops.group_sums``: fixed-point limbs added as
integers, rounded to float64 once): the table is the same bit for bit from run to run, for any
batch split and for any number of ranks.  :func:`per_90` is the notebook's normalisation.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd
import torch

from . import ops

By = Union[str, Sequence[str]]


def _by_list(by: By) -> List[str]:
    return [by] if isinstance(by, str) else list(by)


def factorize(actions: pd.DataFrame, by: By, groups=None) -> Tuple[np.ndarray, pd.DataFrame]:
    """int32 group codes of every row (-1: a NaN key, which ``groupby`` drops) and the groups'
    key frame in code order.  Without ``groups`` the vocabulary is the observed keys in sorted
    order (``groupby(by)``'s row order); ``groups`` (a DataFrame of the ``by`` columns, or a
    sequence of keys for a single column) fixes it, sorted, so that ranks agree on the codes."""
    names = _by_list(by)
    if groups is not None:
        vocab = groups[names] if isinstance(groups, pd.DataFrame) else pd.DataFrame({names[0]: groups})
        vocab = vocab.drop_duplicates().sort_values(names).reset_index(drop=True)
        for c in names:  # the keys' dtype decides the table's (int64 ids stay int64)
            vocab[c] = vocab[c].astype(actions[c].dtype, copy=False)
        if len(names) == 1:
            codes = pd.Index(vocab[names[0]]).get_indexer(actions[names[0]])
        else:
            codes = pd.MultiIndex.from_frame(vocab).get_indexer(pd.MultiIndex.from_frame(actions[names]))
        missing = (codes < 0) & actions[names].notna().all(axis=1).to_numpy()
        if missing.any():
            raise ValueError(f'{int(missing.sum())} rows have keys outside `groups`')
        return codes.astype(np.int32), vocab
    level_codes, levels = [], []
    for c in names:
        k, u = pd.factorize(actions[c], sort=True)
        level_codes.append(k.astype(np.int64))
        levels.append(u)
    if len(names) == 1:
        return level_codes[0].astype(np.int32), pd.DataFrame({names[0]: levels[0]})
    # mixed radix over the sorted levels keeps the lexicographic order; observed tuples only
    nan = np.zeros(len(actions), bool)
    flat = np.zeros(len(actions), np.int64)
    for k, u in zip(level_codes, levels):
        nan |= k < 0
        flat = flat * max(len(u), 1) + np.maximum(k, 0)
    seen, inv = np.unique(flat[~nan], return_inverse=True)
    codes = np.full(len(actions), -1, np.int32)
    codes[~nan] = inv.astype(np.int32)
    cols, rest = {}, seen
    for c, u in list(zip(names, levels))[::-1]:
        r = max(len(u), 1)
        cols[c] = np.asarray(u)[rest % r] if len(u) else np.asarray(u)[:0]
        rest = rest // r
    return codes, pd.DataFrame({c: cols[c] for c in names})


def value_columns(values) -> Tuple[List[str], List[np.ndarray]]:
    """Names and host arrays of ``values`` (DataFrame, Series or a mapping of columns): all
    float32 stays float32, anything else is summed as float64."""
    if isinstance(values, pd.Series):
        values = values.to_frame(values.name if values.name is not None else 'value')
    if not isinstance(values, pd.DataFrame):
        values = pd.DataFrame(values)
    names = [str(c) for c in values.columns]
    f32 = len(names) > 0 and all(values[c].dtype == np.float32 for c in values.columns)
    dt = np.float32 if f32 else np.float64
    return names, [np.ascontiguousarray(values[c].to_numpy(), dtype=dt) for c in values.columns]


def table(acc: 'ops.GroupSums', keys: pd.DataFrame, names: Sequence[str]) -> pd.DataFrame:
    """The ratings frame of a finished table: key columns, one summed column per value column and
    ``count``, groups without a row left out (``groupby`` lists observed groups only).  Only the
    G-row table is copied to the host."""
    acc.check_errors()
    sums = acc.finalize().cpu().numpy()
    count = acc.count.cpu().numpy()
    out = keys.reset_index(drop=True).copy()
    for i, c in enumerate(names):
        out[c] = sums[i]
    out['count'] = count
    return out[count > 0].reset_index(drop=True)


def sum_device(codes: np.ndarray, cols, n_groups: int, scale_exp=None, acc=None, dev=None):
    """``ops.group_sums`` of host codes and host or device columns."""
    from .batch import device
    dev = dev or device()
    k = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)).to(dev)
    cols = [c if isinstance(c, torch.Tensor) else torch.from_numpy(c).to(dev) for c in cols]
    return ops.group_sums(k, cols, n_groups, scale_exp=scale_exp, acc=acc)


def group_sums(actions: pd.DataFrame, values, by: By = 'player_id', groups=None,
               scale_exp: Optional[Sequence[int]] = None) -> pd.DataFrame:
    """``pd.concat([actions[by], values, count=1], axis=1).groupby(by).sum().reset_index()`` on
    the device, order-independent.

    ``values``: one column per row of ``actions`` to sum (up to 8; a DataFrame, a Series or a
    mapping); NaN is skipped as pandas' ``sum`` skips it.  ``by``: a key column or a list of them
    (``['game_id', 'player_id']`` for the per-game table the minutes merge needs); rows with a
    NaN key are dropped.  Keys are factorised on the host.  ``groups`` fixes the vocabulary and
    ``scale_exp`` the columns' scale exponents (default: each column's largest finite magnitude
    decides); ranks that join their tables (:func:`factorize`, :func:`sum_device`,
    ``shard.allreduce_group_sums``, :func:`table`) must agree on both.  Rows are the observed
    groups in sorted key order."""
    names, cols = value_columns(values)
    if any(len(c) != len(actions) for c in cols):
        raise ValueError('values must hold one row per action')
    codes, keys = factorize(actions, by, groups)
    if not names:
        raise ValueError('no value column to sum')
    if len(keys) == 0:
        out = keys.copy()
        for c in names:
            out[c] = np.zeros(0, np.float64)
        out['count'] = np.zeros(0, np.int64)
        return out
    acc = sum_device(codes, cols, len(keys), scale_exp=scale_exp)
    return table(acc, keys, names)


def per_90(ratings: pd.DataFrame, minutes_played: pd.DataFrame, min_minutes: float = 180,
           by: By = 'player_id') -> pd.DataFrame:
    """The notebook's normalisation, on the host: merge the minutes played (summed per ``by``),
    keep players with more than ``min_minutes`` and add ``<name>_rating = <name>_value * 90 /
    minutes_played`` for every ``*_value`` column (``vaep_rating``, ``offensive_rating``,
    ``defensive_rating``); a table without ``*_value`` columns rates every summed column."""
    names = _by_list(by)
    mp = minutes_played[names + ['minutes_played']].groupby(names).sum().reset_index()
    stats = ratings.merge(mp)
    stats = stats[stats.minutes_played > min_minutes].reset_index(drop=True)
    cols = [c for c in ratings.columns if c.endswith('_value')] or \
        [c for c in ratings.columns if c not in names and c != 'count']
    for c in cols:
        rating = c[:-len('_value')] + '_rating' if c.endswith('_value') else c + '_rating'
        stats[rating] = stats[c] * 90 / stats.minutes_played
    return stats
