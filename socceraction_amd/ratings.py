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


def top_rows_host(values: np.ndarray, k: int, keep: Optional[np.ndarray] = None,
                  largest: bool = True) -> np.ndarray:
    """``ops.top_rows``' row numbers in numpy, by its definition: the eligible rows (kept, not
    NaN) ordered by value -- ``-0.0 == +0.0`` -- then by row number, the first ``k`` of them."""
    values = np.asarray(values)
    k = int(k)
    if not 1 <= k <= ops._native.SA_TOP_MAX_K:
        raise ValueError(f'k must be in [1, {ops._native.SA_TOP_MAX_K}]')
    ok = ~np.isnan(values)
    if keep is not None:
        ok &= np.asarray(keep, bool)
    rows = np.flatnonzero(ok)
    v = values[rows] + 0.0  # -0.0 + 0.0 = +0.0: the zeros tie
    order = np.lexsort((rows, -v if largest else v))
    return rows[order[:k]].astype(np.int64)


def mask_bytes(where, n: int, index=None) -> Optional[np.ndarray]:
    """``where`` (None, a boolean Series, array or tensor: one entry per action) as uint8 [n]
    host bytes.  A Series is taken by position; its index must be the actions'."""
    if where is None:
        return None
    if isinstance(where, torch.Tensor):
        where = where.cpu().numpy()
    if isinstance(where, pd.Series):
        if index is not None and not where.index.equals(index):
            raise ValueError('`where` must carry the actions\' index')
        where = where.to_numpy()
    where = np.asarray(where)
    if where.shape != (n,):
        raise ValueError('`where` must hold one entry per action')
    if where.dtype != np.bool_:
        where = where != 0
    return np.ascontiguousarray(where).view(np.uint8)


def mask_tensor(where, n: int, dev, index=None) -> Optional[torch.Tensor]:
    """``where`` as a uint8 [n] tensor on ``dev``: a device tensor stays where it is, anything
    else is uploaded at one byte per row."""
    if isinstance(where, torch.Tensor) and where.is_cuda:
        if where.dim() != 1 or where.numel() != n:
            raise ValueError('`where` must hold one entry per action')
        return where if where.dtype in (torch.bool, torch.uint8) else (where != 0)
    m = mask_bytes(where, n, index)
    return None if m is None else torch.from_numpy(m).to(dev)


def top_actions(actions: pd.DataFrame, values, k: int = 10, column: Optional[str] = None, where=None,
                largest: bool = True) -> pd.DataFrame:
    """The last cell of the reference's notebook 4: ``pd.concat([actions, values],
    axis=1).loc[where].dropna(subset=[column]).sort_values(column, ascending=not largest,
    kind='stable').head(k)`` -- the ``k`` most (``largest=False``: least) valuable actions of a
    selection, in rank order, ``actions``' index kept so that ``A.loc[i - 3:i + 1]`` shows an
    action with its neighbours.

    ``values``: one row per action (a DataFrame, a Series or a mapping, as :func:`group_sums`
    takes); ``column``: the value column to rank by (default: the last).  ``where``: a boolean
    mask per action (Series, array or device tensor; None: every action).  NaN values are never
    selected; equal values come in row order.  With a ROCm device the column and one mask byte
    per row are uploaded and selected by ``ops.top_rows``, and only the row numbers come back;
    without one the same definition runs in numpy (:func:`top_rows_host`)."""
    if isinstance(values, pd.Series):
        values = values.to_frame(values.name if values.name is not None else 'value')
    if not isinstance(values, pd.DataFrame):
        values = pd.DataFrame(values)
    n = len(actions)
    if values.shape[1] == 0:
        raise ValueError('no value column to rank by')
    if len(values) != n:
        raise ValueError('values must hold one row per action')
    column = values.columns[-1] if column is None else column
    if column not in values.columns:
        raise ValueError(f'no value column {column!r}')
    col = values[column].to_numpy()
    col = np.ascontiguousarray(col, np.float32 if col.dtype == np.float32 else np.float64)
    if n == 0 or not torch.cuda.is_available():
        rows = top_rows_host(col, k, mask_bytes(where, n, actions.index), largest)
    else:
        from .batch import device
        dev = device()
        rows = ops.top_rows(torch.from_numpy(col).to(dev), k, mask_tensor(where, n, dev, actions.index),
                            largest)[0].cpu().numpy()
    out = actions.iloc[rows].copy()
    for c in values.columns:
        out[c] = values[c].to_numpy()[rows]
    return out


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
