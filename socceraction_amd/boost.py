"""Reproducible histogram gradient boosting on the device feature blocks (``learner='device'``).

``VAEP.fit`` (reference vaep/base.py:139-213) hands the feature frame to xgboost, catboost or
lightgbm on the host.  This module trains the same kind of model -- binary logistic gradient
boosting, depth-limited trees, xgboost's ``hist`` rules (float32 values, ``x < threshold`` goes
left) -- where the features already are, with the kernels of ``csrc/sa_boost.hip``, and exports it
in the xgboost-1.6 JSON shape that :meth:`socceraction_amd.trees.TreeEnsemble.from_xgboost_json`
reads, so the device ``rate`` paths consume it unchanged.

The arithmetic contract (DESIGN.md §3 "Boosted-tree training"; ``tests/boost_reference.py``
restates it in numpy): float32 cuts, ``bin(x) = #{i : cut_i <= x32}`` with NaN -> 255, gradients
quantised to int32 at scale 2^30, int64 histograms, float64 gains, ties to the lowest feature then
the lowest cut.  Every sum is an integer sum: the model is the same bit for bit from run to run
and for any row order.

Held-out evaluation and early stopping (contract items 9-12; ``tests/boost_stop_reference.py``):
rows given as ``eval_rows`` / ``eval_set`` are pushed through every finished tree by
``sa_boost_apply`` and scored by the integer sums of ``sa_metric_sums`` (log loss) or the integer
pair count of ``sa_auc_count`` (AUROC).  Rounds are compared by those integers
(:func:`stop_decision`: xgboost's rule, zero tolerance), so the early-stopped model is as
reproducible as the full one.

Sample weights, ``scale_pos_weight``, the L1 penalty and row / column subsampling (contract items
13-17; ``tests/boost_sample_reference.py``): weights are folded in before the quantisation with an
exact power-of-two rescale, a round's samples come from a counter hash of ``(random_state, round,
row key or feature)``, so a tuned model is as reproducible as a plain one.  Every kernel has one
entry point: a plain fit passes the neutral :class:`Tuning`, which is the unweighted arithmetic
bit for bit.  The tuning parameters are :class:`TunedGBTClassifier`'s;
:class:`DeviceGBTClassifier` keeps its seven.  No weighted evaluation, bylevel / bynode column
sampling, categorical splits or learned default directions (missing values always go right).

The sharded fit (contract items 18-22; ``tests/test_gpu_boost_shard.py``): with ``process_group=``
every rank of a ``torch.distributed`` group holds a shard of the rows; the cuts come from the
ranks' joint sample, each level's histogram is joined by one int64 all-reduce of its used entries
(:func:`exchange_layout`, ``sa_boost_hist_pack`` / ``sa_boost_hist_unpack``,
``shard.allreduce_boost_level``), and every rank ends with the trees of the single-device fit of
the ranks' rows in rank order, byte for byte.  Without a process group none of it runs.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple
from dataclasses import dataclass, make_dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _native

NODE_DTYPE = np.dtype([('G', '<i8'), ('H', '<i8'), ('gain', '<f8'), ('feature', '<i4'), ('cut', '<i4'),
                       ('thr', '<f4'), ('value', '<f4'), ('exists', '<i4'), ('pad', '<i4')])
assert NODE_DTYPE.itemsize == 48
MAX_CUTS = _native.SA_BOOST_MAX_CUTS
MISSING_BIN = _native.SA_BOOST_MISSING_BIN
NO_NODE = _native.SA_BOOST_NO_NODE
MAX_DEPTH = _native.SA_BOOST_MAX_DEPTH
SAMPLE_ROWS = 65536
GRAD_SCALE = 2 ** 30
DEFAULTS = dict(n_estimators=100, max_depth=3, learning_rate=0.3, reg_lambda=1.0, min_child_weight=1.0,
                gamma=0.0, base_score=0.5)
# the tuning parameters of contract items 13-17 (TunedGBTClassifier, VAEP's tree_params), neutral
TUNING_DEFAULTS = dict(subsample=1.0, colsample_bytree=1.0, reg_alpha=0.0, scale_pos_weight=1.0, random_state=0)
ALL_DEFAULTS = {**DEFAULTS, **TUNING_DEFAULTS}
THR_ALL = 1 << 32  # the row threshold that takes every row


# ----------------------------------------------------------------------------- cuts (host)
def sample_rows(n: int) -> np.ndarray:
    """The deterministic row sample the cuts are chosen from: rows ``floor(i * n / S)``,
    ``i < S = min(n, 65536)``."""
    S = min(int(n), SAMPLE_ROWS)
    if S <= 0:
        return np.zeros(0, np.int64)
    return (np.arange(S, dtype=np.int64) * int(n)) // S


def cast32(col) -> np.ndarray:
    """A host column as the float32 values the tree predictor compares (csrc/sa_trees.hip's
    ``(float)feature_value(...)``: an integer column goes int64 -> double -> float)."""
    col = np.asarray(col)
    if col.dtype == np.float32:
        return col
    if col.dtype.kind in 'iu':
        return col.astype(np.int64).astype(np.float64).astype(np.float32)
    with np.errstate(over='ignore'):  # a double beyond float32's range becomes +-inf
        return col.astype(np.float64).astype(np.float32)


def cuts_from_sample(sample, is_bool: bool = False) -> np.ndarray:
    """One feature's strictly ascending float32 cuts (at most 254) from its sampled values: a
    bool feature has the single cut 0.5; a sample of at most 255 distinct non-NaN values gives
    every distinct value but the smallest; otherwise the values at ranks ``floor(i * L / 255)``,
    ``i = 1..254``, of the sorted sample of length L, deduplicated, without the sample minimum."""
    if is_bool:
        return np.array([0.5], np.float32)
    s = cast32(sample).ravel()
    s = np.sort(s[~np.isnan(s)])
    if not len(s):
        return np.zeros(0, np.float32)
    u = np.unique(s)
    if len(u) <= MAX_CUTS + 1:
        return u[1:].astype(np.float32)
    L = len(s)
    c = np.unique(s[(np.arange(1, MAX_CUTS + 1, dtype=np.int64) * L) // (MAX_CUTS + 1)])
    return c[c > s[0]].astype(np.float32)


def bin_values(x32, cuts) -> np.ndarray:
    """``bin(x) = #{i : cut_i <= x32}``, NaN -> 255 (host statement of ``sa_boost_bin``)."""
    x32 = np.asarray(x32, np.float32)
    b = np.searchsorted(np.asarray(cuts, np.float32), x32, side='right').astype(np.uint8)
    b[np.isnan(x32)] = MISSING_BIN
    return b


def _host_columns(X):
    """``(names, [column arrays])`` of a host frame or 2-D array."""
    if hasattr(X, 'columns'):
        return [str(c) for c in X.columns], [X[c].to_numpy() for c in X.columns]
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError('X must be two-dimensional')
    return [f'f{j}' for j in range(X.shape[1])], [X[:, j] for j in range(X.shape[1])]


def _kind(col: np.ndarray) -> str:
    return 'b' if col.dtype == np.bool_ else ('i' if col.dtype.kind in 'iu' else 'f')


def shard_sample_rows(counts: Sequence[int], rank: int) -> np.ndarray:
    """The part of the global cut sample that falls to ``rank`` (contract item 19): the ranks'
    training rows, ``counts[q]`` of rank q, are numbered rank 0's first, then rank 1's, ...; the
    sample is ``sample_rows(sum(counts))``; returned are its rows inside rank ``rank``'s slice as
    indices into that rank's own training rows, ascending.  The ranks' parts, concatenated in rank
    order, are the global sample."""
    counts = [int(c) for c in counts]
    off = sum(counts[:rank])
    idx = sample_rows(sum(counts))
    return idx[(idx >= off) & (idx < off + counts[rank])] - off


def _gather_records(group, dev, record) -> np.ndarray:
    """Every rank's float64 ``record`` (equal lengths) as ``[world, len]`` on the host: one
    all-gather (``shard._all_gather``), the exchange behind every agreement of a sharded fit."""
    import torch
    import torch.distributed as dist

    from . import shard
    rec = torch.from_numpy(np.asarray(record, np.float64).ravel().copy()).to(dev)
    out = torch.empty(dist.get_world_size(group) * rec.numel(), dtype=torch.float64, device=dev)
    shard._all_gather(out, rec, group=group)
    return out.cpu().numpy().reshape(dist.get_world_size(group), -1)


def _group_device(group):
    """Where a host-side exchange stages its tensors: the current GPU under RCCL, else the host."""
    import torch

    from . import shard
    return torch.device('cuda', torch.cuda.current_device()) if shard._on_device(group) else torch.device('cpu')


def agree(group, dev, err: Optional[Exception], what: str = 'fit') -> None:
    """One rank's ``ValueError`` raised on every rank (contract item 22): every rank calls this
    with its pending error or None; the failing rank re-raises its own, the others a ``ValueError``
    naming it.  No rank goes on to a collective another rank will not reach."""
    import torch.distributed as dist
    flags = _gather_records(group, dev, [0.0 if err is None else 1.0])[:, 0]
    if err is not None:
        raise err
    if flags.any():
        raise ValueError(f'sharded {what}: rank {int(np.flatnonzero(flags)[0])} of the process group refused its '
                         f'arguments (this is rank {dist.get_rank(group)})')


def _gather_sample(group, dev, local, counts: Sequence[int]) -> np.ndarray:
    """The ranks' float32 sample parts ``[S_r, C]`` (a device or host tensor on ``dev``) as the one
    host array ``[S, C]`` every rank computes its cuts from: padded to the largest part, ONE
    all-gather, the true parts concatenated in rank order."""
    import torch

    from . import shard
    W = len(counts)
    sizes = [len(shard_sample_rows(counts, q)) for q in range(W)]
    C, top = local.shape[1], max(max(sizes), 1)
    send = torch.zeros((top, C), dtype=torch.float32, device=dev)
    send[:local.shape[0]] = local
    recv = torch.empty((W, top, C), dtype=torch.float32, device=dev)
    shard._all_gather(recv.reshape(-1), send.reshape(-1), group=group)
    host = recv.cpu().numpy()
    return np.concatenate([host[q, :sizes[q]] for q in range(W)], 0)


def _train_counts(group, dev, count: int) -> List[int]:
    return [int(c) for c in _gather_records(group, dev, [float(count)])[:, 0]]


def make_cuts(data, rows=None, process_group=None) -> List[np.ndarray]:
    """Every feature's cuts (model order) from the deterministic row sample of ``data``: device
    feature blocks (``ops.FeatureBlocks``; the sample is gathered on the device and copied back
    once) or a host frame / 2-D array.  ``rows``: the training rows (indices) the sample is
    taken from, default all.  With ``process_group`` every rank passes its own shard of the rows
    and all get the cuts of the concatenated table (contract item 19): an all-gather of the row
    counts, then one of the ranks' parts of the global sample (:func:`shard_sample_rows`)."""
    if hasattr(data, 'plan'):
        return _make_cuts_blocks(data, rows, process_group)
    names, cols = _host_columns(data)
    n = len(cols[0]) if cols else 0
    sel = None if rows is None else np.asarray(rows, np.int64)
    if process_group is not None:
        import torch
        import torch.distributed as dist
        dev = _group_device(process_group)
        counts = _train_counts(process_group, dev, n if sel is None else len(sel))
        idx = shard_sample_rows(counts, dist.get_rank(process_group))
        if sel is not None:
            idx = sel[idx]
        local = np.zeros((len(idx), len(cols)), np.float32)
        for j, c in enumerate(cols):
            local[:, j] = cast32(c[idx])
        host = _gather_sample(process_group, dev, torch.from_numpy(local).to(dev), counts)
        return [cuts_from_sample(host[:, j], _kind(c) == 'b') for j, c in enumerate(cols)]
    idx = sample_rows(n if sel is None else len(sel))
    if sel is not None:
        idx = sel[idx]
    return [cuts_from_sample(c[idx], _kind(c) == 'b') for c in cols]


def _make_cuts_blocks(blocks, rows=None, group=None) -> List[np.ndarray]:
    import torch
    dev = blocks.device
    sel = None if rows is None else torch.as_tensor(rows, device=dev).to(torch.int64)
    n_train = blocks.n if sel is None else sel.numel()
    if group is None:
        idx = torch.from_numpy(sample_rows(n_train)).to(dev)
    else:
        import torch.distributed as dist
        counts = _train_counts(group, dev, n_train)
        idx = torch.from_numpy(shard_sample_rows(counts, dist.get_rank(group))).to(dev)
    if sel is not None:
        idx = sel[idx]
    parts = []
    for t in (blocks.f64_block, blocks.i64_block):
        R = t.shape[2]
        v = t[idx // R, :, idx % R]  # [S, C]
        if v.dtype == torch.int64:
            v = v.to(torch.float64)
        parts.append(v.to(torch.float32))
    nf = parts[0].shape[1]
    if group is not None:
        host = _gather_sample(group, dev, torch.cat(parts, 1), counts)
    else:
        host = torch.cat(parts, 1).cpu().numpy() if len(idx) else np.zeros((0, nf + parts[1].shape[1]), np.float32)
    out = []
    for _, kind, col in blocks.plan.order:
        if kind == 'b':
            out.append(cuts_from_sample(None, True))
        else:
            out.append(cuts_from_sample(host[:, col if kind == 'f' else nf + col]))
    return out


def check_cuts(cuts: Sequence[np.ndarray], n_features: int) -> List[np.ndarray]:
    if len(cuts) != n_features:
        raise ValueError(f'{len(cuts)} cut lists for {n_features} features')
    out = []
    for f, c in enumerate(cuts):
        c = np.asarray(c, np.float32).ravel()
        if len(c) > MAX_CUTS or np.isnan(c).any() or (len(c) > 1 and not (np.diff(c) > 0).all()):
            raise ValueError(f'feature {f}: cuts must be at most {MAX_CUTS} strictly ascending float32 values')
        out.append(c)
    return out


# ----------------------------------------------------------------------------- export (host)
def trees_to_xgboost_json(trees: np.ndarray, feature_names: Sequence[str], base_score: float = 0.5) -> dict:
    """Node tables ``[n_trees, 2^(max_depth+1) - 1]`` (:data:`NODE_DTYPE`, heap order) as an
    xgboost-1.6-shaped ``binary:logistic`` gbtree JSON model: each tree's existing nodes in heap
    order, ``default_left = 0`` everywhere (missing goes right)."""
    out = []
    for t, tab in enumerate(np.asarray(trees)):
        heap = np.flatnonzero(tab['exists'] != 0)
        if not len(heap):
            heap = np.array([0])
        new = {int(h): i for i, h in enumerate(heap)}
        m = len(heap)
        left, right, parent = [-1] * m, [-1] * m, [2147483647] * m
        sidx, cond, gains, hess, bw = [0] * m, [0.0] * m, [0.0] * m, [0.0] * m, [0.0] * m
        for h, i in new.items():
            nd = tab[h]
            bw[i] = float(nd['value'])
            hess[i] = float(nd['H']) / GRAD_SCALE
            if nd['feature'] >= 0 and nd['exists']:
                left[i], right[i] = new[2 * h + 1], new[2 * h + 2]
                parent[left[i]] = parent[right[i]] = i
                sidx[i] = int(nd['feature'])
                cond[i] = float(nd['thr'])
                gains[i] = float(nd['gain'])
            else:
                cond[i] = float(nd['value'])
        out.append({'left_children': left, 'right_children': right, 'parents': parent,
                    'split_indices': sidx, 'split_conditions': cond, 'default_left': [0] * m,
                    'split_type': [0] * m, 'base_weights': bw, 'loss_changes': gains, 'sum_hessian': hess,
                    'categories': [], 'categories_nodes': [], 'categories_segments': [], 'categories_sizes': [],
                    'tree_param': {'num_deleted': '0', 'num_feature': str(len(feature_names)),
                                   'num_nodes': str(m), 'size_leaf_vector': '0'}, 'id': t})
    return {'learner': {
        'attributes': {}, 'feature_names': [str(c) for c in feature_names], 'feature_types': [],
        'objective': {'name': 'binary:logistic', 'reg_loss_param': {'scale_pos_weight': '1'}},
        'gradient_booster': {'name': 'gbtree', 'model': {
            'gbtree_model_param': {'num_parallel_tree': '1', 'num_trees': str(len(out)), 'size_leaf_vector': '0'},
            'trees': out, 'tree_info': [0] * len(out)}},
        'learner_model_param': {'base_score': repr(float(base_score)), 'num_feature': str(len(feature_names)),
                                'num_class': '0', 'num_target': '1'}}, 'version': [1, 6, 2]}


def base_margin(base_score: float) -> np.float32:
    """The float32 base margin of ``base_score`` as ``TreeEnsemble.from_xgboost_json`` computes it."""
    p = np.float32(float(base_score))
    return np.float32(-np.log(np.float32(1.0) / p - np.float32(1.0)))


def predict_tables(trees: np.ndarray, X32: np.ndarray, base_score: float = 0.5) -> np.ndarray:
    """Host ``P(class 1)`` (float32) of node tables on float32 values ``X32 [n, F]``: the
    predictor's walk (``x < thr`` left, NaN right), leaves added in tree order in float32."""
    n = X32.shape[0]
    m = np.full(n, base_margin(base_score), np.float32)
    rows = np.arange(n)
    for tab in np.asarray(trees):
        node = np.zeros(n, np.int64)
        while True:
            f = tab['feature'][node]
            live = f >= 0
            if not live.any():
                break
            with np.errstate(invalid='ignore'):
                left = X32[rows[live], f[live]] < tab['thr'][node[live]]
            node[live] = 2 * node[live] + 2 - left
        m = (m + tab['value'][node]).astype(np.float32)
    with np.errstate(over='ignore'):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-m))).astype(np.float32)


# ----------------------------------------------------------------------------- binned data (device)
@dataclass
class BinnedData:
    """The trainer's view of a feature table: the numeric features as a feature-major uint8 bin
    matrix ``bins [F_num, ld]``, the bool features as the Arrow bitmaps ``bits [rows, words]``
    (never expanded to bytes), every feature's cuts, and the maps between feature numbers and
    rows of the two."""

    n: int
    ld: int
    names: List[str]
    cuts: List[np.ndarray]
    bits: Any
    bins: Any
    bit_rows: np.ndarray
    bit_feat: np.ndarray
    num_feat: np.ndarray
    fmap: np.ndarray
    dev: Dict[str, Any]

    @property
    def n_features(self) -> int:
        return len(self.names)

    @property
    def device(self):
        return self.bins.device

    def host_bins(self) -> np.ndarray:
        """``[F, n]`` uint8 bins of every feature (a bool feature: its bit) on the host."""
        out = np.zeros((self.n_features, self.n), np.uint8)
        if len(self.num_feat):
            out[self.num_feat] = self.bins[:, :self.n].cpu().numpy()
        if len(self.bit_feat):
            raw = self.bits.cpu().numpy().view(np.uint8)
            un = np.unpackbits(raw, axis=1, bitorder='little')[:, :self.n]
            out[self.bit_feat] = un[self.bit_rows]
        return out


def _ld(n: int) -> int:
    return max(16, (n + 15) // 16 * 16)


def _flat_cuts(cuts: Sequence[np.ndarray]):
    """``(cut_start [F + 1] int32, every feature's cuts in one float32 array)`` as the kernels take them."""
    cut_start = np.zeros(len(cuts) + 1, np.int32)
    cut_start[1:] = np.cumsum([len(c) for c in cuts])
    return cut_start, np.concatenate(list(cuts) + [np.zeros(1, np.float32)]).astype(np.float32)


class ExchangeLayout(namedtuple('ExchangeLayout', 'pairs n_bool n_num n_features')):
    """One node's payload pairs of the level exchange (:func:`exchange_layout`): ``pairs`` (int32)
    = ``feature * 256 + bin`` of its ``n_bool`` bool pairs, then of its ``n_num`` numeric pairs."""

    def words(self, n_nodes: int) -> int:
        """The payload's length in int64 words for a level of ``n_nodes`` nodes."""
        return 2 * int(n_nodes == 1) + 2 * int(n_nodes) * (self.n_bool + self.n_num)

    def dense_pairs(self, n_nodes: int) -> np.ndarray:
        """The dense pair index ``(node * F + feature) * 256 + bin`` of every payload pair after
        the level-0 head, in payload order (int64): every node's bool pairs, then every node's
        numeric pairs."""
        base = np.arange(int(n_nodes), dtype=np.int64)[:, None] * (self.n_features * 256)
        p = self.pairs.astype(np.int64)
        return np.concatenate([(base + p[None, :self.n_bool]).ravel(), (base + p[None, self.n_bool:]).ravel()])


def exchange_layout(cut_start, is_bool) -> ExchangeLayout:
    """The layout of the level exchange (contract item 18), from the features' cut counts and
    kinds alone, so every rank derives the same: of a node's dense ``[F, 256]`` pairs the payload
    carries bin 1 of every bool feature (model order; bin 0 is rebuilt from the node total after
    the sum) and then, of every numeric feature with m cuts (model order), bins ``0 .. m`` and the
    missing bin 255."""
    cut_start = np.asarray(cut_start, np.int64).ravel()
    is_bool = np.asarray(is_bool, bool).ravel()
    F = len(is_bool)
    if len(cut_start) != F + 1:
        raise ValueError('cut_start has one entry per feature and one more')
    m = np.diff(cut_start)
    if (m < 0).any() or (m > MAX_CUTS).any():
        raise ValueError(f'a feature has 0 .. {MAX_CUTS} cuts')
    out = [f * 256 + 1 for f in range(F) if is_bool[f]]
    n_bool = len(out)
    for f in range(F):
        if not is_bool[f]:
            out.extend(range(f * 256, f * 256 + int(m[f]) + 1))
            out.append(f * 256 + MISSING_BIN)
    return ExchangeLayout(np.array(out, np.int32), n_bool, len(out) - n_bool, F)


def _exchange(data: 'BinnedData'):
    """``data``'s :class:`ExchangeLayout` and its pair table on the device, built once per table."""
    import torch
    if 'exchange' not in data.dev:
        is_bool = np.zeros(data.n_features, bool)
        is_bool[data.bit_feat] = True
        lay = exchange_layout(_flat_cuts(data.cuts)[0], is_bool)
        table = torch.from_numpy(np.concatenate([lay.pairs, np.zeros(1, np.int32)])).to(data.device)  # (never empty)
        data.dev['exchange'] = (lay, table)
    return data.dev['exchange']


def _padded_block(cols, n: int, ld: int, dtype) -> np.ndarray:
    """Host columns as one zero-padded ``[1, C, ld]`` block of ``dtype``."""
    h = np.zeros((1, len(cols), ld), dtype)
    for r, c in enumerate(cols):
        h[0, r, :n] = c
    return h


def _bin(names, kinds_cols, bits, f_blk, i_blk, f32: bool, n: int, cuts) -> BinnedData:
    """kinds_cols[f] = (kind, column in its block / bitmap row)."""
    import torch

    from .batch import stream_handle
    dev = f_blk.device
    F = len(names)
    cuts = check_cuts(cuts, F)
    ld = _ld(n)
    cut_start, flat = _flat_cuts(cuts)
    bool_f = [f for f, (k, _) in enumerate(kinds_cols) if k == 'b']
    num_f = [f for f, (k, _) in enumerate(kinds_cols) if k != 'b']
    for f in bool_f:
        if len(cuts[f]) != 1 or cuts[f][0] != np.float32(0.5):
            raise ValueError(f'feature {f} is a bool feature: its only cut is 0.5')
    bit_rows = np.array([kinds_cols[f][1] for f in bool_f], np.int32)
    bit_feat = np.array(bool_f, np.int32)
    num_feat = np.array(num_f, np.int32)
    slots = np.array([((1 if kinds_cols[f][0] == 'f' else 2) << 24) | kinds_cols[f][1] for f in num_f], np.int32)
    fmap = np.zeros(F, np.int32)
    fmap[bit_feat] = bit_rows
    fmap[num_feat] = (1 << 24) | np.arange(len(num_f), dtype=np.int32)
    if bool_f and (bits is None or bits.dtype != torch.int64 or bits.shape[1] * 64 < n):
        raise ValueError('the bool features must come as bitmaps (ops.features(..., bool_bits=True))')
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    d = {'cut_start': t(cut_start), 'cuts': t(flat), 'bit_rows': t(bit_rows) if bool_f else None,
         'bit_feat': t(bit_feat) if bool_f else None, 'num_feat': t(num_feat) if num_f else None,
         'fmap': t(fmap), 'slots': t(slots) if num_f else None}
    bins = torch.empty((max(len(num_f), 1), ld), dtype=torch.uint8, device=dev)
    if num_f and n:
        blk = []
        for tns in (f_blk, i_blk):
            b = _native.SaBlock()
            b.data = tns.data_ptr() if tns.numel() else None
            b.n_cols, b.tile_rows = tns.shape[1], tns.shape[2]
            blk.append(b)
        _native.check(_native.lib().sa_boost_bin(
            ctypes.byref(blk[0]), ctypes.byref(blk[1]), int(f32), d['slots'].data_ptr(), d['num_feat'].data_ptr(),
            d['cut_start'].data_ptr(), d['cuts'].data_ptr(), len(num_f), n, bins.data_ptr(), ld, stream_handle()))
    return BinnedData(n, ld, list(names), cuts, bits if bool_f else None, bins, bit_rows, bit_feat, num_feat,
                      fmap, d)


def plan_columns(plan, columns: Sequence[str]) -> List[int]:
    """The positions in ``plan.order`` of the feature names ``columns``; an unknown or repeated
    name is a ``ValueError``."""
    where = {name: j for j, name in enumerate(plan.names)}
    names = [str(c) for c in columns]
    unknown = [c for c in names if c not in where]
    if unknown:
        raise ValueError(f'{" and ".join(unknown)} are not available in the features')
    if len(set(names)) != len(names):
        raise ValueError(f'repeated feature names: {sorted({c for c in names if names.count(c) > 1})}')
    return [where[c] for c in names]


def bin_blocks(blocks, cuts: Optional[Sequence[np.ndarray]] = None, rows=None, process_group=None,
               columns: Optional[Sequence[str]] = None) -> BinnedData:
    """Bin device feature blocks (``ops.features(..., bool_bits=True)``; float64 / int64 or
    float32 numeric blocks): ``sa_boost_bin`` for the numeric features, the bitmaps as they are.
    ``cuts``: explicit cut lists (model order), default :func:`make_cuts` on ``rows`` (with
    ``process_group``: of all ranks' rows).  ``columns``: the feature names of the plan the model
    uses, in the model's feature order (default: every feature, in plan order); ``cuts`` then has
    one entry per name of ``columns``."""
    plan = blocks.plan
    if plan.n_bool and blocks.bool_bits is None:
        raise ValueError('the bool features must come as bitmaps (ops.features(..., bool_bits=True))')
    order = list(plan.order)
    pick = None if columns is None else plan_columns(plan, columns)  # before the cut sample's device work
    if cuts is None:
        cuts = make_cuts(blocks, rows, process_group)
        if pick is not None:
            cuts = [cuts[j] for j in pick]
    if pick is not None:
        order = [order[j] for j in pick]
    kc = [(kind, col) for _, kind, col in order]
    return _bin([name for name, _, _ in order], kc, blocks.bool_bits, blocks.f64_block, blocks.i64_block,
                blocks.num32, blocks.n, cuts)


def bin_host(X, cuts: Optional[Sequence[np.ndarray]] = None, rows=None, device=None, process_group=None) -> BinnedData:
    """Upload a host frame / 2-D array -- bool columns as bitmaps, float and integer columns as
    float64 / int64 blocks -- and bin it with the same kernel (``process_group``: as in
    :func:`bin_blocks`)."""
    import torch
    names, cols = _host_columns(X)
    n = len(cols[0]) if cols else 0
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if cuts is None:
        cuts = make_cuts(X, rows, process_group)
    ld = _ld(n)
    kinds = [_kind(c) for c in cols]
    kc, per = [], {'b': [], 'f': [], 'i': []}
    for k, c in zip(kinds, cols):
        kc.append((k, len(per[k])))
        per[k].append(c)
    words = max(1, (n + 63) // 64)
    hb = np.zeros((max(len(per['b']), 1), words * 8), np.uint8)
    for r, c in enumerate(per['b']):
        pk = np.packbits(c.astype(bool), bitorder='little')
        hb[r, :len(pk)] = pk
    hf, hi = _padded_block(per['f'], n, ld, np.float64), _padded_block(per['i'], n, ld, np.int64)
    return _bin(names, kc, torch.from_numpy(hb.view(np.int64)).to(dev), torch.from_numpy(hf).to(dev),
                torch.from_numpy(hi).to(dev), False, n, cuts)


# ----------------------------------------------------------------------------- single kernels
def _stream():
    from .batch import stream_handle
    return stream_handle()


def _run(family, fn, *args) -> None:
    """A launch outside a fit (``DeviceGBTClassifier._launch`` without events)."""
    _native.check(fn(*args))


def _ptr(t):
    return None if t is None else t.data_ptr()


# The tuning arguments of a fit's (or one launch's) kernels (contract items 13-16): the float32 device
# weight column (None: every weight 1), scale_pos_weight, the quantisation shift e (the scale is
# 2^(30 - e)), the int64 device key column (None: a row's key is its index), the seed, the row sample's
# raw threshold, the L1 penalty.  The defaults are the neutral values: the plain learner.
Tuning = namedtuple('Tuning', 'weight scale_pos_weight shift keys seed thr reg_alpha',
                    defaults=(None, 1.0, 0, None, 0, THR_ALL, 0.0))


class ColumnSamples:
    """Every round's column sample (contract item 17) as the compacted int32 device lists the
    histogram kernels take, built on the host, uploaded once and sliced once: ``rounds[t]`` holds
    round t's views ``(bit_rows, bit_feat, n_bool, num_feat, num_rows, n_num)`` of them.
    ``mask [T, F]`` (uint8, on the device) is the split search's; ``features[t]`` is the sample."""

    def __init__(self, data: BinnedData, seed: int, T: int, colsample_bytree: float) -> None:
        import torch
        F = data.n_features
        mask = np.zeros((max(T, 1), F), np.uint8)
        lists = [], [], [], []  # bit_rows, bit_feat, num_feat, num_rows
        self.features, bit_off, num_off = [], [0], [0]
        for t in range(T):
            self.features.append(column_sample(seed, t, F, colsample_bytree))
            mask[t, self.features[t]] = 1
            bsel, nsel = np.flatnonzero(mask[t, data.bit_feat]), np.flatnonzero(mask[t, data.num_feat])
            for part, v in zip(lists, (data.bit_rows[bsel], data.bit_feat[bsel], data.num_feat[nsel], nsel)):
                part.append(v)
            bit_off.append(bit_off[t] + len(bsel))
            num_off.append(num_off[t] + len(nsel))
        br, bf, nf, nr = (  # (a spare entry: no list is empty)
            torch.from_numpy(np.concatenate(v + [np.zeros(1, np.int32)]).astype(np.int32)).to(data.device)
            for v in lists)
        self.rounds = [(br[bit_off[t]:], bf[bit_off[t]:], bit_off[t + 1] - bit_off[t], nf[num_off[t]:],
                        nr[num_off[t]:], num_off[t + 1] - num_off[t]) for t in range(T)]
        self.mask = torch.from_numpy(mask).to(data.device)


def _grad(run, st, margin, y, mask, n: int, gq, hq, p, node, tu: Tuning = Tuning(), t: int = 0) -> None:
    """Round ``t``'s gradient launch (``sa_boost_grad``)."""
    run('grad', _native.lib().sa_boost_grad, margin.data_ptr(), _ptr(y), _ptr(mask), n, _ptr(tu.weight),
        tu.scale_pos_weight, tu.shift, _ptr(tu.keys), tu.seed, t, tu.thr, _ptr(gq), _ptr(hq), _ptr(p), _ptr(node), st)


def _hist(run, st, data: BinnedData, gq, hq, node, n_nodes: int, hist, tree, add_totals: bool, cols=None) -> None:
    """Both histogram kernels of the level of ``n_nodes`` nodes into the zeroed ``hist``.  With
    ``cols`` (a round of :class:`ColumnSamples`) the kernels visit its features only, else every
    feature; the bitmap kernel is launched even for none (it carries the level-0 node totals)."""
    lib, d = _native.lib(), data.dev
    bit_rows, bit_feat, nb, num_feat, num_rows, nn = cols or (
        d['bit_rows'], d['bit_feat'], len(data.bit_feat), d['num_feat'], None, len(data.num_feat))
    level = (gq.data_ptr(), hq.data_ptr(), node.data_ptr(), data.n, n_nodes - 1, n_nodes, data.n_features,
             hist.data_ptr())
    run('hist_bits', lib.sa_boost_hist_bits, data.bits.data_ptr() if nb else None,
        data.bits.shape[1] * 8 if nb else 0, bit_rows.data_ptr() if nb else None, bit_feat.data_ptr() if nb else None,
        nb, *level, tree.data_ptr(), int(add_totals), st)
    if nn:
        run('hist_bins', lib.sa_boost_hist_bins, data.bins.data_ptr(), data.ld, num_feat.data_ptr(), _ptr(num_rows),
            len(data.num_feat) if cols else 0, nn, *level, st)


def _split(run, st, hist, cut_start, cuts, F: int, n_nodes: int, params, bg, bc, tree, tu: Tuning = Tuning(),
           fmask=None, leaf_only: bool = False) -> None:
    """The split search of the level of ``n_nodes`` nodes (``leaf_only``: its leaf values only);
    ``params = (reg_lambda, min_child_weight, gamma, learning_rate)``, ``tu``'s L1 penalty and shift,
    and the ``[F]`` uint8 device mask ``fmask`` (None: every feature is a candidate)."""
    run('split', _native.lib().sa_boost_split, _ptr(hist), _ptr(cut_start), _ptr(cuts), F, n_nodes - 1, n_nodes,
        int(leaf_only), *params, tu.reg_alpha, tu.shift, _ptr(fmask), _ptr(bg), _ptr(bc), tree.data_ptr(), st)


def gradients(margin, y, row_mask=None, *, weight=None, scale_pos_weight: float = 1.0, shift: int = 0,
              row_keys=None, seed: int = 0, round: int = 0, thr: Optional[int] = None):
    """``sa_boost_grad`` on device columns: ``(gq, hq, p)`` -- int32, int32, float32.  ``weight``
    (float32 device column, default every weight 1), ``scale_pos_weight``, the quantisation
    ``shift`` e (the caller keeps every effective weight ``<= 2^e``), and the round's row sample --
    ``row_keys`` (int64 device column, default the row index), ``seed``, ``round`` and the raw
    threshold ``thr`` in ``0 .. 2^32`` (default ``2^32``: every row)."""
    import torch
    n = margin.numel()
    margin = margin.to(torch.float32).contiguous()
    y = y.view(torch.uint8) if y.dtype == torch.bool else y.to(torch.uint8)
    gq = torch.empty(max(n, 1), dtype=torch.int32, device=margin.device)
    hq = torch.empty_like(gq)
    p = torch.empty(max(n, 1), dtype=torch.float32, device=margin.device)
    if weight is not None:
        weight = weight.to(torch.float32).contiguous()
        if weight.numel() < n:
            raise ValueError('one weight per row')
    if row_keys is not None:
        row_keys = row_keys.to(torch.int64).contiguous()
        if row_keys.numel() < n:
            raise ValueError('one key per row')
    tu = Tuning(weight, float(scale_pos_weight), int(shift), row_keys, int(seed), THR_ALL if thr is None else int(thr))
    _grad(_run, _stream(), margin, y.contiguous(), row_mask, n, gq, hq, p, None, tu=tu, t=int(round))
    return gq[:n], hq[:n], p[:n]


def row_keys(game_id, action_id, device=None):
    """``sa_boost_row_keys``: the int64 device column ``fm(game_id) + action_id`` (wrapping) that
    names an action whatever its position (contract item 16), from two host integer columns."""
    import torch
    g = np.ascontiguousarray(np.asarray(game_id).ravel().astype(np.int64))
    a = np.ascontiguousarray(np.asarray(action_id).ravel().astype(np.int64))
    if len(g) != len(a):
        raise ValueError('game_id and action_id have different lengths')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    gd, ad = torch.from_numpy(g).to(dev), torch.from_numpy(a).to(dev)
    out = torch.empty(max(len(g), 1), dtype=torch.int64, device=dev)
    _native.check(_native.lib().sa_boost_row_keys(gd.data_ptr(), ad.data_ptr(), len(g), out.data_ptr(), _stream()))
    return out[:len(g)]


def _level(n_nodes: int) -> int:
    if n_nodes < 1 or n_nodes > _native.SA_BOOST_MAX_LEVEL_NODES or n_nodes & (n_nodes - 1):
        raise ValueError('a level has 1, 2, 4, ... 32 nodes')
    return n_nodes - 1


def _pad(t, ld, dtype, fill=0):
    import torch
    out = torch.full((ld,), fill, dtype=dtype, device=t.device)
    out[:t.numel()] = t.to(dtype)
    return out


def histograms(data: BinnedData, gq, hq, node, n_nodes: int, return_totals: bool = False):
    """The dense ``[n_nodes, F, 256, 2]`` int64 histogram of one level: ``node`` holds every row's
    level-local node (0 .. n_nodes-1; ``NO_NODE`` = the row takes no part)."""
    import torch
    node0 = _level(n_nodes)
    dev = data.device
    nd = node.to(torch.int64)
    heap = torch.where(nd == NO_NODE, nd, nd + node0).to(torch.uint8)
    heap = _pad(heap, data.ld, torch.uint8, NO_NODE)
    gq, hq = _pad(gq, data.ld, torch.int32), _pad(hq, data.ld, torch.int32)
    hist = torch.zeros((n_nodes, data.n_features, 256, 2), dtype=torch.int64, device=dev)
    tree = torch.zeros((4 * n_nodes, NODE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    _hist(_run, _stream(), data, gq, hq, heap, n_nodes, hist, tree, True)
    if not return_totals:
        return hist
    tab = tree.cpu().numpy().view(NODE_DTYPE).reshape(-1)[node0:node0 + n_nodes]
    return hist, np.stack([tab['G'], tab['H']], 1)


def level_histogram(data: BinnedData, gq, hq, node, n_nodes: int, totals=None):
    """One rank's part of a level, as the sharded fit forms it before the exchange: ``(hist, tree)``
    on the device -- the dense histogram of this table's rows and the round's node table.
    ``totals`` None: the level's node totals are summed from the rows (level 0 of a fit);
    ``totals [n_nodes, 2]``: they are preset (past level 0 they are the global ones) and every bool
    feature's bin 0 is derived from them."""
    import torch
    node0 = _level(n_nodes)
    dev = data.device
    nd = node.to(torch.int64)
    heap = _pad(torch.where(nd == NO_NODE, nd, nd + node0).to(torch.uint8), data.ld, torch.uint8, NO_NODE)
    gq, hq = _pad(gq, data.ld, torch.int32), _pad(hq, data.ld, torch.int32)
    hist = torch.zeros((n_nodes, data.n_features, 256, 2), dtype=torch.int64, device=dev)
    tab = np.zeros(4 * n_nodes, NODE_DTYPE)
    if totals is not None:
        tot = np.asarray(totals, np.int64).reshape(n_nodes, 2)
        tab['G'][node0:node0 + n_nodes], tab['H'][node0:node0 + n_nodes] = tot[:, 0], tot[:, 1]
    tree = torch.from_numpy(tab.view(np.uint8).reshape(4 * n_nodes, -1).copy()).to(dev)
    _hist(_run, _stream(), data, gq, hq, heap, n_nodes, hist, tree, totals is None)
    return hist, tree


def hist_pack(data: BinnedData, hist, tree, n_nodes: int, out=None, launch=None):
    """``sa_boost_hist_pack``: the level's exchange payload (int64 device vector,
    :meth:`ExchangeLayout.words` long) of the dense ``hist [n_nodes, F, 256, 2]`` and, at level 0,
    the root totals of the device node table ``tree``."""
    import torch
    lay, table = _exchange(data)
    if out is None:
        out = torch.empty(max(lay.words(n_nodes), 2), dtype=torch.int64, device=data.device)
    (launch or _run)('pack', _native.lib().sa_boost_hist_pack, hist.data_ptr(), tree.data_ptr(), table.data_ptr(),
                     lay.n_bool, lay.n_num, _level(n_nodes), n_nodes, data.n_features, out.data_ptr(), _stream())
    return out[:lay.words(n_nodes)]


def hist_unpack(data: BinnedData, payload, hist, tree, n_nodes: int, bit_feat=None, n_bool: Optional[int] = None,
                launch=None) -> None:
    """``sa_boost_hist_unpack``: the (summed) ``payload`` scattered into ``hist`` in place, at level 0
    its first pair stored as the root totals of ``tree``, then bin 0 of the listed bool features
    (device int32 list ``bit_feat`` with ``n_bool`` entries; default every bool feature) rebuilt
    from the node totals."""
    lay, table = _exchange(data)
    if bit_feat is None:
        bit_feat, n_bool = data.dev['bit_feat'], len(data.bit_feat)
    (launch or _run)('unpack', _native.lib().sa_boost_hist_unpack, payload.data_ptr(), table.data_ptr(), lay.n_bool,
                     lay.n_num, bit_feat.data_ptr() if n_bool else None, int(n_bool), _level(n_nodes), n_nodes,
                     data.n_features, hist.data_ptr(), tree.data_ptr(), _stream())


def best_splits(hist, totals, cuts: Sequence[np.ndarray], reg_lambda: float = 1.0, min_child_weight: float = 1.0,
                gamma: float = 0.0, learning_rate: float = 0.3, *, reg_alpha: float = 0.0, shift: int = 0,
                feature_mask=None) -> np.ndarray:
    """``sa_boost_split`` on a level's histograms ``[n_nodes, F, 256, 2]`` and node totals
    ``[n_nodes, 2]``: the level's node records (:data:`NODE_DTYPE`) and, after them, their
    children's -- ``[3 * n_nodes]`` rows: the level, then the children level in heap order.
    ``reg_alpha``, the quantisation ``shift`` and a ``feature_mask`` (``[F]``, 0 = the feature is no
    candidate; default all) are the kernel's."""
    import torch
    n_nodes, F = hist.shape[0], hist.shape[1]
    node0 = _level(n_nodes)
    cuts = check_cuts(cuts, F)
    dev = hist.device
    cut_start, flat = _flat_cuts(cuts)
    tab = np.zeros(4 * n_nodes, NODE_DTYPE)
    tot = np.asarray(totals, np.int64).reshape(n_nodes, 2)
    tab['G'][node0:node0 + n_nodes] = tot[:, 0]
    tab['H'][node0:node0 + n_nodes] = tot[:, 1]
    tab['exists'][node0:node0 + n_nodes] = 1
    tree = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    cs, cf = torch.from_numpy(cut_start).to(dev), torch.from_numpy(flat).to(dev)
    bg = torch.empty(n_nodes * F, dtype=torch.float64, device=dev)
    bc = torch.empty(n_nodes * F, dtype=torch.int32, device=dev)
    tu, fm = Tuning(reg_alpha=float(reg_alpha), shift=int(shift)), None
    if feature_mask is not None:
        fm = np.ascontiguousarray(np.asarray(feature_mask).astype(bool).astype(np.uint8).ravel())
        if len(fm) != F:
            raise ValueError('one mask byte per feature')
        fm = torch.from_numpy(fm).to(dev)
    params = (float(reg_lambda), float(min_child_weight), float(gamma), float(learning_rate))
    _split(_run, _stream(), hist.contiguous(), cs, cf, F, n_nodes, params, bg, bc, tree, tu=tu, fmask=fm)
    return tree.cpu().numpy().view(NODE_DTYPE).reshape(-1)[node0:node0 + 3 * n_nodes]


def _row_list(rows, n: int, dev):
    """Row indices (int64, on ``dev``) of an index list or a bool mask over the ``n`` rows."""
    import torch
    rows = torch.as_tensor(rows, device=dev)
    if rows.dtype == torch.bool:
        return torch.nonzero(rows[:n]).reshape(-1)
    return rows.reshape(-1).to(torch.int64).contiguous()


def _apply(data: BinnedData, tree, max_depth: int, rows, n_rows: int, margin, p, launch=None) -> None:
    """One ``sa_boost_apply`` launch: ``tree`` (device node table) over ``rows`` (device int64
    list or None) into the compact ``margin`` / ``p``."""
    nb = len(data.bit_feat)
    run = launch or _run
    run('apply', _native.lib().sa_boost_apply, tree.data_ptr(), int(max_depth), data.dev['fmap'].data_ptr(),
        data.bits.data_ptr() if nb else None, data.bits.shape[1] * 8 if nb else 0,
        data.bins.data_ptr() if len(data.num_feat) else None, data.ld,
        None if rows is None else rows.data_ptr(), int(n_rows), data.n, margin.data_ptr(),
        None if p is None else p.data_ptr(), _stream())


def apply_tree(data: BinnedData, table, margin, rows=None, max_depth: int = DEFAULTS['max_depth']):
    """``sa_boost_apply``: one tree -- ``table``, ``2^(max_depth+1) - 1`` records of
    :data:`NODE_DTYPE` in heap order (host array) -- applied to the listed rows of ``data``
    (indices; default every row).  ``margin``: one float32 per list entry.  Returns the new
    ``(margin, p)`` device columns; the input is not changed."""
    import torch
    D = int(max_depth)
    if not 1 <= D <= MAX_DEPTH:
        raise ValueError(f'max_depth must be in 1..{MAX_DEPTH}')
    tab = np.ascontiguousarray(np.asarray(table, NODE_DTYPE).reshape(-1))
    if len(tab) != 2 ** (D + 1) - 1:
        raise ValueError(f'a depth-{D} table has {2 ** (D + 1) - 1} records')
    dev = data.device
    if rows is not None:
        rows = _row_list(rows, data.n, dev)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= data.n):
            raise ValueError('rows must be inside the table')
    k = data.n if rows is None else int(rows.numel())
    m = torch.as_tensor(margin, device=dev).to(torch.float32).reshape(-1).clone()
    if m.numel() != k:
        raise ValueError('one margin per list entry')
    m = _pad(m, max(k, 1), torch.float32)
    p = torch.zeros(max(k, 1), dtype=torch.float32, device=dev)
    tree = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    _apply(data, tree, D, rows, k, m, p)
    return m[:k], p[:k]


# ----------------------------------------------------------------------------- early stopping (host)
EVAL_METRICS = ('auc', 'logloss')


def check_stop_params(early_stopping_rounds=None, eval_metric: str = 'auc'):
    """``(early_stopping_rounds or None, eval_metric)`` validated: an int >= 1, 'auc' or 'logloss'."""
    if eval_metric not in EVAL_METRICS:
        raise ValueError(f'eval_metric must be one of {EVAL_METRICS}, not {eval_metric!r}')
    if early_stopping_rounds is not None:
        if isinstance(early_stopping_rounds, bool) or int(early_stopping_rounds) != early_stopping_rounds \
                or int(early_stopping_rounds) < 1:
            raise ValueError('early_stopping_rounds must be an integer >= 1')
        early_stopping_rounds = int(early_stopping_rounds)
    return early_stopping_rounds, eval_metric


def stop_decision(series: Sequence[int], rounds: Optional[int], maximize: bool):
    """xgboost's early-stopping rule with zero tolerance on the integer metric of every round:
    round 0 sets the best score, a later round that is STRICTLY better becomes the best and
    resets a counter, any other round increments it, and training stops after the round at which
    the counter reaches ``rounds`` (None: never).  Returns ``(best_iteration, rounds_run)``:
    the first round holding the best score among the rounds run, and how many rounds are run."""
    best = count = 0
    for t in range(1, len(series)):
        if (series[t] > series[best]) if maximize else (series[t] < series[best]):
            best, count = t, 0
            continue
        count += 1
        if rounds is not None and count >= rounds:
            return best, t + 1
    return best, len(series)


def stop_look(series: Sequence[int], rounds: int, maximize: bool):
    """One look of the host at the rounds finished so far (the last one is the round the look was
    scheduled after): ``(fired, next_look)`` -- whether the rule has fired, i.e. the rounds since
    the best have reached ``rounds``, and otherwise the round after which it could next fire,
    ``best + rounds``.  Looking after round ``rounds`` first and then after every ``next_look``
    meets the stopping round exactly: the rule fires at ``best + rounds`` for the final best, and
    every earlier look's ``next_look`` is at most that."""
    best, stop = stop_decision(series, rounds, maximize)
    return stop - 1 - best >= rounds, best + rounds


def metric_integer(row: Sequence[int], eval_metric: str) -> int:
    """The integer a round is compared by, from its ten words in the ``ops.BinaryMetrics``
    layout: ``U2`` for 'auc', the log-loss limb sums ``l0 + (l1 << 32) + (l2 << 64)`` for 'logloss'."""
    if eval_metric == 'auc':
        return int(row[9])
    return int(row[5]) + (int(row[6]) << 32) + (int(row[7]) << 64)


def metric_score(value: int, eval_metric: str, n_eval: int, n_pos: int) -> float:
    """The float score of :func:`metric_integer`'s integer: ``U2 / (2 n_pos n_neg)``, or the
    fixed-point log-loss total over ``n_eval``."""
    if eval_metric == 'auc':
        return int(value) / (2 * int(n_pos) * (int(n_eval) - int(n_pos)))
    return (int(value) / (1 << (95 - _native.SA_METRIC_LOGLOSS_EXP))) / int(n_eval)


# ----------------------------------------------------------------------------- weights and sampling (host)
_M64 = (1 << 64) - 1


def fmix64(z: int) -> int:
    """splitmix64's finaliser on a wrapping uint64 (contract item 16)."""
    z &= _M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw(salt: int, seed: int, t: int, key: int) -> int:
    """The 64-bit draw of ``key`` in round ``t``: ``fm(fm(fm(seed ^ salt) + t) + key)``."""
    return fmix64(fmix64(fmix64(int(seed) ^ int(salt)) + int(t)) + int(key))


def row_threshold(subsample: float) -> int:
    """``floor(subsample * 2^32)``: a row is in a round's sample iff ``(draw >> 32) < thr``."""
    return int(math.floor(float(subsample) * 4294967296.0))


def column_sample(seed: int, t: int, n_features: int, colsample_bytree: float) -> np.ndarray:
    """Round ``t``'s features (ascending): the ``k = max(1, floor(colsample_bytree * F))`` with
    the smallest ``(draw(SALT_COLS, t, f), f)`` (contract item 17)."""
    F = int(n_features)
    k = max(1, int(math.floor(float(colsample_bytree) * F)))
    order = sorted(range(F), key=lambda f: (draw(_native.SA_BOOST_SALT_COLS, seed, t, f), f))
    return np.array(sorted(order[:k]), np.int32)


def weight_shift(mx: float) -> int:
    """The smallest integer ``e >= 0`` with ``mx <= 2^e`` (contract item 13)."""
    m, ex = math.frexp(float(mx))  # mx = m * 2^ex, 0.5 <= m < 1
    return max(0, ex - 1 if m == 0.5 else ex)


def _check_weight_range(mx: float, mn: float, finite: bool) -> int:
    if not finite or not mn >= 0:
        raise ValueError('sample weights must be finite and not negative')
    if not 0 < mx <= 2.0 ** _native.SA_BOOST_MAX_SHIFT:
        raise ValueError(f'the largest effective training weight must be in (0, 2^{_native.SA_BOOST_MAX_SHIFT}]')
    return weight_shift(mx)


def check_weights(sample_weight, n: int, y=None, scale_pos_weight: float = 1.0, rows=None):
    """A host weight column validated without the device: ``(float32 column, e or None)``.  One
    entry per row, finite, not negative, and the training rows' (``rows``: host indices or bool
    mask, default all) largest effective weight ``w * (y ? scale_pos_weight : 1)`` in
    ``(0, 2^20]``.  Without host labels ``y`` only what holds for any labels is checked and the
    shift is left to the device (None)."""
    w64 = np.asarray(sample_weight, np.float64).ravel()
    if len(w64) != int(n):
        raise ValueError(f'sample_weight has {len(w64)} entries for {int(n)} rows')
    with np.errstate(over='ignore'):
        w = w64.astype(np.float32)
    sel = w if rows is None else w[np.asarray(rows)]
    if not len(sel):
        raise ValueError('no training rows')
    s = np.float32(float(scale_pos_weight))
    if y is not None:
        yy = np.asarray(y).astype(bool).ravel()
        yy = yy if rows is None else yy[np.asarray(rows)]
        we = (sel * np.where(yy, s, np.float32(1.0))).astype(np.float32)
        return w, _check_weight_range(float(we.max()), float(we.min()), bool(np.isfinite(we).all()))
    # whatever the labels are, the largest effective weight is at least max(w) * min(s, 1)
    lo = float(np.float32(sel.max() * min(s, np.float32(1.0)))) if np.isfinite(sel).all() else math.nan
    _check_weight_range(lo, float(sel.min()), bool(np.isfinite(sel).all()))
    return w, None


def weights_to_device(w, dev):
    """A host weight column as a float32 device column, rounded through float64 as :func:`check_weights` does."""
    import torch
    w = np.asarray(w).ravel()
    with np.errstate(over='ignore'):  # a weight beyond float32's range becomes inf, which the range check refuses
        w = w if w.dtype == np.float32 else w.astype(np.float64).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(w)).to(dev)


def check_row_keys(row_keys, n: int) -> np.ndarray:
    """Host row keys validated: one integer per row, as int64 (a uint64 key is its bit pattern)."""
    keys = np.asarray(row_keys).ravel()
    if len(keys) != int(n) or keys.dtype.kind not in 'iu':
        raise ValueError('row_keys takes one integer per row')
    return keys.astype(np.uint64).view(np.int64) if keys.dtype == np.uint64 else keys.astype(np.int64)


IMPORTANCE_TYPES = ('gain', 'total_gain', 'weight', 'cover', 'total_cover')


def importances(trees: np.ndarray, n_features: int, importance_type: str = 'gain', quant_shift: int = 0) -> np.ndarray:
    """xgboost's feature importances of node tables, normalised to sum 1 as its scikit-learn
    wrapper does (all zero when no tree splits): over the split nodes of a feature, their number
    ('weight'), the sum ('total_gain') or mean ('gain') of their stored gain, the sum
    ('total_cover') or mean ('cover') of their hessian sums ``H * 2^(quant_shift - 30)``."""
    if importance_type not in IMPORTANCE_TYPES:
        raise ValueError(f'importance_type must be one of {IMPORTANCE_TYPES}, not {importance_type!r}')
    nodes = np.asarray(trees).reshape(-1)
    nodes = nodes[(nodes['exists'] != 0) & (nodes['feature'] >= 0)]
    f = nodes['feature'].astype(np.int64)
    count = np.bincount(f, minlength=n_features).astype(np.float64)
    if importance_type == 'weight':
        score = count
    else:
        v = nodes['gain'] if 'gain' in importance_type else nodes['H'].astype(np.float64) * 2.0 ** (quant_shift - 30)
        score = np.bincount(f, weights=v, minlength=n_features)
        if not importance_type.startswith('total_'):
            score = np.divide(score, count, out=np.zeros(n_features), where=count > 0)
    total = score.sum()
    return (score / total if total > 0 else np.zeros(n_features)).astype(np.float32)


# ----------------------------------------------------------------------------- the classifier
def check_params(params: Dict[str, Any], known: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    """``params`` over the defaults ``known`` (default :data:`ALL_DEFAULTS`), validated; a key
    outside ``known`` is a ``ValueError``."""
    known = ALL_DEFAULTS if known is None else known
    unknown = set(params) - set(known)
    if unknown:
        raise ValueError(f'unknown parameters {sorted(unknown)} (known: {sorted(known)})')
    p = {**ALL_DEFAULTS, **params}
    for k in ('subsample', 'colsample_bytree'):
        if not 0.0 < float(p[k]) <= 1.0:
            raise ValueError(f'{k} must be inside (0, 1]')
    if not 0.0 <= float(p['reg_alpha']) < math.inf:
        raise ValueError('reg_alpha must be finite and not negative')
    if not 0.0 < float(np.float32(float(p['scale_pos_weight']))) < math.inf:
        raise ValueError('scale_pos_weight must be positive')
    rs = p['random_state']
    if isinstance(rs, (bool, float, np.floating)) or not isinstance(rs, (int, np.integer)) or not 0 <= int(rs) < 2 ** 63:
        raise ValueError('random_state must be an integer in [0, 2^63)')
    if int(p['max_depth']) != p['max_depth'] or not 1 <= int(p['max_depth']) <= MAX_DEPTH:
        raise ValueError(f'max_depth must be in 1..{MAX_DEPTH}')
    if int(p['n_estimators']) < 0:
        raise ValueError('n_estimators must not be negative')
    if not p['reg_lambda'] >= 0 or not p['min_child_weight'] >= 0:
        raise ValueError('reg_lambda and min_child_weight must not be negative')
    if not 0.0 < float(p['base_score']) < 1.0:
        raise ValueError('base_score must be inside (0, 1)')
    return {k: p[k] for k in known}


def is_tuned(params: Dict[str, Any]) -> bool:
    """Whether ``params`` hold a tuning parameter away from its neutral value."""
    return any(k in params and params[k] != v for k, v in TUNING_DEFAULTS.items())


def make_classifier(params: Dict[str, Any], **kw) -> 'DeviceGBTClassifier':
    """The classifier of validated parameters: a :class:`DeviceGBTClassifier` when every tuning
    parameter is neutral or absent (the plain learner, as it was), else a
    :class:`TunedGBTClassifier`."""
    if is_tuned(params):
        return TunedGBTClassifier(**params, **kw)
    return DeviceGBTClassifier(**{k: v for k, v in params.items() if k in DEFAULTS}, **kw)


# The evaluation state of a fit (DeviceGBTClassifier._eval_setup fills it) and the state of one
# fit_binned between its parts (._prepare fills it: `columns` None: every feature; `ev` None: no evaluation rows)
_Eval = make_dataclass('_Eval', 'idx n n_pos minority m y margin p table P keys cursor total total_pos'.split())
_Fit = make_dataclass('_Fit', 'data y mask tu columns T D stream params margin gq hq node p P Mrec trees hist bg bc ev '
                              'group pay'.split())
# (`total` / `total_pos`: the evaluation rows and their positives over all ranks -- without a process
# group `n` / `n_pos`; `group` / `pay`: the process group of a sharded fit and its level payload buffer)


class DeviceGBTClassifier:
    """Binary logistic gradient boosting trained by ``csrc/sa_boost.hip`` (scikit-learn shaped).

    Parameters (xgboost's names and defaults): ``n_estimators=100, max_depth=3 (1..6),
    learning_rate=0.3, reg_lambda=1.0, min_child_weight=1.0, gamma=0.0, base_score=0.5``; any
    other key is a ``ValueError``.  The tuning parameters of contract items 13-17 belong to the
    subclass :class:`TunedGBTClassifier`; ``sample_weight`` is an argument of the fit methods of both.
    ``record=True`` keeps every round's probabilities and the margin after it (``record_['p']``,
    ``record_['margin']``, ``[n_estimators, n]`` on the device) for tests on small tables.
    After a fit: ``trees_`` (the node tables), ``cuts_``, ``feature_names_in_``, and on the device
    the training rows' final ``margin_`` and probabilities ``p_``; ``quant_shift_`` (the e of a
    weighted fit: the node tables' ``G`` / ``H`` are in units of ``2^(e - 30)``), ``column_samples_``
    (every kept round's features under ``colsample_bytree``) and ``feature_importances_``
    (``importance_type`` 'gain', 'total_gain', 'weight', 'cover' or 'total_cover', normalised to sum 1).

    Held-out evaluation: with evaluation rows (``eval_rows`` of :meth:`fit_binned` /
    :meth:`fit_blocks`, ``eval_set`` of :meth:`fit`) every finished tree is applied to them and
    the round is scored by ``eval_metric`` ('auc' or 'logloss') as an integer.  After the fit:
    ``evals_result_ = {'validation_0': {metric: [float per round run]}}``, ``eval_sums_`` (the
    integers behind it), ``best_iteration``, ``best_score``, ``n_rounds_run_`` and, with
    ``record=True``, ``record_['eval_p'] [rounds, n_eval]``.  ``early_stopping_rounds`` (an int
    >= 1, needs evaluation rows) stops training by :func:`stop_decision`; ``trees_`` then holds
    trees ``0..best_iteration`` and ``margin_`` / ``p_`` are those trees replayed over all rows."""

    PARAMS = DEFAULTS

    def __init__(self, record: bool = False, early_stopping_rounds: Optional[int] = None,
                 eval_metric: str = 'auc', importance_type: str = 'gain', **params) -> None:
        p = check_params(params, self.PARAMS)
        importances(np.zeros(0, NODE_DTYPE), 1, importance_type)  # (its check of the name)
        self.importance_type = importance_type
        self.early_stopping_rounds, self.eval_metric = check_stop_params(early_stopping_rounds, eval_metric)
        for k, v in {**TUNING_DEFAULTS, **p}.items():
            setattr(self, k, v)
        self.record = bool(record)
        self._events = None

    def get_params(self, deep: bool = True) -> Dict[str, Any]:
        return {k: getattr(self, k) for k in self.PARAMS}

    # ------------------------------------------------------------------ fitting
    def _check_eval_rows(self, eval_rows) -> Optional[int]:
        if self.early_stopping_rounds is not None and eval_rows is None:
            raise ValueError('early_stopping_rounds needs evaluation rows (eval_rows / eval_set)')
        return self.early_stopping_rounds

    def _launch(self, family, fn, *args) -> None:
        if self._events is None:
            return _native.check(fn(*args))
        self._timed(family, lambda: _native.check(fn(*args)))

    def _timed(self, family, work):
        """``work()`` -- a launch of the library's, or other device work -- and, when ``_events``
        is a list, its ``(family, start event, end event)`` entry."""
        if self._events is None:
            return work()
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = work()
        e1.record()
        self._events.append((family, e0, e1))
        return out

    def _eval_setup(self, data: BinnedData, y, eval_rows, T: int) -> '_Eval':
        """The evaluation state of a fit: the row list, its compact labels and margins, the
        zeroed ``[T, 10]`` metric table, and -- the fit's ONE host read before the first round --
        the list's bounds and its positives (which class is the minority for the AUROC)."""
        import torch
        dev, n = data.device, data.n
        idx = _row_list(eval_rows, n, dev)
        k = int(idx.numel())
        if k == 0:
            raise ValueError('binary scores need at least one row')
        if k >= 2 ** 30:
            raise ValueError('binary scores take fewer than 2**30 rows')
        inside = idx.clamp(0, max(n - 1, 0))
        lo, hi, n_pos = torch.stack([idx.min(), idx.max(), (y[inside] != 0).sum()]).cpu().tolist()
        if lo < 0 or hi >= n:
            raise ValueError('eval_rows must be inside the table')
        if n_pos == 0 or n_pos == k:
            raise ValueError('Only one class present in y. The AUROC is not defined in that case.')
        return self._eval_state(data, y, idx, int(n_pos), T, k, int(n_pos))

    def _eval_local(self, data: BinnedData, y, eval_rows):
        """A rank's part of the evaluation rows in a sharded fit (contract item 21): ``(idx, n_pos)``
        after the rank's one host read; the class and size checks are made on the ranks' sums."""
        import torch
        n = data.n
        idx = _row_list(eval_rows, n, data.device)
        if not idx.numel():
            return idx, 0
        inside = idx.clamp(0, max(n - 1, 0))
        lo, hi, n_pos = torch.stack([idx.min(), idx.max(), (y[inside] != 0).sum()]).cpu().tolist()
        if lo < 0 or hi >= n:
            raise ValueError('eval_rows must be inside the table')
        return idx, int(n_pos)

    def _eval_state(self, data: BinnedData, y, idx, n_pos: int, T: int, total: int, total_pos: int) -> '_Eval':
        import torch
        dev, k = data.device, int(idx.numel())
        minority, auc = int(n_pos <= k - n_pos), self.eval_metric == 'auc'
        m = int(n_pos) if minority else k - int(n_pos)
        return _Eval(idx=idx, n=k, n_pos=int(n_pos), minority=minority, m=m, y=y[idx].contiguous(),
                     total=total, total_pos=total_pos,
                     margin=torch.full((k,), float(base_margin(self.base_score)), dtype=torch.float32, device=dev),
                     p=torch.empty(k, dtype=torch.float32, device=dev),
                     table=torch.zeros((max(T, 1), 10), dtype=torch.int64, device=dev),
                     P=torch.empty((T, k), dtype=torch.float32, device=dev) if self.record else None,
                     keys=torch.empty(m, dtype=torch.int32, device=dev) if auc else None,
                     cursor=torch.zeros(max(T, 1), dtype=torch.int64, device=dev) if auc else None)

    def _eval_round(self, data: BinnedData, ev: '_Eval', tree, t: int, st) -> None:
        """Round t's tree applied to the evaluation rows and the round's integer sums written to
        row t of the metric table: the counts and log-loss limbs always, ``U2`` for 'auc'."""
        import torch
        lib, run = _native.lib(), self._launch
        k, y = ev.n, ev.y
        if k == 0:  # a rank of a sharded fit without evaluation rows: its sums stay zero
            return
        p = ev.P[t] if ev.P is not None else ev.p
        _apply(data, tree, int(self.max_depth), ev.idx, k, ev.margin, p, run)
        row = ev.table[t]
        run('metric', lib.sa_metric_sums, y.data_ptr(), p.data_ptr(), 1, k, row[0:2].data_ptr(), row[2:8].data_ptr(),
            row[8:9].data_ptr(), st)
        if self.eval_metric != 'auc':
            return
        m, mino = ev.m, ev.minority
        run('metric', lib.sa_auc_keys, y.data_ptr(), p.data_ptr(), 1, k, mino, ev.keys.data_ptr(), m,
            ev.cursor[t:t + 1].data_ptr(), st)
        keys = self._timed('sort', lambda: torch.sort(ev.keys).values)  # top bit clear: signed order
        run('metric', lib.sa_auc_count, y.data_ptr(), p.data_ptr(), 1, k, keys.data_ptr(), m, mino,
            row[9:10].data_ptr(), st)

    def _eval_series(self, ev: '_Eval', rounds: int, group=None) -> List[int]:
        """One host read of the metric table's first ``rounds`` rows: the integer series.  With a
        process group the rows are first summed over the ranks (``shard.allreduce_boost_eval``)."""
        if rounds <= 0:
            return []
        from .ops import BinaryMetrics
        table = ev.table[:rounds]
        if group is not None:
            from . import shard
            table = self._timed('allreduce', lambda: shard.allreduce_boost_eval(table, group))
        h = table.cpu().tolist()
        err = 0
        for r in h:
            err |= r[8] & 0xFFFFFFFF
        BinaryMetrics.raise_errors(err)
        return [metric_integer(r, self.eval_metric) for r in h]

    def _weight_stats(self, wd, y, mask, n: int):
        """``(max, min, finite, count)`` of the training rows' effective weights (one host read; no
        training rows: ``(-inf, inf, 1, 0)`` and none), formed on the device by the gradient kernel's
        own float32 product: a rank's part of the shift in a sharded fit (contract item 20)."""
        import torch
        one = torch.ones((), dtype=torch.float32, device=y.device)
        we = torch.where(y[:n] != 0, one * float(np.float32(float(self.scale_pos_weight))), one)
        if wd is not None:
            we = wd[:n] * we
        if mask is not None:
            we = we[mask[:n] != 0]
        if not we.numel():
            return -math.inf, math.inf, 1.0, 0.0
        mx, mn, fin = torch.stack([we.max(), we.min(), torch.isfinite(we).all().to(torch.float32)]).cpu().tolist()
        return mx, mn, fin, float(we.numel())

    def _weight_shift(self, wd, y, mask, n: int) -> int:
        """The quantisation shift e of a weighted fit (contract item 13) -- the fit's one host read
        for it, before the first round."""
        mx, mn, fin, count = self._weight_stats(wd, y, mask, n)
        if not count:
            raise ValueError('no training rows')
        return _check_weight_range(mx, mn, bool(fin))

    def _prepare_sharded(self, data: BinnedData, y_dev, rows, eval_rows, sample_weight, row_keys, group,
                         pending: Optional[Exception]) -> '_Fit':
        """:meth:`_prepare` for a rank of a sharded fit (contract items 20-22).  What can be checked
        on the rank alone is checked first and a failure is kept, not raised; ONE all-gather of a
        small record per rank -- that error flag, the table's rows, the effective weights' range,
        the evaluation rows and their positives, a checksum of the cuts and parameters -- then
        gives every rank the same global figures, and every remaining check is made on those: all
        ranks raise together or none does, before any training launch or level collective."""
        import zlib

        import torch
        import torch.distributed as dist
        dev = data.device if data is not None else y_dev.device if y_dev is not None else _group_device(group)
        n = data.n if data is not None else 0
        err = pending
        y = mask = wd = keys = idx = None
        wstat, weighted, n_pos = (-math.inf, math.inf, 1.0, 0.0), False, 0
        spw, thr = float(self.scale_pos_weight), row_threshold(self.subsample)
        try:
            if err is not None:
                raise err
            if self.eval_metric == 'auc' and (eval_rows is not None or self.early_stopping_rounds is not None):
                raise ValueError("eval_metric='auc' is not available with a process group: the exact pair count "
                                 "needs every rank's minority keys (use 'logloss')")
            y, mask = self._labels_mask(data, y_dev, rows)
            wd = self._device_weights(data, sample_weight, check_host=False)
            weighted = wd is not None or spw != 1.0
            if weighted:
                wstat = self._weight_stats(wd, y, mask, n)
            if row_keys is not None and thr != THR_ALL:
                keys = self._device_keys(data, row_keys)
            if eval_rows is not None:
                idx, n_pos = self._eval_local(data, y, eval_rows)
        except ValueError as e:
            err = e
        cfg = repr((sorted(self.get_params().items()), self.early_stopping_rounds, self.eval_metric, weighted,
                    keys is not None, eval_rows is not None, int(self.record))).encode()
        cuts = data.cuts if data is not None else []
        crc = zlib.crc32(b''.join(np.asarray(c, np.float32).tobytes() + b'|' for c in cuts), zlib.crc32(cfg))
        rec = _gather_records(group, dev, [0.0 if err is None else 1.0, float(n), *wstat,
                                           float(0 if idx is None else idx.numel()), float(n_pos), float(crc)])
        if err is not None:
            raise err
        rank = dist.get_rank(group)
        if rec[:, 0].any():
            raise ValueError(f'sharded fit: rank {int(np.flatnonzero(rec[:, 0])[0])} of the process group refused '
                             f'its arguments (this is rank {rank})')
        if (rec[:, 8] != rec[0, 8]).any():
            raise ValueError('sharded fit: the cuts, the parameters or the kinds of arguments differ between the ranks')
        e = 0
        if weighted:
            if not rec[:, 5].sum():
                raise ValueError('no training rows')
            e = _check_weight_range(float(rec[:, 2].max()), float(rec[:, 3].min()), bool(rec[:, 4].all()))
        ev = None
        if eval_rows is not None:
            total, total_pos = int(rec[:, 6].sum()), int(rec[:, 7].sum())
            if total == 0:
                raise ValueError('binary scores need at least one row')
            if total >= 2 ** 30:
                raise ValueError('binary scores take fewer than 2**30 rows')
            if total_pos == 0 or total_pos == total:
                raise ValueError('Only one class present in y. The AUROC is not defined in that case.')
            ev = self._eval_state(data, y, idx, n_pos, int(self.n_estimators), total, total_pos)
        if keys is None and thr != THR_ALL:  # the default key: the row's index in the concatenated table
            keys = torch.arange(n, dtype=torch.int64, device=dev) + int(rec[:rank, 1].sum())
        f = self._buffers(data, y, mask, wd, e, keys, ev)
        f.group = group
        f.pay = torch.empty(max(_exchange(data)[0].words(2 ** (f.D - 1)), 2), dtype=torch.int64, device=dev)
        return f

    def _labels_mask(self, data: BinnedData, y_dev, rows):
        import torch
        dev, n, ld = data.device, data.n, data.ld
        y = y_dev.view(torch.uint8) if y_dev.dtype == torch.bool else y_dev
        if y.dtype != torch.uint8 or y.numel() < n or y.device != dev:
            raise ValueError('y_dev must be a uint8 / bool device column of at least n rows')
        y = y.contiguous()
        mask = None
        if rows is not None:
            rows = torch.as_tensor(rows, device=dev)
            mask = torch.zeros(ld, dtype=torch.uint8, device=dev)
            if rows.dtype == torch.bool:
                mask[:n] = rows[:n].to(torch.uint8)
            else:
                mask[rows.to(torch.int64)] = 1
        return y, mask

    def _device_weights(self, data: BinnedData, sample_weight, check_host: bool):
        """``sample_weight`` as the float32 device column (None: none given); ``check_host``: a host
        column is validated by :func:`check_weights` before the upload."""
        import torch
        dev, n = data.device, data.n
        if sample_weight is None:
            return None
        if isinstance(sample_weight, torch.Tensor) and sample_weight.device == dev:
            if sample_weight.numel() < n:
                raise ValueError(f'sample_weight has {sample_weight.numel()} entries for {n} rows')
            return sample_weight.reshape(-1).to(torch.float32).contiguous()
        host = sample_weight.numpy() if isinstance(sample_weight, torch.Tensor) else sample_weight
        if check_host:
            host, _ = check_weights(host, n)
        elif len(np.asarray(host).ravel()) != n:
            raise ValueError(f'sample_weight has {len(np.asarray(host).ravel())} entries for {n} rows')
        return weights_to_device(host, dev)

    def _device_keys(self, data: BinnedData, row_keys):
        import torch
        keys = torch.as_tensor(row_keys).reshape(-1).to(data.device).to(torch.int64).contiguous()
        if keys.numel() < data.n:
            raise ValueError(f'row_keys has {keys.numel()} entries for {data.n} rows')
        return keys

    def _prepare(self, data: BinnedData, y_dev, rows, eval_rows, sample_weight, row_keys) -> '_Fit':
        """A fit's state before round 0, in this order: labels, row mask, weights and their shift
        (a weighted fit's one host read), row keys, column samples, buffers, evaluation state (one
        host read).  Every validation error is raised here, before the first training launch."""
        n = data.n
        y, mask = self._labels_mask(data, y_dev, rows)
        spw, thr = float(self.scale_pos_weight), row_threshold(self.subsample)
        wd = self._device_weights(data, sample_weight, check_host=rows is None)
        e = self._weight_shift(wd, y, mask, n) if wd is not None or spw != 1.0 else 0
        keys = self._device_keys(data, row_keys) if row_keys is not None and thr != THR_ALL else None
        f = self._buffers(data, y, mask, wd, e, keys, None)
        if eval_rows is not None:  # before any training launch
            f.ev = self._eval_setup(data, y, eval_rows, f.T)
        return f

    def _buffers(self, data: BinnedData, y, mask, wd, e: int, keys, ev) -> '_Fit':
        """The validated inputs as a fit's state: the :class:`Tuning`, the column samples (None
        unless ``colsample_bytree != 1``) and every device buffer of the rounds."""
        import torch
        dev, ld, F = data.device, data.ld, data.n_features
        T, D = int(self.n_estimators), int(self.max_depth)
        alpha, spw, seed = float(self.reg_alpha), float(self.scale_pos_weight), int(self.random_state)
        thr, colsample = row_threshold(self.subsample), float(self.colsample_bytree)
        columns = ColumnSamples(data, seed, T, colsample) if colsample != 1.0 else None
        tu = Tuning(wd, spw, e, keys, seed, thr, alpha)
        params = (float(self.reg_lambda), float(self.min_child_weight), float(self.gamma), float(self.learning_rate))
        top = 2 ** (D - 1)  # nodes of the deepest level that splits
        rec = lambda: torch.empty((T, ld), dtype=torch.float32, device=dev) if self.record else None  # noqa: E731
        return _Fit(
            data=data, y=y, mask=mask, tu=tu, columns=columns, T=T, D=D, stream=_stream(), params=params,
            margin=torch.full((ld,), float(base_margin(self.base_score)), dtype=torch.float32, device=dev),
            gq=torch.zeros(ld, dtype=torch.int32, device=dev), hq=torch.zeros(ld, dtype=torch.int32, device=dev),
            node=torch.full((ld,), NO_NODE, dtype=torch.uint8, device=dev),
            p=torch.empty(ld, dtype=torch.float32, device=dev), P=rec(), Mrec=rec(),
            trees=torch.zeros((max(T, 1), 2 ** (D + 1) - 1, NODE_DTYPE.itemsize), dtype=torch.uint8, device=dev),
            hist=torch.empty((top, F, 256, 2), dtype=torch.int64, device=dev),
            bg=torch.empty(top * F, dtype=torch.float64, device=dev),
            bc=torch.empty(top * F, dtype=torch.int32, device=dev), ev=ev, group=None, pay=None)

    def _finish(self, f: '_Fit', R: int) -> 'DeviceGBTClassifier':
        """After ``R`` rounds: the evaluation series and the best round, ``margin_`` / ``p_`` of
        the kept trees, the kept trees' one read-back, and the fitted attributes."""
        data, ev, esr, n = f.data, f.ev, self.early_stopping_rounds, f.data.n
        keep = R
        for k in ('evals_result_', 'eval_sums_', 'best_iteration', 'best_score'):
            self.__dict__.pop(k, None)
        if ev is not None:
            series = self._eval_series(ev, R, f.group)
            best, stop = stop_decision(series, esr, self.eval_metric == 'auc')
            assert stop == R, (stop, R)  # every round launched was needed
            self.eval_sums_ = series
            scores = [metric_score(v, self.eval_metric, ev.total, ev.total_pos) for v in series]
            self.evals_result_ = {'validation_0': {self.eval_metric: scores}}
            if series:
                self.best_iteration, self.best_score = best, scores[best]
                if esr is not None:
                    keep = best + 1
        self.n_rounds_run_ = R
        if esr is not None and keep:
            # margin_ / p_ belong to the kept trees: replay them over every row from the base
            # margin (the predictor's walk and its float32 additions, in tree order)
            f.margin.fill_(float(base_margin(self.base_score)))
            for t in range(keep):
                _apply(data, f.trees[t], f.D, None, n, f.margin, f.p if t == keep - 1 else None, self._launch)
        else:
            _grad(self._launch, f.stream, f.margin, None, None, n, None, None, f.p, None)
        M = f.trees.shape[1]
        self.trees_ = f.trees[:keep].cpu().numpy().view(NODE_DTYPE).reshape(keep, M).copy()  # the one read-back
        self.cuts_ = data.cuts
        self.quant_shift_ = f.tu.shift
        self.column_samples_ = None if f.columns is None else f.columns.features[:keep]
        self.feature_names_in_ = np.array(data.names, dtype=object)
        self.n_features_in_ = data.n_features
        self.classes_ = np.array([0, 1])
        self.margin_, self.p_ = f.margin[:n], f.p[:n]
        self.record_ = {'p': f.P[:R, :n], 'margin': f.Mrec[:R, :n]} if f.P is not None else None
        if f.P is not None and ev is not None:
            self.record_['eval_p'] = ev.P[:R]
        self._ensemble = None
        return self

    def fit_binned(self, data: BinnedData, y_dev, rows=None, eval_rows=None, sample_weight=None,
                   row_keys=None, process_group=None, _pending=None) -> 'DeviceGBTClassifier':
        """Fit on binned data and a device label column (uint8 / bool, at least n rows).  The
        whole fit is enqueued on the current stream -- fixed launch sequences per level and per
        round, no host synchronisation -- and the node tables of all trees are read back once.

        ``eval_rows`` (indices or a bool mask; any rows, independent of ``rows``): every round's
        tree is applied to them and scored, still stream-ordered.  With ``early_stopping_rounds``
        the host reads the finished rows of the metric table only when the rule could first
        fire -- after round ``early_stopping_rounds``, then after round ``best + patience`` as
        known at the previous look -- and launches no round after the stopping round.

        ``sample_weight`` (one float32 per row, device or host; the training rows' are used),
        ``scale_pos_weight``, ``reg_alpha``, ``subsample`` and ``colsample_bytree`` (contract items
        13-17) keep the fit bit-identical from run to run: a round's row sample is a counter hash
        of ``(random_state, round, row key)``.  ``row_keys`` (int64, device or host) names the
        rows; with it a sampled fit is also the same for any row order.  The default key is the
        row index, which gives run-to-run identity only: permuting the rows then changes the
        sample.  With every one of these at its neutral value the launches are the unweighted
        fit's and nothing is read from the device before the first round.

        ``process_group`` (a ``torch.distributed`` group; contract items 18-22): every rank passes
        its own shard of the rows -- ``data`` binned with the same cuts (``bin_blocks(...,
        process_group=)``), ``rows`` / ``eval_rows`` / ``sample_weight`` / ``row_keys`` of its own
        table, possibly an empty one -- and the ranks join each level's histogram with ONE int64
        SUM all-reduce of its packed used entries (``sa_boost_hist_pack`` / ``_unpack``).  Every
        rank ends with the same ``trees_``, byte for byte the single-device fit of the ranks' rows
        concatenated in rank order; ``margin_`` / ``p_`` / ``record_`` describe the rank's own rows.
        The evaluation metric is 'logloss' ('auc' raises), summed over the ranks at every look.  A
        ``ValueError`` on one rank is raised on every rank before the first level collective."""
        group = process_group
        if group is None:
            esr = self._check_eval_rows(eval_rows)
            f = self._prepare(data, y_dev, rows, eval_rows, sample_weight, row_keys)
        else:
            try:
                self._check_eval_rows(eval_rows)
            except ValueError as e:
                _pending = _pending or e
            esr = self.early_stopping_rounds
            f = self._prepare_sharded(data, y_dev, rows, eval_rows, sample_weight, row_keys, group, _pending)
        lib, run, st, d, nb = _native.lib(), self._launch, f.stream, data.dev, len(data.bit_feat)
        n, ld, F = data.n, data.ld, data.n_features
        look, R, self.n_polls_ = esr, f.T, 0
        for t in range(f.T):
            tree = f.trees[t]
            cols, fmask = (None, None) if f.columns is None else (f.columns.rounds[t], f.columns.mask[t])
            _grad(run, st, f.margin, f.y, f.mask, n, f.gq, f.hq, f.P[t] if f.P is not None else f.p, f.node,
                  tu=f.tu, t=t)
            for level in range(f.D):
                nn = 2 ** level
                h = f.hist[:nn]
                h.zero_()
                _hist(run, st, data, f.gq, f.hq, f.node, nn, h, tree, level == 0, cols=cols)
                if group is not None:
                    self._exchange_level(f, h, tree, nn, cols)
                _split(run, st, h, d['cut_start'], d['cuts'], F, nn, f.params, f.bg, f.bc, tree, tu=f.tu, fmask=fmask)
                run('advance', lib.sa_boost_advance, tree.data_ptr(), nn - 1, nn, d['fmap'].data_ptr(),
                    data.bits.data_ptr() if nb else None, data.bits.shape[1] * 8 if nb else 0, data.bins.data_ptr(),
                    ld, n, f.node.data_ptr(), None, st)
            _split(run, st, None, None, None, F, 2 ** f.D, f.params, None, None, tree, tu=f.tu, leaf_only=True)
            run('advance', lib.sa_boost_advance, tree.data_ptr(), 0, 1, None, None, 0, None, ld, n,
                f.node.data_ptr(), f.margin.data_ptr(), st)  # the margin
            if f.Mrec is not None:
                f.Mrec[t].copy_(f.margin)
            if f.ev is None:
                continue
            self._eval_round(data, f.ev, tree, t, st)
            if esr is not None and t == look and t + 1 < f.T:  # the rule could first fire here
                self.n_polls_ += 1
                fired, look = stop_look(self._eval_series(f.ev, t + 1, group), esr, self.eval_metric == 'auc')
                if fired:
                    R = t + 1
                    break
        return self._finish(f, R)

    def _exchange_level(self, f: '_Fit', hist, tree, n_nodes: int, cols) -> None:
        """Contract item 18: the level's local histogram (and at level 0 the local root totals)
        packed, summed over the ranks with one int64 all-reduce and unpacked in place -- after it
        every rank holds the global level histogram.  ``cols``: the round's column sample, whose
        bool features are the ones ``sa_boost_hist_bits`` derived a bin 0 for."""
        from . import shard
        pay = hist_pack(f.data, hist, tree, n_nodes, out=f.pay, launch=self._launch)
        self._timed('allreduce', lambda: shard.allreduce_boost_level(pay, f.group))
        bit_feat, nb = (None, None) if cols is None else (cols[1], cols[2])
        hist_unpack(f.data, pay, hist, tree, n_nodes, bit_feat, nb, launch=self._launch)

    def _sharded_bin(self, group, dev, check, bin_fn):
        """The front of a sharded :meth:`fit_blocks` / :meth:`fit`: ``check()`` (the rank's own
        validation) agreed over the ranks, then ``bin_fn()``, whose own ``ValueError`` is kept for
        :meth:`fit_binned`'s agreement.  Returns ``(check's result, data or None, pending error)``."""
        err = out = data = None
        try:
            out = check()
        except ValueError as e:
            err = e
        agree(group, dev, err)
        try:
            data = bin_fn(out)
        except ValueError as e:
            err = e
        return out, data, err

    def fit_blocks(self, blocks, y_dev, rows=None, cuts=None, eval_rows=None, sample_weight=None,
                   row_keys=None, process_group=None) -> 'DeviceGBTClassifier':
        """Fit on device feature blocks (``ops.features(..., bool_bits=True)``) and a device label
        column.  ``rows``: the training rows (indices or a bool mask), default all; ``cuts``:
        explicit cut lists, default :func:`make_cuts` on the training rows; ``eval_rows``: the
        evaluation rows (indices or a bool mask), default none; ``sample_weight`` / ``row_keys``: as
        in :meth:`fit_binned`.  ``process_group``: every rank passes its own blocks (contract items
        18-22); with ``cuts=None`` the cuts come from the ranks' global sample."""
        def check():
            self._check_eval_rows(eval_rows)
            return None if rows is None else _row_list(rows, blocks.n, blocks.device)
        if process_group is not None:
            rows, data, err = self._sharded_bin(process_group, blocks.device, check,
                                                lambda r: bin_blocks(blocks, cuts, r, process_group))
            return self.fit_binned(data, y_dev, rows, eval_rows, sample_weight, row_keys, process_group, err)
        rows = check()
        return self.fit_binned(bin_blocks(blocks, cuts, rows), y_dev, rows, eval_rows, sample_weight, row_keys)

    def fit(self, X, y, cuts=None, eval_set=None, sample_weight=None, row_keys=None,
            process_group=None) -> 'DeviceGBTClassifier':
        """Fit on a host frame or 2-D array: uploaded, binned and trained by the same kernels.
        ``eval_set=[(X_val, y_val)]``: exactly one pair with the same columns; the two frames
        are uploaded as one table whose first ``len(X)`` rows train and whose other rows are the
        evaluation rows (the cuts come from the training rows only).  ``sample_weight`` /
        ``row_keys``: one entry per row of ``X`` (host), validated before anything is uploaded.
        ``process_group``: every rank passes its own frames (contract items 18-22; the weights'
        range is then checked over all ranks, on the device)."""
        group = process_group

        def front():
            self._check_eval_rows(eval_set)
            Xa, w, keys = X, sample_weight, row_keys
            yh = np.asarray(y).astype(bool).astype(np.uint8).ravel()
            n_train = len(yh)
            if w is not None and group is None:
                w, _ = check_weights(w, n_train, yh, self.scale_pos_weight)
            elif w is not None:
                w = np.asarray(w, np.float64).ravel()
                if len(w) != n_train:
                    raise ValueError(f'sample_weight has {len(w)} entries for {n_train} rows')
            if keys is not None:
                keys = check_row_keys(keys, n_train)
            rows = eval_rows = None
            names, cols = _host_columns(Xa)
            if eval_set is not None:
                if len(eval_set) != 1 or len(eval_set[0]) != 2:
                    raise ValueError('eval_set takes exactly one (X_val, y_val) pair')
                vnames, vcols = _host_columns(eval_set[0][0])
                if vnames != names or [_kind(c) for c in vcols] != [_kind(c) for c in cols]:
                    raise ValueError('the evaluation frame must have the training frame\'s columns')
                if cols and len(cols[0]) != n_train:
                    raise ValueError('X and y have different lengths')
                yv = np.asarray(eval_set[0][1]).astype(bool).astype(np.uint8).ravel()
                if vcols and len(vcols[0]) != len(yv):
                    raise ValueError('X_val and y_val have different lengths')
                import pandas as pd
                Xa = pd.DataFrame({c: np.concatenate([a, b]) for c, a, b in zip(names, cols, vcols)}, columns=names)
                yh = np.concatenate([yh, yv])
                rows = np.arange(n_train, dtype=np.int64)
                eval_rows = np.arange(n_train, len(yh), dtype=np.int64)
                if w is not None:  # the evaluation rows are scored unweighted
                    w = np.concatenate([w, np.zeros(len(yv), w.dtype)])
                if keys is not None:
                    keys = np.concatenate([keys, np.zeros(len(yv), np.int64)])
            elif group is not None and cols and len(cols[0]) != n_train:
                raise ValueError('X and y have different lengths')
            return Xa, np.ascontiguousarray(yh), rows, eval_rows, w, keys, n_train

        import torch
        err = None
        if group is None:
            Xa, yh, rows, eval_rows, w, keys, n_train = front()
            data = bin_host(Xa, cuts, rows)
        else:
            dev = torch.device('cuda', torch.cuda.current_device())
            front_out, data, err = self._sharded_bin(group, dev, front,
                                                     lambda v: bin_host(v[0], cuts, v[2], process_group=group))
            Xa, yh, rows, eval_rows, w, keys, n_train = front_out
        if data is not None and len(yh) != data.n:
            raise ValueError('X and y have different lengths')
        yd = None
        if data is not None:
            yd = torch.zeros(data.ld, dtype=torch.uint8, device=data.device)
            yd[:data.n] = torch.from_numpy(yh).to(data.device)
            if w is not None:
                w = weights_to_device(w, data.device)
        if group is None:
            self.fit_binned(data, yd, rows, eval_rows, w, keys)
        else:
            self.fit_binned(data, yd, rows, eval_rows, w, keys, group, err)
        if eval_set is not None:  # the fitted columns are the training frame's
            self.margin_, self.p_ = self.margin_[:n_train], self.p_[:n_train]
            if self.record_ is not None:
                for k in ('p', 'margin'):
                    self.record_[k] = self.record_[k][:, :n_train]
        return self

    # ------------------------------------------------------------------ use
    def _fitted(self) -> None:
        if not hasattr(self, 'trees_'):
            from sklearn.exceptions import NotFittedError
            raise NotFittedError('this DeviceGBTClassifier is not fitted yet')

    def feature_importances(self, importance_type: Optional[str] = None) -> np.ndarray:
        """:func:`importances` of the kept trees (default: ``self.importance_type``)."""
        self._fitted()
        return importances(self.trees_, int(self.n_features_in_), importance_type or self.importance_type,
                           int(getattr(self, 'quant_shift_', 0)))

    @property
    def feature_importances_(self) -> np.ndarray:
        return self.feature_importances()

    def to_xgboost_json(self) -> dict:
        """The kept trees as an xgboost-1.6-shaped model; under early stopping the learner
        ``attributes`` carry ``best_iteration`` and ``best_score`` as strings, as xgboost's do."""
        self._fitted()
        model = trees_to_xgboost_json(self.trees_, list(self.feature_names_in_), float(self.base_score))
        if self.early_stopping_rounds is not None and hasattr(self, 'best_iteration'):
            model['learner']['attributes'] = {'best_iteration': str(int(self.best_iteration)),
                                              'best_score': repr(float(self.best_score))}
        return model

    def predict_proba(self, X) -> np.ndarray:
        """Host ``[n, 2]`` float32 probabilities of a host frame (columns matched by name) or
        array.  The columns are uploaded as feature blocks and walked by the device predictor
        (``TreeEnsemble.predict_blocks``): the same probabilities, bit for bit, as the device
        ``rate`` paths give.  (:func:`predict_tables` is the same walk in numpy.)"""
        self._fitted()
        import torch
        from types import SimpleNamespace

        from .ops import FeatureBlocks
        from .trees import TreeEnsemble
        if hasattr(X, 'columns'):
            missing = [c for c in self.feature_names_in_ if c not in X.columns]
            if missing:
                raise ValueError(f'{" and ".join(missing)} are not available in the features dataframe')
            cols = [X[c].to_numpy() for c in self.feature_names_in_]
        else:
            X = np.asarray(X)
            cols = [X[:, j] for j in range(X.shape[1])]
        if len(cols) != self.n_features_in_:
            raise ValueError(f'X has {len(cols)} features, the model {self.n_features_in_}')
        n = len(cols[0]) if cols else 0
        if n == 0:
            return np.zeros((0, 2), np.float32)
        ld = _ld(n)
        order, per = [], {'b': [], 'f': [], 'i': []}
        for name, c in zip(self.feature_names_in_, cols):
            k = _kind(c)
            order.append((str(name), k, len(per[k])))
            per[k].append(c)
        dts = {'b': np.uint8, 'f': np.float64, 'i': np.int64}
        dev = torch.device('cuda', torch.cuda.current_device())
        blk = {k: torch.from_numpy(_padded_block(per[k], n, ld, dts[k])).to(dev) for k in 'bfi'}
        plan = SimpleNamespace(order=order, names=[o[0] for o in order], n_bool=len(per['b']),
                               n_f64=len(per['f']), n_i64=len(per['i']))
        te = getattr(self, '_ensemble', None)
        if te is None:
            te = self._ensemble = TreeEnsemble.from_xgboost_json(self.to_xgboost_json())
        p1 = te.predict_blocks(FeatureBlocks(plan, n, ld, ld, blk['b'], blk['f'], blk['i']),
                               method='gather').cpu().numpy()
        return np.stack([np.float32(1.0) - p1, p1], 1)

    def predict(self, X) -> np.ndarray:
        return (self.predict_proba(X)[:, 1] > 0.5).astype(np.int64)


class TunedGBTClassifier(DeviceGBTClassifier):
    """:class:`DeviceGBTClassifier` with the tuning parameters of contract items 13-17 beside its
    own: ``subsample=1.0, colsample_bytree=1.0, reg_alpha=0.0, scale_pos_weight=1.0,
    random_state=0`` (xgboost's names and neutral defaults; ``colsample_bylevel`` /
    ``colsample_bynode`` are not built).  It is a class of its own because the plain classifier's
    parameter set is fixed: there ``subsample`` stays an unknown parameter.  With every tuning
    parameter neutral it trains what the plain classifier trains, launch for launch."""

    PARAMS = ALL_DEFAULTS


__all__ = ['DeviceGBTClassifier', 'BinnedData', 'NODE_DTYPE', 'make_cuts', 'cuts_from_sample', 'sample_rows',
           'cast32', 'bin_values', 'bin_blocks', 'bin_host', 'gradients', 'histograms', 'best_splits',
           'trees_to_xgboost_json', 'predict_tables', 'base_margin', 'check_params', 'apply_tree',
           'stop_decision', 'stop_look', 'check_stop_params', 'metric_integer', 'metric_score', 'EVAL_METRICS',
           'fmix64', 'draw', 'row_threshold', 'column_sample', 'weight_shift', 'check_weights', 'importances',
           'IMPORTANCE_TYPES', 'THR_ALL', 'row_keys', 'exchange_layout', 'ExchangeLayout', 'shard_sample_rows',
           'level_histogram', 'hist_pack', 'hist_unpack', 'agree',
           'TunedGBTClassifier', 'TUNING_DEFAULTS', 'ALL_DEFAULTS', 'is_tuned', 'make_classifier']
