"""Boundary models for tests/test_gpu_tree_boundaries.py (a test helper, plain numpy).

Given the host feature matrix ``X`` of a batch (float64, one column per feature) and the kind of
every column ('b' bool, 'f' float64, 'i' int64), :func:`boundary_model` emits an xgboost-shaped
JSON model whose splits sit ON the data -- thresholds are ``float32(x_r)`` of rows of the batch,
their float32 neighbours, +-0.0, integers that occur in an integer column and those +- 0.5, and
{-1, 0, 0.5, 1, 2} on bool columns -- and the same trees as a flat float64 ``x <= thr`` model
(thresholds: the float64 values themselves and their float64 neighbours).  Trees are unbalanced
(leaf depths 1..5 inside every group of 8 trees) and leaf values are multiples of 2^-6 with every
achievable margin within +-4, so a float32 margin sum is exact in any order and one wrong branch
moves the margin by at least 2^-6 (>= 2.8e-4 relative in the probability, as 1 - p >= 0.018).

:func:`model_from_splits` builds a model around a given list of splits (structural cases);
:func:`coverage` counts, from the oracle's rule alone, what a batch exercises in a model.
"""
from __future__ import annotations

import numpy as np

from oracle import tree_oracle as to

F32 = np.float32
LEAF_UNIT = 1.0 / 64.0
MARGIN_MAX = 4.0
BASE_LE = -0.25          # base margin of the float64 `<=` model (the JSON model's is logit(0.5) = 0)
BOOL_THR = (-1.0, 0.0, 0.5, 1.0, 2.0)


class BoundaryModel:
    """``json``: the xgboost-shaped model; ``flat_lt`` / ``flat_le``: its trees as the explicit
    arrays of ``oracle.tree_oracle.predict_flat`` with the float32 `<` / float64 `<=` thresholds;
    ``base_le``: the `<=` model's base margin; ``n_features``."""

    def __init__(self, trees, n_features):
        self.n_features = int(n_features)
        self.base_le = BASE_LE
        self.flat_lt = [self._flat(t, 't32') for t in trees]
        self.flat_le = [self._flat(t, 't64') for t in trees]
        js = []
        for i, f in enumerate(self.flat_lt):
            m = len(f['left'])
            cond = [float(v) for v in f['cond']]
            js.append({'left_children': [int(v) for v in f['left']],
                       'right_children': [int(v) for v in f['right']],
                       'split_indices': [int(v) for v in f['feature']], 'split_conditions': cond,
                       'default_left': [int(v) for v in f['default_left']], 'split_type': [0] * m,
                       'base_weights': cond, 'id': i})
        self.json = {'learner': {
            'objective': {'name': 'binary:logistic'},
            'gradient_booster': {'name': 'gbtree', 'model': {'trees': js, 'tree_info': [0] * len(js)}},
            'learner_model_param': {'base_score': '5E-1', 'num_feature': str(self.n_features),
                                    'num_class': '0'},
            'feature_names': []}, 'version': [1, 6, 2]}
        # every achievable margin within +-4: base + the largest leaf magnitude of every tree
        worst = abs(self.base_le) + sum(float(np.abs(f['cond'][f['left'] < 0]).max()) for f in self.flat_lt)
        assert worst <= MARGIN_MAX, worst
        for f in self.flat_lt:
            leaf = f['cond'][f['left'] < 0].astype(np.float64) / LEAF_UNIT
            assert (leaf == np.round(leaf)).all()
        self.max_margin = worst

    @staticmethod
    def _flat(t, which):
        left, right = np.asarray(t['left'], np.int64), np.asarray(t['right'], np.int64)
        m = len(left)
        feat = np.zeros(m, np.int64)
        dl = np.zeros(m, np.int64)
        cond = np.zeros(m, F32 if which == 't32' else np.float64)
        for k in range(m):
            s = t['spec'][k]
            if s is None:
                cond[k] = t['leaf'][k] * LEAF_UNIT
            else:
                feat[k], dl[k], cond[k] = s['feature'], s['dl'], s[which]
        return {'left': left, 'right': right, 'feature': feat, 'cond': cond, 'default_left': dl}

    @property
    def n_trees(self):
        return len(self.flat_lt)


def ensemble_le(trees_mod, model: BoundaryModel):
    """The flat float64 `<=` trees as a ``TreeEnsemble(..., le=True, f32=False)``."""
    parts, roots, off = [], [], 0
    for f in model.flat_le:
        m = len(f['left'])
        nd = np.zeros(m, trees_mod.NODE_DTYPE)
        leaf = f['left'] < 0
        nd['thr'] = f['cond']
        nd['feature'] = np.where(leaf, -1, f['feature'])
        nd['left'] = np.where(leaf, 0, f['left'] + off)
        r = np.where(leaf, 0, f['right'] + off).astype(np.int64)
        nd['right'] = np.where((f['default_left'] != 0) & ~leaf, r | (1 << 31), r).astype(np.uint32).view(np.int32)
        parts.append(nd)
        roots.append(off)
        off += m
    if parts:
        nodes = np.concatenate(parts)
    else:
        nodes = np.zeros(1, trees_mod.NODE_DTYPE)
        nodes['feature'] = -1
    return trees_mod.TreeEnsemble(nodes, np.asarray(roots, np.int32), model.n_features, None,
                                  float(model.base_le), le=True, f32=False)


# ------------------------------------------------------------------------------ tree shapes
def _grow(rng, depth: int, extra: int):
    """A random unbalanced tree whose longest path has ``depth`` splits: a spine of ``depth``
    splits turning left or right at random, then ``extra`` more splits at random leaves above
    that depth (fewer when no such leaf is left).  Returns (left, right, depth of every node)."""
    left, right, dep = [-1], [-1], [0]

    def split(k):
        a = len(left)
        left.extend([-1, -1])
        right.extend([-1, -1])
        dep.extend([dep[k] + 1] * 2)
        left[k], right[k] = a, a + 1
        return a, a + 1

    k = 0
    for _ in range(depth):
        a, b = split(k)
        k = a if rng.random() < 0.5 else b
    for _ in range(extra):
        cand = [q for q in range(len(left)) if left[q] < 0 and dep[q] < depth]
        if not cand:
            break
        split(cand[int(rng.integers(len(cand)))])
    return left, right, dep


def _leaves(rng, left, right, L: int):
    """Leaf values in units of 2^-6 within +-L; the two leaves of one split differ."""
    m = len(left)
    leaf = np.zeros(m, np.int64)
    for k in range(m):
        if left[k] < 0:
            leaf[k] = int(rng.integers(-L, L + 1))
    for k in range(m):
        if left[k] >= 0 and left[left[k]] < 0 and left[right[k]] < 0 and leaf[left[k]] == leaf[right[k]]:
            leaf[right[k]] = leaf[left[k]] + 1 if leaf[left[k]] < L else leaf[left[k]] - 1
    return leaf


def _leaf_bound(n_trees: int) -> int:
    L = min(32, int((MARGIN_MAX - abs(BASE_LE)) / LEAF_UNIT) // max(n_trees, 1))
    assert L >= 1, 'too many trees for margins within +-4 in units of 2^-6'
    return L


# ------------------------------------------------------------------------------ split choice
class _Columns:
    def __init__(self, X, kinds):
        self.X = X
        self.kinds = list(kinds)
        self.by = {k: [j for j, q in enumerate(kinds) if q == k] for k in 'bfi'}
        self.nan_f = [j for j in self.by['f'] if np.isnan(X[:, j]).any()]
        self.clean_f = [j for j in self.by['f'] if j not in self.nan_f] or self.by['f']
        self.zero_f = [j for j in self.by['f'] if (X[:, j] == 0).any()]


def _f_split(rng, C: _Columns, j: int, rows, variant: str, dl=None):
    col = C.X[:, j]
    fin = rows[np.isfinite(col[rows])]
    if not len(fin):
        fin = np.flatnonzero(np.isfinite(col))
    dl = int(rng.integers(0, 2)) if dl is None else dl
    if variant in ('zero+', 'zero-') and (col == 0).any():
        z = 0.0 if variant == 'zero+' else -0.0
        return {'feature': j, 't32': F32(z), 't64': z, 'dl': dl, 'variant': variant}
    x32 = col[fin].astype(F32).astype(np.float64)
    pool = fin
    if variant == 'tie_up' and (x32 > col[fin]).any():     # float32(x_r) > x_r: a float64 compare
        pool = fin[x32 > col[fin]]                          # of that row against float32(x_r) differs
    elif variant == 'tie_down' and (x32 < col[fin]).any():
        pool = fin[x32 < col[fin]]
    x = float(col[pool[int(rng.integers(len(pool)))]])
    t = F32(x)
    if variant == 'next_up':
        t, x = np.nextafter(t, F32(np.inf)), float(np.nextafter(x, np.inf))
    elif variant == 'next_down':
        t, x = np.nextafter(t, F32(-np.inf)), float(np.nextafter(x, -np.inf))
    return {'feature': j, 't32': F32(t), 't64': x, 'dl': dl, 'variant': variant}


def _i_split(rng, C: _Columns, j: int, rows, variant: str, common: bool = False):
    col = C.X[:, j]
    rows = rows if len(rows) else np.arange(len(col))
    if common:
        vals, cnt = np.unique(col[rows], return_counts=True)
        v = float(vals[np.argmax(cnt)])
    else:
        v = float(col[rows[int(rng.integers(len(rows)))]])
    v += {'exact': 0.0, 'plus': 0.5, 'minus': -0.5}[variant]
    return {'feature': j, 't32': F32(v), 't64': v, 'dl': int(rng.integers(0, 2)), 'variant': 'int_' + variant}


def _b_split(rng, j: int, thr=None):
    t = float(rng.choice(BOOL_THR, p=[0.15, 0.2, 0.3, 0.2, 0.15])) if thr is None else float(thr)
    return {'feature': j, 't32': F32(t), 't64': t, 'dl': int(rng.integers(0, 2)), 'variant': 'bool'}


_F_VARIANTS = ['tie_up', 'tie_down', 'next_up', 'next_down', 'zero+', 'zero-']


def _random_split(rng, C: _Columns, rows):
    present = [k for k in 'fib' if C.by[k]]
    w = np.array([{'f': 0.55, 'i': 0.15, 'b': 0.30}[k] for k in present])
    kind = present[int(rng.choice(len(present), p=w / w.sum()))]
    if kind == 'b':
        return _b_split(rng, int(rng.choice(C.by['b'])))
    if kind == 'i':
        return _i_split(rng, C, int(rng.choice(C.by['i'])), rows,
                        str(rng.choice(['exact', 'plus', 'minus'], p=[0.5, 0.25, 0.25])))
    variant = str(rng.choice(_F_VARIANTS, p=[0.3, 0.3, 0.1, 0.1, 0.1, 0.1]))
    u = rng.random()
    if variant.startswith('zero') and C.zero_f:
        j = int(rng.choice(C.zero_f))
    elif u < 0.4 and C.nan_f:
        j = int(rng.choice(C.nan_f))
    else:
        j = int(rng.choice(C.by['f']))
    return _f_split(rng, C, j, rows, variant)


def _forced_root(rng, C: _Columns, t: int, rows):
    """Roots of the first seven trees, reached by every row: what the coverage floor needs whatever
    the seed (None where the plan has no such column)."""
    if t == 0 and C.clean_f:
        return _f_split(rng, C, int(rng.choice(C.clean_f)), rows, 'tie_up')
    if t in (1, 2) and C.nan_f:
        return _f_split(rng, C, int(rng.choice(C.nan_f)), rows, 'tie_up', dl=2 - t)
    if t == 3 and C.by['i']:
        return _i_split(rng, C, int(rng.choice(C.by['i'])), rows, 'exact', common=True)
    if t == 4 and C.clean_f:  # float64 `<=`: x_r against its lower neighbour, equal in float32
        return _f_split(rng, C, int(rng.choice(C.clean_f)), rows, 'next_down')
    if t in (5, 6) and C.by['b']:
        return _b_split(rng, int(rng.choice(C.by['b'])), 2.0 if t == 5 else -1.0)
    return None


def _goes_left_lt(X, rows, s):
    v = X[rows, s['feature']].astype(F32)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(v), bool(s['dl']), v < s['t32'])


def boundary_model(X: np.ndarray, kinds, n_trees: int, seed: int) -> BoundaryModel:
    """The boundary model of the module docstring: tree t's longest path has 1 + t % 5 splits;
    every split's threshold is drawn from the rows that reach it under xgboost's rule."""
    rng = np.random.default_rng([seed, n_trees])
    C = _Columns(X, kinds)
    L = _leaf_bound(n_trees)
    all_rows = np.arange(X.shape[0])
    trees = []
    for t in range(n_trees):
        depth = 1 + t % 5
        left, right, _ = _grow(rng, depth, int(rng.integers(0, depth)))
        spec = [None] * len(left)
        reach = {0: all_rows}
        for k in range(len(left)):  # children are numbered after their parent
            if left[k] < 0:
                continue
            rows = reach[k] if len(reach[k]) else all_rows
            s = _forced_root(rng, C, t, rows) if k == 0 else None
            spec[k] = s = s or _random_split(rng, C, rows)
            gl = _goes_left_lt(X, reach[k], s)
            reach[left[k]], reach[right[k]] = reach[k][gl], reach[k][~gl]
        trees.append({'left': left, 'right': right, 'spec': spec, 'leaf': _leaves(rng, left, right, L)})
    return BoundaryModel(trees, X.shape[1])


def model_from_splits(splits, n_features: int, seed: int, per_tree: int = 9) -> BoundaryModel:
    """A model whose splits are exactly ``splits`` (dicts of feature, t32, t64, dl), in trees of
    up to ``per_tree`` splits (longest path <= 5) in random unbalanced shapes."""
    rng = np.random.default_rng([seed, len(splits)])
    sizes, left_over = [], len(splits)
    while left_over:
        s = min(left_over, int(rng.integers(max(1, per_tree - 2), per_tree + 1)))
        sizes.append(s)
        left_over -= s
    L = _leaf_bound(len(sizes))
    trees, it = [], iter(splits)
    for s in sizes:
        depth = min(5, s)
        left, right, _ = _grow(rng, depth, s - depth)
        assert sum(v >= 0 for v in left) == s
        spec = [next(it) if left[k] >= 0 else None for k in range(len(left))]
        trees.append({'left': left, 'right': right, 'spec': spec, 'leaf': _leaves(rng, left, right, L)})
    return BoundaryModel(trees, n_features)


def f_splits(X, j: int, count: int, seed: int, dl=None):
    """``count`` splits of float64 column j with distinct float32 thresholds taken from its rows."""
    rng = np.random.default_rng([seed, j, count])
    col = X[:, j]
    vals = np.unique(col[np.isfinite(col)].astype(F32))
    assert len(vals) >= count, (j, len(vals), count)
    out = []
    for t in rng.choice(vals, count, replace=False):
        out.append({'feature': j, 't32': F32(t), 't64': float(t), 'dl': int(rng.integers(0, 2)) if dl is None else dl,
                    'variant': 'tie'})
    return out


def i_splits(X, j: int, count: int, seed: int):
    """``count`` distinct (threshold, default) splits of int64 column j: its values and +- 0.5."""
    rng = np.random.default_rng([seed, j, count])
    vals = np.unique(X[:, j])
    keys = [(float(v) + d, dl) for v in vals for d in (0.0, 0.5, -0.5) for dl in (0, 1)]
    keys = sorted(set(keys))
    assert len(keys) >= count, (j, len(keys), count)
    pick = rng.choice(len(keys), count, replace=False)
    return [{'feature': j, 't32': F32(keys[q][0]), 't64': keys[q][0], 'dl': keys[q][1], 'variant': 'int'}
            for q in pick]


def b_splits(kinds, count: int, seed: int):
    rng = np.random.default_rng([seed, count])
    cols = [j for j, k in enumerate(kinds) if k == 'b']
    return [_b_split(rng, int(rng.choice(cols))) for _ in range(count)]


def shuffled(splits, seed: int):
    rng = np.random.default_rng(seed)
    return [splits[q] for q in rng.permutation(len(splits))]


# ------------------------------------------------------------------------------ coverage
def coverage(flat, X: np.ndarray, kinds, lt: bool, dtype) -> dict:
    """What the rows of X exercise in the flat model under the rule (lt, dtype), from the oracle's
    ``condition_bits`` alone: ``tie_rows`` rows that visit a split with dtype(x) == thr
    (``num_tie_fraction``: the share of rows that do on a numeric column);
    ``f_tie_visits`` such visits on float64 columns; ``disagree_splits`` visited splits where the
    float64 and the float32 compare send a visiting row different ways; ``nan_left`` /
    ``nan_right`` visits of a NaN value by default direction; ``const_left`` / ``const_right``
    visited bool splits that send 0 and 1 the same way."""
    dtype = np.dtype(dtype).type
    n = X.shape[0]
    tie = np.zeros(n, bool)
    num_tie = np.zeros(n, bool)
    out = {'f_tie_visits': 0, 'disagree_splits': 0, 'nan_left': 0, 'nan_right': 0, 'const_left': 0,
           'const_right': 0, 'neg_zero_splits': 0}
    for f in flat:
        reach = {0: np.arange(n)}
        for k in range(len(f['left'])):
            if f['left'][k] < 0:
                continue
            rows = reach[k]  # (children are numbered after their parent)
            if not len(rows):
                reach[int(f['left'][k])] = reach[int(f['right'][k])] = rows
                continue
            j, thr, dl = int(f['feature'][k]), f['cond'][k], bool(f['default_left'][k])
            Xr = X[rows]
            right = to.condition_bits(Xr, j, thr, dl, lt, dtype)
            v = Xr[:, j]
            nan = np.isnan(v)
            eq = (v.astype(dtype) == dtype(thr)) & ~nan
            tie[rows[eq]] = True
            if kinds[j] != 'b':
                num_tie[rows[eq]] = True
            if kinds[j] == 'f':
                out['f_tie_visits'] += int(eq.sum())
            r64 = to.condition_bits(Xr, j, thr, dl, lt, np.float64)
            r32 = to.condition_bits(Xr, j, thr, dl, lt, np.float32)
            out['disagree_splits'] += int((r64 != r32).any())
            out['nan_left'] += int((nan & ~right).sum())
            out['nan_right'] += int((nan & right).sum())
            if kinds[j] == 'b':
                r01 = to.condition_bits(np.array([[0.0], [1.0]]), 0, thr, dl, lt, dtype)
                if r01[0] == r01[1]:
                    out['const_right' if r01[0] else 'const_left'] += 1
            if thr == 0 and np.signbit(thr):
                out['neg_zero_splits'] += 1
            reach[int(f['left'][k])], reach[int(f['right'][k])] = rows[~right], rows[right]
    out['tie_rows'] = int(tie.sum())
    out['tie_fraction'] = float(tie.mean()) if n else 0.0
    out['num_tie_fraction'] = float(num_tie.mean()) if n else 0.0
    return out
