"""Order-independent grouped sums on the GPU (sa_group_sums / sa_group_finalize) and the rating
tables built on them (ops.group_sums, ratings.group_sums, VAEP.rate_players,
ExpectedThreat.rate_players).  Comparisons are bit-exact against the Python-integer restatement
of tests/test_ratings_host.py unless a bound is stated."""
import math
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from test_ratings_host import FRAC, py_finalize, py_quantize

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, CHUNK, HASH_MUL = 256, 8192, 2654435761
WG_PER_CU = 4  # the grid's cap: workgroups per compute unit
SIZES = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 5000]
NMAX = 8208  # >= max(SIZES), a multiple of 16: every row of the value block is 16-byte aligned
EXPS = [2, 1, 0, 3, 2, 5, -3, 2]


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, ops
    _native.load_library()
    assert (_native.SA_GROUP_LDS_SLOTS, _native.SA_GROUP_CHUNK_ROWS, _native.SA_GROUP_HASH_MUL) == \
        (SLOTS, CHUNK, HASH_MUL)
    assert _native.SA_GROUP_WG_PER_CU == WG_PER_CU
    return ops


def kernel_hash(key):
    return ((np.asarray(key, np.uint64) * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)


# ----------------------------------------------------------------------------- shared reference
_VALUES = {}


def values(f32: bool):
    """[8, NMAX] host values (column c inside its exponent EXPS[c]) and their Python-integer
    limbs [8, NMAX, 3] (int64; a NaN's limbs are 0), computed once per dtype."""
    if f32 not in _VALUES:
        rng = np.random.default_rng([77, int(f32)])
        v = np.empty((8, NMAX), np.float32 if f32 else np.float64)
        for c, E in enumerate(EXPS):
            x = (rng.beta(0.5, 30, NMAX) - rng.beta(0.5, 60, NMAX)) * 2.0 ** E
            x[rng.random(NMAX) < 0.02] = 0.0
            x[rng.random(NMAX) < 0.02] *= 2.0 ** -70  # far below the column's usual magnitude
            x[rng.random(NMAX) < 0.01] = np.nextafter(2.0 ** E, 0) * 0.999
            x[rng.random(NMAX) < 0.01] = -0.0
            x[rng.random(NMAX) < 0.03] = np.nan
            v[c] = x
        assert all((np.abs(v[c][~np.isnan(v[c])]) < 2.0 ** E).all() for c, E in enumerate(EXPS))
        limbs = np.array([[py_quantize(x, E) for x in v[c].astype(np.float64).tolist()]
                          for c, E in enumerate(EXPS)], np.int64)
        _VALUES[f32] = (v, limbs)
    return _VALUES[f32]


def reference(keys, limbs, V, G, drop=None):
    """Limb sums [G, V, 3] and counts [G] of rows 0..n-1: the Python-integer limbs of each value
    added in int64 (exact: < 2^32 * rows).  ``drop``: rows that add nothing."""
    n = len(keys)
    ok = (keys >= 0) & (keys < G)
    if drop is not None:
        ok &= ~drop
    out = np.zeros((G, V, 3), np.int64)
    for c in range(V):
        for i in range(3):
            np.add.at(out[:, c, i], keys[ok], limbs[c, :n, i][ok])
    return out, np.bincount(keys[ok], minlength=G).astype(np.int64)


def check_finalize(acc, exps):
    """finalize() == the Python-integer rounding of the table's limbs (all groups of a small
    table, the first and last 200 of a large one)."""
    out = acc.finalize().cpu().numpy()
    limbs = acc.limbs.cpu().numpy()
    G = acc.n_groups
    assert out.shape == (acc.n_cols, G) and out.dtype == np.float64
    groups = range(G) if G <= 400 else list(range(200)) + list(range(G - 200, G))
    for c, E in enumerate(exps):
        want = np.array([py_finalize(*limbs[g, c].tolist(), E) for g in groups])
        assert out[c, list(groups)].view(np.int64).tolist() == want.view(np.int64).tolist()


def key_pattern(name: str, n: int, rng):
    if name == 'one_group':
        return np.zeros(n, np.int32), 1
    if name == 'distinct':
        return rng.permutation(n).astype(np.int32), max(n, 1)
    if name == 'identity_slots':
        return rng.integers(0, SLOTS, n).astype(np.int32), SLOTS
    if name == 'hashed_slots':
        return rng.integers(0, SLOTS + 1, n).astype(np.int32), SLOTS + 1
    if name == 'arange':  # hashed, every row a new key: the table fills inside a chunk
        return np.arange(n, dtype=np.int32), n + SLOTS + 1
    if name == 'colliding':  # every key hashes to slot 7
        G = 200000
        pool = np.flatnonzero(kernel_hash(np.arange(G)) == 7)
        assert len(pool) > 300
        return rng.choice(pool[:300], n).astype(np.int32), G
    if name == 'skipped':
        k = rng.integers(0, 40, n).astype(np.int32)
        k[rng.random(n) < 0.2] = -1
        return k, 40
    raise KeyError(name)


PATTERNS = ['one_group', 'distinct', 'identity_slots', 'hashed_slots', 'arange', 'colliding', 'skipped']


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('V', [1, 3, 8])
@pytest.mark.parametrize('pattern', PATTERNS)
def test_small_shapes_equal_the_integer_restatement(sa, pattern, V, f32):
    v, limbs = values(f32)
    dev_v = torch.from_numpy(v).cuda()
    rng = np.random.default_rng([PATTERNS.index(pattern), V, int(f32)])
    for n in SIZES:
        keys, G = key_pattern(pattern, n, rng)
        acc = sa.group_sums(torch.from_numpy(keys).cuda(), [dev_v[c, :n] for c in range(V)], G,
                            scale_exp=EXPS[:V])
        acc.check_errors()
        want_l, want_c = reference(keys, limbs, V, G)
        assert torch.equal(acc.limbs.cpu(), torch.from_numpy(want_l)), (pattern, n)
        assert torch.equal(acc.count.cpu(), torch.from_numpy(want_c)), (pattern, n)
        assert acc.rows == n
        check_finalize(acc, EXPS[:V])


def test_unaligned_columns_take_the_scalar_loads(sa):
    """Columns that do not start on 16 bytes (a slice from row 1) give the same table."""
    v, limbs = values(False)
    n = 5000
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 300, n + 1).astype(np.int32)
    dk = torch.from_numpy(keys).cuda()
    dv = torch.from_numpy(v[:3, :n + 1].copy()).cuda()
    acc = sa.group_sums(dk[1:].clone(), [dv[c, 1:] for c in range(3)], 300, scale_exp=EXPS[:3])
    acc2 = sa.group_sums(dk[1:], [dv[c, 1:].clone() for c in range(3)], 300, scale_exp=EXPS[:3])
    want_l, want_c = reference(keys[1:], limbs[:, 1:], 3, 300)
    for a in (acc, acc2):
        assert torch.equal(a.limbs.cpu(), torch.from_numpy(want_l))
        assert torch.equal(a.count.cpu(), torch.from_numpy(want_c))


# ----------------------------------------------------------------------------- order independence
@pytest.mark.parametrize('G', [40, 3000])
def test_tables_do_not_depend_on_order_chunking_or_shards(sa, G):
    n, V = 3 * CHUNK + 776, 3  # a multiple of 8: the rows of v are 16-byte aligned
    rng = np.random.default_rng([G, 5])
    v = torch.from_numpy((rng.beta(0.5, 30, (V, n)) - rng.beta(0.5, 60, (V, n)))).cuda()
    # game-like keys: consecutive rows share about 22 keys
    keys = ((np.arange(n) // 1600 * 22 + rng.integers(0, 22, n)) % G).astype(np.int32)
    k = torch.from_numpy(keys).cuda()
    E = [1, 1, 1]
    one = sa.group_sums(k, list(v), G, scale_exp=E)
    again = sa.group_sums(k, list(v), G, scale_exp=E)
    assert torch.equal(one.buf, again.buf)  # run to run
    p = torch.from_numpy(rng.permutation(n)).cuda()
    perm = sa.group_sums(k[p].contiguous(), [c[p].contiguous() for c in v], G, scale_exp=E)
    assert torch.equal(one.buf, perm.buf)  # permuted rows
    h = n // 2 + 1  # an odd split: the second half starts off 16-byte alignment
    halves = sa.group_sums(k[:h], [c[:h] for c in v], G, scale_exp=E)
    halves = sa.group_sums(k[h:], [c[h:] for c in v], G, scale_exp=E, acc=halves)
    assert torch.equal(one.buf, halves.buf) and halves.rows == n  # accumulated batches
    cuts = [0, 5000, 5000 + CHUNK + 3, n]
    ranks = [sa.group_sums(k[a:b].clone(), [c[a:b].clone() for c in v], G, scale_exp=E)
             for a, b in zip(cuts, cuts[1:])]
    assert torch.equal(one.buf, ranks[0].buf + ranks[1].buf + ranks[2].buf)  # "rank" shards
    assert torch.equal(one.finalize(), perm.finalize())
    one.check_errors()
    assert int(one.count.sum()) == n


# ----------------------------------------------------------------------------- past the grid cap
PERIOD = 4099  # prime: consecutive chunks start at different offsets of the base table


def past_the_cap_rows():
    """(R, n): the grid's cap in workgroups on this device and a row count just past it --
    workgroups 0 and 1 take a second chunk, the last chunk is partial, n is a multiple of 8."""
    R = WG_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    n = R * CHUNK + CHUNK + 776
    assert n < 2 ** 30, f'{R} resident workgroups put n = {n} past the 2^30 rows a table takes'
    assert n > R * CHUNK and (n + CHUNK - 1) // CHUNK == R + 2 and n % 8 == 0
    return R, n


@pytest.mark.parametrize('G,V,f32', [(40, 3, False), (3000, 3, False), (3000, 1, True)],
                         ids=['identity-V3-f64', 'hashed-V3-f64', 'hashed-V1-f32'])
def test_more_chunks_than_resident_workgroups(sa, G, V, f32):
    """A workgroup that takes a second chunk (c += gridDim.x) after the flush that ends its
    first.  Row i holds row i % PERIOD of the shared value table, so the exact limb sums are
    counts[G, PERIOD] @ limbs[PERIOD, 3V] in int64: counts < 2^12 and |limbs| < 2^32, no overflow.
    A skipped chunk cannot cancel against a doubled one: their offsets into the table differ."""
    R, n = past_the_cap_rows()
    v, limbs = values(f32)
    base, L = v[:V, :PERIOD], limbs[:V, :PERIOD].transpose(1, 0, 2).reshape(PERIOD, 3 * V)
    assert np.isnan(base).any()  # NaN under a valid key: nothing to its column, the row counts
    rng = np.random.default_rng([G, V, int(f32), 11])
    keys = rng.integers(0, G, n).astype(np.int32)
    skip = np.concatenate([rng.integers(1, n, 200), rng.integers(R * CHUNK, n, 150)])
    keys[skip] = -1  # rows that add nothing and raise no error bit
    dv = torch.from_numpy(np.stack([np.resize(base[c], n) for c in range(V)])).cuda()
    late = torch.from_numpy(skip[skip >= R * CHUNK]).cuda()
    assert len(late) >= 150
    dv[:, late] = float('nan')  # ... whatever their values are
    dk = torch.from_numpy(keys).cuda()

    live = np.flatnonzero(keys >= 0)
    assert keys[0] >= 0 and len(live) == n - len(np.unique(skip))
    counts = np.bincount(keys[live].astype(np.int64) * PERIOD + live % PERIOD, minlength=G * PERIOD)
    counts = counts.reshape(G, PERIOD).astype(np.int64)
    assert counts.max() < 2 ** 12 and np.abs(L).max() < 2 ** 32
    want_l, want_c = (counts @ L).reshape(G, V, 3), counts.sum(1)

    acc = sa.group_sums(dk, list(dv), G, scale_exp=EXPS[:V])
    assert int(acc.err.item()) == 0 and acc.rows == n
    assert torch.equal(acc.limbs.cpu(), torch.from_numpy(want_l))
    assert torch.equal(acc.count.cpu(), torch.from_numpy(want_c))
    check_finalize(acc, EXPS[:V])
    # the same columns from row 1: off 16-byte alignment, the scalar loads; row 0 (a live row
    # holding base row 0) leaves the sums
    acc = sa.group_sums(dk[1:], [c[1:] for c in dv], G, scale_exp=EXPS[:V])
    want_l[keys[0]] -= L[0].reshape(V, 3)
    want_c[keys[0]] -= 1
    assert int(acc.err.item()) == 0 and acc.rows == n - 1
    assert torch.equal(acc.limbs.cpu(), torch.from_numpy(want_l))
    assert torch.equal(acc.count.cpu(), torch.from_numpy(want_c))


# ----------------------------------------------------------------------------- exactness
def test_exact_values_sum_to_fsum(sa):
    """Integer multiples of 2^-60 (E = 1) lose nothing to the quantisation: finalize() is the
    correctly rounded exact sum, math.fsum."""
    rng = np.random.default_rng(8)
    n, G = 20000, 37
    j = rng.integers(-(1 << 52), 1 << 52, n) << rng.integers(0, 8, n)  # |j| < 2^60
    v = j.astype(np.float64) * 2.0 ** -60  # exact: 53 significant bits, |v| < 1
    assert (np.abs(v) < 2).all() and (v * 2.0 ** 60 == j).all()
    keys = rng.integers(0, G, n).astype(np.int32)
    acc = sa.group_sums(torch.from_numpy(keys).cuda(), [torch.from_numpy(v).cuda()], G, scale_exp=[1])
    got = acc.finalize().cpu().numpy()[0]
    want = np.array([math.fsum(v[keys == g].tolist()) for g in range(G)])
    assert got.view(np.int64).tolist() == want.view(np.int64).tolist()


def test_vaep_like_values_stay_inside_the_format_bound(sa):
    """300 synthetic games, value = P_scores - P_concedes per action, summed per player:
    |device - fsum| <= count * 2^(E - 95) (one truncation per row) + 2^-53 * |fsum| (the one
    rounding), E = 1."""
    from socceraction_amd import ratings, synthetic
    d = synthetic.spadl_games(300, seed=31)
    frame = synthetic.to_frame(d)
    p = synthetic.probabilities(len(frame))
    v = p['scores'] - p['concedes']
    codes, keys = ratings.factorize(frame, 'player_id')
    G = len(keys)
    acc = sa.group_sums(torch.from_numpy(codes).cuda(), [torch.from_numpy(v).cuda()], G, scale_exp=[1])
    acc.check_errors()
    got = acc.finalize().cpu().numpy()[0]
    count = acc.count.cpu().numpy()
    order = np.argsort(codes, kind='stable')
    bounds = np.searchsorted(codes[order], np.arange(G + 1))
    sv = v[order]
    fs = np.array([math.fsum(sv[a:b].tolist()) for a, b in zip(bounds, bounds[1:])])
    assert (count == np.diff(bounds)).all() and G > 6000
    err = np.abs(got - fs)
    bound = count * 2.0 ** (1 - FRAC) + 2.0 ** -53 * np.abs(fs)
    print('max |device - fsum| =', err.max(), 'groups equal to fsum:', int((got == fs).sum()), 'of', G)
    assert (err <= bound).all()


# ----------------------------------------------------------------------------- errors
def test_error_bits_raise_and_their_rows_add_nothing(sa):
    v, limbs = values(False)
    n, G, V = 3000, 50, 3
    rng = np.random.default_rng(6)
    keys0 = rng.integers(0, G, n).astype(np.int32)
    dv0 = torch.from_numpy(v[:V, :n].copy())
    bit = {'key >= G': 1, 'key < -1': 1, '+inf': 2, 'value == 2^E': 4}
    for what, rows in (('key >= G', [5, 1500]), ('key < -1', [77]), ('+inf', [0, 2999]),
                       ('value == 2^E', [1234])):
        keys, dv = keys0.copy(), dv0.clone()
        if what == 'key >= G':
            keys[rows] = [G, 2 ** 31 - 1]
        elif what == 'key < -1':
            keys[rows] = -2
        elif what == '+inf':
            dv[1, rows[0]] = float('inf')
            dv[2, rows[1]] = float('-inf')
        else:
            dv[0, rows] = 2.0 ** EXPS[0]
        acc = sa.group_sums(torch.from_numpy(keys).cuda(), list(dv.cuda()), G, scale_exp=EXPS[:V])
        assert int(acc.err.item()) == bit[what], what
        with pytest.raises(ValueError):
            acc.check_errors()
        drop = np.zeros(n, bool)
        drop[rows] = True
        want_l, want_c = reference(keys0, limbs, V, G, drop=drop)  # the whole row adds nothing
        assert torch.equal(acc.limbs.cpu(), torch.from_numpy(want_l)), what
        assert torch.equal(acc.count.cpu(), torch.from_numpy(want_c)), what
    # NaN: skipped in its column, the row still counts
    nan_rows = np.isnan(v[:V, :n]).any(axis=0)
    acc = sa.group_sums(torch.from_numpy(keys0).cuda(), list(dv0.cuda()), G, scale_exp=EXPS[:V])
    acc.check_errors()
    assert nan_rows.sum() > 50 and int(acc.count.sum()) == n
    # a later batch that overflows the table's scale: raised before the launch when the scale is
    # left to the call, flagged by the kernel when the caller insists on it
    big = [c * 64 for c in dv0.cuda()]
    with pytest.raises(ValueError, match='scale_exp'):
        sa.group_sums(torch.from_numpy(keys0).cuda(), big, G, acc=acc)
    sa.group_sums(torch.from_numpy(keys0).cuda(), big, G, scale_exp=EXPS[:V], acc=acc)
    with pytest.raises(ValueError, match='scale_exp'):
        acc.check_errors()


def test_auto_scale_takes_the_largest_finite_magnitude(sa):
    k = torch.zeros(6, dtype=torch.int32).cuda()
    c0 = torch.tensor([0.3, -0.9, float('nan'), 0.0, 0.99, 0.5], dtype=torch.float64).cuda()
    c1 = torch.tensor([1.0, -5.0, 2.0, 0.0, 7.99, 8.0], dtype=torch.float64).cuda()
    c2 = torch.zeros(6, dtype=torch.float64).cuda()
    acc = sa.group_sums(k, [c0, c1, c2], 1)
    assert acc.scale_exp == (0, 4, 0)  # 0.99 < 2^0, 8.0 < 2^4
    acc.check_errors()
    assert acc.finalize().cpu().numpy()[:, 0].tolist() == \
        [math.fsum([0.3, -0.9, 0.0, 0.99, 0.5]), math.fsum([1.0, -5.0, 2.0, 0.0, 7.99, 8.0]), 0.0]
    assert int(acc.count.item()) == 6


# ----------------------------------------------------------------------------- drop-in
@pytest.fixture(scope='module')
def games40():
    from socceraction_amd import synthetic
    d = synthetic.spadl_games(40, seed=13)
    frame = synthetic.to_frame(d)
    p = synthetic.probabilities(len(frame), seed=3)
    q = synthetic.probabilities(len(frame), seed=4)
    vals = pd.DataFrame({'offensive_value': p['scores'] - q['scores'],
                         'defensive_value': q['concedes'] - p['concedes']})
    vals['vaep_value'] = vals.offensive_value + vals.defensive_value
    return d, frame, vals


@pytest.mark.parametrize('case', ['player_id', 'game_player', 'type_id', 'nan_player'])
def test_ratings_group_sums_equals_pandas_groupby(sa, games40, case):
    """ratings.group_sums == frame.groupby(by).sum().reset_index(): groups, order, key dtypes
    and count exactly; float columns within (count + 3) * 2^-53 * sum|v| (the bound a Kahan or a
    plain sequential float64 sum keeps)."""
    from socceraction_amd import ratings
    d, frame, vals = games40
    by = {'player_id': 'player_id', 'game_player': ['game_id', 'player_id'], 'type_id': 'type_id',
          'nan_player': 'player_id'}[case]
    actions = frame
    if case == 'nan_player':
        actions = frame.copy()
        actions['player_id'] = actions['player_id'].astype(np.float64)
        actions.loc[np.random.default_rng(2).random(len(frame)) < 0.05, 'player_id'] = np.nan
    names = [by] if isinstance(by, str) else by
    got = ratings.group_sums(actions, vals, by)
    full = pd.concat([actions[names], vals], axis=1).assign(count=1)
    ref = full.groupby(by).sum().reset_index()
    mag = pd.concat([actions[names], vals.abs()], axis=1).groupby(by).sum().reset_index()
    assert list(got.columns) == list(ref.columns)
    pd.testing.assert_frame_equal(got[names + ['count']], ref[names + ['count']], check_exact=True)
    for c in vals.columns:
        err = np.abs(got[c].to_numpy() - ref[c].to_numpy())
        bound = (ref['count'].to_numpy() + 3) * 2.0 ** -53 * mag[c].to_numpy()
        print(case, c, 'max err / bound =', float((err / np.maximum(bound, 1e-300)).max()))
        assert got[c].dtype == np.float64 and (err <= bound).all(), c


def test_ratings_group_sums_with_a_vocabulary(sa, games40):
    """groups=: the same table when the vocabulary is a superset of the observed keys."""
    from socceraction_amd import ratings
    d, frame, vals = games40
    ref = ratings.group_sums(frame, vals, 'player_id', scale_exp=(1, 1, 1))
    vocab = np.concatenate([frame.player_id.unique(), [10 ** 9, -5]])
    got = ratings.group_sums(frame, vals, 'player_id', groups=vocab, scale_exp=(1, 1, 1))
    pd.testing.assert_frame_equal(got, ref, check_exact=True)


def test_ratings_group_sums_of_no_rows(sa, games40):
    from socceraction_amd import ratings
    d, frame, vals = games40
    for groups in (None, [1, 2, 3]):
        got = ratings.group_sums(frame.iloc[:0], vals.iloc[:0], 'player_id', groups=groups)
        assert len(got) == 0 and list(got.columns) == ['player_id'] + list(vals.columns) + ['count']
    nokey = frame.iloc[:50].assign(player_id=np.nan)
    assert len(ratings.group_sums(nokey, vals.iloc[:50], 'player_id')) == 0


def _bits_equal(a: pd.DataFrame, b: pd.DataFrame):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        assert a[c].dtype == b[c].dtype, c
        x, y = a[c].to_numpy(), b[c].to_numpy()
        if x.dtype.kind == 'f':
            x, y = x.view(np.int64), y.view(np.int64)
        assert (x == y).all(), c


@pytest.fixture(scope='module')
def fitted():
    from socceraction_amd import synthetic
    import socceraction_amd.vaep as vaep
    d = synthetic.spadl_games(6, seed=21)
    actions = synthetic.to_frame(d)
    games = synthetic.games_frame(d)
    model = vaep.VAEP()
    X = model.compute_features_batch(games, actions)
    Y = model.compute_labels_batch(games, actions)
    return model, games, actions, X, Y


@pytest.mark.parametrize('learner', ['sklearn_hgb', 'xgboost_format', 'host_fallback'])
def test_vaep_rate_players(sa, fitted, learner):
    """rate_players == ratings.group_sums(actions, rate_batch(...)) at the same scale (E = 2),
    bit for bit: HistGradientBoosting pair (f64), xgboost-format pair (f32 columns), and a
    learner the device does not evaluate (host predict_proba, the same kernel)."""
    from socceraction_amd import ratings, trees
    model, games, actions, X, Y = fitted
    if learner == 'sklearn_hgb':
        from sklearn.ensemble import HistGradientBoostingClassifier
        models = {c: HistGradientBoostingClassifier(max_iter=20, max_depth=3, random_state=0).fit(X, Y[c])
                  for c in ('scores', 'concedes')}
    elif learner == 'xgboost_format':
        kinds = ['f'] * X.shape[1]
        models = {c: trees.synthetic_xgboost_json(X.shape[1], n_trees=20, seed=s, feature_kinds=kinds)
                  for s, c in enumerate(('scores', 'concedes'))}
    else:
        from sklearn.tree import DecisionTreeClassifier
        models = {c: DecisionTreeClassifier(max_depth=4, random_state=0).fit(X, Y[c])
                  for c in ('scores', 'concedes')}
    model._VAEP__models = models
    assert (model._device_models() is None) == (learner == 'host_fallback')
    values = model.rate_batch(games, actions)
    assert values['vaep_value'].dtype == (np.float32 if learner == 'xgboost_format' else np.float64)
    for by in ('player_id', ['game_id', 'player_id']):
        got = model.rate_players(games, actions, by=by)
        want = ratings.group_sums(actions, values, by, scale_exp=(2, 2, 2))
        _bits_equal(got, want)
        assert int(got['count'].sum()) == len(actions)
    ref = pd.concat([actions[['player_id']], values.astype(np.float64)], axis=1).groupby('player_id').sum()
    got = model.rate_players(games, actions)
    np.testing.assert_allclose(got['vaep_value'].to_numpy(), ref['vaep_value'].to_numpy(), rtol=0,
                               atol=1e-12 if learner != 'xgboost_format' else 1e-4)


def test_atomic_vaep_rate_players(sa):
    """AtomicVAEP.rate_players on atomic actions: the same identity, device learners."""
    from sklearn.ensemble import HistGradientBoostingClassifier
    from socceraction_amd import ratings, synthetic
    import socceraction_amd.atomic.vaep as avaep
    d = synthetic.atomic_games(3, seed=23)
    actions = synthetic.to_frame(d, atomic=True)
    games = synthetic.games_frame(d)
    model = avaep.AtomicVAEP()
    X = model.compute_features_batch(games, actions)
    Y = model.compute_labels_batch(games, actions)
    model._VAEP__models = {c: HistGradientBoostingClassifier(max_iter=10, max_depth=3, random_state=0)
                           .fit(X, Y[c]) for c in ('scores', 'concedes')}
    assert model._device_models() is not None
    got = model.rate_players(games, actions)
    want = ratings.group_sums(actions, model.rate_batch(games, actions), 'player_id', scale_exp=(2, 2, 2))
    _bits_equal(got, want)
    assert int(got['count'].sum()) == len(actions)


@pytest.mark.parametrize('interp', [False, True], ids=['grid', 'interpolated'])
def test_xthreat_rate_players(sa, interp):
    """ExpectedThreat.rate_players == ratings.group_sums(actions, rate(...)) at E = 1, bit for
    bit; non-move actions rate NaN, add nothing and still count."""
    from socceraction_amd import ratings, synthetic, xthreat
    if interp and xthreat.interp2d is None:
        pytest.skip('scipy is not installed')
    d = synthetic.spadl_games(8, seed=17)
    actions = synthetic.to_frame(d)
    model = xthreat.ExpectedThreat(l=16, w=12).fit(actions)
    r = model.rate(actions, use_interpolation=interp)
    assert np.isnan(r).sum() > 1000 and (~np.isnan(r)).sum() > 1000
    for by in ('player_id', ['game_id', 'player_id']):
        got = model.rate_players(actions, by=by, use_interpolation=interp)
        want = ratings.group_sums(actions, pd.Series(r, name='xT_value'), by, scale_exp=(1,))
        _bits_equal(got, want)
        assert int(got['count'].sum()) == len(actions)
    ref = pd.DataFrame({'player_id': actions.player_id, 'xT_value': r}).groupby('player_id').sum()
    nokey = actions.iloc[:50].assign(player_id=np.nan)  # every key NaN: the empty table
    empty = model.rate_players(nokey, use_interpolation=interp)
    assert len(empty) == 0 and list(empty.columns) == ['player_id', 'xT_value', 'count']
    np.testing.assert_allclose(model.rate_players(actions, use_interpolation=interp)['xT_value'].to_numpy(),
                               ref['xT_value'].to_numpy(), rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------- debug build
def test_golden_sized_case(sa):
    """One game's worth of rows, identity and hashed slots (also run through the debug build)."""
    v, limbs = values(False)
    n, V = 1700, 3
    rng = np.random.default_rng(9)
    for G in (28, 700):
        keys = rng.integers(-1, G, n).astype(np.int32)
        acc = sa.group_sums(torch.from_numpy(keys).cuda(), list(torch.from_numpy(v[:V, :n].copy()).cuda()), G,
                            scale_exp=EXPS[:V])
        acc.check_errors()
        want_l, want_c = reference(keys, limbs, V, G)
        assert torch.equal(acc.limbs.cpu(), torch.from_numpy(want_l))
        assert torch.equal(acc.count.cpu(), torch.from_numpy(want_c))
        check_finalize(acc, EXPS[:V])


def test_golden_sized_case_through_the_debug_build():
    """The same case with the device bounds checks compiled in and sa_debug_check() after every
    call (a child process: the library is chosen when socceraction_amd loads)."""
    path = [ROOT, os.path.join(ROOT, 'tests')] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]
    env = dict(os.environ, SOCCERACTION_AMD_DEBUG='1', PYTHONPATH=os.pathsep.join(path))
    check = ('import sys, pytest\n'
             'from socceraction_amd import _native\n'
             'assert _native.lib().sa_debug_enabled() == 1\n'
             'sys.exit(pytest.main(["-x", "-q", "-p", "no:cacheprovider", "tests/test_gpu_ratings.py", '
             '"-k", "test_golden_sized_case and not debug"]))\n')
    p = subprocess.run([sys.executable, '-c', check], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert '1 passed' in p.stdout
