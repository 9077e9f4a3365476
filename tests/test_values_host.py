"""The conditions tests/test_gpu_values.py rests on, asserted without a device: the value batch of
tests/value_cases.py puts every special value in every window under both flip states; a
contracted sum of squares would change its length columns; the oracle's own angles lie within 1
ulp of the 200-bit value; the two new assertions of tests/golden_io.py reject seven plausible
wrong kernels, three of which ``assert_close`` accepts; and the committed goldens were made from
the builders as they are now."""
import numpy as np
import pytest

import threshold_cases as tc
import value_cases as vc
from golden_io import assert_close, assert_same_floats, assert_within_ulps, load
from oracle import vaep_oracle as vo

PACKAGES = [False, True]
K = 3


def _xfns(atomic):
    return vo.ATOMIC_DEFAULT if atomic else vo.SPADL_DEFAULT


_CACHE = {}


def _case(atomic):
    """(batch, windows, {name: oracle column}, {name: exact angle}) at k = 3, computed once."""
    if atomic not in _CACHE:
        d = vc.batch(atomic)
        W = vo.windows(vc.cols_of(d, atomic), K, atomic, d['game_off'], d['home_team_id'])
        ref = {nm: v for nm, kind, v in vo.features_frames(W, _xfns(atomic), atomic, d['game_off'])
               if kind == 'f'}
        _CACHE[atomic] = d, W, ref, vc.exact_angles_frames(W, atomic)
    return _CACHE[atomic]


# ------------------------------------------------------------------------------- the batch
@pytest.mark.parametrize('atomic', PACKAGES)
def test_batch_shape(atomic):
    d = vc.batch(atomic)
    off = d['game_off']
    n = int(off[-1])
    assert n == vc.N_ROWS and n % 2 == 1 and n > 4 * 512 and n > 2 * 1024
    assert len(off) == 6 and (np.diff(off) > 60).all()
    g = np.repeat(np.arange(5), np.diff(off))
    away = d['team_id'] != d['home_team_id'][g]
    for s in range(5):
        teams = d['team_id'][off[s]:off[s + 1]]
        assert len(set(teams.tolist())) == 2
        assert 0.2 < away[off[s]:off[s + 1]].mean() < 0.8
        runs = np.diff(np.flatnonzero(np.diff(teams) != 0))
        assert len(set(runs.tolist())) > 1   # no regular alternation
    assert set(d['period_id'].tolist()) == {1, 2, 3, 4, 5}
    t = d['time_seconds']
    assert ((t * 8) % 1 != 0).mean() > 0.8   # fractional parts that are not dyadic
    ordinary = np.ones(n, bool)
    ordinary[vc.special_rows(atomic).reshape(-1)] = False
    for c, hi in zip(vc.COORDS[atomic][:2], (105, 68)):
        v = d[c][ordinary]
        on_grid = np.round(v, 2) == v
        assert 0.4 < on_grid.mean() < 0.6 and v.min() >= 0 and v.max() <= hi
    if atomic:
        assert 0.4 < (np.round(d['dy'][ordinary], 2) == d['dy'][ordinary]).mean() < 0.6


@pytest.mark.parametrize('atomic', PACKAGES)
def test_every_special_value_in_every_window_under_both_flips(atomic):
    d = vc.batch(atomic)
    off = d['game_off']
    n = int(off[-1])
    g = np.repeat(np.arange(len(off) - 1), np.diff(off))
    away = d['team_id'] != d['home_team_id'][g]
    rows = vc.special_rows(atomic)
    sp = vc.specials(atomic)
    assert rows.shape == (2, len(sp)) and len(sp) > 20
    win = [vo.window_rows(n, off, i) for i in range(K)]
    for s, (vals, why) in enumerate(sp):
        assert why
        seen = set()
        for r in rows[:, s]:
            got = np.array([d[c][r] for c in vc.COORDS[atomic]])
            assert_same_floats(got, np.array(vals, np.float64), why)   # the row holds the value
            for i in range(K):
                assert win[i][r + i] == r, (why, i)   # window i of row r + i is the special row
                seen.add((i, bool(away[r + i])))
            assert not set(rows.reshape(-1).tolist()) & {r + 1, r + 2}  # followed by ordinary rows
            assert d['team_id'][r + 1] != d['team_id'][r + 2]
        assert seen == {(i, f) for i in range(K) for f in (False, True)}, why
    whys = ' '.join(w for _, w in sp)
    for word in ('goal point', 'goal line', 'goal axis', 'beyond', 'one ulp', 'own corner',
                 'overflows', 'subnormal', 'NaN in', '+inf'):
        assert word in whys, word


def test_probabilities_hold_the_edge_values():
    ps, pc = vc.probabilities(vc.N_ROWS, np.float64)
    p32, _ = vc.probabilities(vc.N_ROWS, np.float32)
    assert p32.dtype == np.float32 and (p32 == ps.astype(np.float32)).all()
    for v in (0.0, 1.0, vc.TINY, 1.0 - 2.0 ** -53):
        assert (ps == v).sum() >= 3 and (pc == v).sum() >= 3
    rest = np.r_[ps[:5], ps[17:]]
    assert ((rest * 2.0 ** 32) % 1 != 0).mean() > 0.99   # full-precision doubles


# ------------------------------------------------------------------------------- contraction
def _length_inputs(atomic, W, family):
    """(a, b, column) with column = sqrt(a*a + b*b), window 0 (mov_a0i: window 1 against 0)."""
    a0 = W[0]
    if family in ('start_dist_to_goal', 'end_dist_to_goal', 'dist_to_goal'):
        cx, cy = {'start_dist_to_goal': ('start_x', 'start_y'), 'end_dist_to_goal': ('end_x', 'end_y'),
                  'dist_to_goal': ('x', 'y')}[family]
        return np.abs(105.0 - a0[cx]), np.abs(34.0 - a0[cy]), family + '_a0'
    if family == 'movement':
        return a0['end_x'] - a0['start_x'], a0['end_y'] - a0['start_y'], 'movement_a0'
    if family == 'mov_a0i':
        return W[1]['end_x'] - a0['start_x'], W[1]['end_y'] - a0['start_y'], 'mov_a01'
    return a0['dx'], a0['dy'], 'mov_d_a0'


def _fused_lengths(a, b, col):
    """The column with either fused sum of squares (exact, rounded once) on its finite rows."""
    with np.errstate(invalid='ignore'):
        fin = (np.abs(a) < 1e150) & (np.abs(b) < 1e150)   # NaN compares False
    fa, fb = tc.fused_d2(a[fin], b[fin])
    one, two = col.copy(), col.copy()
    one[fin], two[fin] = np.sqrt(fa), np.sqrt(fb)
    return one, two


@pytest.mark.parametrize('atomic', PACKAGES)
def test_a_fused_sum_of_squares_changes_every_length_column(atomic):
    """-ffp-contract=off is observable: dx*dx + dy*dy fused either way moves at least 50 rows of
    every length column (about 200 are expected; the floor is a condition on the inputs)."""
    _, W, ref, _ = _case(atomic)
    for family in vc.LENGTH_COLUMNS[atomic]:
        a, b, name = _length_inputs(atomic, W, family)
        with np.errstate(invalid='ignore', over='ignore'):
            assert_same_floats(np.sqrt(a * a + b * b), ref[name], name)   # the oracle's own form
        for fused in _fused_lengths(a, b, ref[name]):
            changed = int((fused != ref[name])[~np.isnan(ref[name])].sum())
            print(f'atomic={atomic} {name}: {changed} rows change under a fused sum')
            assert changed >= 50, (name, changed)


# ------------------------------------------------------------------------------- the oracle's angles
@pytest.mark.parametrize('atomic', PACKAGES)
def test_oracle_angles_within_one_ulp_of_exact(atomic):
    """numpy's arctan (at the rounded quotient) and arctan2 within 1 ulp of the 200-bit value on
    every row and window of the batch: what lets a golden stand in for the exact value at
    ANGLE_ULPS + 1."""
    _, _, ref, exact = _case(atomic)
    names = [nm for nm in ref if vc.is_angle(nm)]
    assert len(names) == (2 if atomic else 2) * K and set(names) == set(exact)
    worst = {}
    for nm in names:
        fn = 'arctan2' if nm.startswith('mov_angle') else 'arctan'
        worst[fn] = max(worst.get(fn, 0.0), assert_within_ulps(ref[nm], exact[nm], 1, nm))
    print(f'atomic={atomic} numpy angle maxima (ulps): {worst}')
    assert all(0 < w <= 1 for w in worst.values())


# ------------------------------------------------------------------------------- mutants
def _q(W, i, cx, cy):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.abs(34.0 - W[i][cy]) / np.abs(105.0 - W[i][cx])


def _polar_columns(atomic):
    return [('angle_to_goal', 'dist_to_goal', 'x', 'y')] if atomic else \
        [('start_angle_to_goal', 'start_dist_to_goal', 'start_x', 'start_y'),
         ('end_angle_to_goal', 'end_dist_to_goal', 'end_x', 'end_y')]


def _mutants(atomic):
    """name -> [(column, mutated values, the assertion that must reject it)] on the value batch."""
    _, W, ref, exact = _case(atomic)
    same = lambda nm, v: assert_same_floats(v, ref[nm], nm)                       # noqa: E731
    ulps = lambda nm, v: assert_within_ulps(v, exact[nm], vc.ANGLE_ULPS, nm)      # noqa: E731
    m = {k: [] for k in ('float32 arctan', 'float32 sqrt', 'fused sum of squares',
                         'arctan without nan_to_num', '0.0 for -0.0')}
    with np.errstate(all='ignore'):
        for i in range(K):
            for ang, dist, cx, cy in _polar_columns(atomic):
                q = _q(W, i, cx, cy)
                m['float32 arctan'].append((f'{ang}_a{i}', np.nan_to_num(
                    np.arctan(q.astype(np.float32))).astype(np.float64), ulps))
                m['arctan without nan_to_num'].append((f'{ang}_a{i}', np.arctan(q), ulps))
                dx, dy = np.abs(105.0 - W[i][cx]), np.abs(34.0 - W[i][cy])
                m['float32 sqrt'].append((f'{dist}_a{i}', np.sqrt(
                    (dx * dx + dy * dy).astype(np.float32)).astype(np.float64), same))
        for family in vc.LENGTH_COLUMNS[atomic]:
            a, b, name = _length_inputs(atomic, W, family)
            m['fused sum of squares'].append((name, _fused_lengths(a, b, ref[name])[0], same))
        for nm, v in ref.items():
            if not vc.is_angle(nm) and (np.signbit(v) & (v == 0)).any():
                m['0.0 for -0.0'].append((nm, np.where(v == 0, 0.0, v), same))
        if atomic:
            m['arctan2 without the dy == 0 override'] = [
                (f'mov_angle_a{i}', np.arctan2(W[i]['dy'], W[i]['dx']), ulps) for i in range(K)]
            m['direction dividing when totald == 0'] = []
            for i in range(K):
                td = np.sqrt(W[i]['dx'] ** 2 + W[i]['dy'] ** 2)
                m['direction dividing when totald == 0'] += [
                    (f'dx_a{i}', W[i]['dx'] / td, same), (f'dy_a{i}', W[i]['dy'] / td, same)]
    return m, ref


@pytest.mark.parametrize('atomic', PACKAGES)
def test_the_new_assertions_reject_every_mutant(atomic):
    mutants, ref = _mutants(atomic)
    assert len(mutants) == (7 if atomic else 5)
    for what, columns in mutants.items():
        assert columns, what
        for nm, v, check in columns:   # every affected column, every window
            with pytest.raises(AssertionError):
                check(nm, v)
            assert v.shape == ref[nm].shape and v.dtype == np.float64


@pytest.mark.parametrize('atomic', PACKAGES)
def test_assert_close_accepts_the_float32_and_fused_mutants(atomic):
    """The gap, written down: the old bar passes a kernel that takes arctan or sqrt in float32
    or contracts the sum of squares."""
    mutants, ref = _mutants(atomic)
    for what in ('float32 arctan', 'float32 sqrt', 'fused sum of squares'):
        for nm, v, _ in mutants[what]:
            with np.errstate(invalid='ignore'):   # inf - inf on the overflow rows
                assert_close(v, ref[nm], f'{what} {nm}')


def test_formula_sign_of_zero_is_visible():
    """-(pc - prev_c) is -0.0 on every first row of a segment: 0.0 there passes assert_close and
    fails assert_same_floats, in both dtypes."""
    d = vc.batch(False)
    for dt in (np.float64, np.float32):
        ps, pc = vc.probabilities(vc.N_ROWS, dt)
        fo = vo.formula(vc.cols_of(d, False), ps, pc, seg_off=d['game_off'])
        v = fo['defensive_value']
        assert v.dtype == dt and (np.signbit(v) & (v == 0))[d['game_off'][:-1]].all()
        wrong = np.where(v == 0, dt(0), v)
        assert_close(wrong, v)
        with pytest.raises(AssertionError):
            assert_same_floats(wrong, v)


def test_assertions_on_their_own_edges():
    a = np.array([1.0, np.nan, -0.0, np.inf])
    assert_same_floats(a, a.copy())
    assert_same_floats(a, np.array([1.0, -np.nan, -0.0, np.inf]))   # NaN payload / sign: no matter
    for wrong in (np.array([1.0, np.nan, 0.0, np.inf]), np.array([1.0, 0.0, -0.0, np.inf]),
                  a.astype(np.float32), a[:3], np.array([np.nextafter(1.0, 2), np.nan, -0.0, np.inf])):
        with pytest.raises(AssertionError):
            assert_same_floats(wrong, a)
    one = np.array([1.0])
    up = np.nextafter(one, 2.0)
    assert assert_within_ulps(up, (one, one), 1) == 1.0
    assert assert_within_ulps(up, (one, up), 1) == 1.0   # an upper estimate against a bracket
    with pytest.raises(AssertionError):
        assert_within_ulps(np.nextafter(up, 2.0), (one, one), 1)
    with pytest.raises(AssertionError):
        assert_within_ulps(up, (np.nextafter(one, 0.0), one), 1)   # may be 2 ulps from the value
    with pytest.raises(AssertionError):
        assert_within_ulps(np.array([-0.0]), (np.zeros(1), np.zeros(1)), 4)   # the sign
    with pytest.raises(AssertionError):
        assert_within_ulps(np.array([5e-324]), (np.zeros(1), np.zeros(1)), 4)  # zero is exact
    import mpmath
    with mpmath.workprec(vc.PREC):
        third = np.array([mpmath.mpf(1) / 3], object)
    d = assert_within_ulps(np.array([1 / 3]), third, 1)
    assert 0 < d < 0.5
    # float32: a value a hair above a float32 midpoint may round either way within the bound
    mid = np.array([1.0 + 2.0 ** -24])
    for f in (np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))):
        assert_within_ulps(np.array([f], np.float32), (mid, mid), 1)
    with pytest.raises(AssertionError):
        assert_within_ulps(np.array([1.0 + 2.0 ** -22], np.float32), (mid, mid), 1)


# ------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize('atomic', PACKAGES)
def test_golden_inputs_are_the_builders(atomic):
    """tests/golden/{spadl,atomic}_values.npz were made from golden_game as it is now, and the
    oracle reproduces the reference on every special row: non-angle columns and the formula bit
    for bit, angles within 1 + 1 ulp (both numpy, on any machine)."""
    prefix = 'atomic' if atomic else 'spadl'
    g = load(prefix, 'values')
    df = vc.golden_game(atomic)
    for c in (vc.ATOMIC_COLS if atomic else vc.SPADL_COLS):
        a, b = g['in_' + c], df[c].to_numpy()
        assert a.dtype == b.dtype, c
        (assert_same_floats if a.dtype == np.float64 else np.testing.assert_array_equal)(a, b, c)
    assert int(g['home_team_id'][0]) == vc.GOLDEN_HOME
    cols = {c: df[c].to_numpy() for c in (vc.ATOMIC_COLS if atomic else vc.SPADL_COLS)}
    ref = vo.features(cols, K, _xfns(atomic), atomic=atomic, home=[vc.GOLDEN_HOME])
    assert [c[0] for c in ref] == list(g[f'k{K}_names_all'])
    names = list(g[f'k{K}_names_f'])
    mine = np.stack([v for nm, kind, v in ref if kind == 'f'])
    assert [nm for nm, kind, _ in ref if kind == 'f'] == names
    gold = np.ascontiguousarray(g[f'k{K}_feat_f'].T)
    exact = {nm: (gold[j], gold[j]) for j, nm in enumerate(names) if vc.is_angle(nm)}
    vc.check_float_columns(names, mine, gold, exact, f'{prefix} values golden', bound=2)
    np.testing.assert_array_equal(np.stack([v for _, kind, v in ref if kind == 'i']).T, g[f'k{K}_feat_i'])
    np.testing.assert_array_equal(np.stack([v for _, kind, v in ref if kind == 'b']).T.astype(np.uint8),
                                  g[f'k{K}_feat_b'])
    for tag, dt in (('64', np.float64), ('32', np.float32)):
        fo = vo.formula(cols, g['ps'].astype(dt), g['pc'].astype(dt), atomic=atomic)
        for c in vc.VALUES:
            assert_same_floats(fo[c], g[f'{c}_{tag}'], f'{prefix} values {c} {tag}')
