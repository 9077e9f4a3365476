"""The filtered top-k on the device (sa_top_hist, sa_top_pick, sa_top_tie_count, sa_top_collect,
ops.top_rows) and the layers above it (ratings.top_actions, VAEP / AtomicVAEP / ExpectedThreat
.top_actions).  Every comparison is exact: rows as integers, values through an integer view,
against the numpy restatement of tests/top_rows_reference.py (itself held to the pandas
expression by tests/test_top_rows_host.py)."""
import numpy as np
import pandas as pd
import pytest

import top_rows_reference as tr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

C = tr.CHUNK
DTYPES = pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
LARGEST = pytest.mark.parametrize('largest', [True, False], ids=['largest', 'smallest'])


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, ops
    _native.load_library()
    assert (_native.SA_TOP_CHUNK_ROWS, _native.SA_TOP_MAX_K) == (tr.CHUNK, tr.MAX_K)
    return ops


def aligned(a):
    """A device copy at the allocator's alignment (the vector path, with a scalar tail)."""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(sa, v, k, keep=None, largest=True, dv=None, dkeep=None):
    """ops.top_rows of the host column (or its given device views) against the restatement."""
    dv = aligned(v) if dv is None else dv
    dkeep = (aligned(keep) if keep is not None else None) if dkeep is None else dkeep
    rows, vals = sa.top_rows(dv, k, dkeep, largest)
    want_rows, want_vals = tr.top_rows(v, k, keep, largest)
    assert rows.dtype == torch.int64 and vals.dtype == dv.dtype and rows.is_cuda and vals.is_cuda
    assert rows.cpu().numpy().tolist() == want_rows.tolist()
    assert tr.bits(vals.cpu().numpy()).tolist() == tr.bits(want_vals).tolist()
    return rows, vals


# ----------------------------------------------------------------------------- shapes
@DTYPES
@pytest.mark.parametrize('n', tr.SHAPE_NS)
def test_shapes_with_ties(sa, n, f32):
    """Values from a pool of 17: ties dominate, every k cuts one (but k >= #eligible)."""
    v, keep = tr.pool_column(n, f32)
    dv, dkeep = aligned(v), aligned(keep)
    for k in tr.shape_ks(n):
        check(sa, v, k, None, True, dv=dv)
        check(sa, v, k, keep, True, dv=dv, dkeep=dkeep)
    check(sa, v, min(2, n), keep, False, dv=dv, dkeep=dkeep.bool())  # smallest-first, a bool mask


# ----------------------------------------------------------------------------- special values
@DTYPES
@LARGEST
def test_special_values_at_every_cut(sa, f32, largest):
    """+-0.0, subnormals, +-inf, NaN of both signs and two payloads, +-max and nextafter
    neighbours, k swept over every cut position, those inside the run of zeros included: the
    zeros selected are the lowest-numbered ones whatever their sign, each with its own sign bit."""
    v = tr.special_column(f32)
    dv = aligned(v)
    eligible = int((~np.isnan(v)).sum())
    zero_rows = np.flatnonzero(v == 0)
    seen_partial = False
    for k in range(1, len(v) + 2):
        rows, vals = check(sa, v, k, None, largest, dv=dv)
        assert len(rows) == min(k, eligible)
        h, hv = rows.cpu().numpy(), vals.cpu().numpy()
        z = h[hv == 0]
        assert z.tolist() == zero_rows[:len(z)].tolist()
        assert np.signbit(hv[hv == 0]).tolist() == np.signbit(v[z]).tolist()
        seen_partial |= 0 < len(z) < len(zero_rows)
    assert seen_partial


# ----------------------------------------------------------------------------- all equal
@DTYPES
@pytest.mark.parametrize('k', [5, C + 3])
def test_all_equal_column_takes_the_first_rows(sa, k, f32):
    """Every row ties: rows 0 .. k-1, the second k carrying the tie ranks across a chunk."""
    v = tr.all_equal_column(f32)
    assert len(v) == 3 * C + 1
    rows, _ = check(sa, v, k)
    assert rows.cpu().numpy().tolist() == list(range(k))


# ----------------------------------------------------------------------------- every digit decides
@DTYPES
@LARGEST
def test_the_last_and_the_first_digit_decide(sa, f32, largest):
    from socceraction_amd import _native
    bits = _native.SA_TOP_DIGIT_BITS
    width = 32 if f32 else 64
    last_bits = width - (-(-width // bits) - 1) * bits  # what the last digit holds
    ld = tr.last_digit_column(f32)
    key = tr.order_key(ld)
    assert len(np.unique(key >> key.dtype.type(last_bits))) == 1 and len(np.unique(key)) == len(ld)
    check(sa, ld, len(ld) // 2, None, largest)
    fd = tr.first_digit_column(f32)
    key = tr.order_key(fd)
    low = key & key.dtype.type((1 << (width - bits)) - 1)
    # below the first digit every key of one sign holds the same bits (the negatives' complemented)
    assert len(np.unique(low[fd > 0])) == 1 and len(np.unique(low[fd < 0])) == 1
    assert len(np.unique(key >> key.dtype.type(width - bits))) == len(fd)
    check(sa, fd, len(fd) // 2, None, largest)


# ----------------------------------------------------------------------------- past one resident grid
def test_more_chunks_than_resident_workgroups(sa):
    """n = CUs * SA_TOP_WG_PER_CU * C + 1 float32 rows: workgroup 0 takes a second chunk.  The
    threshold value is in every chunk and the ties needed end in the last chunk (its one row)."""
    from socceraction_amd import _native
    R = _native.SA_TOP_WG_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    n = R * C + 1
    assert n < 2 ** 31 and (n + C - 1) // C == R + 1
    rng = np.random.default_rng(12)
    v = rng.choice(np.array([-0.5, 0.0, 0.125], np.float32), n)
    v[::C] = 0.25                             # the threshold value: the first row of every chunk, the last one's only row
    better = rng.choice(n, 300, replace=False)
    better = better[better % C != 0]
    v[better] = 0.5 + rng.random(len(better)).astype(np.float32)
    k = len(better) + (R + 1)                 # every row above the threshold and every tie
    dv = aligned(v)
    rows, vals = sa.top_rows(dv, k)
    # the restatement, without sorting 8M rows: the rows above 0.25 by value then row, then the ties by row
    order = np.lexsort((better, -v[better]))
    want = np.concatenate([better[order], np.arange(0, n, C)])
    assert len(want) == k and want[-1] == n - 1
    assert rows.cpu().numpy().tolist() == want.tolist()
    assert tr.bits(vals.cpu().numpy()).tolist() == tr.bits(v[want]).tolist()
    # one tie fewer: the last chunk's row stays out
    rows, _ = sa.top_rows(dv, k - 1)
    assert rows.cpu().numpy().tolist() == want[:-1].tolist()


# ----------------------------------------------------------------------------- fewer eligible than k
@DTYPES
def test_fewer_eligible_rows_than_k(sa, f32):
    v, _ = tr.pool_column(C + 1, f32)
    keep = np.zeros(len(v), np.uint8)
    keep[[5, C - 1, C]] = 1
    rows, _ = check(sa, v, 10, keep)
    assert len(rows) == 3
    rows, vals = check(sa, v, 10, np.zeros(len(v), np.uint8))
    assert rows.shape == (0,) and vals.shape == (0,)
    nan = np.full(len(v), np.nan, tr.dtype_of(f32))
    nan[1::2] = -nan[1::2]
    rows, vals = check(sa, nan, 10)
    assert rows.shape == (0,) and vals.shape == (0,)
    rows, vals = sa.top_rows(aligned(v)[:0], 3)  # n = 0: no launch
    assert rows.shape == (0,) and vals.shape == (0,) and vals.dtype == aligned(v).dtype
    for bad in (0, tr.MAX_K + 1):
        with pytest.raises(ValueError):
            sa.top_rows(aligned(v), bad)


# ----------------------------------------------------------------------------- unaligned views
@DTYPES
def test_unaligned_views_give_the_aligned_result(sa, f32):
    """values[1:] / keep[1:]: the scalar path; an aligned copy of the same rows: the vector path
    with a scalar tail (n is odd)."""
    v, keep = tr.pool_column(2 * C + 2, f32)
    dv, dkeep = aligned(v), aligned(keep)
    assert dv.data_ptr() % 16 == 0 and dv[1:].data_ptr() % 16 != 0 and dkeep[1:].data_ptr() % 4 != 0
    for k in (1, 7, C + 3):
        for largest in (True, False):
            check(sa, v[1:], k, keep[1:], largest, dv=dv[1:], dkeep=dkeep[1:])
            check(sa, v[1:], k, keep[1:], largest)                      # aligned copies
            check(sa, v[1:], k, keep[1:], largest, dkeep=dkeep[1:])     # aligned values, unaligned keep
            check(sa, v[1:], k, None, largest, dv=dv[1:])


# ----------------------------------------------------------------------------- determinism
@DTYPES
def test_two_runs_and_a_permutation(sa, f32):
    n = 3 * C + 17
    rng = np.random.default_rng([9, int(f32)])
    v = rng.normal(0, 0.05, n).astype(tr.dtype_of(f32))
    v[rng.random(n) < 0.3] = 0.12  # a heavy tie 2.4 sigma up: a few dozen rows above it, thousands in it
    v[rng.random(n) < 0.05] = np.nan
    keep = (rng.random(n) < 0.7).astype(np.uint8)
    dv, dkeep = aligned(v), aligned(keep)
    first = sa.top_rows(dv, 500, dkeep)
    again = sa.top_rows(dv, 500, dkeep)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1].view(torch.uint8), again[1].view(torch.uint8))
    perm = rng.permutation(n)
    for k in (500, 10):
        rows, vals = sa.top_rows(dv, k, dkeep)
        prow, pvals = sa.top_rows(aligned(v[perm]), k, aligned(keep[perm]))
        assert tr.bits(pvals.cpu().numpy()).tolist() == tr.bits(vals.cpu().numpy()).tolist()
        back = perm[prow.cpu().numpy()]
        hv = vals.cpu().numpy()
        eligible = (keep != 0) & ~np.isnan(v)
        cut = int((eligible & (v == hv[-1])).sum()) != int((hv == hv[-1]).sum())  # is a tie cut at k?
        sure = hv != hv[-1] if cut else np.ones(len(hv), bool)
        assert set(back[sure].tolist()) == set(rows.cpu().numpy()[sure].tolist())
        assert cut == (k == 500)  # both kinds of cut are exercised: the tie is cut at 500, not at 10


# ----------------------------------------------------------------------------- the debug build
def test_the_debug_build_checks_every_index_of_the_new_kernels():
    """The tie-heavy, short and unaligned cases through libsocceraction_amd_debug.so: every call is
    followed by sa_debug_check(), which raises on the first failed SA_DCHECK / SA_DGUARD.  A child
    process, because the library is chosen when socceraction_amd loads."""
    from test_gpu_debug import _run
    out = _run(['-m', 'pytest', '-x', '-q', '-p', 'no:cacheprovider', 'tests/test_gpu_top_rows.py',
                '-k', 'all_equal or fewer_eligible or unaligned or special_values'])
    assert 'passed' in out and 'failed' not in out


# ----------------------------------------------------------------------------- ratings.top_actions
def test_ratings_top_actions_on_the_device(sa):
    from socceraction_amd import ratings
    from test_top_rows_host import notebook_cell, notebook_frame
    actions, values = notebook_frame(5000, seed=4)
    where = (actions.team_name == 'Belgium') & ~actions.type_name.str.contains('shot')
    for w in (where, where.to_numpy(), torch.from_numpy(where.to_numpy()).cuda(), None):
        got = ratings.top_actions(actions, values, k=10, where=w)
        pd.testing.assert_frame_equal(got, notebook_cell(actions, values, 'vaep_value', None if w is None else where, 10))
    got = ratings.top_actions(actions, values.astype(np.float32), k=40, column='defensive_value', largest=False)
    pd.testing.assert_frame_equal(got, notebook_cell(actions, values.astype(np.float32), 'defensive_value', None, 40,
                                                     False))


# ----------------------------------------------------------------------------- model methods
def notebook_where(actions, atomic):
    """One team, no shot types -- the notebook's selection."""
    if atomic:
        from socceraction_amd.atomic.spadl.config import actiontypes
    else:
        from socceraction_amd.spadl.config import actiontypes
    names = pd.Series(np.asarray(actiontypes)[actions.type_id.to_numpy()], index=actions.index)
    where = (actions.team_id == actions.team_id.iloc[0]) & ~names.str.contains('shot')
    assert 0 < where.sum() < len(actions) and names.str.contains('shot').any()
    return where


def check_vaep_top_actions(model, games, actions, atomic):
    from sklearn.exceptions import NotFittedError
    where = notebook_where(actions, atomic)
    rated = pd.concat([actions, model.rate_batch(games, actions)], axis=1)
    for column, largest, w, k in (('vaep_value', True, where, 10), ('offensive_value', False, where.to_numpy(), 7),
                                  ('defensive_value', True, None, 25)):
        got = model.top_actions(games, actions, k=k, column=column, where=w, largest=largest)
        want = rated if w is None else rated.loc[where]
        want = want.dropna(subset=[column]).sort_values(column, ascending=not largest, kind='stable').head(k)
        pd.testing.assert_frame_equal(got, want)
        assert len(got) == k
    with pytest.raises(ValueError):
        model.top_actions(games, actions, column='xT_value')
    fitted = model._VAEP__models
    model._VAEP__models = {}
    with pytest.raises(NotFittedError):
        model.top_actions(games, actions)
    model._VAEP__models = fitted


def test_vaep_top_actions(sa):
    from sklearn.ensemble import HistGradientBoostingClassifier
    from socceraction_amd import synthetic
    import socceraction_amd.vaep as vaep
    d = synthetic.spadl_games(24, seed=27, mean_actions=200.0)
    actions, games = synthetic.to_frame(d), synthetic.games_frame(d)
    model = vaep.VAEP()
    X = model.compute_features_batch(games, actions)
    Y = model.compute_labels_batch(games, actions)
    model._VAEP__models = {c: HistGradientBoostingClassifier(max_iter=10, max_depth=3, random_state=0).fit(X, Y[c])
                           for c in ('scores', 'concedes')}
    assert model._device_models() is not None
    check_vaep_top_actions(model, games, actions, atomic=False)


def test_atomic_vaep_top_actions(sa):
    from sklearn.ensemble import HistGradientBoostingClassifier
    from socceraction_amd import synthetic
    import socceraction_amd.atomic.vaep as avaep
    d = synthetic.atomic_games(24, seed=29, mean_actions=300.0)
    actions, games = synthetic.to_frame(d, atomic=True), synthetic.games_frame(d)
    model = avaep.AtomicVAEP()
    X = model.compute_features_batch(games, actions)
    Y = model.compute_labels_batch(games, actions)
    model._VAEP__models = {c: HistGradientBoostingClassifier(max_iter=10, max_depth=3, random_state=0).fit(X, Y[c])
                           for c in ('scores', 'concedes')}
    assert model._device_models() is not None
    check_vaep_top_actions(model, games, actions, atomic=True)


@pytest.mark.parametrize('interp', [False, True], ids=['grid', 'interpolated'])
def test_xthreat_top_actions(sa, interp):
    from sklearn.exceptions import NotFittedError
    from socceraction_amd import synthetic, xthreat
    if interp and xthreat.interp2d is None:
        pytest.skip('scipy is not installed')
    d = synthetic.spadl_games(24, seed=17, mean_actions=200.0)
    actions = synthetic.to_frame(d)
    model = xthreat.ExpectedThreat(l=16, w=12).fit(actions)
    r = model.rate(actions, use_interpolation=interp)
    assert np.isnan(r).sum() > 100 and (~np.isnan(r)).sum() > 100
    rated = pd.concat([actions, pd.Series(r, name='xT_value', index=actions.index)], axis=1)
    where = notebook_where(actions, atomic=False)
    for largest, w, k in ((True, where, 10), (False, where, 10), (True, None, 33)):
        got = model.top_actions(actions, k=k, use_interpolation=interp, where=w, largest=largest)
        want = rated if w is None else rated.loc[where]
        want = want.dropna(subset=['xT_value']).sort_values('xT_value', ascending=not largest, kind='stable').head(k)
        pd.testing.assert_frame_equal(got, want)
        assert len(got) == k and not got.xT_value.isna().any()
    with pytest.raises(NotFittedError):
        xthreat.ExpectedThreat(l=16, w=12).top_actions(actions)
