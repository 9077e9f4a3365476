"""The filtered top-k without a GPU: the numpy restatement (top_rows_reference) against the
pandas expression that defines it, ratings.top_actions' host path against the notebook cell, and
the C entry points' argument checks (before any HIP call)."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

import top_rows_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
LARGEST = pytest.mark.parametrize('largest', [True, False], ids=['largest', 'smallest'])


def test_constants_mirror_the_header():
    from socceraction_amd import _native
    assert (_native.SA_TOP_CHUNK_ROWS, _native.SA_TOP_MAX_K) == (tr.CHUNK, tr.MAX_K)
    assert _native.SA_TOP_DIGIT_BITS in (11, 12) and _native.SA_TOP_WG_PER_CU >= 1
    with open(os.path.join(ROOT, 'include', 'socceraction_amd.h')) as f:
        src = f.read()
    for name in ('SA_TOP_CHUNK_ROWS', 'SA_TOP_WG_PER_CU', 'SA_TOP_DIGIT_BITS', 'SA_TOP_MAX_K', 'SA_TOP_STATE_WORDS'):
        assert f'#define {name} {getattr(_native, name)}\n' in src, name
    lib = _native.load_library()
    bits = _native.SA_TOP_DIGIT_BITS
    assert lib.sa_top_passes(1) == -(-32 // bits) and lib.sa_top_passes(0) == -(-64 // bits)


@DTYPES
@LARGEST
def test_restatement_equals_the_pandas_expression(f32, largest):
    for name, v, keep, ks in tr.host_cases(f32):
        for k in ks:
            rows, vals = tr.top_rows(v, k, keep, largest)
            want_rows, want_vals = tr.pandas_top_rows(v, k, keep, largest)
            assert rows.tolist() == want_rows.tolist(), (name, k)
            assert tr.bits(vals).tolist() == tr.bits(want_vals).tolist(), (name, k)


@DTYPES
def test_special_column_orders_as_the_contract_says(f32):
    """What the pandas comparison cannot say on its own: NaN of either sign is never returned,
    the zeros tie whatever their sign and come back with their own sign bit."""
    v = tr.special_column(f32)
    rows, vals = tr.top_rows(v, len(v), None, True)
    assert len(rows) == int((~np.isnan(v)).sum()) and not np.isnan(vals).any()
    zeros = rows[vals == 0]
    assert zeros.tolist() == np.flatnonzero(v == 0).tolist()
    assert np.signbit(vals[vals == 0]).tolist() == np.signbit(v[v == 0]).tolist()
    assert vals[0] == np.inf and vals[-1] == -np.inf
    assert (np.diff(vals.astype(np.float64)) <= 0).all()
    key = tr.order_key(v[~np.isnan(v)])
    a = v[~np.isnan(v)].astype(np.float64)
    assert ((key[:, None] < key[None, :]) == (a[:, None] < a[None, :])).all()


# ----------------------------------------------------------------------------- ratings.top_actions
def notebook_frame(n=500, seed=3):
    rng = np.random.default_rng(seed)
    actions = pd.DataFrame({
        'game_id': np.repeat(np.arange(5), n // 5),
        'team_name': rng.choice(['Belgium', 'Brazil', 'Japan'], n),
        'type_name': rng.choice(['pass', 'shot', 'dribble', 'shot_penalty', 'cross'], n),
        'player_id': rng.integers(1, 40, n)}, index=pd.RangeIndex(100, 100 + n))
    vaep = np.round(rng.normal(0, 0.02, n), 3)  # rounded: ties
    vaep[rng.random(n) < 0.05] = np.nan
    vaep[7], vaep[9] = 0.0, -0.0
    values = pd.DataFrame({'offensive_value': rng.normal(0, 0.01, n), 'defensive_value': rng.normal(0, 0.01, n),
                           'vaep_value': vaep}, index=actions.index)
    return actions, values


def notebook_cell(actions, values, column, where, k, largest=True):
    A = pd.concat([actions, values], axis=1)
    if where is not None:
        A = A.loc[where]
    return A.dropna(subset=[column]).sort_values(column, ascending=not largest, kind='stable').head(k)


def test_ratings_top_actions_equals_the_notebook_cell():
    """Without a ROCm device this is the numpy path; with one, the upload and ops.top_rows."""
    from socceraction_amd import ratings
    actions, values = notebook_frame()
    where = (actions.team_name == 'Belgium') & ~actions.type_name.str.contains('shot')
    for k in (1, 10, 100, 1000):
        got = ratings.top_actions(actions, values, k=k, where=where)
        pd.testing.assert_frame_equal(got, notebook_cell(actions, values, 'vaep_value', where, k))
    got = ratings.top_actions(actions, values, k=10, column='offensive_value', where=where.to_numpy(), largest=False)
    pd.testing.assert_frame_equal(got, notebook_cell(actions, values, 'offensive_value', where, 10, False))
    got = ratings.top_actions(actions, values['vaep_value'], k=25)
    pd.testing.assert_frame_equal(got, notebook_cell(actions, values[['vaep_value']], 'vaep_value', None, 25))
    none = ratings.top_actions(actions, values, k=10, where=np.zeros(len(actions), bool))
    assert len(none) == 0 and list(none.columns) == list(actions.columns) + list(values.columns)
    empty = ratings.top_actions(actions.iloc[:0], values.iloc[:0], k=3)
    assert len(empty) == 0
    with pytest.raises(ValueError):
        ratings.top_actions(actions, values, k=0)
    with pytest.raises(ValueError):
        ratings.top_actions(actions, values, k=10, column='no_such_value')
    with pytest.raises(ValueError):
        ratings.top_actions(actions, values, k=10, where=where.iloc[:-1])
    with pytest.raises(ValueError):
        ratings.top_actions(actions, values.iloc[:-1], k=10)


@DTYPES
@LARGEST
def test_host_rows_equal_the_restatement(f32, largest):
    """ratings.top_rows_host (what top_actions runs without a device) on every case builder."""
    from socceraction_amd import ratings
    for name, v, keep, ks in tr.host_cases(f32):
        for k in ks:
            got = ratings.top_rows_host(v, k, keep, largest)
            assert got.tolist() == tr.top_rows(v, k, keep, largest)[0].tolist(), (name, k)


# ----------------------------------------------------------------------------- the C entry points
def test_top_entry_points_reject_bad_arguments_without_a_gpu():
    from socceraction_amd import _native
    lib = _native.load_library()
    fake = ctypes.c_void_p(256)  # never dereferenced on the host
    EINVAL, MAX_K = _native.SA_EINVAL, _native.SA_TOP_MAX_K

    def rejected(rc, word):
        assert rc == EINVAL, word
        assert word in lib.sa_last_error(), (word, lib.sa_last_error())
        with pytest.raises(ValueError):
            _native.check(rc)

    for f32 in (0, 1):
        passes = lib.sa_top_passes(f32)
        # k = 0, k > SA_TOP_MAX_K
        for k in (0, -1, MAX_K + 1):
            rejected(lib.sa_top_pick(f32, k, 0, fake, fake, None), b'k must be')
            rejected(lib.sa_top_collect(fake, f32, fake, 10, 1, k, fake, fake, fake, None), b'k must be')
        # n < 0, n >= 2^31
        for n in (-1, 2 ** 31):
            word = b'n < 0' if n < 0 else b'2^31'
            rejected(lib.sa_top_hist(fake, f32, fake, n, 1, 0, fake, fake, None), word)
            rejected(lib.sa_top_tie_count(fake, f32, fake, n, 1, fake, fake, None), word)
            rejected(lib.sa_top_collect(fake, f32, fake, n, 1, 10, fake, fake, fake, None), word)
        # null outputs (and inputs)
        rejected(lib.sa_top_hist(fake, f32, None, 10, 1, 0, fake, None, None), b'null')
        rejected(lib.sa_top_hist(fake, f32, None, 10, 1, 0, None, fake, None), b'null')
        rejected(lib.sa_top_hist(None, f32, None, 10, 1, 0, fake, fake, None), b'null')
        rejected(lib.sa_top_pick(f32, 10, 0, None, fake, None), b'null')
        rejected(lib.sa_top_pick(f32, 10, 0, fake, None, None), b'null')
        rejected(lib.sa_top_tie_count(fake, f32, None, 10, 1, fake, None, None), b'null')
        rejected(lib.sa_top_tie_count(fake, f32, None, 10, 1, None, fake, None), b'null')
        rejected(lib.sa_top_collect(fake, f32, None, 10, 1, 10, fake, fake, None, None), b'null')
        rejected(lib.sa_top_collect(fake, f32, None, 10, 1, 10, fake, None, fake, None), b'null')
        rejected(lib.sa_top_collect(fake, f32, None, 10, 1, 10, None, fake, fake, None), b'null')
        # a digit the key does not have
        for p in (-1, passes):
            rejected(lib.sa_top_hist(fake, f32, None, 10, 1, p, fake, fake, None), b'pass')
            rejected(lib.sa_top_pick(f32, 10, p, fake, fake, None), b'pass')
        # n = 0 launches nothing
        assert lib.sa_top_hist(None, f32, None, 0, 1, 0, fake, fake, None) == _native.SA_OK
        assert lib.sa_top_tie_count(None, f32, None, 0, 1, fake, fake, None) == _native.SA_OK
        assert lib.sa_top_collect(None, f32, None, 0, 1, 10, fake, fake, fake, None) == _native.SA_OK
