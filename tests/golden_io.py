"""Load the golden fixtures of tests/golden (written by tests/golden/make_golden.py)."""
import glob
import os

import mpmath
import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

SPADL_IN = ['game_id', 'period_id', 'time_seconds', 'team_id', 'start_x', 'start_y', 'end_x',
            'end_y', 'type_id', 'result_id', 'bodypart_id']
ATOMIC_IN = ['game_id', 'period_id', 'time_seconds', 'team_id', 'x', 'y', 'dx', 'dy', 'type_id',
             'bodypart_id']


def cases(prefix):
    """Names of the golden cases with a given prefix ('spadl', 'atomic', 'xt')."""
    return sorted(os.path.basename(p)[len(prefix) + 1:-4]
                  for p in glob.glob(os.path.join(GOLDEN, f'{prefix}_*.npz')))


def load(prefix, name):
    with np.load(os.path.join(GOLDEN, f'{prefix}_{name}.npz'), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def inputs(g, atomic=False):
    """Input columns of a case as a dict of numpy arrays (raw reference dtypes)."""
    return {c: g['in_' + c] for c in (ATOMIC_IN if atomic else SPADL_IN)}


def frame(g, atomic=False):
    """The case's input as a reference-shaped DataFrame."""
    cols = inputs(g, atomic)
    df = pd.DataFrame(cols)
    df.insert(1, 'original_event_id', None)
    df.insert(2, 'action_id', np.arange(len(df)))
    df.insert(6, 'player_id', 0)
    return df


def ks(g):
    return sorted(int(k[1:k.index('_')]) for k in g if k.startswith('k') and k.endswith('_names_all'))


def assert_close(a, b, name=''):
    """float parity bar: |a-b| <= 1e-6*|b| + 1e-12, NaNs in the same places."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert (na == nb).all(), f'{name}: NaN pattern differs'
    ok = ~nb
    err = np.abs(a[ok] - b[ok])
    tol = 1e-6 * np.abs(b[ok]) + 1e-12
    bad = err > tol
    assert not bad.any(), f'{name}: {bad.sum()} mismatches, max err {err.max()}'


def _bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def assert_same_floats(got, ref, name=''):
    """Bit-for-bit float parity: equal shape and dtype, NaN in the same places (payloads do not
    count), equal bit patterns elsewhere, so 0.0 is not -0.0."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.dtype in (np.float64, np.float32), (name, got.dtype, ref.dtype)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    ng, nr = np.isnan(got), np.isnan(ref)
    assert (ng == nr).all(), f'{name}: NaN pattern differs at {np.argwhere(ng != nr)[:5].tolist()}'
    bad = (_bits(got) != _bits(ref)) & ~nr
    if bad.any():
        at = np.argwhere(bad)
        first = tuple(at[0])
        raise AssertionError(f'{name}: {len(at)} values differ in their bits, first at {first}: '
                             f'got {got[first]!r}, reference {ref[first]!r}')


_PARTS = {}  # mpf value -> (nearest double, exact - nearest)
_SPLIT = {}  # id(mpf array) -> (the array, nearest double, residual, ulp, sign)


def _parts(e):
    t = _PARTS.get(e)
    if t is None:
        near = float(e)
        with mpmath.workprec(200):
            t = (near, float('nan') if near != near else float(e - mpmath.mpf(near)))
        _PARTS[e] = t
    return t


def _split_exact(exact):
    """An array of mpmath.mpf as (nearest double, exact - nearest, spacing(|exact|), sign bit),
    once per array and once per value: the callers compute a reference once and share it."""
    key = id(exact)
    if key not in _SPLIT:
        parts = np.array([_parts(e) for e in exact.reshape(-1).tolist()], np.float64).reshape(-1, 2)
        near, res = parts[:, 0].reshape(exact.shape), parts[:, 1].reshape(exact.shape)
        # spacing at |exact|: of the double at or below it in magnitude
        inward = np.where((res != 0) & (np.signbit(res) != np.signbit(near)), np.nextafter(near, 0.0), near)
        with np.errstate(invalid='ignore'):
            ulp = np.spacing(np.abs(inward))
        _SPLIT[key] = (exact, near, res, ulp, np.signbit(near))   # float() keeps the sign of a tiny value
    return _SPLIT[key][1:]


def assert_within_ulps(got, exact, bound, name=''):
    """``got`` within ``bound`` float64 ulps of a high-precision value; returns the largest
    distance seen, in ulps.

    ``exact`` is an array of ``mpmath.mpf`` (distances are exact; an exact zero is +0.0, mpf has
    no signed zero), or a pair ``(lo, hi)`` of float64 arrays with lo <= value <= hi (``got`` must
    lie in [hi - bound ulp, lo + bound ulp], which implies the bound; the distance returned is the
    larger of the distances to lo and hi, an upper estimate).

    NaN in the same places and the same sign; |got - exact| <= bound * spacing(|exact|); an
    exact zero is matched exactly.  A float32 ``got`` must lie in
    [float32(exact - bound ulp), float32(exact + bound ulp)] (ulp of float64), which does not
    charge a float32 rounding midpoint to the code under test; the distance returned is then 0
    inside float32(exact)'s own bracket, else the excess in float64 ulps.
    """
    got = np.ascontiguousarray(got)
    assert got.dtype in (np.float64, np.float32), (name, got.dtype)
    if isinstance(exact, tuple):
        lo, hi = (np.ascontiguousarray(v, dtype=np.float64) for v in exact)
        assert lo.shape == hi.shape and (np.isnan(lo) == np.isnan(hi)).all(), name
        with np.errstate(invalid='ignore'):
            assert (lo[~np.isnan(lo)] <= hi[~np.isnan(lo)]).all(), name
            ulp = np.spacing(np.minimum(np.abs(lo), np.abs(hi)))
        sign, zero, nan = np.signbit(lo), (lo == 0) & (hi == 0), np.isnan(lo)
        res_lo = res_hi = 0.0
    else:
        assert exact.dtype == object, name
        near, res, ulp, sign = _split_exact(exact)
        nan = np.isnan(near)
        zero = (near == 0) & (res == 0)
        lo = hi = near
        res_lo = res_hi = res
    assert got.shape == lo.shape, (name, got.shape, lo.shape)
    ng = np.isnan(got)
    assert (ng == nan).all(), f'{name}: NaN pattern differs at {np.argwhere(ng != nan)[:5].tolist()}'
    ok = ~nan
    wrong = (np.signbit(got) != sign) & ok
    assert not wrong.any(), (f'{name}: sign differs at {np.argwhere(wrong)[:5].tolist()}, '
                             f'got {got[wrong][:5].tolist()}')
    wrong = zero & (got != 0)
    assert not wrong.any(), f'{name}: exact zero missed at {np.argwhere(wrong)[:5].tolist()}'
    L = np.longdouble
    with np.errstate(invalid='ignore', over='ignore'):
        if got.dtype == np.float32:
            # bounds rounded to float32 through the nearest float64: a double rounding can move a
            # bound by one float32 step only when it lands on a float32 midpoint to within 2^-53
            lo32 = ((lo.astype(L) + res_lo) - bound * ulp.astype(L)).astype(np.float64).astype(np.float32)
            hi32 = ((hi.astype(L) + res_hi) + bound * ulp.astype(L)).astype(np.float64).astype(np.float32)
            g = got.astype(L)
            d = np.maximum(np.maximum(lo32.astype(L) - g, g - hi32.astype(L)), 0) / ulp.astype(L)
        else:
            g = got.astype(L)
            d = np.maximum(np.abs((g - lo.astype(L)) - res_lo), np.abs((g - hi.astype(L)) - res_hi)) \
                / ulp.astype(L)
    d = np.where(ok, d, 0).astype(np.float64)
    bad = d > (0 if got.dtype == np.float32 else bound)
    if bad.any():
        at = np.argwhere(bad)
        first = tuple(at[0])
        raise AssertionError(f'{name}: {len(at)} values beyond {bound} ulps, largest {d.max():.3f}, '
                             f'first at {first}: got {got[first]!r}, exact ~ {lo[first]!r}')
    return float(d.max()) if d.size else 0.0


CONVERT_IN = ['game_id', 'original_event_id', 'action_id', 'period_id', 'time_seconds', 'team_id',
              'player_id', 'start_x', 'start_y', 'end_x', 'end_y', 'type_id', 'result_id',
              'bodypart_id']
CONVERT_OUT = ['game_id', 'original_event_id', 'action_id', 'period_id', 'time_seconds',
               'team_id', 'player_id', 'x', 'y', 'dx', 'dy', 'type_id', 'bodypart_id']


def _convert_cols(g, prefix, names):
    out = {}
    for c in names:
        v = g[prefix + c]
        if c == 'original_event_id':
            v = np.array([None if m else s for s, m in zip(v, g[prefix + c + '_isna'])],
                         dtype=object)
        out[c] = v
    return out


def convert_input(g):
    """Input SPADL frame of a convert_* golden (tests/golden/make_golden_convert.py)."""
    return pd.DataFrame(_convert_cols(g, 'in_', CONVERT_IN))


def convert_output(g):
    """The reference's Atomic-SPADL output of a convert_* golden as columns."""
    return _convert_cols(g, 'out_', CONVERT_OUT)


def assert_convert_equal(got: dict, ref: dict, name=''):
    """Bit-exact ids / codes / counts; floats within the assert_close bar; same NaN pattern
    of original_event_id."""
    assert set(got) >= set(CONVERT_OUT), name
    n = len(ref['type_id'])
    for c in CONVERT_OUT:
        a, b = got[c], ref[c]
        assert len(a) == n, (name, c, len(a), n)
        if c == 'original_event_id':
            ma = np.array([x is None or (isinstance(x, float) and np.isnan(x)) for x in a], bool)
            mb = np.array([x is None for x in b], bool)
            np.testing.assert_array_equal(ma, mb, err_msg=f'{name} {c} missing pattern')
            np.testing.assert_array_equal(np.asarray(a, object)[~ma].astype(str),
                                          np.asarray(b, object)[~mb].astype(str), err_msg=name)
        elif np.asarray(b).dtype.kind == 'f':
            assert_close(a, b, f'{name} {c}')
        else:
            np.testing.assert_array_equal(np.asarray(a).astype(np.int64),
                                          np.asarray(b).astype(np.int64), err_msg=f'{name} {c}')


def dribbles_frame(g, prefix='in_'):
    """A dribbles_* golden's input (``in_``) or the reference's output (``out_``) as a DataFrame
    with the stored dtypes (tests/golden/make_golden_dribbles.py)."""
    cols = {}
    for c in g[prefix + '__columns']:
        c = str(c)
        dt = str(g[prefix + c + '__dtype'])
        v = g[prefix + c]
        if dt == 'object':
            v = np.array([np.nan if m else s for s, m in zip(v, g[prefix + c + '__isna'])],
                         dtype=object)
        cols[c] = pd.Series(v, dtype=dt)
    return pd.DataFrame(cols)


def assert_frame_same(got: pd.DataFrame, ref: pd.DataFrame, name=''):
    """Same columns, order and dtypes; values bit-exact (floats too; NaN where the reference
    has NaN); object columns equal as strings with the same missing pattern."""
    assert list(got.columns) == list(ref.columns), (name, list(got.columns), list(ref.columns))
    assert len(got) == len(ref), (name, len(got), len(ref))
    assert got.index.equals(pd.RangeIndex(len(ref))), name
    for c in ref.columns:
        a, b = got[c], ref[c]
        assert a.dtype == b.dtype, (name, c, a.dtype, b.dtype)
        if b.dtype == object:
            ma, mb = a.isna().to_numpy(), b.isna().to_numpy()
            np.testing.assert_array_equal(ma, mb, err_msg=f'{name} {c} missing pattern')
            np.testing.assert_array_equal(a[~ma].astype(str).to_numpy(),
                                          b[~mb].astype(str).to_numpy(), err_msg=f'{name} {c}')
        else:
            np.testing.assert_array_equal(a.to_numpy(), b.to_numpy(), err_msg=f'{name} {c}')
