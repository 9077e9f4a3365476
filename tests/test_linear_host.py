"""Host tests of the device logistic regression: the numpy oracle (tests/linear_reference.py)
against sklearn's Newton solver, the oracle's limb format against the C header the kernels
compile, and every error the Python layer raises before any device work.  No GPU needed."""
import os
import struct
import subprocess

import numpy as np
import pytest

import linear_reference as lr

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def sets():
    return lr.shot_like_sets()


# ----------------------------------------------------------------------------- the optimum
@pytest.mark.parametrize('n, C, fit_intercept', sorted(lr.MEASURED_VS_SKLEARN, key=str))
def test_oracle_newton_reaches_sklearns_optimum(sets, n, C, fit_intercept):
    """The oracle's Newton loop against ``LogisticRegression(solver='newton-cholesky', tol=1e-12)``.
    Measured max |p difference| (rows, C, intercept): (300, 1, yes) 3.7e-12, (300, 0.01, yes)
    3.4e-16, (300, 1, no) 2.1e-12, (5000, 1, yes) 6.7e-16, (5000, 0.01, yes) 6.2e-16, (5000, 1, no)
    3.7e-10; max |coefficient difference| 1.1e-10 .. 2.5e-9.  The bound is 10 x the measured
    probability figure (``linear_reference.MEASURED_VS_SKLEARN``): two finite-precision solves of
    a 1e7-conditioned system differ in their last digits.  sklearn's own default lbfgs fit is
    0.03 - 0.06 away from this optimum."""
    X, y = sets[n]
    beta, it = lr.newton(X, y, C=C, tol=1e-10, fit_intercept=fit_intercept)
    ref = lr.sklearn_fit(X, y, C, fit_intercept)
    diff = np.abs(lr.sigmoid_of(X, beta) - ref.predict_proba(X)[:, 1]).max()
    print(f'n={n} C={C} intercept={fit_intercept}: {it} iterations, max |p - sklearn| = {diff:.3g}')
    assert diff <= 10 * lr.MEASURED_VS_SKLEARN[(n, C, fit_intercept)]
    assert it <= 10
    g0 = np.abs(lr.objective_gradient(X, y, np.zeros(len(beta)), C, fit_intercept)).max()
    assert np.abs(lr.objective_gradient(X, y, beta, C, fit_intercept)).max() <= 1e-10 * max(1.0, g0)
    if not fit_intercept:
        assert beta[-1] == 0.0


def test_oracle_moments_are_the_derivatives_of_the_loss(sets):
    """The gradient and the Hessian against central differences of the loss and the gradient."""
    X, y = sets[300]
    rng = np.random.default_rng(5)
    beta = rng.normal(size=X.shape[1] + 1) * 0.01
    g, H, f = lr.moments(X, y, beta)
    for j in (0, 5, 27, 30, X.shape[1]):
        e = np.zeros(len(beta))
        e[j] = 1e-5
        gp, _, fp = lr.moments(X, y, beta + e)
        gm, _, fm = lr.moments(X, y, beta - e)
        assert abs((fp - fm) / 2e-5 - g[j]) <= 1e-6 * max(1.0, abs(g[j]))
        np.testing.assert_allclose((gp - gm) / 2e-5, H[j], rtol=1e-6, atol=1e-6 * np.abs(H).max())
    mask = (np.arange(300) % 3 != 0)
    gm_, Hm, fm_ = lr.moments(X, y, beta, mask)
    g2, H2, f2 = lr.moments(X[mask], y[mask], beta)
    assert gm_.tobytes() == g2.tobytes() and Hm.tobytes() == H2.tobytes() and fm_ == f2


# ----------------------------------------------------------------------------- the limb format
@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('fixed_sum') / 'fixed_sum_host')
    subprocess.run(['g++', '-O1', '-std=c++17', os.path.join(ROOT, 'scripts', 'fixed_sum_host.cc'), '-o', exe],
                   check=True)
    return exe


@pytest.mark.parametrize('E', [-7, 1, 12])
def test_limb_oracle_matches_the_kernels_header(host_program, tmp_path, E):
    """``quantize`` / ``quantize_columns`` against ``sa_fx_quantize`` as scripts/fixed_sum_host.cc
    runs it (one group per value: the group's limb sums are the value's limbs), and the totals
    against ``sa_fx_finalize`` through ``linear.fixed_value`` and ``ops.fixed_sum_value``."""
    from socceraction_amd import linear, ops
    top = 2.0 ** E
    rng = np.random.default_rng(E + 100)
    vals = np.array([0.0, -0.0, top / 2, -top / 2, np.nextafter(top, 0), 2.0 ** (E - 95), -2.0 ** (E - 95),
                     2.0 ** (E - 96), top / 3, -top / 7, 1e-300, 0.25 * 0.1 * top, np.pi * top / 4]
                    + list(rng.uniform(-1, 1, 20) * top * 2.0 ** rng.integers(-60, 0, 20)))
    n = len(vals)
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        f.write(struct.pack('<iiqq', 0, E, n, n))
        f.write(np.ascontiguousarray(vals, '<f8').tobytes())
        f.write(np.arange(n, dtype='<i4').tobytes())
    subprocess.run([host_program, src, dst], check=True)
    raw = open(dst, 'rb').read()
    got = np.frombuffer(raw, '<i8')[:3 * n].reshape(n, 3)
    sums = np.frombuffer(raw, '<f8')[4 * n + 1:]
    scalar = [lr.limbs_of(lr.quantize(v, E)) for v in vals]
    assert got.tolist() == scalar
    vec = lr.quantize_columns(vals[None, :], [E] * n)
    assert vec[:, 0, :].T.tolist() == scalar
    for limbs, s in zip(scalar, sums):
        assert linear.fixed_value(linear.limb_total(*limbs), E) == s == ops.fixed_sum_value(*limbs, E)
    # beyond 2^95 the shift changes sign
    assert linear.fixed_value(3, 97) == 12.0 and linear.fixed_value(-(1 << 60) - 1, 100) == -float((1 << 65) + 32)


def test_item_layout_and_native_constants():
    from socceraction_amd import _native, linear
    with open(os.path.join(ROOT, 'include', 'socceraction_amd.h')) as f:
        src = f.read()
    for name in ('SA_LOGIT_MAX_COLS', 'SA_LOGIT_TILE_ROWS', 'SA_LOGIT_BLOCK_J', 'SA_LOGIT_BLOCK_K', 'SA_LOGIT_WG_PER_CU',
                 'SA_LOGIT_ERR_NAN', 'SA_LOGIT_ERR_NONFINITE', 'SA_LOGIT_ERR_RANGE'):
        assert f'#define {name} {getattr(_native, name)}\n' in src, name
    assert f'#define SA_LOGIT_EXP_MIN ({_native.SA_LOGIT_EXP_MIN})\n' in src
    assert f'#define SA_LOGIT_EXP_MAX {_native.SA_LOGIT_EXP_MAX}\n' in src
    assert {'sa_logit_moments', 'sa_logit_predict'} <= set(_native.EXPORTED_SYMBOLS)
    assert linear.n_items(46) == 47 * 48 // 2 + 47 + 1 == len(lr.item_exps([0] * 47, 0))
    assert linear.item_exps([3, -1, 1], 7) == lr.item_exps([3, -1, 1], 7) == [4, 0, 2, -4, -2, 0, 3, -1, 1, 7]
    # the item table of D + 2 rows and D columns in blocks of 16 x 64
    assert linear.item_grid(0) == (1, 1) and linear.item_grid(46) == (4, 1) and linear.item_grid(568) == (36, 9)
    assert linear.item_splits(46) == 4 and linear.item_grid(_native.SA_LOGIT_MAX_COLS) == (41, 11)
    # a workgroup's LDS does not depend on the width, and the by-value column table fits the kernel arguments
    assert _native.SA_LOGIT_TILE_ROWS * (_native.SA_LOGIT_BLOCK_J + _native.SA_LOGIT_BLOCK_K + 1) * 8 <= 65536
    assert 2 * _native.SA_LOGIT_MAX_COLS + 2 * (_native.SA_LOGIT_MAX_COLS + 1) <= 3072
    assert linear.loss_exponent(np.zeros(4), [7, 7, 7, 1]) == 1
    assert linear.loss_exponent(np.array([1.0, -2.0, 0.5]), [3, 1, 1]) == 4  # 8 + 4 + 0.5 + 1 < 16


def test_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes

    from socceraction_amd import _native
    lib = _native.load_library()
    blk = _native.SaBlock()
    blk.data, blk.n_cols, blk.tile_rows = None, 2, 16
    slots = (ctypes.c_int32 * 2)(1 << 24, (1 << 24) | 5)
    exps = (ctypes.c_int32 * 3)(0, 0, 1)
    one = ctypes.c_void_p(16)  # never dereferenced: every check below fails first

    def moments(**kw):
        a = dict(f=ctypes.byref(blk), i=ctypes.byref(blk), bits=None, words=0, n_bool=0, slots=slots, d=2, beta=one,
                 exps=exps, loss_exp=1, y=one, n=0, grid=0, rowbuf=one, limbs=one, err=one)
        a.update(kw)
        return lib.sa_logit_moments(a['f'], a['i'], 0, a['bits'], a['words'], a['n_bool'], a['slots'], a['d'],
                                    a['beta'], a['exps'], a['loss_exp'], a['y'], None, a['n'], a['grid'], a['rowbuf'],
                                    a['limbs'], a['err'], None)

    assert moments() == _native.SA_EINVAL and b'column 5 of 2' in lib.sa_last_error()
    slots[1] = (1 << 24) | 1
    assert moments(d=_native.SA_LOGIT_MAX_COLS + 1) == _native.SA_EINVAL
    assert moments(n=1 << 30) == _native.SA_EINVAL
    assert moments(beta=None) == _native.SA_EINVAL
    assert moments(limbs=None) == _native.SA_EINVAL
    assert moments(grid=-1) == _native.SA_EINVAL
    assert moments(loss_exp=901) == _native.SA_EINVAL
    exps[0] = 441
    assert moments() == _native.SA_EINVAL and b'col_exp[0]' in lib.sa_last_error()
    exps[0] = 0
    slots[0] = 3 << 24
    assert moments() == _native.SA_EINVAL and b'unknown kind' in lib.sa_last_error()
    slots[0] = 0  # a bitmap row without bitmaps
    assert moments() == _native.SA_EINVAL
    slots[0] = 1 << 24
    assert moments(n=5) == _native.SA_EINVAL and b'null numeric block' in lib.sa_last_error()
    slots[0], slots[1] = (1 << 24) | (1 << 14), 1 << 24
    blk.n_cols = 1 << 15
    assert moments() == _native.SA_EINVAL and b'below 16384' in lib.sa_last_error()
    blk.n_cols, slots[0] = 2, 1 << 24
    assert lib.sa_logit_predict(ctypes.byref(blk), ctypes.byref(blk), 0, None, 0, 0, slots, 2, None, 0, 0, None,
                                None) == _native.SA_EINVAL
    assert lib.sa_logit_predict(None, ctypes.byref(blk), 0, None, 0, 0, slots, 2, one, 0, 0, None,
                                None) == _native.SA_EINVAL


# ----------------------------------------------------------------------------- host-side errors
def _cpu_blocks(bitmaps=True):
    """Feature blocks on the host: enough for every check that runs before a launch."""
    from socceraction_amd import ops
    from socceraction_amd.catalog import FeaturePlan
    n = 40
    plan = FeaturePlan((), 1, False, 2, 2, 1, [('b0', 'b', 0), ('f0', 'f', 0), ('i0', 'i', 0), ('b1', 'b', 1),
                                              ('f1', 'f', 1)], None)
    return ops.FeatureBlocks(plan, n, 1024, 48, None if bitmaps else torch.zeros((1, 2, 48), dtype=torch.uint8),
                             torch.zeros((1, 2, 48), dtype=torch.float64), torch.zeros((1, 1, 48), dtype=torch.int64),
                             torch.zeros((2, 1), dtype=torch.int64) if bitmaps else None)


def test_host_side_errors_come_before_any_device_work():
    from socceraction_amd.linear import DeviceLogisticRegression
    blocks = _cpu_blocks()
    y = torch.zeros(40, dtype=torch.uint8)
    y[::2] = 1
    with pytest.raises(ValueError, match='C must be positive'):
        DeviceLogisticRegression(C=0).fit_blocks(blocks, y)
    with pytest.raises(ValueError, match='C must be positive'):
        DeviceLogisticRegression(C=-1.0).fit(np.zeros((4, 2)), [0, 1, 0, 1])
    with pytest.raises(ValueError, match='not available'):
        DeviceLogisticRegression().fit_blocks(blocks, y, columns=['f0', 'nope'])
    with pytest.raises(ValueError, match='repeated'):
        DeviceLogisticRegression().fit_blocks(blocks, y, columns=['f0', 'b1', 'f0'])
    with pytest.raises(ValueError, match='bitmaps'):
        DeviceLogisticRegression().fit_blocks(_cpu_blocks(bitmaps=False), y)
    # without a bool column the block form does not matter: the next check is the labels'
    with pytest.raises(ValueError, match='only one class'):
        DeviceLogisticRegression().fit_blocks(_cpu_blocks(bitmaps=False), torch.ones(40, dtype=torch.uint8),
                                              columns=['f0', 'i0'])
    with pytest.raises(ValueError, match='only one class'):
        DeviceLogisticRegression().fit_blocks(blocks, torch.zeros(40, dtype=torch.uint8))
    with pytest.raises(ValueError, match='only one class'):  # both classes, but not among the rows
        DeviceLogisticRegression().fit_blocks(blocks, y, rows=torch.arange(0, 40, 2))
    with pytest.raises(ValueError, match='only one class'):
        DeviceLogisticRegression().fit(np.zeros((5, 2)), np.ones(5))
    with pytest.raises(ValueError, match='two classes'):
        DeviceLogisticRegression().fit(np.zeros((6, 2)), [0, 1, 2, 0, 1, 2])
    with pytest.raises(ValueError, match='uint8'):
        DeviceLogisticRegression().fit_blocks(blocks, y.to(torch.int64))
    with pytest.raises(ValueError, match='at most 640 columns: got 641'):
        DeviceLogisticRegression().fit(np.zeros((4, 641)), [0, 1, 0, 1])
    with pytest.raises(ValueError, match='inside'):
        DeviceLogisticRegression().fit_blocks(blocks, y, rows=[0, 40])
    from sklearn.exceptions import NotFittedError
    with pytest.raises(NotFittedError):
        DeviceLogisticRegression().predict_proba(np.zeros((3, 2)))


def test_expected_goals_rejects_what_the_linear_learner_cannot_do():
    import pandas as pd

    from socceraction_amd import xg
    model = xg.ExpectedGoals()
    with pytest.raises(ValueError, match='early_stopping_rounds'):
        model.fit_batch(pd.DataFrame(), pd.DataFrame(), learner='logistic', val_size=0.25, early_stopping_rounds=5)
    with pytest.raises(ValueError, match='C must be positive'):
        model.fit_batch(pd.DataFrame(), pd.DataFrame(), learner='logistic', linear_params=dict(C=0.0))
    with pytest.raises(ValueError, match='tree_params'):
        model.fit_batch(pd.DataFrame(), pd.DataFrame(), learner='logistic', tree_params=dict(max_depth=3))
    with pytest.raises(ValueError, match='linear_params'):
        model.fit_batch(pd.DataFrame(), pd.DataFrame(), linear_params=dict(C=2.0))
    with pytest.raises(ValueError, match='not supported'):
        model.fit_batch(pd.DataFrame(), pd.DataFrame(), learner='svm')
