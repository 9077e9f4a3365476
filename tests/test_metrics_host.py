"""socceraction_amd.metrics without a GPU: the numpy path of binary_scores (the definitions of
sa_metric_sums / sa_auc_count) against scikit-learn, its errors, the baselines, the host-side
layers and the C ABI's argument checks."""
import math
import os

import numpy as np
import pandas as pd
import pytest
from sklearn.metrics import brier_score_loss, log_loss, roc_auc_score

from test_ratings_host import py_finalize, py_quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 3, 64, 65, 5000]


def ulps(a: float, b: float) -> int:
    x, y = np.array([a, b], np.float64).view(np.int64)
    return abs(int(x) - int(y))


def columns(n: int, ties: bool, f32: bool, seed: int = 0):
    rng = np.random.default_rng([n, int(ties), seed])
    y = (rng.random(n) < 0.3).astype(np.uint8)
    y[0], y[1] = 0, 1  # both classes present
    p = np.clip(0.25 * y + rng.beta(1.0, 3.0, n), 0, 1)
    if ties:
        p = np.round(p * 16) / 16
    return y, p.astype(np.float32 if f32 else np.float64)


def clip32(p):
    eps = np.finfo(np.float32).eps
    return np.clip(p, eps, np.float32(1) - eps)


def sklearn_scores(y, p):
    """(brier, log_loss, auroc) of scikit-learn.  Brier score and AUROC of a float32 column are
    those of the widened column.  Its log loss is sklearn's on the float32 column itself: there
    sklearn takes the complement 1 - p and the clip to [eps, 1 - eps] in float32 -- the kernel's
    contract -- and evaluates and sums -log in float64 (xlogy of integer labels).  log_loss(y,
    widened clipped column) forms the complement in float64 instead and agrees only where 1 - p
    is exact in float32; test_numpy_path_equals_sklearn checks that case against it as well."""
    wide = p.astype(np.float64)
    return brier_score_loss(y, wide), log_loss(y, p), roc_auc_score(y, wide)


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('ties', [False, True], ids=['distinct', 'ties'])
@pytest.mark.parametrize('n', SIZES)
def test_numpy_path_equals_sklearn(n, ties, f32):
    from socceraction_amd import metrics
    y, p = columns(n, ties, f32)
    got = metrics.binary_scores_host(y, p)
    brier, ll, auc = sklearn_scores(y, p)
    print(n, ties, f32, 'brier rel', abs(got['brier'] - brier) / brier, 'log_loss rel',
          abs(got['log_loss'] - ll) / ll, 'auroc ulps', ulps(got['auroc'], auc))
    assert set(got) == set(metrics.KEYS)
    assert got['n'] == n and got['n_pos'] == int(y.sum())
    assert ulps(got['auroc'], auc) <= 2
    assert abs(got['brier'] - brier) <= 1e-14 * brier
    assert abs(got['log_loss'] - ll) <= 1e-14 * ll
    if f32:
        # sklearn itself on the column widened after the float32 clip: the same number where the
        # float32 complement is exact (multiples of 1/16); elsewhere 1 - p rounds in float32, as
        # it does inside sklearn for a float32 column, and the two differ by about 1e-9
        sk = log_loss(y, clip32(p).astype(np.float64))
        print('   log_loss rel to sklearn(widened clipped column)', abs(got['log_loss'] - sk) / sk)
        if ties:
            assert abs(got['log_loss'] - sk) <= 1e-14 * sk


def test_f32_log_loss_clips_in_float32():
    """p = 1 for a negative and p = 0 for a positive: the terms are -log(eps of float32)."""
    from socceraction_amd import metrics
    y = np.array([0, 1, 0, 1], np.uint8)
    p = np.array([1.0, 0.0, 0.25, 0.75], np.float32)
    got = metrics.binary_scores_host(y, p)
    eps = float(np.finfo(np.float32).eps)
    want = (2 * -math.log(eps) + 2 * -math.log(0.75)) / 4
    assert abs(got['log_loss'] - want) <= 1e-14 * want
    assert got['brier'] == (1 + 1 + 0.0625 + 0.0625) / 4
    assert got['auroc'] == 0.25  # one ordered pair of four


def test_binary_scores_input_forms():
    """Every input form gives one dict.  With a device present the inputs are uploaded and the
    dict is the kernels': everything but the log loss (the device's log) equals the numpy path
    bit for bit."""
    import torch

    from socceraction_amd import metrics
    y, p = columns(65, True, False)
    want = metrics.binary_scores_host(y, p)
    got = metrics.binary_scores(y, p)
    if torch.cuda.is_available():
        assert abs(got['log_loss'] - want['log_loss']) <= 1e-12 * want['log_loss']
        want = dict(want, log_loss=got['log_loss'])
    assert got == want
    assert metrics.binary_scores(pd.Series(y.astype(bool)), pd.Series(p)) == want
    assert metrics.binary_scores(torch.from_numpy(y), torch.from_numpy(p)) == want
    assert metrics.binary_scores(list(y), list(p)) == want


def test_numpy_path_does_not_depend_on_row_order():
    from socceraction_amd import metrics
    for f32 in (False, True):
        y, p = columns(5000, True, f32)
        perm = np.random.default_rng(5).permutation(len(y))
        assert metrics.binary_scores_host(y, p) == metrics.binary_scores_host(y[perm], p[perm])


def test_limb_sums_equal_the_python_integer_restatement():
    from socceraction_amd import metrics, ops
    rng = np.random.default_rng(9)
    for E in (1, 6):
        v = rng.random(300) * (2.0 ** E) * 0.999
        v[:8] = [0.0, -0.0, 5e-324, 2.0 ** -60, 2.0 ** -94, 2.0 ** -95, 2.0 ** -96, np.nextafter(2.0 ** E, 0)]
        want = [sum(py_quantize(x, E)[i] for x in v.tolist()) for i in range(3)]
        got = metrics._limb_sums(v, E)
        assert list(got) == want
        assert ops.fixed_sum_value(*got, E) == py_finalize(*want, E)
    with pytest.raises(ValueError):
        metrics._limb_sums(np.array([2.0]), 1)
    with pytest.raises(ValueError):
        metrics._limb_sums(np.array([-0.5]), 1)


@pytest.mark.parametrize('case', ['nan', 'above_one', 'below_zero', 'inf', 'label_2', 'single_class',
                                  'single_class_ones', 'empty'])
def test_errors_are_value_errors(case):
    from socceraction_amd import metrics
    y, p = columns(64, False, False)
    y = y.astype(np.int64)
    if case == 'nan':
        p[5] = np.nan
    elif case == 'above_one':
        p[5] = 1.5
    elif case == 'below_zero':
        p[5] = -0.25
    elif case == 'inf':
        p[5] = np.inf
    elif case == 'label_2':
        y[7] = 2
    elif case == 'single_class':
        y[:] = 0
    elif case == 'single_class_ones':
        y[:] = 1
    else:
        y, p = y[:0], p[:0]
    with pytest.raises(ValueError):
        metrics.binary_scores_host(y, p)
    with pytest.raises(ValueError):
        metrics.binary_scores_host(y, p.astype(np.float32))


@pytest.mark.parametrize('n', SIZES)
def test_baselines_are_the_scores_of_the_base_rate(n):
    from socceraction_amd import metrics
    y, p = columns(n, False, False)
    got = metrics.binary_scores_host(y, p)
    base = np.full(n, y.mean())
    want_b, want_l = brier_score_loss(y, base), log_loss(y, base)
    assert abs(got['brier_baseline'] - want_b) <= 1e-14 * want_b
    assert abs(got['log_loss_baseline'] - want_l) <= 1e-14 * want_l


def test_native_constants_match_the_header():
    from socceraction_amd import _native
    with open(os.path.join(ROOT, 'include', 'socceraction_amd.h')) as f:
        src = f.read()
    for name in ('SA_METRIC_BRIER_EXP', 'SA_METRIC_LOGLOSS_EXP', 'SA_METRIC_CHUNK_ROWS', 'SA_METRIC_ERR_NAN',
                 'SA_METRIC_ERR_RANGE', 'SA_METRIC_ERR_LABEL', 'SA_AUC_LDS_SAMPLE', 'SA_METRIC_WG_PER_CU'):
        line = [ln for ln in src.splitlines() if ln.startswith(f'#define {name} ')]
        assert len(line) == 1, name
        assert int(line[0].split()[2]) == getattr(_native, name), name
    assert _native.load_library().sa_abi_version() == 6


def test_metric_entry_points_validate_without_a_gpu():
    """Every invalid argument is SA_EINVAL before any HIP call; n == 0 is a no-op; and
    sa_metric_finalize (host pointers) rounds as the Python restatement does."""
    import ctypes

    from socceraction_amd import _native, ops
    lib = _native.load_library()
    fake = ctypes.c_void_p(256)  # never dereferenced on the host
    sums = dict(y=fake, p=fake, f32=0, n=10, count=fake, limbs=fake, err=fake, stream=None)
    keys = dict(y=fake, p=fake, f32=1, n=10, minority=1, keys=fake, capacity=3, cursor=fake, stream=None)
    count = dict(y=fake, p=fake, f32=0, n=10, sorted_keys=fake, m=3, minority=0, u2=fake, stream=None)
    cases = [
        (lib.sa_metric_sums, sums, [dict(y=None), dict(p=None), dict(count=None), dict(limbs=None), dict(err=None),
                                    dict(n=-1), dict(n=1 << 30)]),
        (lib.sa_auc_keys, keys, [dict(y=None), dict(p=None), dict(keys=None), dict(cursor=None), dict(n=-1),
                                 dict(n=1 << 30), dict(minority=2), dict(minority=-1), dict(capacity=-1)]),
        (lib.sa_auc_count, count, [dict(y=None), dict(p=None), dict(sorted_keys=None), dict(u2=None), dict(n=-1),
                                   dict(n=1 << 30), dict(minority=2), dict(m=0), dict(m=11), dict(n=0)]),
    ]
    for fn, good, bad in cases:
        for kw in bad:
            a = dict(good, **kw)
            assert fn(*a.values()) == _native.SA_EINVAL, (fn.__name__, kw)
            assert fn.__name__.encode() in lib.sa_last_error(), (fn.__name__, kw)
    assert lib.sa_metric_sums(*dict(sums, n=0).values()) == _native.SA_OK
    assert lib.sa_auc_keys(*dict(keys, n=0).values()) == _native.SA_OK

    rng = np.random.default_rng(4)
    terms = [rng.random(100) * 1.99, rng.random(100) * 63.9]
    limbs = [sum(py_quantize(x, E)[i] for x in t.tolist()) for t, E in zip(terms, (1, 6)) for i in range(3)]
    out = (ctypes.c_double * 2)()
    assert lib.sa_metric_finalize((ctypes.c_int64 * 2)(100, 40), (ctypes.c_int64 * 6)(*limbs), out) == _native.SA_OK
    assert out[0] == py_finalize(*limbs[:3], 1) / 100 == ops.fixed_sum_value(*limbs[:3], 1) / 100
    assert out[1] == py_finalize(*limbs[3:], 6) / 100 == ops.fixed_sum_value(*limbs[3:], 6) / 100
    assert lib.sa_metric_finalize((ctypes.c_int64 * 2)(0, 0), (ctypes.c_int64 * 6)(), out) == _native.SA_EINVAL
    assert lib.sa_metric_finalize(None, (ctypes.c_int64 * 6)(), out) == _native.SA_EINVAL


def test_python_layer_argument_checks():
    import torch

    from socceraction_amd import ops
    y = torch.zeros(4, dtype=torch.uint8)
    p = torch.zeros(4, dtype=torch.float64)
    acc = ops.BinaryMetrics(torch.zeros(10, dtype=torch.int64))
    assert acc.count.shape == (2,) and acc.limbs.shape == (2, 3) and acc.err.shape == (1,) and acc.u2.shape == (1,)
    with pytest.raises(TypeError):
        acc.add(y.long(), p)
    with pytest.raises(TypeError):
        acc.add(y, p.half())
    with pytest.raises(ValueError):
        acc.add(y, p[:3])
    acc.rows = ops.GROUP_MAX_ROWS - 3
    with pytest.raises(ValueError, match='2\\*\\*30'):
        acc.add(y, p)
    assert acc.add(y[:0], p[:0]) is acc  # no rows: nothing is launched
    for bit in (1, 2, 4):
        acc.buf[8] = bit
        with pytest.raises(ValueError):
            acc.finalize()
    # the dict from the integer sums: 4 rows, 1 positive, U2 = 3 of 6
    res = ops.scores_from_sums(4, 1, (0, 0, 1 << 29), (0, 0, 1 << 27), 3)
    assert res['brier'] == 0.125 and res['log_loss'] == 1.0 and res['auroc'] == 0.5
    assert res['brier_baseline'] == (0.75 ** 2 + 3 * 0.25 ** 2) / 4
    assert res['log_loss_baseline'] == -(math.log(0.25) + 3 * math.log(0.75)) / 4
    assert ops.scores_from_sums(3, 1, (0, 0, 0), (0, 0, 0), None)['auroc'] is None
    assert ops.scores_from_sums(3, 3, (0, 0, 0), (0, 0, 0), 0)['auroc'] is None


def test_score_batch_needs_a_fitted_model():
    from sklearn.exceptions import NotFittedError

    import socceraction_amd.atomic.vaep as avaep
    import socceraction_amd.vaep as vaep
    for model in (vaep.VAEP(), avaep.AtomicVAEP()):
        with pytest.raises(NotFittedError):
            model.score_batch(pd.DataFrame(), pd.DataFrame())
