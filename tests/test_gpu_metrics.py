"""The binary score kernels (sa_metric_sums, sa_auc_keys, sa_auc_count) and the layers above
them (ops.binary_metrics, metrics.binary_scores, VAEP.score_batch) on the device: counts, Brier
limbs and U2 against Python-integer / numpy restatements bit for bit, the finalised scores
against scikit-learn, order independence, the error bits."""
import math

import numpy as np
import pandas as pd
import pytest
from sklearn.metrics import brier_score_loss, log_loss, roc_auc_score

from test_metrics_host import ulps
from test_ratings_host import py_finalize, py_quantize

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

CHUNK, SAMPLE = 4096, 1024
WG_PER_CU = 8  # the row kernels' grid cap: workgroups per compute unit
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 5000]
NMAX = 5008  # >= max(SIZES), a multiple of 16
BRIER_EXP, LOGLOSS_EXP = 1, 6
DTYPES = pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, ops
    _native.load_library()
    assert (_native.SA_METRIC_CHUNK_ROWS, _native.SA_AUC_LDS_SAMPLE) == (CHUNK, SAMPLE)
    assert _native.SA_METRIC_WG_PER_CU == WG_PER_CU
    assert (_native.SA_METRIC_BRIER_EXP, _native.SA_METRIC_LOGLOSS_EXP) == (BRIER_EXP, LOGLOSS_EXP)
    return ops


# ----------------------------------------------------------------------------- shared reference
_ROWS = {}


def rows(f32: bool):
    """NMAX host rows (y uint8, p) and the Python-integer Brier limbs of every row [NMAX, 3],
    computed once per dtype."""
    if f32 not in _ROWS:
        rng = np.random.default_rng([31, int(f32)])
        y = (rng.random(NMAX) < 0.2).astype(np.uint8)
        p = np.clip(0.3 * y + rng.beta(0.8, 4.0, NMAX), 0, 1)
        p[rng.random(NMAX) < 0.02] = 0.0
        p[rng.random(NMAX) < 0.02] = 1.0
        p[rng.random(NMAX) < 0.01] = -0.0
        p[rng.random(NMAX) < 0.01] = 5e-324 if not f32 else 1e-45  # the smallest subnormal
        p[rng.random(NMAX) < 0.02] *= 2.0 ** -40
        p = p.astype(np.float32 if f32 else np.float64)
        d = p.astype(np.float64) - y
        limbs = np.array([py_quantize(x, BRIER_EXP) for x in (d * d).tolist()], np.int64)
        _ROWS[f32] = (y, p, limbs)
    return _ROWS[f32]


def padded(y, p):
    """Device views of n rows inside ld-padded blocks whose padding holds label 7 and NaN."""
    n = len(y)
    ld = max(16, (n + 15) // 16 * 16) + 16
    yb = torch.full((ld,), 7, dtype=torch.uint8)
    pb = torch.full((ld,), float('nan'), dtype=torch.float32 if p.dtype == np.float32 else torch.float64)
    yb[:n] = torch.from_numpy(np.ascontiguousarray(y))
    pb[:n] = torch.from_numpy(np.ascontiguousarray(p))
    return yb.cuda()[:n], pb.cuda()[:n]


def ref_log_loss(y, p):
    """sklearn's log loss of the column in its own dtype: for float32 it takes the complement and
    the clip in float32 and -log in float64 (test_metrics_host.sklearn_scores)."""
    return log_loss(y, p, labels=[0, 1])


def u2_reference(y, p):
    """U2 by its definition, in numpy: every positive against the sorted negatives."""
    pos = y == 1
    a, b = p[pos].astype(np.float64), np.sort(p[~pos].astype(np.float64))
    lo, hi = np.searchsorted(b, a, 'left').astype(np.int64), np.searchsorted(b, a, 'right').astype(np.int64)
    return int((2 * lo + (hi - lo)).sum())


def new_acc(sa):
    return sa.BinaryMetrics(torch.zeros(10, dtype=torch.int64, device='cuda'))


# ----------------------------------------------------------------------------- sums
@DTYPES
@pytest.mark.parametrize('n', SIZES)
def test_sums_equal_the_integer_restatement(sa, n, f32):
    """count and the Brier limbs bit for bit (f64 subtract and multiply are IEEE on both
    sides); the log loss, through the device's log, within 1e-12 of scikit-learn's: the terms
    share a sign and each is off by a few ulp."""
    y, p, limbs = rows(f32)
    acc = new_acc(sa).add(*padded(y[:n], p[:n]))
    h = acc.buf.cpu().numpy()
    assert h[8] == 0 and h[9] == 0
    assert h[:2].tolist() == [n, int(y[:n].sum())]
    assert h[2:5].tolist() == limbs[:n].sum(axis=0).tolist()
    if n == 0:
        with pytest.raises(ValueError):
            acc.finalize()
        return
    res = acc.finalize()
    assert res['auroc'] is None and res['n'] == n
    assert res['brier'] == py_finalize(*h[2:5].tolist(), BRIER_EXP) / n
    d = p[:n].astype(np.float64) - y[:n]
    want = math.fsum((d * d).tolist()) / n
    assert abs(res['brier'] - want) <= 1e-14 * want
    want = ref_log_loss(y[:n], p[:n])
    print(n, 'f32' if f32 else 'f64', 'log_loss rel', abs(res['log_loss'] - want) / want)
    assert abs(res['log_loss'] - want) <= 1e-12 * want


@DTYPES
def test_two_batches_give_the_limbs_of_one(sa, f32):
    y, p, _ = rows(f32)
    n = 5000
    yd, pd_ = padded(y[:n], p[:n])
    one = new_acc(sa).add(yd, pd_).buf.cpu()
    for split in (1, 64, n - 1):  # the second batch starts unaligned: the scalar loads
        two = new_acc(sa).add(yd[:split], pd_[:split]).add(yd[split:], pd_[split:])
        assert two.rows == n and torch.equal(two.buf.cpu(), one), split


# ----------------------------------------------------------------------------- AUROC
def auc_case(name: str, f32: bool):
    rng = np.random.default_rng([17, int(f32)])
    dt = np.float32 if f32 else np.float64

    def rare(n, m):
        y = np.zeros(n, np.uint8)
        y[rng.choice(n, m, replace=False)] = 1
        return y, np.clip(0.2 * y + rng.beta(1.0, 3.0, n), 0, 1).astype(dt)

    if name.startswith('m='):
        m = int(name[2:].split('_')[0])
        y, p = rare(100000 if m == 40000 else 6000 if m > 2000 else 5000 if m > 3 else 300, m)
        if name.endswith('_negatives'):
            y = 1 - y
    elif name == 'balanced':
        y, p = rare(4000, 2000)
    elif name == 'all_equal':
        y, p = rare(700, 90)
        p[:] = 0.5
    elif name == 'zeros_and_ends':
        y, _ = rare(3000, 1100)
        tiny = 1e-45 if f32 else 5e-324
        p = rng.choice(np.array([0.0, -0.0, 1.0, tiny]), len(y)).astype(dt)
        assert (p == 0).sum() > 1000 and np.signbit(p).any() and (p == dt(tiny)).any()
    elif name == 'heavy_ties':
        y, p = rare(5000, 1300)
        p = (np.round(p * 16) / 16).astype(dt)
    else:  # majority rows below and above every minority key
        assert name == 'both_ends'
        y, _ = rare(3000, 1200)
        p = np.where(y == 1, rng.uniform(0.4, 0.6, len(y)), rng.choice([0.0, 0.1, 0.39, 0.61, 0.9, 1.0], len(y)))
        p = p.astype(dt)
    return y.astype(np.uint8), p


AUC_CASES = ['m=1', 'm=2', 'm=3', 'm=3_negatives', f'm={SAMPLE - 1}', f'm={SAMPLE}', f'm={SAMPLE + 1}',
             f'm={SAMPLE + 1}_negatives', f'm={2 * SAMPLE - 1}', f'm={2 * SAMPLE}', f'm={2 * SAMPLE + 1}',
             'm=40000', 'm=40000_negatives', 'balanced', 'all_equal', 'zeros_and_ends', 'heavy_ties',
             'both_ends']


@DTYPES
@pytest.mark.parametrize('name', AUC_CASES)
def test_auroc_counts_equal_the_searchsorted_restatement(sa, name, f32):
    y, p = auc_case(name, f32)
    acc = sa.binary_metrics(*padded(y, p))
    h = acc.buf.cpu().tolist()
    n, n_pos = len(y), int(y.sum())
    assert h[8] == 0 and h[:2] == [n, n_pos]
    assert h[9] == u2_reference(y, p)
    res = acc.finalize()
    assert res['auroc'] == h[9] / (2 * n_pos * (n - n_pos))
    want = roc_auc_score(y, p.astype(np.float64))
    print(name, 'f32' if f32 else 'f64', 'auroc ulps', ulps(res['auroc'], want))
    assert ulps(res['auroc'], want) <= 2


@DTYPES
@pytest.mark.parametrize('cap', [0, 1, 700, 1300, 1301])
def test_auc_keys_drops_the_keys_past_capacity(sa, cap, f32):
    """The C contract of sa_auc_keys: the cursor advances by every minority row, at most
    `capacity` keys are written (each one a minority row's, none twice) and nothing behind them."""
    from socceraction_amd import _native
    y, p = auc_case('heavy_ties', f32)  # 5000 rows (two workgroups), 1300 positives
    yd, pd_ = padded(y, p)
    m, guard = int(y.sum()), 64
    kdt = np.uint32 if f32 else np.uint64
    fill = -12345
    keys = torch.full((cap + guard,), fill, dtype=torch.int32 if f32 else torch.int64, device='cuda')
    cursor = torch.zeros(1, dtype=torch.int64, device='cuda')
    _native.check(_native.lib().sa_auc_keys(yd.data_ptr(), pd_.data_ptr(), int(f32), len(y), 1, keys.data_ptr(), cap,
                                            cursor.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert int(cursor.item()) == m
    h = keys.cpu().numpy()
    assert (h[cap:] == fill).all()
    want = np.sort(p[y == 1].view(kdt))  # no -0.0 among them: the key is the bit pattern
    got = np.sort(h[:min(cap, m)].view(kdt))
    if cap >= m:
        assert (got == want).all() and (h[m:cap] == fill).all()
    else:  # a sub-multiset of the minority keys
        vals, counts = np.unique(got, return_counts=True)
        ref_vals, ref_counts = np.unique(want, return_counts=True)
        idx = np.searchsorted(ref_vals, vals)
        assert (idx < len(ref_vals)).all() and (ref_vals[idx] == vals).all() and (counts <= ref_counts[idx]).all()


# ----------------------------------------------------------------------------- past the grid cap
PERIOD = 4099  # prime: consecutive chunks start at different offsets of the base rows


def past_the_cap_rows():
    """A row count just past the grid's cap of R workgroups on this device: workgroups 0 and 1
    take a second chunk and the last chunk is partial (n is odd: a scalar tail)."""
    R = WG_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    n = R * CHUNK + CHUNK + 777
    assert n < 2 ** 30, f'{R} resident workgroups put n = {n} past the 2^30 rows the score kernels take'
    assert n > R * CHUNK and (n + CHUNK - 1) // CHUNK == R + 2
    return R, n


@DTYPES
def test_sums_of_more_chunks_than_resident_workgroups(sa, f32):
    """metric_sums_kernel's second trip.  Row i is row i % PERIOD of rows(): every sum is the
    base rows' term times its multiplicity -- integers for the counts and the Brier limbs, and
    math.fsum of the float64 log-loss terms under the 1e-12 bar of
    test_sums_equal_the_integer_restatement (its reasoning does not depend on n)."""
    R, n = past_the_cap_rows()
    y, p, limbs = rows(f32)
    y, p, limbs = y[:PERIOD], p[:PERIOD], limbs[:PERIOD]
    mult = n // PERIOD + (np.arange(PERIOD) < n % PERIOD).astype(np.int64)
    assert int(mult.sum()) == n and mult.max() < 2 ** 12
    acc = new_acc(sa).add(*padded(np.resize(y, n), np.resize(p, n)))
    h = acc.buf.cpu().numpy()
    assert h[8] == 0 and h[9] == 0
    assert h[:2].tolist() == [n, int((mult * y).sum())]
    assert h[2:5].tolist() == (mult[:, None] * limbs).sum(axis=0).tolist()
    res = acc.finalize()
    assert res['n'] == n and res['brier'] == py_finalize(*h[2:5].tolist(), BRIER_EXP) / n
    # the kernel's contract for q: the complement and the clip in p's dtype, -log in float64
    eps = np.finfo(p.dtype).eps
    q = np.clip(np.where(y == 1, p, p.dtype.type(1) - p), eps, p.dtype.type(1) - eps)
    assert q.dtype == p.dtype
    terms = -np.log(q.astype(np.float64))
    assert abs(math.fsum(terms.tolist()) / PERIOD - ref_log_loss(y, p)) <= 1e-12 * ref_log_loss(y, p)
    want = math.fsum((terms * mult).tolist()) / n
    print('f32' if f32 else 'f64', 'n', n, 'log_loss rel', abs(res['log_loss'] - want) / want)
    assert abs(res['log_loss'] - want) <= 1e-12 * want


@DTYPES
@pytest.mark.parametrize('minority', [1, 0], ids=['few_positives', 'few_negatives'])
def test_auroc_of_more_chunks_than_resident_workgroups(sa, minority, f32):
    """The three AUROC kernels' second trip, the key stage carried from chunk to chunk: free
    (not periodic) probabilities, about 20% minority rows, a band of heavy ties, exact 0 and 1."""
    from socceraction_amd import _native
    R, n = past_the_cap_rows()
    rng = np.random.default_rng([23, minority, int(f32)])
    y = (rng.random(n) < 0.2).astype(np.uint8)
    p = np.clip(0.25 * y + 0.8 * rng.random(n), 0, 1)
    band = rng.random(n) < 0.15
    p[band] = np.round(p[band] * 64) / 64
    p[rng.random(n) < 0.01] = 0.0
    p[rng.random(n) < 0.01] = 1.0
    p = p.astype(np.float32 if f32 else np.float64)
    if not minority:
        y = 1 - y
    n_pos = int(y.sum())
    m = n_pos if minority else n - n_pos
    assert 0.15 * n < m < 0.25 * n and not np.signbit(p).any()
    yd, pd_ = padded(y, p)
    acc = sa.binary_metrics(yd, pd_)
    h = acc.buf.cpu().tolist()
    assert h[8] == 0 and h[:2] == [n, n_pos]
    # U2 is a function of the multiset of rows: u2_reference on the rows reordered -- the positives
    # first, ascending -- looks up sorted values, several times faster at this size
    a, b = np.sort(p[y == 1]), p[y == 0]
    assert len(a) == n_pos and len(a) + len(b) == n
    assert h[9] == u2_reference(np.repeat(np.array([1, 0], np.uint8), [len(a), len(b)]), np.concatenate([a, b]))
    assert acc.finalize()['auroc'] == h[9] / (2 * n_pos * (n - n_pos))
    # sa_auc_keys itself: the cursor counts every minority row, the keys are their bit patterns
    guard, fill = 64, -12345
    keys = torch.full((m + guard,), fill, dtype=torch.int32 if f32 else torch.int64, device='cuda')
    cursor = torch.zeros(1, dtype=torch.int64, device='cuda')
    _native.check(_native.lib().sa_auc_keys(yd.data_ptr(), pd_.data_ptr(), int(f32), n, minority, keys.data_ptr(), m,
                                            cursor.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert int(cursor.item()) == m
    got = keys.cpu().numpy()
    assert (got[m:] == fill).all()
    kdt = np.uint32 if f32 else np.uint64
    assert (np.sort(got[:m].view(kdt)) == np.sort(p[y == minority].view(kdt))).all()


# ----------------------------------------------------------------------------- order independence
@DTYPES
def test_a_row_permutation_gives_the_same_dict(sa, f32):
    from socceraction_amd import metrics
    y, p, _ = rows(f32)
    yd, pd_ = padded(y[:5000], p[:5000])
    first = metrics.binary_scores(yd, pd_)
    perm = torch.from_numpy(np.random.default_rng(8).permutation(5000)).cuda()
    again = metrics.binary_scores(yd[perm], pd_[perm])
    assert set(first) == set(metrics.KEYS)
    assert {k: np.float64(v).tobytes() for k, v in first.items()} == \
        {k: np.float64(v).tobytes() for k, v in again.items()}
    assert metrics.binary_scores(yd, pd_) == first  # and from run to run
    host = metrics.binary_scores_host(y[:5000], p[:5000])  # the numpy path: all but the device's log
    assert {k: v for k, v in host.items() if k != 'log_loss'} == {k: v for k, v in first.items() if k != 'log_loss'}


# ----------------------------------------------------------------------------- error bits
@DTYPES
def test_error_bits_raise_and_their_rows_add_nothing(sa, f32):
    from socceraction_amd import _native, metrics
    y, p, limbs = rows(f32)
    n = 3000
    for what, bit in (('nan', _native.SA_METRIC_ERR_NAN), ('negative', _native.SA_METRIC_ERR_RANGE),
                      ('above', _native.SA_METRIC_ERR_RANGE), ('inf', _native.SA_METRIC_ERR_RANGE),
                      ('label', _native.SA_METRIC_ERR_LABEL)):
        yy, pp = y[:n].copy(), p[:n].copy()
        row = {'nan': 5, 'negative': 1500, 'above': 2999, 'inf': 64, 'label': 255}[what]
        if what == 'label':
            yy[row] = 2
        else:
            pp[row] = {'nan': np.nan, 'negative': -0.25, 'above': 1.5, 'inf': np.inf}[what]
        yd, pd_ = padded(yy, pp)
        acc = new_acc(sa).add(yd, pd_)
        h = acc.buf.cpu().numpy()
        keep = np.arange(n) != row
        assert h[8] == bit, what
        assert h[:2].tolist() == [n - 1, int(y[:n][keep].sum())], what
        assert h[2:5].tolist() == limbs[:n][keep].sum(axis=0).tolist(), what
        with pytest.raises(ValueError):
            acc.finalize()
        with pytest.raises(ValueError):
            metrics.binary_scores(yd, pd_)
    yd, pd_ = padded(np.zeros(n, np.uint8), p[:n])
    with pytest.raises(ValueError, match='one class'):
        metrics.binary_scores(yd, pd_)
    with pytest.raises(ValueError, match='one class'):
        metrics.binary_scores(yd + 1, pd_)
    # a following valid call
    res = metrics.binary_scores(*padded(y[:n], p[:n]))
    wide = p[:n].astype(np.float64)
    assert ulps(res['auroc'], roc_auc_score(y[:n], wide)) <= 2
    assert abs(res['brier'] - brier_score_loss(y[:n], wide)) <= 1e-14 * res['brier']
    assert abs(res['log_loss'] - ref_log_loss(y[:n], p[:n])) <= 1e-12 * res['log_loss']
    base = np.full(n, y[:n].mean())
    assert abs(res['brier_baseline'] - brier_score_loss(y[:n], base)) <= 1e-14 * res['brier_baseline']
    assert abs(res['log_loss_baseline'] - log_loss(y[:n], base)) <= 1e-14 * res['log_loss_baseline']


def test_host_arrays_are_uploaded(sa):
    """numpy arrays and pandas Series go through the same kernels as device tensors."""
    from socceraction_amd import metrics
    y, p, _ = rows(False)
    want = metrics.binary_scores(*padded(y[:999], p[:999]))
    assert metrics.binary_scores(y[:999], p[:999]) == want
    assert metrics.binary_scores(pd.Series(y[:999].astype(bool)), pd.Series(p[:999])) == want
    with pytest.raises(ValueError):
        metrics.binary_scores(np.where(np.arange(999) == 7, 2, y[:999]), p[:999])


# ----------------------------------------------------------------------------- VAEP.score_batch
SCORE_KEYS = {'brier', 'auroc', 'log_loss', 'brier_baseline', 'log_loss_baseline'}


def check_score_batch(model, games, actions, X, Y, f64: bool):
    from socceraction_amd import metrics
    n = len(actions)
    got = model.score_batch(games, actions)
    _, proba = model._probabilities_batch(games, actions)  # what rate_batch's path produces
    assert set(got) == set(proba) == {'scores', 'concedes'}
    for c in got:
        y_hat = proba[c][:n].cpu().numpy()
        assert y_hat.dtype == (np.float64 if f64 else np.float32)
        want = metrics.binary_scores(Y[c].to_numpy(), y_hat)
        assert set(got[c]) == SCORE_KEYS
        for k in SCORE_KEYS:
            assert np.float64(got[c][k]).tobytes() == np.float64(want[k]).tobytes(), (c, k)
    if f64:
        ref = model.score(X, Y)
        for c in got:
            print(c, 'auroc ulps', ulps(got[c]['auroc'], ref[c]['auroc']), 'brier rel',
                  abs(got[c]['brier'] - ref[c]['brier']) / ref[c]['brier'])
            assert ulps(got[c]['auroc'], ref[c]['auroc']) <= 2
            assert abs(got[c]['brier'] - ref[c]['brier']) <= 1e-14 * ref[c]['brier']


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
def test_vaep_score_batch(sa, fitted, learner):
    """score_batch == metrics.binary_scores(labels, the probabilities of rate_batch's path) bit
    for bit, and == VAEP.score for the float64 learners; rate_batch is unchanged by it."""
    from sklearn.exceptions import NotFittedError
    from socceraction_amd import trees
    model, games, actions, X, Y = fitted
    model._VAEP__models = {}
    with pytest.raises(NotFittedError):
        model.score_batch(games, actions)
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
    check_score_batch(model, games, actions, X, Y, f64=learner != 'xgboost_format')
    # another look-ahead changes the labels, not the probabilities
    short = model.score_batch(games, actions, nr_actions=3)
    assert short['scores']['brier_baseline'] < model.score_batch(games, actions)['scores']['brier_baseline']


def test_atomic_vaep_score_batch(sa):
    from sklearn.ensemble import HistGradientBoostingClassifier
    from socceraction_amd import synthetic
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
    check_score_batch(model, games, actions, X, Y, f64=True)
