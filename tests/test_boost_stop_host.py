"""Host side of held-out evaluation and early stopping for the device learner, no GPU: the
stopping rule on hand-written integer series, the numpy restatement of contract items 9-12
(tests/boost_stop_reference.py) on a table whose AUROC series is not monotone, the error paths
that must come before any device call, and ``sa_boost_apply``'s argument validation."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import boost_reference as br
import boost_stop_reference as bs


@pytest.fixture(scope='module')
def boost():
    from socceraction_amd import boost
    return boost


# ----------------------------------------------------------------------------- the rule
def _both(boost, series, rounds, maximize):
    got = boost.stop_decision(series, rounds, maximize)
    assert got == bs.stopping(series, rounds, maximize)
    return got


def test_stop_decision_strict_improvement_only(boost):
    # a tie does not reset the counter, and the first round holding the best score is kept
    assert _both(boost, [5, 7, 7, 7, 7, 9], 3, True) == (1, 5)
    assert _both(boost, [5, 5, 5], 2, True) == (0, 3)
    assert _both(boost, [5, 5, 5, 5], 2, True) == (0, 3)


def test_stop_decision_counter_resets_after_a_dip(boost):
    #               0  1  2  3  4  5  6  7  8
    series = [10, 12, 11, 11, 13, 12, 12, 12, 20]
    assert _both(boost, series, 3, True) == (4, 8)   # two rounds after 1, reset at 4, three after it
    assert _both(boost, series, 2, True) == (1, 4)
    assert _both(boost, series, 4, True) == (8, 9)   # round 8 arrives before the counter reaches 4


def test_stop_decision_fires_exactly_at_best_plus_rounds(boost):
    for rounds in (1, 2, 5, 10):
        series = [1, 2, 3] + [0] * 20
        best, run = _both(boost, series, rounds, True)
        assert (best, run) == (2, 2 + rounds + 1)     # the last round run is round best + rounds
    assert _both(boost, [3, 2, 1], 1, True) == (0, 2)


def test_stop_decision_never_firing_gives_argbest_and_len(boost):
    series = [1, 5, 2, 6, 3, 7, 4]
    assert _both(boost, series, 2, True) == (5, 7)
    assert _both(boost, series + [7, 7, 7], None, True) == (5, 10)
    assert _both(boost, [4], 1, True) == (0, 1)
    assert _both(boost, [], 3, True) == (0, 0)
    big = [2 ** 90 + 1, 2 ** 90 + 2, 2 ** 90]        # Python integers: no rounding to a double
    assert _both(boost, big, 5, True) == (1, 3)


def test_stop_decision_minimising(boost):
    series = [9, 7, 8, 7, 6, 6, 7, 8, 1]
    assert _both(boost, series, 3, False) == (4, 8)
    assert _both(boost, series, 4, False) == (8, 9)
    assert _both(boost, series, 3, True) == (0, 4)


def test_polling_schedule_meets_the_stopping_round(boost):
    """The host looks after round ``rounds``, then after ``best + rounds`` as known at the last
    look (``boost.stop_look``): it launches exactly the rounds the rule asks for, with few looks."""
    rng = np.random.default_rng(0)
    for case in range(400):
        T = int(rng.integers(1, 60))
        rounds = int(rng.integers(1, 12))
        kind = case % 4
        series = rng.integers(0, (3, 50, 10 ** 6)[case % 3], T).tolist()  # many ties, some, none
        if kind == 1:
            series = np.cumsum(np.abs(series)).tolist()  # improves (weakly) to the end: never fires
        elif kind == 2:
            series = (np.cumsum(rng.integers(-2, 4, T)) * 3).tolist()  # a drifting walk with dips
        for maximize in (True, False):
            look, launched, looks = rounds, T, 0
            for t in range(T):
                if t == look and t + 1 < T:
                    looks += 1
                    fired, look = boost.stop_look(series[:t + 1], rounds, maximize)
                    if fired:
                        launched = t + 1
                        break
            want = bs.stopping(series, rounds, maximize)
            assert launched == want[1], (series, rounds, maximize)
            assert bs.stopping(series[:launched], rounds, maximize) == want
            assert looks <= 2 * (-(-T // (rounds + 1))) + 1
            if kind == 1 and maximize and len(set(series)) == T:  # every look finds the newest round best
                assert looks <= -(-T // rounds)
    assert boost.stop_look([1, 2, 3, 3], 3, True) == (False, 5)     # the ambiguity of (best, len) resolved:
    assert boost.stop_look([3, 3, 3, 3], 3, True) == (True, 3)      # a series that fires at its last round
    assert boost.stop_look([3, 2, 1, 0], 3, False) == (False, 6)


# ----------------------------------------------------------------------------- the restatement
def _table(seed=0, n=12000):
    """The synthetic table of tests/test_boost_host.py: 5 normal + 5 Bernoulli(0.2) columns."""
    rng = np.random.default_rng(seed)
    Xn = rng.normal(size=(n, 5))
    Xb = rng.random((n, 5)) < 0.2
    logit = 1.2 * Xn[:, 0] - 0.8 * (Xn[:, 1] > 0.3) + 1.5 * Xb[:, 0] * Xn[:, 2] - 1.0 * Xb[:, 1] - 1.5
    y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(int)
    return Xn, Xb, y


def stop_table():
    """1,500 rows of seed 0: the first 1,000 train (and give the cuts), the last 500 are held
    out.  ``(frame, y, cuts, B)``; also used by tests/test_gpu_boost_stop.py."""
    Xn, Xb, y = _table(seed=0, n=1500)
    cols = {f'n{j}': Xn[:, j] for j in range(5)}
    cols.update({f'b{j}': Xb[:, j] for j in range(5)})
    X = pd.DataFrame(cols)
    cuts = [br.cuts_of(X[c].to_numpy()[:1000], X[c].dtype == np.bool_) for c in X.columns]
    B = np.stack([br.bins_of(br.cast32(X[c].to_numpy()), k) for c, k in zip(X.columns, cuts)])
    return X, y, cuts, B


@pytest.fixture(scope='module')
def restated():
    """One 40-round restated fit per metric without stopping: the stopping rule is a function of
    the series, so every patience is read off it."""
    X, y, cuts, B = stop_table()
    train = np.arange(1500) < 1000
    out = {m: bs.fit(B, y, cuts, train, np.arange(1000, 1500), metric=m, n_estimators=40)
           for m in ('auc', 'logloss')}
    return X, y, cuts, B, out


def test_restated_trainer_with_held_out_rows(boost, restated):
    X, y, cuts, B, out = restated
    assert int(y[1000:].sum()) == 87
    auc, ll = out['auc']['series'], out['logloss']['series']
    print('auc', [round(v / (2 * 87 * 413), 5) for v in auc])
    print('logloss', [round(bs.metric_score(v, 'logloss', y[1000:]), 5) for v in ll])
    assert auc[5] < auc[4] and auc[8] < auc[7]  # not monotone: the rule has dips to sit out
    want = {('auc', 3): (9, 13), ('logloss', 3): (11, 15), ('auc', 5): (9, 15), ('logloss', 5): (11, 17)}
    for (metric, rounds), res in want.items():
        series = out[metric]['series']
        assert bs.stopping(series, rounds, metric == 'auc') == res, (metric, rounds)
        assert boost.stop_decision(series, rounds, metric == 'auc') == res, (metric, rounds)
    # the trainer that stops by itself runs exactly those rounds and builds the same trees
    train = np.arange(1500) < 1000
    short = bs.fit(B, y, cuts, train, np.arange(1000, 1500), metric='auc', early_stopping_rounds=3,
                   n_estimators=40)
    assert (short['best_iteration'], short['rounds_run']) == (9, 13) and len(short['kept']) == 10
    assert short['series'] == auc[:13]
    assert np.stack(short['tables']).tobytes() == np.stack(out['auc']['tables'][:13]).tobytes()
    # evaluation never touches training: the held-out rows take no part in any tree
    assert np.stack(out['auc']['tables']).tobytes() == np.stack(out['logloss']['tables']).tobytes()
    alone, _, _ = br.fit(B[:, :1000], y[:1000], cuts, n_estimators=13)
    assert alone.tobytes() == np.stack(short['tables']).tobytes()


def test_restated_metrics_are_the_library_definitions(boost, restated):
    """U2 by brute force and the fixed-point log-loss integer against the host statement of
    ``sa_auc_count`` / ``sa_metric_sums`` (socceraction_amd.metrics), and the applied margins
    against the predictor's walk on values."""
    from socceraction_amd import metrics
    X, y, cuts, B, out = restated
    ye = y[1000:]
    X32 = np.stack([br.cast32(X[c].to_numpy()) for c in X.columns], 1)
    for t in (0, 5, 12, 39):
        ep = out['auc']['eval_p'][t]
        assert ep.dtype == np.float32
        host = metrics.binary_scores_host(ye.astype(bool), ep)
        assert out['auc']['series'][t] / (2 * 87 * 413) == host['auroc']
        assert bs.metric_score(out['logloss']['series'][t], 'logloss', ye) == host['log_loss']
        assert boost.metric_score(out['logloss']['series'][t], 'logloss', 500, 87) == host['log_loss']
        assert boost.metric_score(out['auc']['series'][t], 'auc', 500, 87) == host['auroc']
        np.testing.assert_array_equal(ep, br.predict(out['auc']['tables'][:t + 1], X32[1000:]))
    # the clip of the log-loss terms: p = 0 and p = 1 on the wrong side cost -log(eps32)
    eps = np.finfo(np.float32).eps
    terms = bs.logloss_terms([1, 0, 1, 0], np.array([0.0, 1.0, 1.0, 0.0], np.float32))
    np.testing.assert_array_equal(terms[:2], [-np.log(np.float64(eps))] * 2)
    np.testing.assert_array_equal(terms[2:], [-np.log(np.float64(np.float32(1.0) - eps))] * 2)
    assert bs.u2_of([1, 1, 0, 0], [0.5, 0.2, 0.5, 0.1]) == 1 + 2 + 0 + 2
    # metric_integer reads the BinaryMetrics layout: count[2], brier[3], logloss[3], err, u2
    row = [500, 87, 1, 2, 3, 7, 8, 9, 0, 12345]
    assert boost.metric_integer(row, 'auc') == 12345
    assert boost.metric_integer(row, 'logloss') == 7 + (8 << 32) + (9 << 64)


# ----------------------------------------------------------------------------- error paths
def test_early_stopping_errors_come_before_any_device_call(boost, monkeypatch):
    import socceraction_amd.vaep as vaep
    from socceraction_amd import _native
    import torch

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(_native, 'lib', no_device)
    monkeypatch.setattr(torch, 'as_tensor', no_device)
    monkeypatch.setattr(boost, 'bin_host', no_device)
    monkeypatch.setattr(boost, 'bin_blocks', no_device)
    with pytest.raises(ValueError, match='eval_metric'):
        boost.DeviceGBTClassifier(eval_metric='error')
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='early_stopping_rounds'):
            boost.DeviceGBTClassifier(early_stopping_rounds=bad)
    with pytest.raises(ValueError, match='early_stopping_rounds'):
        boost.check_stop_params(0, 'auc')
    assert boost.check_stop_params(None, 'logloss') == (None, 'logloss')
    assert boost.check_stop_params(np.int64(4), 'auc') == (4, 'auc')
    clf = boost.DeviceGBTClassifier(early_stopping_rounds=3, eval_metric='logloss')
    assert (clf.early_stopping_rounds, clf.eval_metric) == (3, 'logloss')
    assert clf.get_params() == dict(boost.DEFAULTS)  # the tree parameters only, as before
    X = pd.DataFrame({'a': np.arange(8.0), 'b': np.arange(8) % 2 == 0})
    y = np.arange(8) % 2
    # patience without evaluation rows
    with pytest.raises(ValueError, match='needs evaluation rows'):
        clf.fit(X, y)
    with pytest.raises(ValueError, match='needs evaluation rows'):
        clf.fit_binned(None, None)
    with pytest.raises(ValueError, match='needs evaluation rows'):
        clf.fit_blocks(None, None, rows=[0, 1])
    # eval_set takes exactly one pair
    with pytest.raises(ValueError, match='exactly one'):
        clf.fit(X, y, eval_set=[(X, y), (X, y)])
    with pytest.raises(ValueError, match='exactly one'):
        boost.DeviceGBTClassifier().fit(X, y, eval_set=[])
    with pytest.raises(ValueError, match='columns'):
        clf.fit(X, y, eval_set=[(X[['b', 'a']], y)])
    # the public path
    model = vaep.VAEP()
    none = pd.DataFrame({'game_id': [], 'home_team_id': []})
    with pytest.raises(ValueError, match='val_size'):
        model.fit_batch(none, pd.DataFrame(), early_stopping_rounds=3)            # val_size == 0
    with pytest.raises(ValueError, match='early_stopping_rounds'):
        model.fit_batch(none, pd.DataFrame(), val_size=0.25, early_stopping_rounds=0)
    with pytest.raises(ValueError, match='eval_metric'):
        model.fit_batch(none, pd.DataFrame(), val_size=0.25, early_stopping_rounds=3, eval_metric='rmse')
    cols = model._fs.feature_column_names(model.xfns, model.nb_prev_actions)
    Xv = pd.DataFrame(np.zeros((8, len(cols))), columns=cols)
    yv = pd.DataFrame({'scores': np.zeros(8, bool), 'concedes': np.zeros(8, bool)})
    with pytest.raises(ValueError, match='eval_metric'):
        model.fit(Xv, yv, learner='device', fit_params=dict(early_stopping_rounds=3, eval_metric='rmse'))
    with pytest.raises(ValueError, match='early_stopping_rounds'):
        model.fit(Xv, yv, learner='device', fit_params=dict(early_stopping_rounds=0))
    with pytest.raises(ValueError, match='val_size'):
        model.fit(Xv, yv, learner='device', val_size=0, fit_params=dict(early_stopping_rounds=3))


def test_boost_apply_validates_without_a_gpu():
    """Every invalid argument is SA_EINVAL before any HIP call; n_rows == 0 is a no-op."""
    from socceraction_amd import _native
    lib = _native.load_library()
    one = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced
    E = _native.SA_EINVAL
    order = ('tree', 'depth', 'fmap', 'bits', 'stride', 'bins', 'ld', 'rows', 'n_rows', 'n', 'margin', 'p', 'st')
    ap = lambda **k: lib.sa_boost_apply(*[{**dict(  # noqa: E731
        tree=one, depth=3, fmap=one, bits=one, stride=8, bins=one, ld=16, rows=one, n_rows=0, n=8, margin=one,
        p=one, st=None), **k}[a] for a in order])
    assert ap() == 0 and ap(rows=None) == 0 and ap(p=None) == 0 and ap(bits=None, stride=0) == 0
    assert ap(bins=None) == 0 and ap(depth=1) == 0 and ap(depth=_native.SA_BOOST_MAX_DEPTH) == 0
    assert ap(depth=0) == E and ap(depth=_native.SA_BOOST_MAX_DEPTH + 1) == E and ap(depth=-1) == E
    assert ap(tree=None) == E and ap(fmap=None) == E and ap(margin=None) == E
    assert ap(ld=7) == E and ap(n=-1) == E and ap(n_rows=-1) == E
    assert ap(stride=4) == E and ap(stride=12) == E and ap(n=65) == E   # 65 rows need 16 bytes a row
    assert ap(n=65, ld=80, stride=16) == 0
    assert ap(bits=ctypes.c_void_p(20)) == E                            # 8-byte alignment
    assert ap(n_rows=5, tree=None) == E                                 # with rows, still before any launch
    assert b'sa_boost_apply' in lib.sa_last_error()
    assert 'sa_boost_apply' in _native.EXPORTED_SYMBOLS
