"""Host side of the device learner's sample weights, row / column subsampling and L1 penalty
(contract items 13-17), no GPU: the counter hash, the numpy restatement
(tests/boost_sample_reference.py) against ``boost_reference`` at neutral parameters, parameter and
weight validation before any device call, the quantisation shift at its boundaries, the feature
importances, and the weight-duplication property that does not depend on the restatement's own
arithmetic."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import boost_reference as br
import boost_sample_reference as bs


def _table(seed=0, n=12000):
    """The synthetic table of tests/test_boost_host.py: 5 normal + 5 Bernoulli(0.2) columns."""
    rng = np.random.default_rng(seed)
    Xn = rng.normal(size=(n, 5))
    Xb = rng.random((n, 5)) < 0.2
    logit = 1.2 * Xn[:, 0] - 0.8 * (Xn[:, 1] > 0.3) + 1.5 * Xb[:, 0] * Xn[:, 2] - 1.0 * Xb[:, 1] - 1.5
    y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(int)
    return Xn, Xb, y


@pytest.fixture(scope='module')
def boost():
    from socceraction_amd import boost
    return boost


@pytest.fixture(scope='module')
def table():
    Xn, Xb, y = _table(n=3000)
    cols = [Xn[:, j] for j in range(5)] + [Xb[:, j] for j in range(5)]
    cuts = [br.cuts_of(c, c.dtype == np.bool_) for c in cols]
    B = np.stack([br.bins_of(br.cast32(c), k) for c, k in zip(cols, cuts)])
    return B, y, cuts


# ----------------------------------------------------------------------------- the hash
def test_hash_check_values_and_the_host_statement(boost):
    assert int(bs.fm(1)) == 0x5692161d100b05e5 and int(bs.fm(2)) == 0xdbd238973a2b148a
    assert boost.fmix64(1) == 0x5692161d100b05e5 and boost.fmix64(2) == 0xdbd238973a2b148a
    rng = np.random.default_rng(0)
    keys = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    keys[:4] = np.array([0, 2 ** 63, 2 ** 64 - 1, 2 ** 63 - 1], np.uint64)
    for salt, seed, t in ((bs.SALT_ROWS, 0, 0), (bs.SALT_COLS, 7, 3), (bs.SALT_ROWS, 2 ** 63 - 1, 99)):
        want = bs.draw(salt, seed, t, keys)
        assert [boost.draw(salt, seed, t, int(k)) for k in keys] == [int(v) for v in want]
    # an int64 key is its uint64 bit pattern
    np.testing.assert_array_equal(bs.draw(1, 2, 3, np.array([-1, -2 ** 63], np.int64)),
                                  bs.draw(1, 2, 3, np.array([2 ** 64 - 1, 2 ** 63], np.uint64)))
    from socceraction_amd import _native
    assert (_native.SA_BOOST_SALT_ROWS, _native.SA_BOOST_SALT_COLS) == (bs.SALT_ROWS, bs.SALT_COLS)
    assert boost.row_threshold(1.0) == 2 ** 32 == bs.threshold(1.0) and boost.row_threshold(0.5) == 2 ** 31
    assert boost.row_threshold(np.nextafter(1.0, 0.0)) == 2 ** 32 - 1
    for F, c in ((10, 0.3), (10, 0.01), (154, 0.5), (7, 1.0)):
        for t in range(4):
            np.testing.assert_array_equal(boost.column_sample(7, t, F, c), bs.column_sample(7, t, F, c))
    assert len(bs.column_sample(7, 0, 10, 0.01)) == 1 and len(bs.column_sample(7, 0, 10, 0.39)) == 3


# ----------------------------------------------------------------------------- the restatement
def test_neutral_parameters_restate_the_plain_trainer_byte_for_byte(table):
    B, y, cuts = table
    tabs, m, ps = br.fit(B, y, cuts, n_estimators=8)
    got, gm, gps, e = bs.fit(B, y, cuts, sample_weight=np.ones(len(y), np.float32), n_estimators=8,
                             subsample=1.0, colsample_bytree=1.0, reg_alpha=0.0, scale_pos_weight=1.0, random_state=5)
    assert e == 0 and got.tobytes() == tabs.tobytes() and gm.tobytes() == m.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ps, gps))


ALL_ON = dict(n_estimators=8, max_depth=3, subsample=0.5, colsample_bytree=0.3, reg_alpha=0.5, scale_pos_weight=3.0,
              random_state=7)


def test_every_option_on_still_splits_and_depends_on_seed_and_keys(table):
    B, y, cuts = table
    rng = np.random.default_rng(1)
    w = (rng.random(len(y)) * 5).astype(np.float32)
    w[::17] = 0
    w[5] = 8.0
    tabs, m, _, e = bs.fit(B, y, cuts, sample_weight=w, **ALL_ON)
    assert e == (5 if y[5] else 4)  # 8 * 3 = 24 <= 2^5 when the row of weight 8 is positive, else 5 * 3 < 2^4
    is_split = (tabs['feature'] >= 0) & (tabs['exists'] != 0)  # (a record that does not exist is all zero)
    print('splits per round', is_split.sum(1).tolist())
    assert (is_split.sum(1) >= 1).all()
    for t in range(8):  # a feature outside the round's column sample never splits
        used = set(tabs[t]['feature'][is_split[t]].tolist())
        assert used <= set(bs.column_sample(7, t, 10, 0.3).tolist())
    other, _, _, _ = bs.fit(B, y, cuts, sample_weight=w, **{**ALL_ON, 'random_state': 8})
    assert other.tobytes() != tabs.tobytes()
    perm = np.random.default_rng(2).permutation(len(y))
    moved, mm, _, _ = bs.fit(B[:, perm], y[perm], cuts, sample_weight=w[perm], row_keys=perm, **ALL_ON)
    assert moved.tobytes() == tabs.tobytes() and mm.tobytes() == m[perm].tobytes()
    dropped, _, _, _ = bs.fit(B[:, perm], y[perm], cuts, sample_weight=w[perm], **ALL_ON)
    assert dropped.tobytes() != tabs.tobytes()


def test_weight_duplication_property(table):
    """Uniform weight 2 against the table stacked twice: the same trees, G and H exactly doubled
    in the stacked fit (e = 1 halves the unit), the first copy's margins byte-equal."""
    B, y, cuts = table
    n = len(y)
    tw, mw, _, e = bs.fit(B, y, cuts, sample_weight=np.full(n, 2.0, np.float32), n_estimators=6)
    ts, ms, _, e2 = bs.fit(np.concatenate([B, B], 1), np.concatenate([y, y]), cuts, n_estimators=6)
    assert (e, e2) == (1, 0)
    for field in ('feature', 'cut', 'thr', 'gain', 'value', 'exists'):
        assert tw[field].tobytes() == ts[field].tobytes(), field
    np.testing.assert_array_equal(ts['G'], 2 * tw['G'])
    np.testing.assert_array_equal(ts['H'], 2 * tw['H'])
    assert ms[:n].tobytes() == mw.tobytes() and ms[n:].tobytes() == mw.tobytes()
    assert ((tw['feature'] >= 0) & (tw['exists'] != 0)).sum() >= 6


# ----------------------------------------------------------------------------- the shift
def test_shift_boundaries(boost):
    f32 = np.float32
    for mx, e in ((f32(1), 0), (np.nextafter(f32(1), f32(2)), 1), (f32(8), 3), (np.nextafter(f32(8), f32(9)), 4),
                  (f32(0.25), 0), (f32(2.0 ** 20), 20), (np.nextafter(f32(2.0 ** 19), f32(2.0 ** 20)), 20),
                  (f32(1e-45), 0)):
        assert boost.weight_shift(float(mx)) == e == bs.shift_of(mx), mx
    with pytest.raises(ValueError):
        bs.shift_of(np.nextafter(f32(2.0 ** 20), f32(2.0 ** 21)))
    with pytest.raises(ValueError):
        bs.shift_of(0.0)


# ----------------------------------------------------------------------------- validation
def test_new_parameters_and_weights_are_validated_before_any_device_call(boost, monkeypatch):
    import socceraction_amd.vaep as vaep
    from socceraction_amd import _native

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(_native, 'lib', no_device)
    monkeypatch.setattr(boost, 'bin_host', no_device)
    monkeypatch.setattr(boost, 'bin_blocks', no_device)
    good = dict(subsample=0.5, colsample_bytree=0.25, reg_alpha=2.0, scale_pos_weight=3.0, random_state=2 ** 63 - 1)
    p = boost.check_params(good)
    assert all(p[k] == v for k, v in good.items())
    assert boost.check_params(dict(subsample=1, colsample_bytree=1, random_state=np.int64(4)))['random_state'] == 4
    clf = boost.TunedGBTClassifier(**good)
    assert clf.get_params() == {**boost.ALL_DEFAULTS, **good}
    # the plain classifier keeps its parameter set: the tuning parameters belong to the subclass
    with pytest.raises(ValueError, match='unknown parameters'):
        boost.DeviceGBTClassifier(subsample=0.5)
    assert boost.DeviceGBTClassifier().get_params() == dict(boost.DEFAULTS) and len(boost.DEFAULTS) == 7
    assert boost.TunedGBTClassifier().get_params() == boost.ALL_DEFAULTS
    assert type(boost.make_classifier(boost.check_params({}))) is boost.DeviceGBTClassifier
    neutral = boost.check_params(dict(n_estimators=3, subsample=1.0))
    assert type(boost.make_classifier(neutral)) is boost.DeviceGBTClassifier
    tuned = boost.make_classifier(boost.check_params(dict(reg_alpha=0.5)), early_stopping_rounds=None)
    assert type(tuned) is boost.TunedGBTClassifier and tuned.reg_alpha == 0.5
    assert {k: boost.TUNING_DEFAULTS[k] for k in ('subsample', 'colsample_bytree', 'reg_alpha', 'scale_pos_weight',
                                           'random_state')} == dict(subsample=1.0, colsample_bytree=1.0,
                                                                    reg_alpha=0.0, scale_pos_weight=1.0, random_state=0)
    bad = [dict(subsample=0.0), dict(subsample=1.0000001), dict(subsample=-0.5), dict(subsample=float('nan')),
           dict(colsample_bytree=0.0), dict(colsample_bytree=1.5), dict(colsample_bytree=float('nan')),
           dict(reg_alpha=-1e-9), dict(reg_alpha=float('nan')), dict(reg_alpha=float('inf')),
           dict(scale_pos_weight=0.0), dict(scale_pos_weight=-1.0), dict(scale_pos_weight=float('nan')),
           dict(random_state=-1), dict(random_state=1.5), dict(random_state=2.0), dict(random_state=2 ** 63),
           dict(random_state=True), dict(random_state=None), dict(colsample_bylevel=0.5), dict(colsample_bynode=0.5)]
    model = vaep.VAEP()
    none = pd.DataFrame({'game_id': [], 'home_team_id': []})
    cols = model._fs.feature_column_names(model.xfns, model.nb_prev_actions)
    X = pd.DataFrame(np.zeros((8, len(cols))), columns=cols)
    y = pd.DataFrame({'scores': np.arange(8) % 2 == 0, 'concedes': np.zeros(8, bool)})
    for params in bad:
        with pytest.raises(ValueError):
            boost.check_params(params)
        with pytest.raises(ValueError):
            boost.TunedGBTClassifier(**params)
        with pytest.raises(ValueError):
            model.fit(X, y, learner='device', tree_params=params)
        with pytest.raises(ValueError):
            model.fit_batch(none, pd.DataFrame(), tree_params=params)
    with pytest.raises(ValueError, match='unknown parameters'):
        boost.check_params(dict(colsample_bylevel=0.5))
    # weights
    ok = np.array([0, 1, 2.5, 0, 1, 1, 1, 2.0 ** 20])
    w, e = boost.check_weights(ok, 8, y['scores'].to_numpy())
    assert w.dtype == np.float32 and e == 20
    assert boost.check_weights(ok, 8, y['scores'].to_numpy(), 1.0, rows=np.arange(7))[1] == 2
    assert boost.check_weights(ok, 8)[1] is None  # without labels the shift is the device's
    bad_w = {'nan': np.array([1, np.nan, 1, 1, 1, 1, 1, 1.0]), 'negative': np.array([1, -1e-30, 1, 1, 1, 1, 1, 1.0]),
             'zero': np.zeros(8), 'large': np.array([1, 1, 1, 1, 1, 1, 1, 2.0 ** 20 + 1]),
             'inf': np.array([1, np.inf, 1, 1, 1, 1, 1, 1.0]), 'short': np.ones(7), 'long': np.ones(9)}
    for name, bw in bad_w.items():
        with pytest.raises(ValueError):
            boost.check_weights(bw, 8, y['scores'].to_numpy())
        with pytest.raises(ValueError):
            boost.check_weights(bw, 8)
        with pytest.raises(ValueError):
            model.fit(X, y, learner='device', val_size=0, fit_params=dict(sample_weight=bw))
        with pytest.raises(ValueError):
            boost.DeviceGBTClassifier().fit(X, y['scores'], sample_weight=bw)
        with pytest.raises(ValueError):
            model.fit_batch(none, pd.DataFrame({'game_id': np.zeros(8, int), 'action_id': np.arange(8)}),
                            sample_weight=bw)
    # the positive class's factor counts: 2^19 * 3 > 2^20 on a positive row only
    edge = np.ones(8)
    edge[0] = 2.0 ** 19
    with pytest.raises(ValueError):
        boost.check_weights(edge, 8, y['scores'].to_numpy(), 3.0)
    assert boost.check_weights(edge[::-1].copy(), 8, y['scores'].to_numpy(), 3.0)[1] == 19
    # the training rows alone count
    with pytest.raises(ValueError):
        boost.check_weights(np.array([0, 0, 0, 0, 1, 1, 1, 1.0]), 8, None, 1.0, rows=np.arange(4))
    with pytest.raises(ValueError, match='row_keys'):
        boost.TunedGBTClassifier(subsample=0.5).fit(X, y['scores'], row_keys=np.arange(7))
    with pytest.raises(ValueError, match='game_id and action_id'):
        model.fit_batch(none, pd.DataFrame({'game_id': np.zeros(8, int)}), tree_params=dict(subsample=0.5))
    with pytest.raises(ValueError, match='importance_type'):
        boost.DeviceGBTClassifier(importance_type='split')


def test_sample_entry_points_validate_without_a_gpu():
    """Every invalid argument is SA_EINVAL before any HIP call; n == 0 is a no-op."""
    from socceraction_amd import _native
    lib = _native.load_library()
    one = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced
    E = _native.SA_EINVAL
    order = ('margin', 'y', 'mask', 'n', 'w', 'spw', 'e', 'keys', 'seed', 'round', 'thr', 'gq', 'hq', 'p', 'node', 'st')
    gr = lambda **k: lib.sa_boost_grad(*[{**dict(  # noqa: E731
        margin=one, y=one, mask=None, n=0, w=None, spw=1.0, e=0, keys=None, seed=0, round=0, thr=2 ** 32, gq=one,
        hq=one, p=one, node=one, st=None), **k}[a] for a in order])
    assert gr() == 0 and gr(w=one, keys=one, e=20, spw=3.0, thr=0, seed=2 ** 63 - 1, round=10 ** 6) == 0
    assert gr(margin=None) == E and gr(y=None) == E and gr(hq=None) == E and gr(n=-1) == E
    assert gr(e=-1) == E and gr(e=21) == E and gr(spw=0.0) == E and gr(spw=-1.0) == E and gr(spw=float('nan')) == E
    assert gr(spw=float('inf')) == E and gr(thr=2 ** 32 + 1) == E and gr(round=-1) == E
    assert gr(n=5, e=21) == E  # with rows, still before any launch
    assert b'sa_boost_grad:' in lib.sa_last_error()
    order = ('hist', 'cs', 'cuts', 'F', 'node0', 'nn', 'leaf', 'lam', 'mcw', 'gamma', 'eta', 'alpha', 'e', 'mask',
             'bg', 'bc', 'tree', 'st')
    sp = lambda **k: lib.sa_boost_split(*[{**dict(  # noqa: E731
        hist=None, cs=one, cuts=one, F=1, node0=0, nn=1, leaf=0, lam=1.0, mcw=1.0, gamma=0.0, eta=0.3, alpha=0.0,
        e=0, mask=None, bg=one, bc=one, tree=one, st=None), **k}[a] for a in order])
    assert sp() == E  # hist is NULL: every case below fails before a launch whatever it changes
    assert sp(hist=one, alpha=-1.0) == E and sp(hist=one, alpha=float('nan')) == E
    assert sp(hist=one, alpha=float('inf')) == E and sp(hist=one, e=-1) == E and sp(hist=one, e=21) == E
    assert sp(hist=one, F=0) == E and sp(hist=one, nn=3) == E and sp(hist=one, lam=-1.0) == E
    assert lib.sa_boost_hist_bins(one, 16, one, one, 0, 1, one, one, one, 8, 0, 1, 1, one, None) == E
    assert lib.sa_boost_hist_bins(one, 16, one, one, 1, 1, one, one, one, 17, 0, 1, 1, one, None) == E
    assert lib.sa_boost_hist_bins(None, 16, one, one, 1, 1, one, one, one, 8, 0, 1, 1, one, None) == E
    assert lib.sa_boost_hist_bins(one, 16, one, one, 1, 1, one, one, one, 0, 0, 1, 1, one, None) == 0
    assert lib.sa_boost_hist_bins(one, 16, one, None, 0, 0, one, one, one, 8, 0, 1, 1, one, None) == 0
    assert lib.sa_boost_row_keys(None, one, 4, one, None) == E and lib.sa_boost_row_keys(one, one, -1, one, None) == E
    assert lib.sa_boost_row_keys(one, one, 4, None, None) == E and lib.sa_boost_row_keys(None, None, 0, None, None) == 0
    for name in ('sa_boost_grad', 'sa_boost_split', 'sa_boost_hist_bins', 'sa_boost_row_keys'):
        assert name in _native.EXPORTED_SYMBOLS
    assert not [name for name in _native.EXPORTED_SYMBOLS if name.startswith('sa_boost_') and name.endswith('_ex')]


# ----------------------------------------------------------------------------- importances
def test_feature_importances_of_a_hand_written_table(boost):
    trees = np.zeros((3, 7), boost.NODE_DTYPE)
    trees['feature'] = -1

    def split(t, k, f, gain, H):
        trees[t, k]['exists'], trees[t, k]['feature'], trees[t, k]['gain'], trees[t, k]['H'] = 1, f, gain, H
        for c in (2 * k + 1, 2 * k + 2):
            trees[t, c]['exists'] = 1
            trees[t, c]['H'] = H // 2  # leaves: their H must not count
    split(0, 0, 0, 8.0, 4 << 28)   # cover 4 * 2^28 * 2^(2-30) = 4
    split(0, 1, 2, 2.0, 2 << 28)   # cover 2
    split(1, 0, 0, 4.0, 8 << 28)   # cover 8
    split(2, 0, 2, 1.0, 1 << 28)   # cover 1
    split(2, 2, 2, 3.0, 3 << 28)   # cover 3
    trees[1, 3]['gain'] = 99.0      # not existing, not a split: ignored
    want = {'weight': [2, 0, 3, 0], 'total_gain': [12, 0, 6, 0], 'gain': [6, 0, 2, 0],
            'total_cover': [12, 0, 6, 0], 'cover': [6, 0, 2, 0]}
    for kind, v in want.items():
        got = boost.importances(trees, 4, kind, quant_shift=2)
        assert got.dtype == np.float32 and got.shape == (4,)
        np.testing.assert_array_equal(got, (np.array(v, np.float64) / sum(v)).astype(np.float32))
    # the shift scales every cover alike: the normalised figures do not move, the raw unit does
    np.testing.assert_array_equal(boost.importances(trees, 4, 'cover', 0), boost.importances(trees, 4, 'cover', 2))
    clf = boost.DeviceGBTClassifier(importance_type='total_gain')
    with pytest.raises(Exception, match='not fitted'):
        clf.feature_importances_
    clf.trees_, clf.n_features_in_, clf.quant_shift_ = trees, 4, 2
    np.testing.assert_array_equal(clf.feature_importances_, np.array([12 / 18, 0, 6 / 18, 0], np.float32))
    np.testing.assert_array_equal(clf.feature_importances('weight'), np.array([0.4, 0, 0.6, 0], np.float32))
    assert boost.DeviceGBTClassifier().importance_type == 'gain'
    np.testing.assert_array_equal(boost.importances(np.zeros((2, 7), boost.NODE_DTYPE)[:0], 3), np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        boost.importances(trees, 4, 'split')
