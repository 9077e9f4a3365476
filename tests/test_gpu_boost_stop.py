"""Held-out evaluation and early stopping of the device learner (``sa_boost_apply``,
socceraction_amd.boost) against the numpy restatement of contract items 9-12
(tests/boost_stop_reference.py).  Margins, integers, trees and models are compared exactly; only
``expf`` against numpy's ``exp`` gets the 1e-6 relative bar of tests/test_gpu_boost.py, and the
log loss the 1e-12 relative bar of tests/test_gpu_metrics.py."""
import json

import numpy as np
import pandas as pd
import pytest

import boost_reference as br
import boost_stop_reference as bs
from golden_io import frame, load
from test_boost_stop_host import stop_table

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, batch, boost, ops, trees
    _native.load_library()
    return dict(batch=batch, ops=ops, trees=trees, boost=boost, native=_native)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ----------------------------------------------------------------------------- the kernel alone
def _bin_table(n, f_num, n_bool, seed):
    """Numeric columns holding bins directly (value v in 0..254 -> bin v with the cuts 1..254,
    NaN -> 255) and bool columns; bool column 0 is all ones, column 1 all zeros."""
    rng = np.random.default_rng(seed)
    cols, cuts = {}, []
    for j in range(f_num):
        v = rng.integers(0, 256, n).astype(np.float64)
        v[v == 255] = np.nan
        cols[f'n{j}'] = v
        cuts.append(np.arange(1, 255, dtype=np.float32))
    for j in range(n_bool):
        b = rng.random(n) < 0.5
        if j == 0:
            b[:] = True
        elif j == 1:
            b[:] = False
        cols[f'b{j}'] = b
        cuts.append(np.array([0.5], np.float32))
    return pd.DataFrame(cols), cuts


def _complete_table(depth, cuts, rng):
    """A complete tree: every node above the deepest level splits, node k on feature k mod F (the
    root on a numeric one) at a random cut from the middle half of the feature's cuts."""
    tab = np.zeros(2 ** (depth + 1) - 1, br.NODE_DTYPE)
    tab['exists'] = 1
    tab['feature'] = tab['cut'] = -1
    tab['value'] = rng.normal(size=len(tab)).astype(np.float32)
    for k in range(2 ** depth - 1):
        f = k % len(cuts)
        m = len(cuts[f])
        c = int(rng.integers(m // 4, m - m // 4))
        tab['feature'][k], tab['cut'][k], tab['thr'][k] = f, c, cuts[f][c]
    return tab


N_ROWS = 300


@pytest.fixture(scope='module')
def small(sa):
    X, cuts = _bin_table(N_ROWS, 3, 3, seed=11)
    data = sa['boost'].bin_host(X, cuts=cuts)
    B = data.host_bins()
    assert (B[:3] == 255).any() and B[3].all() and not B[4].any()
    return data, B, cuts


def _row_lists(n):
    rng = np.random.default_rng(n)
    lists = {'all': None, 'word_sides': np.array([63, 64, n - 1, 5, 5, 0], np.int64)}
    for k in (1, 255, 256, 257):
        lists[f'len{k}'] = rng.integers(0, n, k).astype(np.int64)
    return lists


@pytest.mark.parametrize('depth', [1, 3, 6])
def test_apply_equals_the_numpy_walk(sa, small, depth):
    data, B, cuts = small
    rng = np.random.default_rng(depth)
    tab = _complete_table(depth, cuts, rng)
    if depth == 6:  # every feature kind and the missing bin are on some path
        assert set(tab['feature'][:63].tolist()) == set(range(6))
    for name, rows in _row_lists(N_ROWS).items():
        k = N_ROWS if rows is None else len(rows)
        m0 = rng.normal(size=k).astype(np.float32)
        m, p = sa['boost'].apply_tree(data, tab, _dev(m0), rows, max_depth=depth)
        m, p = m.cpu().numpy(), p.cpu().numpy()
        want = bs.apply_tree(tab, B, np.arange(N_ROWS) if rows is None else rows, m0, depth)
        assert m.dtype == np.float32 and m.tobytes() == want.tobytes(), (depth, name)
        np.testing.assert_allclose(p, br.probability(want), rtol=1e-6, atol=0, err_msg=name)
    leaves = bs.walk(tab, B, np.arange(N_ROWS), depth)
    assert leaves.min() >= 2 ** depth - 1 and len(set(leaves.tolist())) > depth  # many paths are taken


def test_apply_a_root_that_is_a_leaf_and_a_row_outside_the_table(sa, small):
    data, B, cuts = small
    boost = sa['boost']
    tab = _complete_table(3, cuts, np.random.default_rng(0))
    tab['feature'][0] = tab['cut'][0] = -1  # the walk ends at the root whatever lies below it
    m0 = np.linspace(-2, 2, 7).astype(np.float32)
    rows = np.array([0, 63, 64, 299, 7, 7, 128], np.int64)
    m, p = boost.apply_tree(data, tab, _dev(m0), rows, max_depth=3)
    assert m.cpu().numpy().tobytes() == (m0 + tab['value'][0]).astype(np.float32).tobytes()
    np.testing.assert_allclose(p.cpu().numpy(), br.probability(m0 + tab['value'][0]), rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        boost.apply_tree(data, tab, _dev(m0[:2]), [0, N_ROWS], max_depth=3)
    with pytest.raises(ValueError):
        boost.apply_tree(data, tab, _dev(m0[:2]), [-1, 0], max_depth=3)
    with pytest.raises(ValueError):
        boost.apply_tree(data, tab[:7], _dev(m0), rows, max_depth=3)
    # the entry point itself guards a row outside [0, n): that entry keeps its margin and p
    tab = _complete_table(3, cuts, np.random.default_rng(1))
    bad = np.array([5, -1, N_ROWS, 2 ** 40, 6], np.int64)
    margin, p = _dev(m0[:5].copy()), _dev(np.full(5, -7.0, np.float32))
    tree = _dev(tab.view(np.uint8).copy())
    boost._apply(data, tree, 3, _dev(bad), 5, margin, p)
    want = m0[:5].copy()
    want[[0, 4]] = bs.apply_tree(tab, B, bad[[0, 4]], m0[[0, 4]], 3)
    assert margin.cpu().numpy().tobytes() == want.tobytes()
    assert p.cpu().numpy()[1:4].tolist() == [-7.0] * 3


# ----------------------------------------------------------------------------- per-round evaluation
@pytest.fixture(scope='module')
def game(sa):
    """spadl_full0 as in tests/test_gpu_boost.py: the bitmap-form feature blocks, their host
    values and the labels (scores, every fifth row positive)."""
    from oracle import vaep_oracle as vo
    g = load('spadl', 'full0')
    df = frame(g)
    ab = sa['batch'].ActionBatch.from_frame(df, home_team_id=g['home_team_id'][0])
    fb = sa['ops'].features(ab, vo.SPADL_DEFAULT, 3, bool_bits=True)
    full = sa['ops'].features(ab, vo.SPADL_DEFAULT, 3)
    b, f, i = full.to_numpy()
    host = {'b': b.astype(bool), 'f': f, 'i': i}
    cols = [np.ascontiguousarray(host[k][c, :fb.n]) for _, k, c in fb.plan.order]
    y = g['scores'].astype(np.uint8).copy()
    y[::5] = 1
    cuts = [br.cuts_of(c, c.dtype == np.bool_) for c in cols]
    yd = torch.zeros(fb.n + 16, dtype=torch.uint8, device=ab.device)
    yd[:fb.n] = _dev(y)
    ev = np.flatnonzero(np.arange(fb.n) % 4 == 3)
    tr = np.flatnonzero(np.arange(fb.n) % 4 != 3)
    plain = {d: sa['boost'].DeviceGBTClassifier(n_estimators=8, max_depth=d).fit_blocks(
        fb, yd, rows=tr, cuts=cuts).trees_ for d in (3, 6)}
    return dict(ab=ab, fb=fb, y=y, yd=yd, cuts=cuts, ev=ev, tr=tr, plain=plain,
                X32=np.stack([br.cast32(c) for c in cols], 1))


@pytest.mark.parametrize('metric', ['auc', 'logloss'])
@pytest.mark.parametrize('depth', [3, 6])
def test_per_round_evaluation_replayed(sa, game, depth, metric):
    from sklearn.metrics import log_loss
    boost, fb, ev = sa['boost'], game['fb'], game['ev']
    clf = boost.DeviceGBTClassifier(record=True, n_estimators=8, max_depth=depth, eval_metric=metric)
    clf.fit_blocks(fb, game['yd'], rows=game['tr'], cuts=game['cuts'], eval_rows=ev)
    # evaluation does not perturb training
    assert clf.trees_.tobytes() == game['plain'][depth].tobytes()
    assert clf.n_rounds_run_ == 8 and len(clf.trees_) == 8
    EP = clf.record_['eval_p'].cpu().numpy()
    assert EP.shape == (8, len(ev)) and EP.dtype == np.float32
    ye = game['y'][ev]
    n_pos = int(ye.sum())
    scores = clf.evals_result_['validation_0'][metric]
    assert list(clf.evals_result_) == ['validation_0'] and list(clf.evals_result_['validation_0']) == [metric]
    assert len(scores) == 8 and len(clf.eval_sums_) == 8
    for t in range(8):
        model = boost.trees_to_xgboost_json(clf.trees_[:t + 1], fb.plan.names, 0.5)
        te = sa['trees'].TreeEnsemble.from_xgboost_json(model)
        want = te.predict_blocks(fb).cpu().numpy()[ev]
        assert EP[t].tobytes() == want.tobytes(), t
        np.testing.assert_allclose(EP[t], br.predict(clf.trees_[:t + 1], game['X32'][ev]), rtol=1e-6, atol=0)
        if metric == 'auc':
            u2 = bs.u2_of(ye, EP[t])
            assert clf.eval_sums_[t] == u2, t
            assert scores[t] == u2 / (2 * n_pos * (len(ye) - n_pos))
        else:
            ref = log_loss(ye, EP[t], labels=[0, 1])
            print(depth, t, 'log loss', scores[t], 'host', ref)
            assert abs(scores[t] - ref) <= 1e-12 * ref, t
            assert scores[t] == bs.metric_score(clf.eval_sums_[t], 'logloss', ye)
    best, run = boost.stop_decision(clf.eval_sums_, None, metric == 'auc')
    assert (clf.best_iteration, run) == (best, 8) and clf.best_score == scores[best]
    assert 'attributes' in clf.to_xgboost_json()['learner'] and clf.to_xgboost_json()['learner']['attributes'] == {}
    # a mask selects the same rows as the index list
    mask = np.zeros(fb.n, bool)
    mask[ev] = True
    again = boost.DeviceGBTClassifier(n_estimators=8, max_depth=depth, eval_metric=metric)
    again.fit_blocks(fb, game['yd'], rows=game['tr'], cuts=game['cuts'], eval_rows=mask)
    assert again.eval_sums_ == clf.eval_sums_ and again.record_ is None
    assert not hasattr(boost.DeviceGBTClassifier(n_estimators=1).fit_blocks(fb, game['yd']), 'best_iteration')


def test_a_single_class_among_the_evaluation_rows_is_an_error(sa, game):
    boost = sa['boost']
    one_class = np.flatnonzero(game['y'] == 0)[:50]
    clf = boost.DeviceGBTClassifier(n_estimators=2)
    clf._events = []
    with pytest.raises(ValueError, match='Only one class present'):
        clf.fit_blocks(game['fb'], game['yd'], cuts=game['cuts'], eval_rows=one_class)
    assert clf._events == []  # raised before any training launch
    with pytest.raises(ValueError, match='inside the table'):
        clf.fit_blocks(game['fb'], game['yd'], cuts=game['cuts'], eval_rows=[0, game['fb'].n])
    with pytest.raises(ValueError):
        clf.fit_blocks(game['fb'], game['yd'], cuts=game['cuts'], eval_rows=[])
    assert clf._events == []


# ----------------------------------------------------------------------------- early stopping
@pytest.fixture(scope='module')
def table():
    X, y, cuts, B = stop_table()
    return X, y, cuts


@pytest.mark.parametrize('metric', ['auc', 'logloss'])
@pytest.mark.parametrize('rounds', [3, 5])
def test_early_stopping_end_to_end(sa, table, rounds, metric):
    boost = sa['boost']
    X, y, cuts = table
    Xt, yt, Xv, yv = X.iloc[:1000], y[:1000], X.iloc[1000:].reset_index(drop=True), y[1000:]

    def fit():
        return boost.DeviceGBTClassifier(n_estimators=40, early_stopping_rounds=rounds, eval_metric=metric).fit(
            Xt, yt, eval_set=[(Xv, yv)])
    clf = fit()
    for a, b in zip(clf.cuts_, cuts):  # the cuts come from the training rows only
        np.testing.assert_array_equal(a, b)
    best, run = boost.stop_decision(clf.eval_sums_, rounds, metric == 'auc')
    print(metric, rounds, 'best', best, 'rounds run', run, 'polls', clf.n_polls_)
    assert (clf.best_iteration, clf.n_rounds_run_) == (best, run)
    assert clf.n_rounds_run_ < 40  # the restatement stops after 13 to 17 rounds
    assert run == best + rounds + 1  # the last round trained is the round the rule fires at
    assert len(clf.trees_) == best + 1
    scores = clf.evals_result_['validation_0'][metric]
    assert len(scores) == run and clf.best_score == scores[best]
    assert scores[best] == (max(scores) if metric == 'auc' else min(scores))
    assert 1 <= clf.n_polls_ <= 2 * (-(-40 // (rounds + 1))) + 1
    p = clf.p_.cpu().numpy()
    assert p.shape == (1000,) and p.tobytes() == clf.predict_proba(Xt)[:, 1].tobytes()
    model = json.loads(json.dumps(clf.to_xgboost_json()))
    assert model['learner']['attributes'] == {'best_iteration': str(best), 'best_score': repr(scores[best])}
    te = sa['trees'].TreeEnsemble.from_xgboost_json(model)
    assert te.n_trees == best + 1
    assert sa['trees'].xgb_classifier_iterations(object(), model) == best + 1
    first = json.dumps(clf.to_xgboost_json())
    assert json.dumps(fit().to_xgboost_json()) == first
    # the same table with its rows permuted: the same cuts, rows and eval_rows permuted alike
    perm = np.random.default_rng(1).permutation(1500)
    data = boost.bin_host(X.iloc[perm].reset_index(drop=True), cuts=cuts)
    yd = torch.zeros(data.ld, dtype=torch.uint8, device=data.device)
    yd[:1500] = _dev(y[perm].astype(np.uint8))
    shuffled = boost.DeviceGBTClassifier(n_estimators=40, early_stopping_rounds=rounds, eval_metric=metric)
    shuffled.fit_binned(data, yd, rows=np.flatnonzero(perm < 1000), eval_rows=np.flatnonzero(perm >= 1000))
    assert json.dumps(shuffled.to_xgboost_json()) == first
    assert shuffled.eval_sums_ == clf.eval_sums_
    # under early stopping p_ covers every row of the table: the kept trees replayed
    inv = np.argsort(perm)
    assert shuffled.p_.cpu().numpy()[inv][:1000].tobytes() == p.tobytes()
    assert shuffled.p_.cpu().numpy()[inv][1000:].tobytes() == clf.predict_proba(Xv)[:, 1].tobytes()


# ----------------------------------------------------------------------------- the public path
def _two_games():
    gs = [load('spadl', 'full0'), load('spadl', 'full1')]
    actions = pd.concat([frame(g) for g in gs], ignore_index=True)
    games = pd.DataFrame({'game_id': [int(frame(g).game_id.iloc[0]) for g in gs],
                          'home_team_id': [int(g['home_team_id'][0]) for g in gs]})
    return games, actions


def _stopped(models, limit):
    for col in ('scores', 'concedes'):
        clf = models[col]
        n_trees = len(clf.trees_)
        print(col, 'trees', n_trees, 'rounds run', clf.n_rounds_run_, 'best', clf.best_score)
        assert 1 <= n_trees <= limit and clf.best_iteration == n_trees - 1
        assert clf.n_rounds_run_ <= limit


def test_public_path_fit_batch_and_fit_with_early_stopping(sa):
    import socceraction_amd.vaep as vaep
    games, actions = _two_games()
    np.random.seed(7)
    model = vaep.VAEP().fit_batch(games, actions, val_size=0.25, early_stopping_rounds=3,
                                  tree_params=dict(n_estimators=30))
    _stopped(model._VAEP__models, 30)
    assert set(model.device_eval_) == {'scores', 'concedes'}
    assert all(0 < v['log_loss'] < 1 and 0 < v['auroc'] <= 1 for v in model.device_eval_.values())
    trees = model._device_models()
    assert all(trees[c].n_trees == len(model._VAEP__models[c].trees_) for c in trees)
    game = games.iloc[0]
    ga = actions[actions.game_id == game.game_id].reset_index(drop=True)
    rated = model.rate(game, ga)
    assert len(rated) == len(ga) and np.isfinite(rated['vaep_value']).all()
    m2 = vaep.VAEP()
    X = m2.compute_features_batch(games, actions)
    Y = m2.compute_labels_batch(games, actions)
    np.random.seed(7)
    m2.fit(X, Y, learner='device', val_size=0.25, tree_params=dict(n_estimators=30),
           fit_params=dict(early_stopping_rounds=3))
    _stopped(m2._VAEP__models, 30)
    assert set(m2.device_eval_) == {'scores', 'concedes'}
    assert m2._VAEP__models['scores'].eval_metric == 'auc'
    np.random.seed(7)
    m3 = vaep.VAEP().fit(X, Y, learner='device', val_size=0.25, tree_params=dict(n_estimators=12),
                         fit_params=dict(verbose=True))
    for col in ('scores', 'concedes'):
        assert len(m3._VAEP__models[col].trees_) == 12 and not hasattr(m3._VAEP__models[col], 'best_iteration')
    assert set(m3.device_eval_) == {'scores', 'concedes'}


def test_public_path_atomic_fit_batch_with_early_stopping(sa):
    from socceraction_amd.atomic.vaep import AtomicVAEP
    g = load('atomic', 'full0')
    actions = frame(g, atomic=True)
    games = pd.DataFrame({'game_id': [int(actions.game_id.iloc[0])], 'home_team_id': [int(g['home_team_id'][0])]})
    np.random.seed(7)
    model = AtomicVAEP().fit_batch(games, actions, val_size=0.25, early_stopping_rounds=3, eval_metric='logloss',
                                   tree_params=dict(n_estimators=30))
    _stopped(model._VAEP__models, 30)
    assert set(model.device_eval_) == {'scores', 'concedes'}
    rated = model.rate(games.iloc[0], actions)
    assert len(rated) == len(actions) and np.isfinite(rated['vaep_value']).all()


# ----------------------------------------------------------------------------- off means off
def _families(clf):
    out = {}
    for fam, _, _ in clf._events:
        out[fam] = out.get(fam, 0) + 1
    return out


def test_launch_families_with_and_without_evaluation(sa, game):
    boost, fb = sa['boost'], game['fb']
    today = dict(grad=6, hist_bits=15, hist_bins=15, split=20, advance=20)
    clf = boost.DeviceGBTClassifier(n_estimators=5, max_depth=3)
    clf._events = []
    clf.fit_blocks(fb, game['yd'], rows=game['tr'], cuts=game['cuts'])
    assert _families(clf) == today
    for metric, extra in (('auc', dict(apply=5, metric=15, sort=5)), ('logloss', dict(apply=5, metric=5))):
        clf = boost.DeviceGBTClassifier(n_estimators=5, max_depth=3, eval_metric=metric)
        clf._events = []
        clf.fit_blocks(fb, game['yd'], rows=game['tr'], cuts=game['cuts'], eval_rows=game['ev'])
        assert _families(clf) == {**today, **extra}, metric
        assert clf.n_polls_ == 0
