"""Column subsets in the learner's binning and the expected-goals model (socceraction_amd.xg) on
six synthetic games: the compact fit against the masked fit on the full table, the default
model against the numpy restatement of the trainer (tests/boost_reference.py), and rate, score
and get_shots against the paths they shorten.  Models and probabilities are compared exactly."""
import json

import numpy as np
import pandas as pd
import pytest

import boost_reference as br

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, batch, boost, metrics, ops, synthetic, trees, xg
    _native.load_library()
    return dict(batch=batch, ops=ops, synthetic=synthetic, boost=boost, trees=trees, xg=xg, metrics=metrics)


@pytest.fixture(scope='module')
def shots(sa):
    """Six synthetic games: the frames, the batch, the notebook's features of every action in
    bitmap form, the shot rows and the labels of every action."""
    xg, syn = sa['xg'], sa['synthetic']
    d = syn.spadl_games(6, seed=3)
    actions, games = syn.to_frame(d), syn.games_frame(d)
    ab = sa['batch'].ActionBatch.from_frame(actions, home_team_id=games.set_index('game_id')['home_team_id'],
                                            segments='game')
    fb = sa['ops'].features(ab, [f._sa_xfn for f in xg.XFNS], xg.NB_PREV_ACTIONS, bool_bits=True)
    rows = xg.shot_rows(ab)
    host_rows = rows.cpu().numpy()
    mask = actions['type_id'].isin(xg.SHOT_TYPES).to_numpy()
    np.testing.assert_array_equal(host_rows, np.flatnonzero(mask))
    y_host = (actions['result_id'].to_numpy() == xg.SUCCESS)
    y = xg.shot_labels(ab, rows)
    np.testing.assert_array_equal(y.cpu().numpy().astype(bool), y_host[host_rows])
    # both classes are present among the shots, before anything else
    assert 0 < int(y.sum()) < len(host_rows) and len(host_rows) > 200
    y_full = torch.from_numpy(y_host.astype(np.uint8)).cuda()
    return dict(actions=actions, games=games, ab=ab, fb=fb, rows=rows, host_rows=host_rows, mask=mask, y=y,
                y_full=y_full, names=xg.feature_names())


# ----------------------------------------------------------------------------- column subsets
SUBSET = ['start_x_a0', 'type_shot_a1', 'team_1', 'dy_a01', 'bodypart_head_a0', 'start_angle_to_goal_a1',
          'type_pass_a0', 'movement_a0']


def test_binned_column_subset_equals_the_rows_of_the_whole(sa, shots):
    boost, fb = sa['boost'], shots['fb']
    names = fb.plan.names
    kinds = {name: kind for name, kind, _ in fb.plan.order}
    assert {kinds[c] for c in SUBSET} == {'b', 'f'} and [names.index(c) for c in SUBSET] != sorted(
        names.index(c) for c in SUBSET)
    whole = boost.bin_blocks(fb)
    part = boost.bin_blocks(fb, columns=SUBSET)
    assert part.names == SUBSET and whole.names == names
    pick = [names.index(c) for c in SUBSET]
    np.testing.assert_array_equal(part.host_bins(), whole.host_bins()[pick])
    for a, j in zip(part.cuts, pick):
        np.testing.assert_array_equal(a, whole.cuts[j])
    # explicit cuts: one list per name of `columns`
    again = boost.bin_blocks(fb, cuts=[whole.cuts[j] for j in pick], columns=SUBSET)
    np.testing.assert_array_equal(again.host_bins(), part.host_bins())
    with pytest.raises(ValueError, match='cut lists'):
        boost.bin_blocks(fb, cuts=whole.cuts, columns=SUBSET)
    with pytest.raises(ValueError, match='not available'):
        boost.bin_blocks(fb, columns=SUBSET + ['no_such_feature'])
    with pytest.raises(ValueError, match='repeated'):
        boost.bin_blocks(fb, columns=SUBSET + ['team_1'])
    # the same with a row list, as the masked fit bins
    rows = shots['rows']
    np.testing.assert_array_equal(boost.bin_blocks(fb, rows=rows, columns=SUBSET).host_bins(),
                                  boost.bin_blocks(fb, rows=rows).host_bins()[pick])


def test_a_model_fitted_on_a_subset_lists_its_names(sa, shots):
    boost = sa['boost']
    data = boost.bin_blocks(shots['fb'], columns=SUBSET)
    clf = boost.DeviceGBTClassifier(n_estimators=3, max_depth=2).fit_binned(data, shots['y_full'])
    model = clf.to_xgboost_json()
    assert model['learner']['feature_names'] == SUBSET
    assert list(clf.feature_names_in_) == SUBSET
    assert model['learner']['learner_model_param']['num_feature'] == str(len(SUBSET))
    te = sa['trees'].TreeEnsemble.from_model(clf)  # the predictor maps the names back onto the plan
    assert te.predict_blocks(shots['fb']).cpu().numpy().tobytes() == clf.p_.cpu().numpy().tobytes()


# ----------------------------------------------------------------------------- expected goals
SMALL = dict(n_estimators=10, max_depth=3)


def test_compact_fit_equals_the_masked_fit_on_the_full_table(sa, shots):
    boost, xg, fb, rows = sa['boost'], sa['xg'], shots['fb'], shots['rows']
    model = xg.ExpectedGoals().fit_batch(shots['games'], shots['actions'], tree_params=SMALL)
    # both sides cut at the same values: the two samples are the same rows
    compact = sa['ops'].select_rows(fb, rows)
    cuts_masked, cuts_compact = boost.make_cuts(fb, rows=rows), boost.make_cuts(compact)
    assert len(cuts_masked) == len(cuts_compact) == len(fb.plan.names)
    for a, b in zip(cuts_masked, cuts_compact):
        assert a.tobytes() == b.tobytes()
    data = boost.bin_blocks(fb, rows=rows, columns=shots['names'])
    masked = boost.DeviceGBTClassifier(**SMALL).fit_binned(data, shots['y_full'], rows=rows)
    assert model.to_xgboost_json() == masked.to_xgboost_json()
    assert model.feature_names_in_ == shots['names'] == model.to_xgboost_json()['learner']['feature_names']
    assert len(model.model_.trees_) == 10 and (model.model_.trees_['feature'][:, 0] >= 0).all()
    np.testing.assert_array_equal(boost.bin_blocks(compact, columns=shots['names']).host_bins(),
                                  data.host_bins()[:, shots['host_rows']])


@pytest.fixture(scope='module')
def default_model(sa, shots):
    return sa['xg'].ExpectedGoals().fit_batch(shots['games'], shots['actions'])


def test_default_model_equals_the_restatement(sa, shots, default_model):
    """100 trees of depth 6 replayed round by round on the host-selected frame: each restated tree
    is built from the device's probabilities of the restated margin (``sa_boost_grad``: expf is
    the one function numpy does not share), node tables and the final margin compared as bytes."""
    boost, clf, names = sa['boost'], default_model.model_, shots['names']
    X = shots['fb'].to_frame().iloc[shots['host_rows']][names]
    cols = [X[c].to_numpy() for c in names]
    y = shots['y'].cpu().numpy()
    cuts = [br.cuts_of(c, c.dtype == np.bool_) for c in cols]
    B = np.stack([br.bins_of(br.cast32(c), k) for c, k in zip(cols, cuts)])
    params = dict(sa['xg'].TREE_PARAMS)
    assert params == dict(n_estimators=100, max_depth=6, learning_rate=0.3)
    assert clf.trees_.shape == (100, 127) and list(clf.feature_names_in_) == names
    for a, b in zip(clf.cuts_, cuts):
        np.testing.assert_array_equal(a, b)
    m = np.full(len(y), br.base_margin(0.5), np.float32)
    for t in range(100):
        _, _, p = boost.gradients(torch.from_numpy(m).cuda(), shots['y'])
        p = p.cpu().numpy()
        np.testing.assert_allclose(p, br.probability(m), rtol=1e-6, atol=0)
        gq, hq = br.quantise(p, y)
        tab, node = br.build_tree(B, gq, hq, cuts, params)
        assert tab.tobytes() == clf.trees_[t].tobytes(), t
        m = br.update_margin(m, tab, node)
    assert m.tobytes() == clf.margin_.cpu().numpy().tobytes()
    assert (clf.trees_['exists'][:, 63:] != 0).any()  # the deepest level is reached


def test_rate_equals_the_full_table_walk_at_the_shot_rows(sa, shots, default_model):
    actions, games, rows = shots['actions'], shots['games'], shots['host_rows']
    got = default_model.rate_batch(games, actions)
    assert list(got.columns) == ['xg'] and got['xg'].dtype == np.float32
    np.testing.assert_array_equal(got.index.to_numpy(), actions.index[rows].to_numpy())
    te = sa['trees'].TreeEnsemble.from_model(default_model.model_)
    full = te.predict_blocks(shots['fb'])[shots['rows']].cpu().numpy()
    assert got['xg'].to_numpy().tobytes() == full.tobytes()
    assert 0 < got['xg'].min() and got['xg'].max() < 1
    # one game: its slice of the batch, under the frame's own index
    game = games.iloc[2]
    ga = actions[actions.game_id == game.game_id]
    one = default_model.rate(game, ga)
    want = got.loc[got.index.isin(ga.index)]
    assert len(one) == len(want) > 0 and one.index.equals(want.index)
    assert one['xg'].to_numpy().tobytes() == want['xg'].to_numpy().tobytes()


def test_scores_and_the_shots_frame(sa, shots, default_model):
    from socceraction_amd.vaep import VAEP
    actions, games = shots['actions'], shots['games']
    xgv = torch.from_numpy(default_model.rate_batch(games, actions)['xg'].to_numpy()).cuda()
    want = sa['metrics'].binary_scores(shots['y'], xgv)
    got = default_model.score_batch(games, actions)
    assert set(got) == set(want) == set(sa['metrics'].KEYS)
    for k in want:
        assert got[k] == want[k], k
    assert got['n'] == len(shots['host_rows']) and got['log_loss'] < got['log_loss_baseline']
    frame = sa['xg'].get_shots(games, actions)
    full = VAEP().compute_features_batch(games, actions)[shots['mask']]
    assert list(frame.columns) == list(full.columns)
    np.testing.assert_array_equal(frame.index.to_numpy(), full.index.to_numpy())
    for c in full.columns:
        assert frame[c].dtype == full[c].dtype, c
        assert frame[c].to_numpy().tobytes() == full[c].to_numpy().tobytes(), c


def test_fit_is_the_same_for_any_game_order(sa, shots):
    xg, actions, games = sa['xg'], shots['actions'], shots['games']
    params = dict(n_estimators=20)
    first = xg.ExpectedGoals().fit_batch(games, actions, tree_params=params).to_xgboost_json()
    rev_games = games.iloc[::-1].reset_index(drop=True)
    rev_actions = pd.concat([actions[actions.game_id == g] for g in rev_games.game_id], ignore_index=True)
    assert rev_actions.game_id.iloc[0] != actions.game_id.iloc[0]
    second = xg.ExpectedGoals().fit_batch(rev_games, rev_actions, tree_params=params).to_xgboost_json()
    assert json.dumps(first) == json.dumps(second)
    assert len(first['learner']['gradient_booster']['model']['trees']) == 20


def test_held_out_shots_weights_and_errors(sa, shots):
    boost, xg, actions, games = sa['boost'], sa['xg'], shots['actions'], shots['games']
    m = len(shots['host_rows'])
    np.random.seed(4)
    held = xg.ExpectedGoals().fit_batch(games, actions, tree_params=SMALL, val_size=0.25, early_stopping_rounds=3,
                                        eval_metric='logloss')
    assert held.device_eval_['n'] == m - int(np.floor(m * 0.75)) - 1
    assert held.model_.best_iteration + 1 == len(held.model_.trees_) <= 10
    # weights come per action and are gathered at the shots
    w = np.random.default_rng(2).integers(1, 3, len(actions)).astype(np.float32)
    weighted = xg.ExpectedGoals().fit_batch(games, actions, tree_params=SMALL, sample_weight=w)
    data = boost.bin_blocks(sa['ops'].select_rows(shots['fb'], shots['rows']), columns=shots['names'])
    direct = boost.DeviceGBTClassifier(**SMALL).fit_binned(data, shots['y'], sample_weight=w[shots['host_rows']])
    assert weighted.to_xgboost_json() == direct.to_xgboost_json()
    plain = xg.ExpectedGoals().fit_batch(games, actions, tree_params=SMALL)
    assert weighted.to_xgboost_json() != plain.to_xgboost_json()
    # no shots, one class
    passes = actions[actions.type_id == 0].reset_index(drop=True)
    with pytest.raises(ValueError, match='no shots'):
        xg.ExpectedGoals().fit_batch(games, passes)
    missed = actions[~shots['mask'] | (actions.result_id != xg.SUCCESS)].reset_index(drop=True)
    with pytest.raises(ValueError, match='one class'):
        xg.ExpectedGoals().fit_batch(games, missed)
    assert len(plain.rate_batch(games, passes)) == 0
