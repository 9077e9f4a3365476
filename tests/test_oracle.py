"""The CPU oracle reproduces the reference's goldens (CPU only, no GPU)."""
import os

import numpy as np
import pandas as pd
import pytest

import value_cases as vc
from golden_io import GOLDEN, assert_close, assert_same_floats, cases, inputs, ks, load
from oracle import vaep_oracle as vo
from oracle import xt_oracle as xo


def _check_features(got, g, k):
    names = list(g[f'k{k}_names_all'])
    assert [c[0] for c in got] == names
    kinds = list(g[f'k{k}_kinds_all'])
    assert [c[1] for c in got] == kinds
    for kind in 'bfi':
        ref = g[f'k{k}_feat_{kind}']
        mine = [c[2] for c in got if c[1] == kind]
        if not mine:
            assert ref.shape[1] == 0
            continue
        M = np.stack(mine, axis=1)
        if kind == 'f':  # numpy against numpy: non-angle columns bit for bit, angles within 1 + 1 ulp
            fnames = list(g[f'k{k}_names_f'])
            exact = {nm: (ref[:, j], ref[:, j]) for j, nm in enumerate(fnames) if vc.is_angle(nm)}
            vc.check_float_columns(fnames, M.T, ref.T, exact, f'k{k} float features', bound=2)
        else:
            np.testing.assert_array_equal(M.astype(ref.dtype), ref)


@pytest.mark.parametrize('name', cases('spadl'))
def test_spadl_oracle(name):
    g = load('spadl', name)
    cols = inputs(g)
    home = [g['home_team_id'][0]]
    for k in ks(g):
        _check_features(vo.features(cols, k, vo.SPADL_DEFAULT, home=home), g, k)
    lab = vo.labels(cols)
    np.testing.assert_array_equal(lab['scores'], g['scores'].astype(bool))
    np.testing.assert_array_equal(lab['concedes'], g['concedes'].astype(bool))
    np.testing.assert_array_equal(lab['goal_from_shot'], g['goal_from_shot'].astype(bool))
    for tag, dt in (('64', np.float64), ('32', np.float32)):
        v = vo.formula(cols, g['ps'].astype(dt), g['pc'].astype(dt))
        for c in ('offensive_value', 'defensive_value', 'vaep_value'):
            assert v[c].dtype == dt
            assert_same_floats(v[c], g[f'{c}_{tag}'], c)


@pytest.mark.parametrize('name', cases('atomic'))
def test_atomic_oracle(name):
    g = load('atomic', name)
    cols = inputs(g, atomic=True)
    home = [g['home_team_id'][0]]
    for k in ks(g):
        _check_features(vo.features(cols, k, vo.ATOMIC_DEFAULT, atomic=True, home=home), g, k)
    lab = vo.labels(cols, atomic=True)
    np.testing.assert_array_equal(lab['scores'], g['scores'].astype(bool))
    np.testing.assert_array_equal(lab['concedes'], g['concedes'].astype(bool))
    np.testing.assert_array_equal(lab['goal_from_shot'], g['goal_from_shot'].astype(bool))
    for tag, dt in (('64', np.float64), ('32', np.float32)):
        v = vo.formula(cols, g['ps'].astype(dt), g['pc'].astype(dt), atomic=True)
        for c in ('offensive_value', 'defensive_value', 'vaep_value'):
            assert v[c].dtype == dt
            assert_same_floats(v[c], g[f'{c}_{tag}'], c)


@pytest.mark.parametrize('atomic', [False, True])
def test_explicit_frames_oracle(atomic):
    """features_frames on frames that are not shifts of one another == the reference's own
    module-level transformers on them (tests/golden/make_golden_explicit.py), as built and after
    the reference's play_left_to_right; and features() on one frame still equals its emitter."""
    import window_cases as wc
    g = wc.explicit_golden(atomic)
    xfns = vo.ATOMIC_DEFAULT if atomic else vo.SPADL_DEFAULT
    for tag in ('plain', 'ltr'):
        frames = wc.frame_cols(wc.golden_frames(g, tag, atomic), atomic)
        assert len(frames) == 4 and len(frames[0]['type_id']) == 70
        got = vo.features_frames(frames, xfns, atomic)
        _check_features(got, {f'k4_{key[len(tag) + 1:]}': v for key, v in g.items()
                              if key.startswith(tag + '_')}, 4)
    t = [f['time_seconds'] for f in frames]
    assert (t[1] != t[0][np.maximum(np.arange(70) - 1, 0)]).mean() > 0.9  # no shifted copies
    a = vo.features(frames[0], 1, xfns, atomic=atomic)
    b = vo.features_frames(frames[:1], xfns, atomic)
    assert [c[:2] for c in a] == [c[:2] for c in b]
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x[2], y[2])


@pytest.mark.parametrize('name', cases('xt'))
def test_xt_oracle(name):
    g = load('xt', name)
    cols = inputs(g)
    grids = sorted({k.split('_')[0] for k in g if k[0].isdigit()})
    for tag in grids:
        l, w = map(int, tag.split('x'))
        f = xo.fit(cols, l, w)
        np.testing.assert_array_equal(f['scoring_prob'], g[f'{tag}_scoring_prob'])
        np.testing.assert_array_equal(f['shot_prob'], g[f'{tag}_shot_prob'])
        np.testing.assert_array_equal(f['move_prob'], g[f'{tag}_move_prob'])
        np.testing.assert_array_equal(f['transition'], g[f'{tag}_transition'])
        assert f['heatmaps'].shape == g[f'{tag}_heatmaps'].shape  # same iteration count
        np.testing.assert_array_equal(f['xT'], g[f'{tag}_xT'])  # bit-exact summation order
        assert_close(xo.rate(cols, g[f'{tag}_xT']), g[f'{tag}_rate'], 'rate')
        if f'{tag}_rate_interp' in g:
            assert_close(xo.rate(cols, g[f'{tag}_xT'], True), g[f'{tag}_rate_interp'], 'interp')


def _xt105():
    with np.load(os.path.join(GOLDEN, 'xt105_interp.npz'), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_xt105_interpolated_rate_oracle():
    """cfg5's rate(use_interpolation=True) at 105 x 68 (reference-generated golden,
    tests/golden/make_golden_xt105.py): surface sample and per-action ratings."""
    g = _xt105()
    cols = inputs(g)
    rows, cs = g['grid_rows'], g['grid_cols']
    for tag in ('fit', 'random'):
        xT = g[f'{tag}_xT']
        assert xT.shape == (68, 105)
        assert_close(xo.interp_grid(xT)[np.ix_(rows, cs)], g[f'{tag}_grid_sample'], f'{tag} grid')
        assert_close(xo.rate(cols, xT), g[f'{tag}_rate'], f'{tag} rate')
        assert_close(xo.rate(cols, xT, True), g[f'{tag}_rate_interp'], f'{tag} interp rate')


@pytest.mark.parametrize('name', cases('dribbles'))
def test_add_dribbles_oracle(name):
    """oracle add_dribbles == the reference's spadl.base._add_dribbles (goldens)."""
    from golden_io import dribbles_frame
    from oracle import atomic_convert_oracle as co
    g = load('dribbles', name)
    df = dribbles_frame(g, 'in_')
    ref = dribbles_frame(g, 'out_')
    got = co.add_dribbles({c: df[c].to_numpy() for c in co.COLS})
    assert len(got['type_id']) == len(ref)
    for c in co.COLS:
        if c == 'original_event_id':
            np.testing.assert_array_equal(pd.isna(got[c]), ref[c].isna().to_numpy())
            continue
        np.testing.assert_array_equal(np.asarray(got[c]), ref[c].to_numpy(), err_msg=c)


@pytest.mark.parametrize('name', cases('convert'))
def test_convert_oracle(name):
    """oracle/atomic_convert_oracle.py == the reference's convert_to_atomic (goldens)."""
    from golden_io import assert_convert_equal, convert_input, convert_output
    from oracle import atomic_convert_oracle as co
    g = load('convert', name)
    df = convert_input(g)
    got = co.convert_to_atomic({c: df[c].to_numpy() for c in co.COLS})
    ref = convert_output(g)
    assert_convert_equal(got, ref, name)
    # floats are produced by the same operations as the reference: bit-exact here
    for c in ('time_seconds', 'x', 'y', 'dx', 'dy'):
        np.testing.assert_array_equal(got[c], ref[c], err_msg=f'{name} {c}')


def test_tree_oracle_matches_sklearn_predict_proba():
    """The tree walk of oracle/tree_oracle.py (float64, x <= threshold) equals scikit-learn's
    own HistGradientBoostingClassifier.predict_proba on VAEP features of a golden game, incl.
    missing values."""
    from sklearn.ensemble import HistGradientBoostingClassifier

    from oracle import tree_oracle as to
    g = load('spadl', 'full0')
    X = np.concatenate([g['k3_feat_b'].astype(np.float64), g['k3_feat_f'],
                        g['k3_feat_i'].astype(np.float64)], axis=1)
    y = g['scores'].astype(int)
    y[::7] = 1  # enough positives to grow real trees
    X = X.copy()
    X[::13, 520] = np.nan
    clf = HistGradientBoostingClassifier(max_iter=30, max_depth=3, random_state=0).fit(X, y)
    np.testing.assert_allclose(to.predict_sklearn_nodes(clf, X), clf.predict_proba(X)[:, 1],
                               rtol=1e-12, atol=0)


def test_tree_oracle_xgboost_rules():
    """Hand-checked xgboost rules: x < threshold goes left (equality goes right), NaN follows
    default_left, leaves sum in tree order in float32 onto logit(base_score)."""
    from oracle import tree_oracle as to
    tree = {'left_children': [1, -1, -1], 'right_children': [2, -1, -1],
            'split_indices': [0, 0, 0], 'split_conditions': [1.0, -0.5, 0.25],
            'default_left': [1, 0, 0]}
    model = {'learner': {'objective': {'name': 'binary:logistic'},
                         'learner_model_param': {'base_score': '5E-1'},
                         'gradient_booster': {'model': {'trees': [tree, tree]}}}}
    X = np.array([[0.5], [1.0], [2.0], [np.nan]])
    p = to.predict_xgboost_json(model, X)
    m = np.array([-1.0, 0.5, 0.5, -1.0], np.float32)
    np.testing.assert_array_equal(p, (1 / (1 + np.exp(-m))).astype(np.float32))


def _flat_of_xgboost_json(model):
    return [{'left': t['left_children'], 'right': t['right_children'], 'feature': t['split_indices'],
             'cond': t['split_conditions'], 'default_left': t['default_left']}
            for t in model['learner']['gradient_booster']['model']['trees']]


def test_predict_flat_equals_predict_xgboost_json():
    """predict_flat under xgboost's rule (`<`, float32) == predict_xgboost_json on a synthetic
    JSON model, bit for bit, with NaN, thresholds hit exactly and a non-default base score."""
    from oracle import tree_oracle as to
    from socceraction_amd.trees import synthetic_xgboost_json
    model = synthetic_xgboost_json(12, n_trees=30, depth=4, seed=9, base_score=0.3)
    rng = np.random.default_rng(0)
    X = rng.normal(0.0, 30.0, (500, 12))
    X[::11, 3] = np.nan
    t0 = model['learner']['gradient_booster']['model']['trees'][0]
    X[::5, t0['split_indices'][0]] = t0['split_conditions'][0]  # equality at a root
    p = np.float32(0.3)
    base = np.float32(-np.log(np.float32(1.0) / p - np.float32(1.0)))
    got = to.predict_flat(_flat_of_xgboost_json(model), base, X, True, np.float32)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, to.predict_xgboost_json(model, X))


def test_predict_flat_equals_sklearn_predict_proba():
    """predict_flat under scikit-learn's rule (`<=`, float64) == predict_proba of a fitted
    HistGradientBoostingClassifier (rtol 1e-12), incl. missing values."""
    from sklearn.ensemble import HistGradientBoostingClassifier

    from oracle import tree_oracle as to
    g = load('spadl', 'full0')
    X = np.concatenate([g['k3_feat_b'].astype(np.float64), g['k3_feat_f'],
                        g['k3_feat_i'].astype(np.float64)], axis=1).copy()
    y = g['scores'].astype(int)
    y[::7] = 1
    X[::13, 520] = np.nan
    clf = HistGradientBoostingClassifier(max_iter=30, max_leaf_nodes=9, random_state=0).fit(X, y)
    flat = []
    for it in clf._predictors:
        nd = it[0].nodes
        leaf = nd['is_leaf'].astype(bool)
        flat.append({'left': np.where(leaf, -1, nd['left'].astype(np.int64)),
                     'right': np.where(leaf, -1, nd['right'].astype(np.int64)),
                     'feature': nd['feature_idx'], 'cond': np.where(leaf, nd['value'], nd['num_threshold']),
                     'default_left': nd['missing_go_to_left']})
    base = float(np.asarray(clf._baseline_prediction).reshape(-1)[0])
    got = to.predict_flat(flat, base, X, False, np.float64)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, clf.predict_proba(X)[:, 1], rtol=1e-12, atol=0)


def test_condition_bits_rules():
    """condition_bits: equality goes right under `<` and left under `<=`; the compare is made in
    the given dtype (a float64 value above its float32 rounding); -0.0 == 0.0; NaN follows the
    default direction."""
    from oracle import tree_oracle as to
    x = 0.1  # float32(0.1) > 0.1
    t = float(np.float32(x))
    X = np.array([[x], [t], [np.nextafter(np.float32(t), np.float32(np.inf))], [-0.0], [np.nan]])
    np.testing.assert_array_equal(to.condition_bits(X, 0, t, True, True, np.float32),
                                  [True, True, True, False, False])
    np.testing.assert_array_equal(to.condition_bits(X, 0, t, False, True, np.float64),
                                  [False, True, True, False, True])
    np.testing.assert_array_equal(to.condition_bits(X, 0, t, False, False, np.float64),
                                  [False, False, True, False, True])
    np.testing.assert_array_equal(to.condition_bits(X, 0, 0.0, True, True, np.float32),
                                  [True, True, True, True, False])


def test_boundary_models_meet_the_coverage_floor():
    """tests/tree_boundary_models.py on the oracle's own features of a synthetic batch with NaN
    coordinates (no device): margins stay within +-4 in units of 2^-6 (asserted by the builder),
    and from 7 trees on the batch visits numeric ties on >= 1 % of its rows, a
    split where the float64 and the float32 compare disagree, NaN defaults in both directions and
    constant bool splits in both directions -- under the float32 `<` and the float64 `<=` rule."""
    import tree_boundary_models as bm
    from oracle import tree_oracle as to
    from socceraction_amd import synthetic
    d = synthetic.spadl_games(2, seed=5)
    off = d['game_off']
    for c in ('start_x', 'end_y'):
        d[c] = d[c].copy()
        d[c][[0, 1, 127, 128, int(off[1]), int(off[2]) - 1]] = np.nan
    cols = {c: d[c] for c in d if c not in ('game_off', 'home_team_id', 'seg', 'pos')}
    feats = vo.features(cols, 3, vo.SPADL_DEFAULT, seg_off=off, home=list(d['home_team_id']))
    X = np.stack([c[2].astype(np.float64) for c in feats], axis=1)
    kinds = [c[1] for c in feats]
    for n_trees in (0, 1, 7, 37):
        m = bm.boundary_model(X, kinds, n_trees, seed=100 + n_trees)
        assert m.n_trees == n_trees and m.max_margin <= 4.0
        np.testing.assert_array_equal(to.predict_flat(m.flat_lt, 0.0, X, True, np.float32),
                                      to.predict_xgboost_json(m.json, X))
        if n_trees < 7:
            continue
        for lt, flat, dt in ((True, m.flat_lt, np.float32), (False, m.flat_le, np.float64)):
            cov = bm.coverage(flat, X, kinds, lt, dt)
            assert cov['num_tie_fraction'] >= 0.01 and cov['disagree_splits'] >= 1, cov
            assert cov['nan_left'] >= 1 and cov['nan_right'] >= 1, cov
            assert cov['const_left'] >= 1 and cov['const_right'] >= 1 and cov['f_tie_visits'] >= 1, cov
