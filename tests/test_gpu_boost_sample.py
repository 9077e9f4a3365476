"""Sample weights, row / column subsampling and the L1 penalty of the device learner
(the tuning arguments of ``sa_boost_grad``, ``sa_boost_split`` and ``sa_boost_hist_bins``,
``sa_boost_row_keys``, socceraction_amd.boost) against the numpy restatement of contract items 13-17
(tests/boost_sample_reference.py).  Integers, node records, margins and models are compared
exactly; only ``expf`` against numpy's ``exp`` gets the 1e-6 relative bar of tests/test_gpu_boost.py."""
import json

import numpy as np
import pandas as pd
import pytest

import boost_reference as br
import boost_sample_reference as bs
from golden_io import frame, load

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

FEATURE_GROUP = 4
BINS_TILE, BINS_WG_PER_CU, BINS_MIN_GRID_X = 1024, 4, 8  # sa_boost_hist_bins' launch shape (tests/test_gpu_boost.py)


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, batch, boost, ops, trees
    _native.load_library()
    assert _native.SA_BOOST_FEATURE_GROUP == FEATURE_GROUP
    assert (_native.SA_BOOST_BINS_TILE, _native.SA_BOOST_BINS_WG_PER_CU, _native.SA_BOOST_BINS_MIN_GRID_X) == \
        (BINS_TILE, BINS_WG_PER_CU, BINS_MIN_GRID_X)
    return dict(batch=batch, ops=ops, trees=trees, boost=boost, native=_native)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def game(sa):
    """spadl_full0 as in tests/test_gpu_boost.py: the bitmap-form feature blocks, their host
    values and the labels (scores, every fifth row positive); weights in [0, 5), every 17th zero
    and one 8.0."""
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
    B = np.stack([br.bins_of(br.cast32(c), k) for c, k in zip(cols, cuts)])
    yd = torch.zeros(fb.n + 16, dtype=torch.uint8, device=ab.device)
    yd[:fb.n] = _dev(y)
    w = (np.random.default_rng(0).random(fb.n) * 5).astype(np.float32)
    w[::17] = 0
    w[3] = 8.0
    return dict(g=g, df=df, ab=ab, fb=fb, cols=cols, y=y, yd=yd, cuts=cuts, B=B, w=w,
                is_bool=np.array([c.dtype == np.bool_ for c in cols]))


# ----------------------------------------------------------------------------- gradients
MARGINS = np.array([0, 1e-3, -1e-3, 20, -20, 88, -88, 104, -104], np.float32)


def _below(x):
    return np.nextafter(np.float32(x), np.float32(0))


@pytest.mark.parametrize('spw', [1.0, 3.0])
@pytest.mark.parametrize('e', [0, 3, 20])
@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_grad_ex_equals_the_restatement(sa, n, e, spw):
    boost = sa['boost']
    m = np.resize(np.repeat(MARGINS, 2), n)
    y = np.resize(np.array([0, 1], np.uint8), n)
    top = np.float32(2.0 ** e)
    w = np.resize(np.array([0, 1, top, _below(top), 1e-45], np.float32), n)  # (5 values against y's period 2)
    # the kernel's precondition: every effective weight is at most 2^e (a quarter is exact)
    w = np.where(bs.effective_weight(w, y, spw) > top, w / np.float32(4), w).astype(np.float32)
    w[(m == 104) & (y == 0)] = top
    if spw == 1.0:
        w[(m == -104) & (y == 1)] = top
    we = bs.effective_weight(w, y, spw)
    assert we.max() <= top
    assert n < 10 or {float(np.float32(v)) for v in (0, 1, top, _below(top), 1e-45)} <= set(w[y == 0].tolist())
    seed, t = 11, 5
    u = (bs.draw(bs.SALT_ROWS, seed, t, np.arange(n)) >> np.uint64(32)).astype(np.int64)
    j = n // 2
    md, yd, wd = _dev(m), _dev(y), _dev(w)

    def check(thr, keys=None, key_values=None, round=t):
        gq, hq, p = boost.gradients(md, yd, weight=wd, scale_pos_weight=spw, shift=e, row_keys=keys, seed=seed,
                                    round=round, thr=thr)
        gq, hq, p = gq.cpu().numpy(), hq.cpu().numpy(), p.cpu().numpy()
        kv = np.arange(n) if key_values is None else key_values
        inside = None if thr is None else bs.row_sample(seed, round, kv, thr)
        wg, wh = bs.quantise(p, y, we, e, inside)  # the restatement applied to the device's p
        np.testing.assert_array_equal(gq, wg)
        np.testing.assert_array_equal(hq, wh)
        np.testing.assert_allclose(p, br.probability(m), rtol=1e-6, atol=0)
        return gq, hq, inside

    gq, hq, _ = check(None)
    assert gq.dtype == np.int32 and hq.dtype == np.int32
    assert (gq[(m == 104) & (y == 0)] == 2 ** 30).all() and (hq[np.abs(m) == 104] == 0).all()
    if spw == 1.0:
        assert (gq[(m == -104) & (y == 1)] == -2 ** 30).all()
    assert (gq[w == 0] == 0).all() and (hq[w == 0] == 0).all() and np.abs(gq.astype(np.int64)).max() <= 2 ** 30
    if n > 1:
        assert np.abs(gq).max() > 0
    # the strict `<` of the row sample: row j is out at thr = u[j] and in at u[j] + 1
    _, _, inside = check(int(u[j]))
    assert not inside[j]
    g1, h1, inside = check(int(u[j]) + 1)
    assert inside[j] and (inside == (u <= u[j])).all()
    g0, h0, inside = check(0)
    assert not inside.any() and not g0.any() and not h0.any()
    gall, hall, inside = check(2 ** 32)  # everybody, although every draw is < 2^32
    assert inside.all() and (gall == gq).all() and (hall == hq).all()
    if n > 1:
        other = check(2 ** 31, round=t + 1)[2]
        assert (other != bs.row_sample(seed, t, np.arange(n), 2 ** 31)).any()  # the round counts
    # keys: the index given explicitly is the default; keys beyond 2^63 are their bit patterns
    ga, ha, _ = check(2 ** 31)
    gb, hb, _ = check(2 ** 31, _dev(np.arange(n, dtype=np.int64)))
    assert (ga == gb).all() and (ha == hb).all()
    big = (np.uint64(2 ** 63) + np.arange(n, dtype=np.uint64))
    check(2 ** 31, _dev(big.view(np.int64)), big)


def test_grad_neutral_arguments_spelled_out_are_the_defaults(sa):
    """One row, and one workgroup minus one, exactly, and plus one row: every neutral argument
    written out -- a weight column of ones, the row index as the key, thr = 2^32, scale_pos_weight
    = 1, shift = 0 -- gives the bytes of the call that leaves it out."""
    boost = sa['boost']
    for n in (1, 255, 256, 257):
        m = np.resize(np.repeat(MARGINS, 2), n)
        y = np.resize(np.array([0, 1], np.uint8), n)
        plain = [a.cpu().numpy().tobytes() for a in boost.gradients(_dev(m), _dev(y))]
        assert [len(b) for b in plain] == [4 * n] * 3
        ones, index = _dev(np.ones(n, np.float32)), _dev(np.arange(n, dtype=np.int64))
        for kw in (dict(weight=ones), dict(row_keys=index), dict(thr=2 ** 32), dict(scale_pos_weight=1.0, shift=0),
                   dict(weight=ones, row_keys=index, thr=2 ** 32, scale_pos_weight=1.0, shift=0)):
            got = [a.cpu().numpy().tobytes() for a in boost.gradients(_dev(m), _dev(y), **kw)]
            assert got == plain, (n, sorted(kw))


# ----------------------------------------------------------------------------- row keys
def test_row_keys_wrap_like_the_restatement(sa):
    gid = np.array([0, 1, 2, -1, 2 ** 62, -2 ** 63, 2 ** 63 - 1, 12345], np.int64)
    aid = np.array([0, 1, -1, 2 ** 63 - 1, 2 ** 62, -2 ** 63, 2 ** 63 - 1, 77], np.int64)
    got = sa['boost'].row_keys(gid, aid).cpu().numpy()
    with np.errstate(over='ignore'):
        want = bs.fm(gid.view(np.uint64)) + aid.view(np.uint64)
    np.testing.assert_array_equal(got.view(np.uint64), want)
    assert got.view(np.uint64)[1] == np.uint64(0x5692161d100b05e5 + 1)
    n = 257  # more than one workgroup
    gid, aid = np.arange(n, dtype=np.int64) // 100 + 7, np.arange(n, dtype=np.int64) % 100
    with np.errstate(over='ignore'):
        want = bs.fm(gid.view(np.uint64)) + aid.view(np.uint64)
    np.testing.assert_array_equal(sa['boost'].row_keys(gid, aid).cpu().numpy().view(np.uint64), want)
    assert sa['boost'].row_keys(gid[:0], aid[:0]).numel() == 0


# ----------------------------------------------------------------------------- splits
c3 = np.array([1.0, 2.0, 3.0], np.float32)


def _hist(F, entries, e):
    """[1, F, 256, 2] from {(feature, bin): (g, h)}: integers in units of 2^(e - 30), so the
    float64 sums are the given numbers exactly."""
    h = np.zeros((1, F, 256, 2), np.int64)
    for (f, b), (g, hh) in entries.items():
        h[0, f, b] = (int(g * 2 ** (30 - e)), int(hh * 2 ** (30 - e)))
    return h


def _expected_level(h, tot, cuts, e, features, **kw):
    """The restated records of a level and of its children level, as best_splits lays them out."""
    p = {**bs.DEFAULTS, **kw}
    nodes = h.shape[0]
    rec = np.zeros(3 * nodes, bs.NODE_DTYPE)
    wins = []
    for k in range(nodes):
        G, H = int(tot[k][0]), int(tot[k][1])
        rec[k]['exists'], rec[k]['G'], rec[k]['H'] = 1, G, H
        rec[k]['feature'] = rec[k]['cut'] = -1
        rec[k]['value'] = bs.leaf_value(G, H, p['learning_rate'], p['reg_lambda'], p['reg_alpha'], e)
        best = bs.best_split(h[k], G, H, cuts, p['reg_lambda'], p['min_child_weight'], p['gamma'], p['reg_alpha'], e,
                             features)
        wins.append(None if best is None else best[:2])
        if best is not None:
            f, i, gain, gl, hl = best
            rec[k]['feature'], rec[k]['cut'], rec[k]['gain'], rec[k]['thr'] = f, i, gain, cuts[f][i]
            for c, (cg, ch) in ((nodes + 2 * k, (gl, hl)), (nodes + 2 * k + 1, (G - gl, H - hl))):
                rec[c]['exists'], rec[c]['G'], rec[c]['H'], rec[c]['feature'] = 1, cg, ch, -1
    return rec, wins


def _same_records(got, rec, what):
    for field in ('feature', 'cut', 'exists', 'G', 'H'):
        np.testing.assert_array_equal(got[field], rec[field], f'{what} {field}')
    for field, bits in (('gain', np.uint64), ('value', np.uint32), ('thr', np.uint32)):
        np.testing.assert_array_equal(got[field].view(bits), rec[field].view(bits), f'{what} {field}')
    assert got.tobytes() == rec.tobytes(), what


def _split_cases(e):
    two = {(0, 0): (-1, 6), (0, 2): (0, 5), (1, 0): (-5, 6), (1, 3): (4, 5), (2, 0): (-3, 6), (2, 1): (2, 5)}
    return {
        # alpha = 2, taken from the integers below.  cut 0: GL = -1 is inside (-alpha, alpha)
        'child_below_alpha': (_hist(1, {(0, 0): (-1, 6), (0, 2): (4, 5)}, e), [c3], dict(reg_alpha=2.0), None, (0, 0)),
        # GL == alpha exactly: neither strict comparison holds, T(GL) = 0
        'child_equals_alpha': (_hist(1, {(0, 0): (2, 6), (0, 2): (-5, 5)}, e), [c3], dict(reg_alpha=2.0), None, (0, 0)),
        # the parent's |G| = 1 < alpha: its leaf is -0.0 and the parent term of the gain vanishes
        'parent_below_alpha': (_hist(1, {(0, 0): (-5, 6), (0, 2): (4, 5)}, e), [c3], dict(reg_alpha=2.0), None,
                               (0, 0)),
        # everything shrinks to zero: no gain above gamma = 0, a leaf
        'alpha_above_everything': (_hist(1, {(0, 0): (-5, 6), (0, 2): (4, 5)}, e), [c3], dict(reg_alpha=9.0), None,
                                   None),
        'no_mask_baseline': (_hist(3, two, e), [c3, c3, c3], {}, None, (1, 0)),
        # the mask hides the unmasked winner (feature 1): the next best feature wins
        'mask_hides_the_winner': (_hist(3, two, e), [c3, c3, c3], {}, [0, 2], (2, 0)),
        'mask_leaves_one': (_hist(3, two, e), [c3, c3, c3], {}, [0], (0, 0)),
        # min_child_weight = 0: an all-zero histogram is a valid candidate of gain exactly 0 that wins by
        # index order over feature 2's negative gain (alpha shrinks its children) -- unless it is masked
        'zero_histograms_unmasked': (_hist(3, {(2, 0): (3, 6), (2, 1): (3, 5)}, e), [c3, c3, c3[:1]],
                                     dict(reg_alpha=2.5, min_child_weight=0.0, gamma=-100.0), None, (0, 0)),
        'zero_histograms_masked': (_hist(3, {(2, 0): (3, 6), (2, 1): (3, 5)}, e), [c3, c3, c3[:1]],
                                   dict(reg_alpha=2.5, min_child_weight=0.0, gamma=-100.0), [2], (2, 0)),
    }


@pytest.mark.parametrize('e', [0, 3])
@pytest.mark.parametrize('case', sorted(_split_cases(0)))
def test_split_ex_equals_the_restatement(sa, case, e):
    h, cuts, kw, features, want = _split_cases(e)[case]
    F = h.shape[1]
    f_tot = 2 if case.startswith('zero_histograms') else 0
    tot = [[int(h[0, f_tot, :, 0].sum()), int(h[0, f_tot, :, 1].sum())]]
    rec, wins = _expected_level(h, tot, cuts, e, features, **kw)
    assert wins[0] == want, wins
    if case == 'parent_below_alpha':
        assert rec[0]['value'] == 0 and np.signbit(rec[0]['value'])
    if case == 'zero_histograms_masked':
        assert rec[0]['gain'] < 0
    mask = None if features is None else np.isin(np.arange(F), features)
    got = sa['boost'].best_splits(_dev(h), tot, cuts, **{k: v for k, v in kw.items()}, shift=e, feature_mask=mask)
    print(case, e, got, rec)
    _same_records(got, rec, case)
    if e == 0 and not kw.get('reg_alpha') and features is None:  # the neutral arguments left out
        assert sa['boost'].best_splits(_dev(h), tot, cuts, **kw).tobytes() == got.tobytes()


@pytest.mark.parametrize('e', [0, 3])
def test_split_ex_of_a_whole_level_under_one_mask(sa, e):
    """32 nodes x (FEATURE_GROUP + 1) features, node 1 absent: one mask, a different outcome per
    node -- the unmasked winner hidden in some nodes and untouched in others."""
    rng = np.random.default_rng(5 + e)
    F, nodes = FEATURE_GROUP + 1, 32
    cuts = [np.arange(1, 1 + m, dtype=np.float32) for m in (254, 3, 1, 17, 254)]
    h = np.zeros((nodes, F, 256, 2), np.int64)
    tot = np.zeros((nodes, 2), np.int64)
    for k in range(nodes):
        if k == 1:
            continue
        rows = 300
        g = rng.integers(-2 ** 29, 2 ** 29, rows)
        hh = rng.integers(1, 2 ** 28, rows)
        for f in range(F):
            b = rng.integers(0, len(cuts[f]) + 1, rows)
            b[rng.random(rows) < 0.05] = 255
            np.add.at(h[k, f, :, 0], b, g)
            np.add.at(h[k, f, :, 1], b, hh)
        tot[k] = (g.sum(), hh.sum())
    alpha = float(np.median(np.abs(tot[:, 0]))) * 2.0 ** (e - 30) / 8  # from the data: some |GL| fall below it
    kw = dict(reg_alpha=alpha, min_child_weight=0.5)
    features = [1, 2, 3]
    free, free_wins = _expected_level(h, tot, cuts, e, None, **kw)
    rec, wins = _expected_level(h, tot, cuts, e, features, **kw)
    hidden = [k for k in range(nodes) if free_wins[k] is not None and free_wins[k][0] in (0, 4)]
    kept = [k for k in range(nodes) if free_wins[k] is not None and free_wins[k][0] in features]
    print('hidden', hidden, 'kept', kept, 'winners', wins)
    assert hidden and kept and len({w[0] for w in wins if w is not None}) >= 2
    mask = np.isin(np.arange(F), features)
    got = sa['boost'].best_splits(_dev(h), tot, cuts, **kw, shift=e, feature_mask=mask)
    assert got[1]['feature'] == -1 and wins[1] is None  # the node without rows: a leaf
    _same_records(got, rec, 'masked level')
    _same_records(sa['boost'].best_splits(_dev(h), tot, cuts, **kw, shift=e), free, 'unmasked level')


# ----------------------------------------------------------------------------- whole fits
ALL_ON = dict(n_estimators=8, max_depth=3, subsample=0.5, colsample_bytree=0.3, reg_alpha=0.5, scale_pos_weight=3.0,
              random_state=7)
# F = 568 (515 bool, 53 numeric): 0.01 keeps 5 features (rounds with no numeric one), 0.002 one
# feature (seed 56: rounds 0 and 4 hold the numeric one, i.e. no bool feature; the others no numeric)
FITS = {'all_on': ALL_ON, 'few_columns': {**ALL_ON, 'colsample_bytree': 0.01},
        'one_column': {**ALL_ON, 'colsample_bytree': 0.002, 'random_state': 56}}


@pytest.fixture(scope='module')
def fits(sa, game):
    return {k: sa['boost'].TunedGBTClassifier(record=True, **p).fit_blocks(
        game['fb'], game['yd'], cuts=game['cuts'], sample_weight=game['w']) for k, p in FITS.items()}


@pytest.mark.parametrize('which', sorted(FITS))
def test_whole_fit_replayed_round_by_round(sa, game, fits, which):
    clf, params = fits[which], FITS[which]
    y, w, B = game['y'], game['w'], game['B']
    F, n = B.shape
    P = clf.record_['p'].cpu().numpy()
    M = clf.record_['margin'].cpu().numpy()
    we = bs.effective_weight(w, y, params['scale_pos_weight'])
    e = bs.shift_of(we.max())
    assert clf.quant_shift_ == e == 4 and clf.trees_.shape == (8, 15)
    m = np.full(n, br.base_margin(0.5), np.float32)
    keys = np.arange(n, dtype=np.int64)
    splits, n_bool, n_num = [], [], []
    for t in range(8):
        np.testing.assert_allclose(P[t], br.probability(m), rtol=1e-6, atol=0)
        rows, cols = bs.round_inputs(params, t, F, keys)
        np.testing.assert_array_equal(clf.column_samples_[t], cols)
        gq, hq = bs.quantise(P[t], y, we, e, rows)       # the restated tree from the device's p_t
        tab, node = bs.build_tree(B, gq, hq, game['cuts'], params, e, cols)
        assert tab.tobytes() == clf.trees_[t].tobytes(), (t, tab, clf.trees_[t])
        m = br.update_margin(m, tab, node)               # a row outside the sample still gets its leaf
        assert m.tobytes() == M[t].tobytes(), t
        splits.append(int(((tab['feature'] >= 0) & (tab['exists'] != 0)).sum()))
        n_bool.append(int(game['is_bool'][cols].sum()))
        n_num.append(int((~game['is_bool'][cols]).sum()))
        assert 0.35 * n < rows.sum() < 0.65 * n
    assert m.tobytes() == clf.margin_.cpu().numpy().tobytes()
    print(which, 'splits', splits, 'bool', n_bool, 'numeric', n_num)
    if which == 'all_on':
        assert min(splits) >= 1  # every round found a split (the restatement alone: 6 7 5 7 6 5 7 7)
    elif which == 'few_columns':
        assert 0 in n_num and max(splits) >= 1
    else:
        assert 0 in n_bool and 0 in n_num and max(splits) >= 1
    imp = clf.feature_importances_
    used = np.unique(clf.trees_['feature'][(clf.trees_['feature'] >= 0) & (clf.trees_['exists'] != 0)])
    assert imp.shape == (F,) and abs(float(imp.sum()) - 1) < 1e-5 and set(np.flatnonzero(imp)) <= set(used.tolist())
    cover = sa['boost'].importances(clf.trees_, F, 'total_cover', e)
    assert abs(float(cover.sum()) - 1) < 1e-5


WIDE_TUNED = dict(n_estimators=2, max_depth=6, subsample=0.5, colsample_bytree=0.5, random_state=7)


def test_tuned_fit_over_many_workgroups(sa):
    """The 40,000 x 388 table of tests/test_gpu_boost.py (more row steps than workgroups at every
    level, twenty bitmap tiles) under a row sample, a column sample -- the sampled bin histograms
    (sa_boost_hist_bins with a row list) past one trip -- and weights with shift 3."""
    from test_gpu_boost import bins_launch, wide_table
    t = wide_table()
    X, y, cuts, B = t['X'], t['y'], t['cuts'], t['B']
    F, n = B.shape
    w = (np.random.default_rng(1).random(n) * 5).astype(np.float32)
    w[::17] = 0
    w[3] = 8.0
    params = WIDE_TUNED
    clf = sa['boost'].TunedGBTClassifier(record=True, **params).fit(X, y, cuts=cuts, sample_weight=w)
    we = bs.effective_weight(w, y, 1.0)
    e = bs.shift_of(we.max())
    assert clf.quant_shift_ == e == 3 and clf.trees_.shape == (2, 127)
    P = clf.record_['p'].cpu().numpy()
    M = clf.record_['margin'].cpu().numpy()
    m = np.full(n, br.base_margin(0.5), np.float32)
    keys = np.arange(n, dtype=np.int64)
    for r in range(2):
        np.testing.assert_allclose(P[r], br.probability(m), rtol=1e-6, atol=0)
        rows, cols = bs.round_inputs(params, r, F, keys)
        np.testing.assert_array_equal(clf.column_samples_[r], cols)
        n_num = int((cols < 128).sum())
        assert len(cols) == F // 2 and 32 < n_num < 96 and 0.45 * n < rows.sum() < 0.55 * n
        assert (n + BINS_TILE - 1) // BINS_TILE > bins_launch(n_num, 32)[2]  # level 5: more row steps than workgroups
        gq, hq = bs.quantise(P[r], y, we, e, rows)       # the restated tree from the device's p_t
        tab, node = bs.build_tree(B, gq, hq, cuts, params, e, cols)
        assert tab.tobytes() == clf.trees_[r].tobytes(), (r, tab, clf.trees_[r])
        m = br.update_margin(m, tab, node)
        assert m.tobytes() == M[r].tobytes(), r
    assert m.tobytes() == clf.margin_.cpu().numpy().tobytes()
    splits = (clf.trees_['feature'] >= 0) & (clf.trees_['exists'] != 0)
    assert splits[:, 0].all() and splits[:, 31:63].any(axis=1).all()  # both rounds split, down to level 5


# where the tuning arguments stand in each entry point's argument list (include/socceraction_amd.h):
# grad: weight, scale_pos_weight, shift, row_keys, thr; hist_bins: num_rows; split: reg_alpha, shift, feature_mask
TUNING_ARGS = {'grad': (4, 5, 6, 7, 10), 'hist_bins': (3,), 'split': (11, 12, 13)}
NEUTRAL_ARGS = {'grad': (None, 1.0, 0, None, 2 ** 32), 'hist_bins': (None,), 'split': (0.0, 0, None)}
GRAD_GQ = 11


def _families(sa, clf, fit, tuning=None):
    """The (family, entry point) sequence of the launches of ``fit(clf)``; ``tuning`` (a list)
    receives, for every launch of a family in TUNING_ARGS, ``(family, its tuning arguments)`` --
    for a gradient launch with its ``gq`` argument appended."""
    seq = []
    plain = clf._launch

    def launch(family, fn, *args):
        seq.append((family, fn.__name__))
        if tuning is not None and family in TUNING_ARGS:
            extra = (args[GRAD_GQ],) if family == 'grad' else ()
            tuning.append((family, tuple(args[i] for i in TUNING_ARGS[family]) + extra))
        plain(family, fn, *args)
    clf._launch = launch
    fit(clf)
    return seq


def test_neutral_parameters_change_nothing(sa, game, monkeypatch):
    boost, fb = sa['boost'], game['fb']
    base = boost.DeviceGBTClassifier(n_estimators=4)
    tun0, tun1 = [], []
    seq0 = _families(sa, base, lambda c: c.fit_blocks(fb, game['yd'], cuts=game['cuts']), tun0)
    neutral = dict(subsample=1.0, colsample_bytree=1.0, reg_alpha=0.0, scale_pos_weight=1.0, random_state=9)
    # explicit neutral values: the plain fit's launches, launch for launch, and no host read for the weights
    same = boost.TunedGBTClassifier(n_estimators=4, **neutral)
    for reader in ('_weight_shift', '_weight_stats'):
        monkeypatch.setattr(boost.DeviceGBTClassifier, reader,
                            lambda *a: (_ for _ in ()).throw(AssertionError('a host read')))
    seq1 = _families(sa, same, lambda c: c.fit_blocks(fb, game['yd'], cuts=game['cuts'],
                                                      row_keys=np.arange(fb.n)[::-1].copy()), tun1)
    monkeypatch.undo()
    assert seq1 == seq0
    # every launch of both fits carries the neutral constants (the last gradient launch no gq besides)
    for tun in (tun0, tun1):
        assert {f for f, _ in tun} == set(TUNING_ARGS) and tun[-1][0] == 'grad' and tun[-1][1][-1] is None
        for family, args in tun:
            assert args[:len(NEUTRAL_ARGS[family])] == NEUTRAL_ARGS[family], (family, args)
    assert same.trees_.tobytes() == base.trees_.tobytes() and same.quant_shift_ == 0
    # ... plus a weight column of ones: the same trees and the same families
    ones = boost.TunedGBTClassifier(n_estimators=4, **neutral)
    seq2 = _families(sa, ones, lambda c: c.fit_blocks(fb, game['yd'], cuts=game['cuts'],
                                                      sample_weight=np.ones(fb.n, np.float32)))
    assert [f for f, _ in seq2] == [f for f, _ in seq0]
    assert ones.trees_.tobytes() == base.trees_.tobytes() and ones.quant_shift_ == 0
    assert ones.margin_.cpu().numpy().tobytes() == base.margin_.cpu().numpy().tobytes()
    assert ones.column_samples_ is None


def test_launch_sequence_of_a_tuned_fit(sa, game, monkeypatch):
    """The (family, entry point) sequence of a tuned fit, written out from the contract: per round
    the gradients; per level the bitmap histograms always, the bin histograms exactly when the
    round's sample holds a numeric feature, the split search and the advance; then the leaf values
    and the margin; after the last round the gradients for ``p_``.  What tells a tuned launch is its
    arguments: every round's gradients carry the weight column, the fit's shift and the row
    threshold, the last launch (no ``gq``) the neutral ones; every bin histogram a row list; every
    split launch the L1 penalty and the shift, and every level's search the round's mask (the leaf
    values' launch searches nothing and gets none)."""
    boost = sa['boost']
    D, T = 2, 5
    F = len(game['fb'].plan.names)
    uploaded = []
    upload = boost.weights_to_device
    monkeypatch.setattr(boost, 'weights_to_device', lambda w, dev: uploaded.append(upload(w, dev)) or uploaded[-1])
    for which in ('all_on', 'one_column'):
        params = {**FITS[which], 'max_depth': D, 'n_estimators': T}
        clf = boost.TunedGBTClassifier(**params)
        tun = []
        seq = _families(sa, clf, lambda c: c.fit_blocks(game['fb'], game['yd'], cuts=game['cuts'],
                                                        sample_weight=game['w']), tun)
        assert len(clf.column_samples_) == T
        numeric = [bool((~game['is_bool'][S]).any()) for S in clf.column_samples_]
        if which == 'one_column':  # one feature a round: rounds with and without a numeric one occur
            assert True in numeric and False in numeric, numeric
        want = []
        for t in range(T):
            want.append(('grad', 'sa_boost_grad'))
            for _ in range(D):
                want.append(('hist_bits', 'sa_boost_hist_bits'))
                if numeric[t]:
                    want.append(('hist_bins', 'sa_boost_hist_bins'))
                want += [('split', 'sa_boost_split'), ('advance', 'sa_boost_advance')]
            want += [('split', 'sa_boost_split'), ('advance', 'sa_boost_advance')]
        want.append(('grad', 'sa_boost_grad'))
        assert seq == want, which
        e, wptr = clf.quant_shift_, uploaded[-1].data_ptr()
        assert e == 4 and wptr
        grads = [a for f, a in tun if f == 'grad']
        assert len(grads) == T + 1
        for a in grads[:T]:  # (the default key: a non-sharded fit passes no key column)
            assert a[:5] == (wptr, params['scale_pos_weight'], e, None, bs.threshold(params['subsample'])) and a[5]
        assert grads[T] == NEUTRAL_ARGS['grad'] + (None,)
        bins = [a for f, a in tun if f == 'hist_bins']
        assert len(bins) == D * sum(numeric) and all(a[0] for a in bins)
        splits = [a for f, a in tun if f == 'split']
        assert len(splits) == T * (D + 1) and splits[0][2]
        for k, a in enumerate(splits):  # round t's mask is row t of the fit's [T, F] byte table
            t, leaves = divmod(k, D + 1)[0], k % (D + 1) == D
            assert a == (params['reg_alpha'], e, None if leaves else splits[0][2] + t * F), (k, a)


def test_weight_duplication_on_the_device(sa, game):
    """Uniform weight 2 against the table stacked twice (tests/test_boost_sample_host.py)."""
    boost, fb = sa['boost'], game['fb']
    X = pd.DataFrame({n: c for n, c in zip(fb.plan.names, game['cols'])})
    n = len(X)
    a = boost.DeviceGBTClassifier(n_estimators=4).fit(X, game['y'], cuts=game['cuts'], sample_weight=np.full(n, 2.0))
    b = boost.DeviceGBTClassifier(n_estimators=4).fit(pd.concat([X, X], ignore_index=True),
                                                      np.concatenate([game['y'], game['y']]), cuts=game['cuts'])
    assert (a.quant_shift_, b.quant_shift_) == (1, 0)
    for field in ('feature', 'cut', 'thr', 'gain', 'value', 'exists'):
        assert a.trees_[field].tobytes() == b.trees_[field].tobytes(), field
    np.testing.assert_array_equal(b.trees_['G'], 2 * a.trees_['G'])
    np.testing.assert_array_equal(b.trees_['H'], 2 * a.trees_['H'])
    assert b.margin_.cpu().numpy()[:n].tobytes() == a.margin_.cpu().numpy().tobytes()


def test_weight_errors_found_on_the_device(sa, game):
    boost, fb = sa['boost'], game['fb']
    clf = boost.DeviceGBTClassifier(n_estimators=1)
    clf._events = []
    rows = np.arange(100)
    bad = {'nan': np.nan, 'negative': -1.0, 'large': 2.0 ** 20 + 1, 'inf': np.inf}
    for name, v in bad.items():
        w = np.ones(fb.n, np.float32)
        w[50] = v
        with pytest.raises(ValueError):
            clf.fit_blocks(fb, game['yd'], cuts=game['cuts'], sample_weight=_dev(w), rows=rows)
        w[50], w[500] = 1.0, v  # a held-out row's weight is not looked at
        if name != 'large':
            continue
        clf.fit_blocks(fb, game['yd'], cuts=game['cuts'], sample_weight=_dev(w), rows=rows)
        assert clf.quant_shift_ == 0 and clf._events
        clf._events = []
    w = np.ones(fb.n, np.float32)
    w[:100] = 0
    with pytest.raises(ValueError):
        clf.fit_blocks(fb, game['yd'], cuts=game['cuts'], sample_weight=_dev(w), rows=rows)
    with pytest.raises(ValueError):  # 2^19 * 3 on a positive row
        boost.TunedGBTClassifier(n_estimators=1, scale_pos_weight=3.0).fit_blocks(
            fb, game['yd'], cuts=game['cuts'], sample_weight=_dev(np.full(fb.n, 2.0 ** 19, np.float32)))
    with pytest.raises(ValueError):
        clf.fit_blocks(fb, game['yd'], cuts=game['cuts'], sample_weight=_dev(w[:fb.n - 1]))
    assert clf._events == []  # every one raised before any training launch


# ----------------------------------------------------------------------------- reproducibility
def test_sampled_fits_are_reproducible(sa, game):
    boost, fb = sa['boost'], game['fb']
    X = pd.DataFrame({n: c for n, c in zip(fb.plan.names, game['cols'])})
    y, w, cuts = game['y'], game['w'], game['cuts']
    params = {**ALL_ON, 'n_estimators': 5}

    def fit(Xf, yf, wf, keys=None, **over):
        clf = boost.TunedGBTClassifier(**{**params, **over}).fit(Xf, yf, cuts=cuts, sample_weight=wf, row_keys=keys)
        return json.dumps(clf.to_xgboost_json())
    first = fit(X, y, w)
    assert fit(X, y, w) == first
    assert json.dumps(boost.TunedGBTClassifier(**params).fit_blocks(
        fb, game['yd'], cuts=cuts, sample_weight=w).to_xgboost_json()) == first
    assert fit(X, y, w, random_state=8) != first
    assert fit(X, y, w, np.arange(len(X))) == first  # the default key is the row index
    perm = np.random.default_rng(0).permutation(len(X))
    Xp = X.iloc[perm].reset_index(drop=True)
    assert fit(Xp, y[perm], w[perm], perm) == first   # the sample belongs to the key, not to the position
    assert fit(Xp, y[perm], w[perm]) != first         # default keys: run-to-run identity only


def test_early_stopping_still_closes(sa, game):
    boost, fb = sa['boost'], game['fb']
    ev = np.flatnonzero(np.arange(fb.n) % 4 == 3)
    tr = np.flatnonzero(np.arange(fb.n) % 4 != 3)
    clf = boost.TunedGBTClassifier(n_estimators=40, subsample=0.5, random_state=3, early_stopping_rounds=3,
                                    eval_metric='logloss')
    clf.fit_blocks(fb, game['yd'], rows=tr, cuts=game['cuts'], eval_rows=ev)
    best, run = boost.stop_decision(clf.eval_sums_, 3, False)
    print('best', best, 'rounds run', run)
    assert (clf.best_iteration, clf.n_rounds_run_) == (best, run) and len(clf.trees_) == best + 1
    assert run == best + 4 or run == 40
    te = sa['trees'].TreeEnsemble.from_model(clf)
    assert te.n_trees == best + 1
    assert clf.p_.cpu().numpy().tobytes() == te.predict_blocks(fb).cpu().numpy().tobytes()
    plain = boost.DeviceGBTClassifier(n_estimators=40, early_stopping_rounds=3, eval_metric='logloss')
    plain.fit_blocks(fb, game['yd'], rows=tr, cuts=game['cuts'], eval_rows=ev)
    assert plain.trees_[:1].tobytes() != clf.trees_[:1].tobytes()  # the sample took part


# ----------------------------------------------------------------------------- the public path
def _two_games(order=(0, 1)):
    gs = [load('spadl', f'full{i}') for i in order]
    actions = pd.concat([frame(g) for g in gs], ignore_index=True)
    games = pd.DataFrame({'game_id': [int(frame(g).game_id.iloc[0]) for g in gs],
                          'home_team_id': [int(g['home_team_id'][0]) for g in gs]})
    return games, actions


def _models(model):
    return {c: json.dumps(model._VAEP__models[c].to_xgboost_json()) for c in ('scores', 'concedes')}


def test_public_path_sampled_fit_batch_is_the_same_for_either_game_order(sa):
    import socceraction_amd.vaep as vaep
    params = dict(n_estimators=5, subsample=0.5, random_state=3)
    games, actions = _two_games()
    assert games.game_id.nunique() == 2 and 'action_id' in actions.columns
    a = vaep.VAEP().fit_batch(games, actions, tree_params=params)
    games_r, actions_r = _two_games((1, 0))
    b = vaep.VAEP().fit_batch(games_r, actions_r, tree_params=params)
    assert _models(a) == _models(b)  # fails if the keys are positions
    assert _models(vaep.VAEP().fit_batch(games, actions, tree_params={**params, 'random_state': 4})) != _models(a)
    assert all(len(a._VAEP__models[c].trees_) == 5 for c in ('scores', 'concedes'))
    game = games.iloc[0]
    ga = actions[actions.game_id == game.game_id].reset_index(drop=True)
    rated = a.rate(game, ga)
    assert len(rated) == len(ga) and np.isfinite(rated['vaep_value']).all()
    imp = a._VAEP__models['scores'].feature_importances_
    assert abs(float(imp.sum()) - 1) < 1e-5


def test_public_path_atomic_accepts_the_new_parameters(sa):
    from socceraction_amd.atomic.vaep import AtomicVAEP
    g = load('atomic', 'full0')
    actions = frame(g, atomic=True)
    games = pd.DataFrame({'game_id': [int(actions.game_id.iloc[0])], 'home_team_id': [int(g['home_team_id'][0])]})
    w = (np.random.default_rng(1).random(len(actions)) * 3).astype(np.float32)
    params = dict(n_estimators=5, subsample=0.5, colsample_bytree=0.5, reg_alpha=0.1, scale_pos_weight=2.0,
                  random_state=3)
    a = AtomicVAEP().fit_batch(games, actions, tree_params=params, sample_weight=w)
    b = AtomicVAEP().fit_batch(games, actions, tree_params=params, sample_weight=w)
    assert _models(a) == _models(b)
    assert a._VAEP__models['scores'].quant_shift_ in (2, 3)  # weights below 3, doubled on a positive row
    rated = a.rate(games.iloc[0], actions)
    assert len(rated) == len(actions) and np.isfinite(rated['vaep_value']).all()


def test_public_path_weights_from_the_host_frame_equal_fit_batch(sa):
    import socceraction_amd.vaep as vaep
    games, actions = _two_games()
    w = (np.random.default_rng(2).random(len(actions)) * 4).astype(np.float32)
    w[::11] = 0
    params = dict(n_estimators=5, reg_alpha=0.25, scale_pos_weight=2.0)
    a = vaep.VAEP().fit_batch(games, actions, tree_params=params, sample_weight=w)
    b = vaep.VAEP()
    X = b.compute_features_batch(games, actions)
    Y = b.compute_labels_batch(games, actions)
    b.fit(X, Y, learner='device', val_size=0, tree_params=params, fit_params=dict(sample_weight=w))
    assert _models(a) == _models(b)
    assert _models(vaep.VAEP().fit_batch(games, actions, tree_params=params)) != _models(a)
    assert a._VAEP__models['scores'].quant_shift_ == b._VAEP__models['scores'].quant_shift_ and \
        a._VAEP__models['scores'].quant_shift_ in (2, 3)
