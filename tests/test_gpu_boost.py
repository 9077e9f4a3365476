"""The device boosted-tree trainer (csrc/sa_boost.hip, socceraction_amd.boost) against the numpy
restatement of its arithmetic contract (tests/boost_reference.py).  Every comparison of integers,
node records, margins and models is exact; only ``expf`` against numpy's ``exp`` gets the 1e-6
relative bar tests/test_gpu_trees.py already uses."""
import json

import numpy as np
import pandas as pd
import pytest

import boost_reference as br
from golden_io import assert_close, frame, load

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

BIN_TILE, BITS_TILE, BINS_TILE, FEATURE_GROUP = 1024, 2048, 1024, 4
# the launch shapes: sa_boost_hist_bins' gx = max(BINS_MIN_GRID_X, BINS_WG_PER_CU * CUs / groups);
# sa_boost_hist_bits keeps the sums of BITS_ACC_BYTES / (16 * nodes) bool columns per pass
BINS_WG_PER_CU, BINS_MIN_GRID_X, BITS_ACC_BYTES = 4, 8, 131072


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, batch, boost, ops, trees
    _native.load_library()
    assert (_native.SA_BOOST_BIN_TILE, _native.SA_BOOST_BITS_TILE, _native.SA_BOOST_BINS_TILE,
            _native.SA_BOOST_FEATURE_GROUP) == (BIN_TILE, BITS_TILE, BINS_TILE, FEATURE_GROUP)
    assert (_native.SA_BOOST_BINS_WG_PER_CU, _native.SA_BOOST_BINS_MIN_GRID_X, _native.SA_BOOST_BITS_ACC_BYTES) == \
        (BINS_WG_PER_CU, BINS_MIN_GRID_X, BITS_ACC_BYTES)
    return dict(batch=batch, ops=ops, trees=trees, boost=boost)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def game(sa):
    """spadl_full0: the bitmap-form feature blocks, their host values and the labels of
    tests/test_gpu_trees.py (scores, every fifth row positive)."""
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
    return dict(g=g, df=df, ab=ab, fb=fb, cols=cols, y=y, yd=yd, cuts=cuts, B=B,
                X=np.stack([c.astype(np.float64) for c in cols], 1))


# ----------------------------------------------------------------------------- bins
@pytest.mark.parametrize('tile', [None, 128])
def test_bins_of_the_golden_game(sa, game, tile):
    from oracle import vaep_oracle as vo
    fb = game['fb'] if tile is None else sa['ops'].features(game['ab'], vo.SPADL_DEFAULT, 3, bool_bits=True,
                                                            num_tile=tile)
    cuts = sa['boost'].make_cuts(fb)
    assert len(cuts) == len(game['cuts'])
    for a, b in zip(cuts, game['cuts']):
        np.testing.assert_array_equal(a, b)
    data = sa['boost'].bin_blocks(fb)
    assert data.bins.dtype == torch.uint8 and data.bins.shape == (len(data.num_feat), data.ld)
    np.testing.assert_array_equal(data.host_bins(), game['B'])


def test_cuts_from_a_sample_of_the_rows(sa):
    """More than 65,536 actions: the cuts come from the rows floor(i * n / 65536), gathered from
    the tiled device blocks, not from every row."""
    from oracle import vaep_oracle as vo
    from socceraction_amd import synthetic
    boost, ops = sa['boost'], sa['ops']
    ab = sa['batch'].ActionBatch.from_columns(synthetic.spadl_games(43, seed=5))
    n = ab.n
    assert boost.SAMPLE_ROWS == 65536 < n < 80000
    assert len(np.unique(br.sample_rows(n))) == 65536 and (np.diff(br.sample_rows(n)) == 2).any()
    fb = ops.features(ab, vo.SPADL_DEFAULT, 3, bool_bits=True)
    b, f, i = ops.features(ab, vo.SPADL_DEFAULT, 3).to_numpy()
    host = {'b': b.astype(bool), 'f': f, 'i': i}
    cols = [np.ascontiguousarray(host[k][c, :n]) for _, k, c in fb.plan.order]
    want = [br.cuts_of(c, c.dtype == np.bool_) for c in cols]
    got = boost.make_cuts(fb)
    assert len(got) == len(want) == 568
    for a, w in zip(got, want):
        np.testing.assert_array_equal(a, w)
    assert max(len(w) for w in want) == 254  # the rank rule of a column with many values
    np.testing.assert_array_equal(boost.bin_blocks(fb).host_bins(),
                                  np.stack([br.bins_of(br.cast32(c), k) for c, k in zip(cols, want)]))
    rows = np.arange(0, n, 2)
    for a, c in zip(boost.make_cuts(fb, rows=rows), cols):
        np.testing.assert_array_equal(a, br.cuts_of(c[rows], c.dtype == np.bool_))


def _edge_table(n):
    cuts_f = np.array([-3.5, 0.1, 1.0, 16777216.0], np.float32)
    vals = []
    for c in cuts_f:
        vals += [c, np.nextafter(c, np.float32(-np.inf), dtype=np.float32),
                 np.nextafter(c, np.float32(np.inf), dtype=np.float32)]
    vals = [np.float64(v) for v in vals] + [np.inf, -np.inf, np.nan,
                                            np.float64(np.float32(0.1)) + 1e-12,   # rounds onto the cut
                                            np.float64(np.float32(0.1)) - 1e-12,
                                            np.float64(np.float32(1.0)) - 1e-12, 0.0, -0.0, 1e300, -1e300]
    cuts_i = np.array([0.0, 16777216.0, 16777218.0, 2.0 ** 53], np.float32)
    ints = [0, -1, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 53 - 1, 2 ** 53,
            2 ** 53 + 1, 2 ** 62, -2 ** 62]
    X = pd.DataFrame({'f': np.resize(np.array(vals, np.float64), n), 'flag': np.resize([True, False, False], n),
                      'i': np.resize(np.array(ints, np.int64), n),
                      'g': np.resize(np.array(vals[::-1], np.float64), n)})
    return X, [cuts_f, np.array([0.5], np.float32), cuts_i, cuts_f[:2]]


@pytest.mark.parametrize('n', [1, 15, 16, 17, BIN_TILE - 1, BIN_TILE, BIN_TILE + 1])
def test_bins_at_the_cut_edges(sa, n):
    X, cuts = _edge_table(n)
    data = sa['boost'].bin_host(X, cuts=cuts)
    want = np.stack([br.bins_of(br.cast32(X[c].to_numpy()), k) for c, k in zip(X.columns, cuts)])
    np.testing.assert_array_equal(data.host_bins(), want)
    if n >= 17:
        assert {0, 1, 2, 3, 4, 255} <= set(want[0].tolist())


# ----------------------------------------------------------------------------- gradients
def test_gradients(sa):
    m = np.array([0, 1e-3, -1e-3, 20, -20, 88, -88, 104, -104], np.float32)
    m = np.repeat(m, 2)
    y = np.resize(np.array([0, 1], np.uint8), len(m))
    gq, hq, p = sa['boost'].gradients(_dev(m), _dev(y))
    gq, hq, p = gq.cpu().numpy(), hq.cpu().numpy(), p.cpu().numpy()
    assert gq.dtype == np.int32 and hq.dtype == np.int32 and p.dtype == np.float32
    print('p', p, 'numpy', br.probability(m))
    wg, wh = br.quantise(p, y)  # the restatement applied to the device's p
    np.testing.assert_array_equal(gq, wg)
    np.testing.assert_array_equal(hq, wh)
    assert hq[m == 104].tolist() == [0, 0] and hq[m == -104].tolist() == [0, 0]
    assert gq[m == 104].tolist() == [2 ** 30, 0] and gq[m == -104].tolist() == [0, -2 ** 30]
    np.testing.assert_allclose(p, br.probability(m), rtol=1e-6, atol=0)


# ----------------------------------------------------------------------------- histograms
def _hist_table(n, f_num, n_bool, seed):
    """Numeric columns holding bins directly (value v in 0..254 -> bin v with the cuts 1..254,
    NaN -> 255) and bool columns.  Column 0 puts every row in one bin (a hot address), column 1
    uses all 256 bins; bool column 0 is all ones, column 1 all zeros."""
    rng = np.random.default_rng(seed)
    cols, cuts = {}, []
    for j in range(f_num):
        v = rng.integers(0, 256, n).astype(np.float64)
        if j == 0:
            v[:] = 7.0
        elif j == 1 or f_num == 1:
            v[:min(n, 256)] = np.arange(min(n, 256))
        v[v == 255] = np.nan
        cols[f'n{j}'] = v
        cuts.append(np.arange(1, 255, dtype=np.float32))
    for j in range(n_bool):
        b = rng.random(n) < (0.5 if j % 7 == 2 else 0.03)
        if j == 0:
            b[:] = True
        elif j == 1:
            b[:] = False
        cols[f'b{j}'] = b
        cuts.append(np.array([0.5], np.float32))
    return pd.DataFrame(cols), cuts


HIST_CASES = [  # n, F_num, n_bool, nodes
    (1, 1, 0, 1), (63, 1, 1, 2), (64, FEATURE_GROUP + 1, 65, 8), (65, 1, 65, 32),
    (4099, FEATURE_GROUP + 1, 65, 32), (BINS_TILE + 1, FEATURE_GROUP + 1, 1, 2), (BITS_TILE + 1, 1, 65, 8),
    (70001, 1, 1, 8), (70001, FEATURE_GROUP + 1, 0, 1), (513, 0, 3, 2)]


def _level_rows(n, nodes):
    """Random gradients and level-local nodes of n rows: node 1 is empty, a tenth of the rows take
    no part; with two nodes, node 0 holds every row."""
    rng = np.random.default_rng(n)
    gq = rng.integers(-2 ** 30, 2 ** 30 + 1, n).astype(np.int32)
    hq = rng.integers(0, 2 ** 28 + 1, n).astype(np.int32)
    node = rng.integers(0, nodes, n).astype(np.uint8)
    if nodes > 1:
        node[node == 1] = 0                    # node 1 is empty
        node[rng.random(n) < 0.1] = 255        # rows that take no part
    if nodes == 2:
        node[:] = 0                            # a node holding every row
    return gq, hq, node


def _check_histograms(sa, X, cuts, n, f_num, n_bool, nodes):
    data = sa['boost'].bin_host(X, cuts=cuts)
    B = data.host_bins()
    if f_num:
        np.testing.assert_array_equal(B[0], np.full(n, 7))
        assert f_num == 1 or n < 256 or set(B[1].tolist()) == set(range(256))
    gq, hq, node = _level_rows(n, nodes)
    hist, tot = sa['boost'].histograms(data, _dev(gq), _dev(hq), _dev(node), nodes, return_totals=True)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (nodes, f_num + n_bool, 256, 2)
    want = br.histograms(B, gq, hq, node, nodes)
    np.testing.assert_array_equal(hist.cpu().numpy(), want)
    np.testing.assert_array_equal(tot, want[:, 0].sum(1))
    if nodes > 1:
        assert not want[1].any()
    return data, B, want


@pytest.mark.parametrize('n,f_num,n_bool,nodes', HIST_CASES)
def test_histograms_equal_add_at(sa, n, f_num, n_bool, nodes):
    X, cuts = _hist_table(n, f_num, n_bool, seed=n + nodes)
    _check_histograms(sa, X, cuts, n, f_num, n_bool, nodes)


def bins_launch(f_num, nodes):
    """(fg, groups, gx before the cap at the row steps) of sa_boost_hist_bins on this device, as
    include/socceraction_amd.h states the launch shape."""
    fg = FEATURE_GROUP
    while fg > 1 and fg * nodes > 32:
        fg >>= 1
    groups = (f_num + fg - 1) // fg
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return fg, groups, max(BINS_MIN_GRID_X, BINS_WG_PER_CU * cus // groups)


def _trip_case(nodes, tail):
    """128 numeric columns and a row count at which some workgroups of the bin histogram kernel
    take three row steps (s += gridDim.x), the last step partial."""
    f_num = 128
    fg, groups, gx = bins_launch(f_num, nodes)
    assert (fg, groups) == ((1, 128) if nodes == 32 else (4, 32))
    n = 2 * gx * BINS_TILE + tail
    assert n < 2 ** 30, f'gx = {gx} puts n = {n} past 2^30 rows'
    steps = (n + BINS_TILE - 1) // BINS_TILE
    assert steps > 2 * gx and n % BINS_TILE
    return n, f_num, gx, steps


@pytest.mark.parametrize('nodes,tail', [(32, BINS_TILE + 3), (1, 1027)], ids=['fg=1-gx-at-its-floor', 'fg=4'])
def test_histograms_over_more_row_steps_than_workgroups(sa, nodes, tail):
    n, f_num, gx, steps = _trip_case(nodes, tail)
    print('nodes', nodes, 'gx', gx, 'n', n, 'steps', steps)
    X, cuts = _hist_table(n, f_num, 0, seed=n + nodes)
    _check_histograms(sa, X, cuts, n, f_num, 0, nodes)


def test_sampled_histograms_over_more_row_steps_than_workgroups(sa):
    """sa_boost_hist_bins with a row list at the first shape: a column list of 64 of the 128 matrix rows, out
    of order.  Only those features' histograms are filled, and they are the restatement's."""
    boost, nodes = sa['boost'], 32
    n, f_num, gx, steps = _trip_case(nodes, BINS_TILE + 3)
    X, cuts = _hist_table(n, f_num, 0, seed=n + nodes)
    # a bool feature first: matrix row r holds feature r + 1, so a list entry's two numbers differ
    X = pd.concat([pd.DataFrame({'flag': np.zeros(n, bool)}), X], axis=1)
    cuts = [np.array([0.5], np.float32)] + cuts
    data = boost.bin_host(X, cuts=cuts)
    B = data.host_bins()
    assert data.num_feat.tolist() == list(range(1, f_num + 1)) and len(data.bit_feat) == 1
    gq, hq, node = _level_rows(n, nodes)
    want = br.histograms(B, gq, hq, node, nodes)
    rows = np.random.default_rng(4).permutation(f_num)[:64].astype(np.int32)
    assert (np.diff(rows) < 0).any() and len(set(rows.tolist())) == 64
    feats = data.num_feat[rows]
    fg, groups, gx64 = bins_launch(len(rows), nodes)
    assert steps > gx64  # the sampled launch has fewer groups: its own gx
    nd = torch.from_numpy(node.astype(np.int64)).cuda()
    heap = boost._pad(torch.where(nd == 255, nd, nd + nodes - 1).to(torch.uint8), data.ld, torch.uint8, 255)
    gd, hd = boost._pad(_dev(gq), data.ld, torch.int32), boost._pad(_dev(hq), data.ld, torch.int32)
    hist = torch.zeros((nodes, data.n_features, 256, 2), dtype=torch.int64, device='cuda')
    tree = torch.zeros((4 * nodes, boost.NODE_DTYPE.itemsize), dtype=torch.uint8, device='cuda')
    cols = (None, None, 0, _dev(feats.astype(np.int32)), _dev(rows), len(rows))  # no bool feature sampled
    boost._hist(boost._run, boost._stream(), data, gd, hd, heap, nodes, hist, tree, True, cols=cols)
    got = hist.cpu().numpy()
    np.testing.assert_array_equal(got[:, feats], want[:, feats])
    rest = np.setdiff1d(np.arange(data.n_features), feats)
    assert len(rest) == 65 and not got[:, rest].any() and want[:, rest[1:]].any()
    tab = tree.cpu().numpy().view(boost.NODE_DTYPE).reshape(-1)[nodes - 1:2 * nodes - 1]
    np.testing.assert_array_equal(np.stack([tab['G'], tab['H']], 1), want[:, 1].sum(1))


@pytest.mark.parametrize('n,f_num,n_bool,nodes', [(4101, 1, 300, 32), (4101, 0, 600, 16)])
def test_bitmap_histograms_over_two_column_passes(sa, n, f_num, n_bool, nodes):
    """More bool columns than the LDS sums of one pass hold (c0 += cc): the second pass holds a
    column of ones and a column of zeros, as the first does."""
    cc = BITS_ACC_BYTES // (16 * nodes)
    assert cc < n_bool <= 2 * cc
    X, cuts = _hist_table(n, f_num, n_bool, seed=n + nodes)
    X[f'b{cc}'] = True
    X[f'b{cc + 1}'] = False
    assert X['b0'].all() and not X['b1'].any() and 0 < X[f'b{cc + 2}'].sum() < n
    _, B, want = _check_histograms(sa, X, cuts, n, f_num, n_bool, nodes)
    assert B[f_num + cc].all() and not B[f_num + cc + 1].any()
    assert not want[:, f_num + cc, 0].any() and want[:, f_num + cc, 1].any()


def test_histograms_do_not_wrap_and_cancel_exactly(sa):
    n = 4099
    X = pd.DataFrame({'a': np.full(n, 3.0), 'b': np.ones(n, bool)})
    cuts = [np.arange(1, 255, dtype=np.float32), np.array([0.5], np.float32)]
    data = sa['boost'].bin_host(X, cuts=cuts)
    big = np.full(n, 2 ** 30, np.int32)
    node = np.zeros(n, np.uint8)
    h = sa['boost'].histograms(data, _dev(big), _dev(big), _dev(node), 1).cpu().numpy()
    assert h[0, 0, 3].tolist() == [n * 2 ** 30, n * 2 ** 30] and n * 2 ** 30 > 2 ** 32  # a 32-bit sum would wrap
    assert h[0, 1, 1].tolist() == [n * 2 ** 30, n * 2 ** 30] and h[0, 1, 0].tolist() == [0, 0]
    assert h.sum() == 4 * n * 2 ** 30
    sign = np.resize(np.array([2 ** 30, -2 ** 30, 12345, -12345], np.int32), n - 3)
    sign = np.concatenate([sign, np.zeros(3, np.int32)])
    h = sa['boost'].histograms(data, _dev(sign), _dev(np.abs(sign)), _dev(node), 1).cpu().numpy()
    assert h[0, 0, 3, 0] == 0 and h[0, 1, 1, 0] == 0 and h[0, 1, 0].tolist() == [0, 0]
    assert h[0, 0, 3, 1] == int(np.abs(sign).astype(np.int64).sum())


# ----------------------------------------------------------------------------- splits
S30 = 2 ** 30


def _hist(F, entries):
    """[1, F, 256, 2] from {(feature, bin): (g, h)} in units of 2^-30."""
    h = np.zeros((1, F, 256, 2), np.int64)
    for (f, b), (g, hh) in entries.items():
        h[0, f, b] = (int(g * S30), int(hh * S30))
    return h


def _expected(h, cuts, **kw):
    G, H = int(h[0, 0, :, 0].sum()), int(h[0, 0, :, 1].sum())
    p = {**br.DEFAULTS, **kw}
    rec = np.zeros(3, br.NODE_DTYPE)
    rec[0]['exists'], rec[0]['G'], rec[0]['H'] = 1, G, H
    rec[0]['feature'] = rec[0]['cut'] = -1
    rec[0]['value'] = br.leaf_value(G, H, p['learning_rate'], p['reg_lambda'])
    best = br.best_split(h[0], G, H, cuts, p['reg_lambda'], p['min_child_weight'], p['gamma'])
    if best is not None:
        f, i, gain, gl, hl = best
        rec[0]['feature'], rec[0]['cut'], rec[0]['gain'], rec[0]['thr'] = f, i, gain, cuts[f][i]
        for c, (cg, ch) in ((1, (gl, hl)), (2, (G - gl, H - hl))):
            rec[c]['exists'], rec[c]['G'], rec[c]['H'], rec[c]['feature'] = 1, cg, ch, -1
    return rec, best


c3 = np.array([1.0, 2.0, 3.0], np.float32)
SPLIT_CASES = {
    # two identical columns: the lower index wins
    'identical_columns': (_hist(2, {(0, 0): (-5, 6), (0, 2): (4, 5), (1, 0): (-5, 6), (1, 2): (4, 5)}),
                          [c3, c3], {}, (0, 0)),
    # bin 1 is empty: cuts 0 and 1 have the same sums and the same gain, the lower cut wins
    'equal_gains_two_cuts': (_hist(1, {(0, 0): (-5, 6), (0, 2): (4, 5)}), [c3], {}, (0, 0)),
    # the better feature is the later one
    'later_feature_better': (_hist(2, {(0, 0): (-1, 6), (0, 2): (0, 5), (1, 0): (-5, 6), (1, 3): (4, 5)}),
                             [c3, c3], {}, (1, 0)),
    # a constant feature (no cuts) does not split
    'constant_feature': (_hist(1, {(0, 0): (-1, 11)}), [np.zeros(0, np.float32)], {}, None),
    # the only gainful cut leaves a child below min_child_weight
    'min_child_weight': (_hist(1, {(0, 0): (-5, 0.5), (0, 1): (4, 10.5)}), [c3[:1]], {}, None),
    'min_child_weight_met': (_hist(1, {(0, 0): (-5, 0.5), (0, 1): (4, 10.5)}), [c3[:1]],
                             dict(min_child_weight=0.5), (0, 0)),
    # gamma above the best gain: a leaf
    'gamma': (_hist(1, {(0, 0): (-5, 6), (0, 2): (4, 5)}), [c3], dict(gamma=100.0), None),
    # the right child holds missing values only
    'missing_only_right': (_hist(1, {(0, 0): (-5, 6), (0, 255): (4, 5)}), [c3[:1]], {}, (0, 0)),
    # every bin used, 254 cuts
    'all_bins': (np.stack([np.arange(-128, 128) * 1000003, np.arange(1, 257) * S30 // 16], 1)
                 .reshape(1, 1, 256, 2).astype(np.int64), [np.arange(1, 255, dtype=np.float32)], {}, 'any'),
}


@pytest.mark.parametrize('case', sorted(SPLIT_CASES))
def test_splits_equal_the_restatement(sa, case):
    h, cuts, kw, want = SPLIT_CASES[case]
    G, H = int(h[0, 0, :, 0].sum()), int(h[0, 0, :, 1].sum())
    # every feature's histogram sums to the node totals
    assert all(int(h[0, f, :, 0].sum()) == G and int(h[0, f, :, 1].sum()) == H for f in range(h.shape[1]))
    rec, best = _expected(h, cuts, **kw)
    if want != 'any':
        assert (None if best is None else best[:2]) == want
    got = sa['boost'].best_splits(_dev(h), [[G, H]], cuts, **kw)
    print(case, got, rec)
    for field in ('feature', 'cut', 'exists', 'G', 'H'):
        np.testing.assert_array_equal(got[field], rec[field], field)
    for field, bits in (('gain', np.uint64), ('value', np.uint32), ('thr', np.uint32)):
        np.testing.assert_array_equal(got[field].view(bits), rec[field].view(bits), field)
    assert got.tobytes() == rec.tobytes()


def test_splits_of_a_whole_level(sa):
    """Four nodes of one level (one of them absent from the data) against the restatement."""
    rng = np.random.default_rng(5)
    F, nodes = 6, 4
    cuts = [np.arange(1, 1 + m, dtype=np.float32) for m in (254, 3, 0, 1, 17, 254)]
    h = np.zeros((nodes, F, 256, 2), np.int64)
    tot = np.zeros((nodes, 2), np.int64)
    for k in (0, 2, 3):
        rows = 300
        g = rng.integers(-2 ** 29, 2 ** 29, rows)
        hh = rng.integers(1, 2 ** 28, rows)
        for f in range(F):
            b = rng.integers(0, len(cuts[f]) + 1, rows)
            b[rng.random(rows) < 0.05] = 255
            np.add.at(h[k, f, :, 0], b, g)
            np.add.at(h[k, f, :, 1], b, hh)
        tot[k] = (g.sum(), hh.sum())
    got = sa['boost'].best_splits(_dev(h), tot, cuts)
    for k in range(nodes):
        best = br.best_split(h[k], int(tot[k, 0]), int(tot[k, 1]), cuts)
        assert got['value'][k] == br.leaf_value(int(tot[k, 0]), int(tot[k, 1]))
        if best is None:
            assert got['feature'][k] == -1
            continue
        f, i, gain, gl, hl = best
        assert (got['feature'][k], got['cut'][k]) == (f, i)
        assert np.float64(got['gain'][k]).view(np.uint64) == np.float64(gain).view(np.uint64)
        kids = got[nodes + 2 * k: nodes + 2 * k + 2]
        assert kids['G'].tolist() == [gl, int(tot[k, 0]) - gl] and kids['H'].tolist() == [hl, int(tot[k, 1]) - hl]
    assert got['feature'][0] >= 0 and got['feature'][1] == -1


# ----------------------------------------------------------------------------- whole fits
FITS = {'d3': dict(n_estimators=12, max_depth=3), 'd1': dict(n_estimators=3, max_depth=1),
        'd6': dict(n_estimators=3, max_depth=6)}


@pytest.fixture(scope='module')
def fits(sa, game):
    return {k: sa['boost'].DeviceGBTClassifier(record=True, **p).fit_blocks(game['fb'], game['yd'])
            for k, p in FITS.items()}


def _replay(clf, params, B, y, cuts):
    """A recorded fit against the restatement, round by round: the restated tree is built from
    the device's p_t; node tables and margins are compared as bytes.  Returns the split nodes."""
    P = clf.record_['p'].cpu().numpy()
    M = clf.record_['margin'].cpu().numpy()
    assert clf.trees_.shape == (params['n_estimators'], 2 ** (params['max_depth'] + 1) - 1)
    for a, b in zip(clf.cuts_, cuts):
        np.testing.assert_array_equal(a, b)
    m = np.full(len(y), br.base_margin(0.5), np.float32)
    split_nodes = 0
    for t in range(params['n_estimators']):
        np.testing.assert_allclose(P[t], br.probability(m), rtol=1e-6, atol=0)
        gq, hq = br.quantise(P[t], y)       # the restated tree from the device's p_t
        tab, node = br.build_tree(B, gq, hq, cuts, params)
        assert tab.tobytes() == clf.trees_[t].tobytes(), (t, tab, clf.trees_[t])
        m = br.update_margin(m, tab, node)
        assert m.tobytes() == M[t].tobytes(), t
        split_nodes += int((tab['feature'] >= 0).sum())
    assert m.tobytes() == clf.margin_.cpu().numpy().tobytes()
    return split_nodes


@pytest.mark.parametrize('which', sorted(FITS))
def test_whole_fit_replayed_round_by_round(sa, game, fits, which):
    clf, params = fits[which], FITS[which]
    split_nodes = _replay(clf, params, game['B'], game['y'], game['cuts'])
    assert split_nodes >= params['n_estimators']  # every round found a split
    if which == 'd6':
        assert (clf.trees_['exists'][:, 63:] != 0).any()  # the deepest level is reached


WIDE_ROWS, WIDE_NUM, WIDE_BOOL, WIDE_VALUES = 40000, 128, 260, 64
WIDE_FIT = dict(n_estimators=2, max_depth=6)
_WIDE = {}


def wide_table():
    """A host table whose fit takes many workgroups at every level: 40,000 rows (twenty bitmap
    tiles, forty bin steps), 128 numeric columns of 64 distinct values (about 3% NaN) and 260 bool
    columns (two bitmap passes at 32 nodes); the labels depend on numeric column 3 and on bool
    columns 256..259, the columns of the second pass, weakly enough for the trees to split on
    them down to level 5.  The cuts are fixed: column j's values are
    k / 4 - j, k < 64, so its cuts are those of k = 1..63 and a value's bin is its k.  Built once."""
    if not _WIDE:
        n = WIDE_ROWS
        rng = np.random.default_rng(40)
        cols, cuts, B = {}, [], np.empty((WIDE_NUM + WIDE_BOOL, n), np.uint8)
        for j in range(WIDE_NUM):
            k = rng.integers(0, WIDE_VALUES, n)
            v = k * 0.25 - j
            nan = rng.random(n) < 0.03
            v[nan] = np.nan
            cols[f'n{j}'] = v
            cuts.append((np.arange(1, WIDE_VALUES) * 0.25 - j).astype(np.float32))
            B[j] = np.where(nan, 255, k)
        for j in range(WIDE_BOOL):
            b = rng.random(n) < (0.5 if j % 7 == 2 else 0.1)
            cols[f'b{j}'] = b
            cuts.append(np.array([0.5], np.float32))
            B[WIDE_NUM + j] = b
        k3 = np.where(B[3] == 255, 32, B[3]).astype(np.float64)
        late = B[WIDE_NUM + 256:].astype(np.float64)  # the four bool columns of the second pass
        z = -1.5 + 0.05 * (k3 - 32) + 0.6 * late[0] + 0.8 * late[1] + 0.6 * late[2] + 0.6 * late[3]
        rng = np.random.default_rng(41)
        y = (rng.random(n) < 1 / (1 + np.exp(-(z + 0.5 * rng.standard_normal(n))))).astype(np.uint8)
        _WIDE.update(X=pd.DataFrame(cols), y=y, cuts=cuts, B=B)
    return _WIDE


def test_whole_fit_over_many_workgroups(sa):
    """Every level's histograms come from more than one row step per workgroup and twenty bitmap
    tiles; level 5 takes two bitmap passes; twenty workgroups add the node totals."""
    t = wide_table()
    X, y, cuts, B = t['X'], t['y'], t['cuts'], t['B']
    n = len(y)
    for nodes in (1, 32):
        fg, groups, gx = bins_launch(WIDE_NUM, nodes)
        assert (n + BINS_TILE - 1) // BINS_TILE > gx, (nodes, gx)
    assert WIDE_BOOL > BITS_ACC_BYTES // (16 * 32) and (n + BITS_TILE - 1) // BITS_TILE == 20
    np.testing.assert_array_equal(sa['boost'].bin_host(X, cuts=cuts).host_bins(), B)
    clf = sa['boost'].DeviceGBTClassifier(record=True, **WIDE_FIT).fit(X, y, cuts=cuts)
    _replay(clf, WIDE_FIT, B, y, cuts)
    splits = (clf.trees_['feature'] >= 0) & (clf.trees_['exists'] != 0)
    assert splits[:, 0].all()  # both rounds split
    assert splits[:, 31:63].any(axis=1).all()  # ... down to level 5, whose histograms decide splits
    assert (clf.trees_['exists'][:, 63:] != 0).any(axis=1).all()
    # level 5 splits on a bool column its second bitmap pass summed, in both rounds
    second_pass = splits & (clf.trees_['feature'] >= WIDE_NUM + BITS_ACC_BYTES // (16 * 32))
    assert second_pass[:, 31:63].any(axis=1).all()


def test_export_closes_the_loop(sa, game, fits):
    from oracle import tree_oracle as to
    clf, fb = fits['d3'], game['fb']
    te = sa['trees'].TreeEnsemble.from_model(clf)
    assert te is not None and te.n_trees == 12 and te.feature_names == fb.plan.names
    p = clf.p_.cpu().numpy()
    for method in ('staged', 'gather'):
        got = te.predict_blocks(fb, method=method).cpu().numpy()
        assert got.tobytes() == p.tobytes(), method
    pair = sa['trees'].predict_pair_conditions(game['ab'], fb.plan, [te, te])
    assert pair[0].cpu().numpy().tobytes() == p.tobytes() and pair[1].cpu().numpy().tobytes() == p.tobytes()
    model = clf.to_xgboost_json()
    assert model['learner']['feature_names'] == fb.plan.names
    np.testing.assert_allclose(p, to.predict_xgboost_json(model, game['X']), rtol=1e-6, atol=0)
    host = clf.predict_proba(pd.DataFrame({n: c for n, c in zip(fb.plan.names, game['cols'])}))
    assert host.shape == (fb.n, 2) and host[:, 1].tobytes() == p.tobytes()
    d6 = sa['trees'].TreeEnsemble.from_model(fits['d6'])
    assert d6.predict_blocks(fb, method='gather').cpu().numpy().tobytes() == fits['d6'].p_.cpu().numpy().tobytes()


def test_fits_are_reproducible(sa, game):
    fb, boost = game['fb'], sa['boost']
    params = dict(n_estimators=6, max_depth=3)
    first = json.dumps(boost.DeviceGBTClassifier(**params).fit_blocks(fb, game['yd']).to_xgboost_json())
    again = json.dumps(boost.DeviceGBTClassifier(**params).fit_blocks(fb, game['yd']).to_xgboost_json())
    assert first == again
    # with the cuts fixed a row permutation (labels alike) gives the same model
    X = pd.DataFrame({n: c for n, c in zip(fb.plan.names, game['cols'])})
    host = json.dumps(boost.DeviceGBTClassifier(**params).fit(X, game['y'], cuts=game['cuts']).to_xgboost_json())
    assert host == first
    perm = np.random.default_rng(0).permutation(len(X))
    shuffled = boost.DeviceGBTClassifier(**params).fit(X.iloc[perm].reset_index(drop=True), game['y'][perm],
                                                       cuts=game['cuts'])
    assert json.dumps(shuffled.to_xgboost_json()) == first
    # a held-out row takes no part: fitting rows [0, 1000) of the table == fitting that table alone
    rows = np.arange(1000)
    part = boost.DeviceGBTClassifier(**params).fit_blocks(fb, game['yd'], rows=rows, cuts=game['cuts'])
    alone = boost.DeviceGBTClassifier(**params).fit(X.iloc[:1000], game['y'][:1000], cuts=game['cuts'])
    assert json.dumps(part.to_xgboost_json()) == json.dumps(alone.to_xgboost_json())


def _two_games():
    gs = [load('spadl', 'full0'), load('spadl', 'full1')]
    actions = pd.concat([frame(g) for g in gs], ignore_index=True)
    games = pd.DataFrame({'game_id': [int(frame(g).game_id.iloc[0]) for g in gs],
                          'home_team_id': [int(g['home_team_id'][0]) for g in gs]})
    return games, actions


def test_fit_from_the_host_frame_equals_fit_batch(sa):
    import socceraction_amd.vaep as vaep
    games, actions = _two_games()
    params = dict(n_estimators=5)
    a = vaep.VAEP().fit_batch(games, actions, tree_params=params)
    b = vaep.VAEP()
    X = b.compute_features_batch(games, actions)
    Y = b.compute_labels_batch(games, actions)
    b.fit(X, Y, learner='device', val_size=0, tree_params=params)
    for col in ('scores', 'concedes'):
        ja = json.dumps(a._VAEP__models[col].to_xgboost_json())
        assert ja == json.dumps(b._VAEP__models[col].to_xgboost_json()), col
        assert len(a._VAEP__models[col].trees_) == 5
    # the reference's split: held-out rows are scored once after training
    c = vaep.VAEP().fit(X, Y, learner='device', val_size=0.25, tree_params=params)
    assert set(c.device_eval_) == {'scores', 'concedes'}
    assert c.device_eval_['scores']['n'] == len(X) - int(np.floor(len(X) * 0.75)) - 1
    d = vaep.VAEP().fit_batch(games, actions, val_size=0.25, tree_params=params)
    assert 0 < d.device_eval_['concedes']['log_loss'] < 1


@pytest.mark.parametrize('atomic', [False, True])
def test_public_path_fit_batch_then_rate_and_score(sa, atomic):
    if atomic:
        from socceraction_amd.atomic.vaep import AtomicVAEP as Model
        g = load('atomic', 'full0')
        actions = frame(g, atomic=True)
        games = pd.DataFrame({'game_id': [int(actions.game_id.iloc[0])], 'home_team_id': [int(g['home_team_id'][0])]})
    else:
        from socceraction_amd.vaep import VAEP as Model
        games, actions = _two_games()
    model = Model().fit_batch(games, actions)
    trees = model._device_models()
    assert trees is not None and all(t.n_trees == 100 and t.f32 for t in trees.values())
    for _, game in games.iterrows():
        ga = actions[actions.game_id == game.game_id].reset_index(drop=True)
        got = model.rate(game, ga)
        host = model.rate(game, ga, game_states=model.compute_features(game, ga))  # predict_proba -> formula.value
        for c in ('offensive_value', 'defensive_value', 'vaep_value'):
            assert_close(got[c].to_numpy(), host[c].to_numpy(), c)
    table = model.rate_players(games, actions, by='team_id')  # the rating table of the same trained learners
    assert int(table['count'].sum()) == len(actions) and np.isfinite(table['vaep_value']).all()
    scores = model.score_batch(games, actions)
    for col in ('scores', 'concedes'):
        print(col, scores[col])
        assert scores[col]['log_loss'] < scores[col]['log_loss_baseline']
