"""Every tree-inference path against the oracle, at split boundaries.

The five implementations of the learners' split rule -- the leaf-checked and the fixed-depth
gather walks, the staged condition walk over feature blocks (float64 / float32 blocks, bool block
or bitmaps), the staged walk over condition bitmaps only, and the COND mode of the numeric feature
pass that writes those bitmaps -- are each compared with oracle/tree_oracle.py (never with one
another) on models whose thresholds sit ON the batch (tests/tree_boundary_models.py): thresholds
equal to float32(x) of rows, their float32 / float64 neighbours, +-0.0, integers of the integer
columns and +-0.5, constant and real bool splits, NaN coordinates routed both ways, trees of
depths 1..5 in one group of 8, 0 / 1 / 7 / 8 / 9 / 37 trees.

Bars: float32 probabilities rtol 1e-6 (expf against numpy.exp, the suite's bar), float64 rtol
1e-12.  Margins are multiples of 2^-6 within +-4, so one wrong branch moves a probability by at
least 2.8e-4 relative.  The features are the device's own (X is read back from the plain
float64 / int64 / bool blocks, as tests/test_gpu_trees.py::_game does): this module pins the
trees, tests/test_gpu_parity.py pins the features.
"""
import numpy as np
import pytest

import tree_boundary_models as bm
from oracle import tree_oracle as to
from oracle import vaep_oracle as vo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ATOMIC_XFNS = ['actiontype', 'actiontype_onehot', 'bodypart', 'bodypart_onehot', 'time', 'team',
               'time_delta', 'location', 'polar', 'movement_polar', 'direction', 'goalscore']
CONFIGS = {'spadl_k1': (False, 1, vo.SPADL_DEFAULT), 'spadl_k2': (False, 2, vo.SPADL_DEFAULT),
           'spadl_k3': (False, 3, vo.SPADL_DEFAULT), 'atomic_k3': (True, 3, ATOMIC_XFNS),
           'spadl_numeric_k3': (False, 3, ['time', 'startlocation', 'goalscore'])}
MAIN = ['spadl_k1', 'spadl_k2', 'spadl_k3', 'atomic_k3']
N_TREES = [0, 1, 7, 8, 9, 37]
N_EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025]
TS_CSTRIDE = 68          # bytes per staged condition (sa_trees.hip)
LDS_LIMIT = 160 * 1024
KIND_CODE = {'b': 0, 'f': 1, 'i': 2}


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, batch, ops, trees
    _native.load_library()
    return dict(batch=batch, ops=ops, trees=trees, native=_native)


_COLUMNS, _CTX = {}, {}


def _columns(atomic):
    """4-5 games, ~8k rows, NaN in start_x / end_y (atomic: x / dy) of a segment's first and last
    row, of the batch's first rows, and of rows next to 128-row wave and 512-row tile boundaries
    (their k - 1 successors' windows then reach back across the boundary)."""
    if atomic not in _COLUMNS:
        from socceraction_amd import synthetic
        d = synthetic.atomic_games(4, seed=5, mean_actions=2000.0) if atomic else synthetic.spadl_games(5, seed=5)
        off = d['game_off']
        n = int(off[-1])
        assert 6000 <= n <= 10000 and len(off) - 1 in (4, 5, 6)
        rows = sorted({0, 1, int(off[1]), int(off[2]) - 1, 126, 127, 128, 1023, 1024, 1025, n - 1})
        for c in (('x', 'dy') if atomic else ('start_x', 'end_y')):
            d[c] = d[c].copy()
            d[c][rows] = np.nan
        _COLUMNS[atomic] = d
    return _COLUMNS[atomic]


def _cut(d, n):
    """The batch's first n rows: segments end at the cut."""
    off = d['game_off']
    g = int(np.searchsorted(off, n, 'left'))  # segments that start before row n
    out = {c: (v[:n] if c not in ('game_off', 'home_team_id') else v) for c, v in d.items()}
    out['game_off'] = np.append(off[:g], n).astype(np.int64)
    out['home_team_id'] = d['home_team_id'][:g]
    return out


def _host_matrix(fb):
    b, f, i = fb.to_numpy()
    blocks = {'b': b, 'f': f, 'i': i}
    X = np.stack([blocks[k][c, :fb.n].astype(np.float64) for _, k, c in fb.plan.order], axis=1)
    X.setflags(write=False)
    return X


def _ctx(sa, name):
    """The batch of a configuration, its feature blocks in every layout, and the host feature
    matrix X (columns in plan order) -- built once and shared, X read-only."""
    if name not in _CTX:
        atomic, k, xfns = CONFIGS[name]
        B, ops = sa['batch'], sa['ops']
        d = _columns(atomic)
        ab = B.ActionBatch.from_columns(d, atomic=atomic)
        plain = ops.features(ab, xfns, k)
        X = _host_matrix(plain)
        assert np.isnan(X).any()
        blocks = {'plain': plain, 'tiled': ops.features(ab, xfns, k, bool_tile=1024, num_tile=128)}
        if plain.plan.n_bool:
            blocks['bits'] = ops.features(ab, xfns, k, num_tile=128, bool_bits=True)
            blocks['bits32'] = ops.features(ab, xfns, k, num_tile=128, bool_bits=True, num32=True)
        plan = plain.plan
        _CTX[name] = dict(name=name, atomic=atomic, k=k, xfns=xfns, d=d, ab=ab, X=X, plan=plan,
                          kinds=[q for _, q, _ in plan.order], blocks=blocks, models={},
                          col_of={(KIND_CODE[q], c): j for j, (_, q, c) in enumerate(plan.order)})
    return _CTX[name]


def _learner(sa, ctx, model, key=None):
    """A boundary model with its device ensembles and the oracle's probabilities on X."""
    if key is not None and key in ctx['models']:
        return ctx['models'][key]
    X = ctx['X']
    ref32 = to.predict_xgboost_json(model.json, X)
    # the explicit-array oracle reproduces the JSON one on the same trees
    np.testing.assert_array_equal(to.predict_flat(model.flat_lt, 0.0, X, True, np.float32), ref32)
    out = dict(model=model, te=sa['trees'].TreeEnsemble.from_model(model.json), ref32=ref32)
    assert out['te'] is not None and out['te'].n_trees == model.n_trees
    if key is not None:
        ctx['models'][key] = out
    return out


def _boundary(sa, ctx, n_trees):
    key = ('boundary', n_trees)
    if key not in ctx['models']:
        _learner(sa, ctx, bm.boundary_model(ctx['X'], ctx['kinds'], n_trees, seed=100 + n_trees), key)
    return ctx['models'][key]


def _coverage(ctx, L, le=False):
    key = 'cov_le' if le else 'cov_lt'
    if key not in L:
        m = L['model']
        L[key] = bm.coverage(m.flat_le if le else m.flat_lt, ctx['X'], ctx['kinds'], not le,
                             np.float64 if le else np.float32)
    return L[key]


def _assert_close(got, ref, rtol, what):
    got = got.cpu().numpy()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    bad = ~(np.abs(got - ref) <= rtol * np.abs(ref))
    if bad.any():
        r = int(np.flatnonzero(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {len(ref)} rows differ from the oracle; first row {r}: '
                             f'got {got[r]!r}, oracle {ref[r]!r}')


def _assert_floor(cov, what):
    """The coverage floor: a condition on the inputs, from the oracle alone."""
    assert cov['num_tie_fraction'] >= 0.01, (what, cov)
    assert cov['disagree_splits'] >= 1, (what, cov)
    assert cov['nan_left'] >= 1 and cov['nan_right'] >= 1, (what, cov)


# ------------------------------------------------------------------------------ block paths
@pytest.mark.parametrize('n_trees', N_TREES)
@pytest.mark.parametrize('config', MAIN)
def test_block_paths_match_oracle(sa, config, n_trees):
    """predict_blocks on every layout and method == the oracle: the fixed-depth and the
    leaf-checked gather walk; the staged walk over the tiled and the plain blocks, over bool
    bitmaps, over bitmaps + float32 numeric blocks; the default method; and the same trees as a
    float64 `x <= thr` model (thresholds: the float64 values and their neighbours) through the
    gather and the staged walks.  The batch meets the coverage floor for both rules (>= 7 trees:
    the first seven roots carry it)."""
    ctx = _ctx(sa, config)
    trees, X, blocks = sa['trees'], ctx['X'], ctx['blocks']
    L = _boundary(sa, ctx, n_trees)
    model, te = L['model'], L['te']
    if 'ref64' not in L:
        L['ref64'] = to.predict_flat(model.flat_le, model.base_le, X, False, np.float64)
    _coverage(ctx, L), _coverage(ctx, L, le=True)
    if n_trees >= 7:
        _assert_floor(L['cov_lt'], 'float32 `<` model')
        _assert_floor(L['cov_le'], 'float64 `<=` model')
        for cov in (L['cov_lt'], L['cov_le']):
            assert cov['const_left'] >= 1 and cov['const_right'] >= 1 and cov['f_tie_visits'] >= 1, cov
        assert sorted(set(te.depths().tolist())) == [1, 2, 3, 4, 5]
    if n_trees:
        assert L['cov_lt']['disagree_splits'] >= 1  # the first root: float32(x_r) > x_r
    le = bm.ensemble_le(trees, model)
    for tag, ens, ref, rtol in (('xgboost', te, L['ref32'], 1e-6), ('sklearn-rule', le, L['ref64'], 1e-12)):
        _assert_close(ens.predict_blocks(blocks['tiled'], method='gather'), ref, rtol, f'{tag} gather fixed-depth')
        _assert_close(ens.predict_blocks(blocks['plain'], method='gather'), ref, rtol, f'{tag} gather plain')
        _assert_close(ens.predict_blocks(blocks['tiled']), ref, rtol, f'{tag} default method')
        if n_trees:  # (a model without trees has no staged form: predict_blocks takes the gather walk)
            layouts = ['tiled', 'plain', 'bits'] + (['bits32'] if ens.f32 and ctx['k'] <= 3 else [])
            for lay in layouts:
                _assert_close(ens.predict_blocks(blocks[lay], method='staged'), ref, rtol, f'{tag} staged {lay}')
        # the leaf-checked walk: no per-tree depths
        ens._device(blocks['tiled'].device)['depth'] = None
        _assert_close(ens.predict_blocks(blocks['tiled'], method='gather'), ref, rtol, f'{tag} gather leaf-checked')
        ens._dev = None
    assert blocks['bits'].bool_block is None  # the bitmap form was read as bitmaps


# ------------------------------------------------------------------------------ condition path
def _unpack(bits):
    return np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder='little')


def _check_condition_bitmaps(sa, ctx, ab, X, learners):
    """trees.condition_bitmaps, written into a buffer preset to all ones, read back: row nb + c ==
    the oracle's condition_bits of the union's condition c, the bool rows == the bool features,
    every bit at a row >= n clear."""
    trees, plan = sa['trees'], ctx['plan']
    tes = [L['te'] for L in learners]
    lay = trees.staged_layout(tes, [te.feature_slots(plan) for te in tes])
    n, nb, n_num = ab.n, plan.n_bool, len(lay['num_slots'])
    words = max(2, -(-n // 128) * 2)
    pre = torch.full((max(nb + n_num, 1), words), -1, dtype=torch.int64, device=ab.device)
    prep, bits, words2 = trees.condition_bitmaps(ab, plan, tes, bits=pre)
    assert prep['n_num'] == n_num and words2 == words
    got = _unpack(bits)[:nb + n_num]
    names = plan.names
    for c in range(nb):
        j = ctx['col_of'][(0, c)]
        bad = got[c, :n] != (X[:n, j] != 0)
        assert not bad.any(), f'bool row {c} ({names[j]}): first wrong row {int(np.flatnonzero(bad)[0])}'
    for c in range(n_num):
        slot = int(lay['num_slots'][c])
        j = ctx['col_of'][(slot >> 24, slot & 0xFFFFFF)]
        thr, dl = lay['num_thr'][c], bool(lay['num_dl'][c])
        want = to.condition_bits(X[:n], j, thr, dl, True, np.float32)
        bad = got[nb + c, :n] != want
        if bad.any():
            r = int(np.flatnonzero(bad)[0])
            raise AssertionError(f'condition {c} of {n_num} (column {names[j]}, float32(x) < {thr!r}, NaN goes '
                                 f'{"left" if dl else "right"}): first wrong row {r} of {n} (x = {X[r, j]!r}): bit '
                                 f'{int(got[nb + c, r])}, oracle {int(want[r])}; {int(bad.sum())} rows wrong')
    tail = got[:, n:]
    if tail.any():
        r, q = np.argwhere(tail)[0]
        raise AssertionError(f'bitmap row {int(r)} ({"bool" if r < nb else "condition"}): bit of row {n + int(q)} >= n = {n} is set')
    return prep


def _check_pair(sa, ctx, ab, learners, what):
    got = sa['trees'].predict_pair_conditions(ab, ctx['plan'], [L['te'] for L in learners])
    for q, (L, g) in enumerate(zip(learners, got)):
        _assert_close(g, L['ref32'][:ab.n], 1e-6, f'{what}: learner {q} of {len(learners)} (conditions)')


@pytest.mark.parametrize('config', MAIN)
def test_pair_conditions_match_oracle(sa, config):
    """trees.predict_pair_conditions (VAEP.rate's default path: the COND feature pass, then each
    learner's staged walk over bitmaps only) with two and with three learners == the oracle, and
    the COND pass's bitmaps themselves == the oracle's condition bits.  A learner without trees
    has no staged walk: ValueError (VAEP.rate then takes predict_blocks)."""
    ctx = _ctx(sa, config)
    L = {t: _boundary(sa, ctx, t) for t in N_TREES}
    _assert_floor(_coverage(ctx, L[37]), 'float32 `<` model')
    _check_pair(sa, ctx, ctx['ab'], [L[37], L[9]], 'two learners')
    _check_pair(sa, ctx, ctx['ab'], [L[1], L[7], L[8]], 'three learners')
    _check_condition_bitmaps(sa, ctx, ctx['ab'], ctx['X'], [L[37], L[9], L[8]])
    with pytest.raises(ValueError):
        sa['trees'].predict_pair_conditions(ctx['ab'], ctx['plan'], [L[9]['te'], L[0]['te']])


@pytest.mark.parametrize('n', N_EDGES)
@pytest.mark.parametrize('config', ['spadl_k3', 'atomic_k3'])
def test_batch_length_edges(sa, config, n):
    """The batch cut to n rows (segments end at the cut) around the 64 / 128-row wave and 512-row
    tile sizes, n odd and n = 1, 2: the COND pass (lanes past the end recompute the last pair, bits
    masked), its bitmaps, and the staged walks over bitmaps == the oracle on the same rows."""
    ctx = _ctx(sa, config)
    B, ops = sa['batch'], sa['ops']
    learners = [_boundary(sa, ctx, 9), _boundary(sa, ctx, 8)]
    ab = B.ActionBatch.from_columns(_cut(ctx['d'], n), atomic=ctx['atomic'])
    assert ab.n == n
    X = ctx['X'][:n]  # every feature looks backwards only: the full batch's first n rows
    _check_pair(sa, ctx, ab, learners, f'n = {n}')
    _check_condition_bitmaps(sa, ctx, ab, X, learners)
    for num32 in (False, True):
        fb = ops.features(ab, ctx['xfns'], ctx['k'], num_tile=128, bool_bits=True, num32=num32)
        for L in learners:
            _assert_close(L['te'].predict_blocks(fb, method='staged'), L['ref32'][:n], 1e-6,
                          f'n = {n}: staged walk over bitmaps' + (' + float32 blocks' if num32 else ''))
            L['te']._dev = None


# ------------------------------------------------------------------------------ structural cases
def _f_cols(ctx):
    """Feature indices of the float64 / int64 columns in block-column order."""
    order = ctx['plan'].order
    f = sorted((c, j) for j, (_, q, c) in enumerate(order) if q == 'f')
    i = sorted((c, j) for j, (_, q, c) in enumerate(order) if q == 'i')
    return [j for _, j in f], [j for _, j in i]


def _spread_f_splits(ctx, count, seed):
    """``count`` float64-column splits spread over every float64 column."""
    fcols, _ = _f_cols(ctx)
    out = []
    for q, j in enumerate(fcols):
        cnt = count // len(fcols) + (q < count % len(fcols))
        out += bm.f_splits(ctx['X'], j, cnt, seed)
    return out


def _slot_of(L, plan, j):
    """The (kind << 24) | column slot of model feature j."""
    return int(L['te'].feature_slots(plan)[j])


def _staged_size(sa, ctx, te):
    lay = sa['trees'].staged_layout([te], [te.feature_slots(ctx['plan'])])
    n_cond = 1 + len(lay['bool_cols']) + len(lay['num_slots'])
    n_nodes = len(lay['models'][0]['nodes'])
    return n_cond, n_nodes, sa['native'].lib().sa_tree_staged_lds_bytes(n_nodes, n_cond, 1)


@pytest.mark.parametrize('case', ['chunk70', 'union64', 'union65', 'union128', 'no_numeric'])
def test_condition_chunks(sa, case):
    """The COND pass keeps a wave's outcomes of 64 conditions at a time (CondAcc): one float64
    column with 70 thresholds (its conditions cross a chunk); unions of exactly 64, 65 and 128
    numeric conditions, carried by the first and the last float64 column and an int64 column only
    (condition-free columns between them); a model with no numeric split at all."""
    ctx = _ctx(sa, 'spadl_k3')
    X, kinds, plan = ctx['X'], ctx['kinds'], ctx['plan']
    fcols, icols = _f_cols(ctx)
    F = X.shape[1]
    if case == 'chunk70':
        j = fcols[len(fcols) // 2]
        mid = bm.f_splits(X, j, 70, 1)  # 70 distinct thresholds on one column, from both learners
        a = bm.f_splits(X, fcols[0], 30, 1) + mid[:40] + bm.b_splits(kinds, 6, 1)
        b = mid[40:] + bm.f_splits(X, fcols[-1], 9, 2) + bm.b_splits(kinds, 6, 2)
        models = [bm.model_from_splits(bm.shuffled(s, 3), F, 3) for s in (a, b)]
    elif case == 'no_numeric':
        models = [bm.model_from_splits(bm.b_splits(kinds, 40, sd), F, sd) for sd in (4, 5)]
    else:
        total = int(case[5:])
        ni = 6
        nf0 = (total - ni) // 2
        s = bm.f_splits(X, fcols[0], nf0, 6) + bm.f_splits(X, fcols[-1], total - ni - nf0, 6) + \
            bm.i_splits(X, icols[len(icols) // 2], ni, 6)
        s = bm.shuffled(s, 7)
        half = len(s) // 2
        # the two learners share a few conditions: the union still counts each once
        models = [bm.model_from_splits(s[:half + 3] + bm.b_splits(kinds, 5, 8), F, 8),
                  bm.model_from_splits(s[half:] + bm.b_splits(kinds, 5, 9), F, 9)]
    learners = [_learner(sa, ctx, m) for m in models]
    prep = _check_condition_bitmaps(sa, ctx, ctx['ab'], X, learners)
    lay = sa['trees'].staged_layout([L['te'] for L in learners], [L['te'].feature_slots(plan) for L in learners])
    if case == 'chunk70':
        own = np.flatnonzero(lay['num_slots'] == _slot_of(learners[0], plan, j))  # the column's conditions
        assert len(own) == 70 and own[-1] - own[0] == 69
        assert own[0] // 64 != own[-1] // 64  # they cross a 64-condition chunk boundary
    elif case == 'no_numeric':
        assert prep['n_num'] == 0
    else:
        assert prep['n_num'] == int(case[5:])
        used = sorted({ctx['col_of'][(int(s) >> 24, int(s) & 0xFFFFFF)] for s in lay['num_slots']})
        assert used == sorted([fcols[0], fcols[-1], icols[len(icols) // 2]])  # nothing between them
    _check_pair(sa, ctx, ctx['ab'], learners, case)
    for L in learners:
        _assert_close(L['te'].predict_blocks(ctx['blocks']['bits'], method='staged'), L['ref32'], 1e-6,
                      f'{case}: staged walk over blocks')


def test_no_bool_split_on_numeric_plan(sa):
    """A plan with no bool column (the condition rows start at bitmap row 0) and learners with no
    bool split."""
    ctx = _ctx(sa, 'spadl_numeric_k3')
    assert ctx['plan'].n_bool == 0 and 'b' not in ctx['kinds']
    learners = [_learner(sa, ctx, bm.boundary_model(ctx['X'], ctx['kinds'], t, seed=200 + t)) for t in (37, 9)]
    _assert_floor(_coverage(ctx, learners[0]), 'numeric plan')
    _check_condition_bitmaps(sa, ctx, ctx['ab'], ctx['X'], learners)
    _check_pair(sa, ctx, ctx['ab'], learners, 'numeric-only plan')
    for L in learners:
        for lay in ('tiled', 'plain'):
            _assert_close(L['te'].predict_blocks(ctx['blocks'][lay], method='staged'), L['ref32'], 1e-6,
                          f'numeric-only plan: staged {lay}')
        _assert_close(L['te'].predict_blocks(ctx['blocks']['tiled'], method='gather'), L['ref32'], 1e-6,
                      'numeric-only plan: gather')


def test_unscaled_staged_walk(sa):
    """More than 963 conditions: the staged nodes keep condition indices, not byte offsets
    (`scaled == false` in tree_cond_kernel: n_cond * TS_CSTRIDE > 0x10000), and the model still
    fits LDS.  Over blocks (float64, bitmaps, float32) and over condition bitmaps."""
    ctx = _ctx(sa, 'spadl_k3')
    X, kinds = ctx['X'], ctx['kinds']
    _, icols = _f_cols(ctx)
    s = _spread_f_splits(ctx, 1000, 11) + bm.i_splits(X, icols[-1], 8, 11) + bm.b_splits(kinds, 60, 11)
    L = _learner(sa, ctx, bm.model_from_splits(bm.shuffled(s, 12), X.shape[1], 12, per_tree=11))
    n_cond, n_nodes, lds = _staged_size(sa, ctx, L['te'])
    assert n_cond * TS_CSTRIDE > 65536, n_cond
    assert lds <= LDS_LIMIT, lds
    for lay in ('tiled', 'bits', 'bits32'):
        _assert_close(L['te'].predict_blocks(ctx['blocks'][lay], method='staged'), L['ref32'], 1e-6,
                      f'unscaled staged walk, {lay} blocks ({n_cond} conditions, {n_nodes} nodes)')
    _check_pair(sa, ctx, ctx['ab'], [L], f'unscaled walk over condition bitmaps ({n_cond} conditions)')


def test_condition_tables_in_global_memory(sa):
    """Three learners whose union of numeric conditions no longer fits the COND pass's staged
    tables, so the pass reads them from global memory, while each learner's walk still fits LDS."""
    ctx = _ctx(sa, 'spadl_k3')
    X, kinds, plan = ctx['X'], ctx['kinds'], ctx['plan']
    learners = []
    for q in range(3):
        s = _spread_f_splits(ctx, 1400, 20 + q) + bm.b_splits(kinds, 20, 20 + q)
        learners.append(_learner(sa, ctx, bm.model_from_splits(bm.shuffled(s, 30 + q), X.shape[1], 30 + q,
                                                               per_tree=11)))
    for L in learners:
        assert _staged_size(sa, ctx, L['te'])[2] <= LDS_LIMIT
    prep = _check_condition_bitmaps(sa, ctx, ctx['ab'], X, learners)
    # cond_lds_bytes(Cf, Ci, n_cond) = 4 (Cf + Ci + 2) + 8 n_cond > COND_LDS_MAX = 32 KiB (sa_vaep.hip):
    # the column starts of both blocks, then a float32 threshold and an int32 default per condition
    assert 4 * (plan.n_f64 + plan.n_i64 + 2) + 8 * prep['n_num'] > 32 * 1024, prep['n_num']
    _check_pair(sa, ctx, ctx['ab'], learners, f"condition tables in global memory ({prep['n_num']} conditions)")


def test_gather_fallback_beyond_lds(sa):
    """More than 2,048 nodes (TR_LDS_NODES: the gather walk reads the model from global memory)
    and a staged form that does not fit LDS: predict_blocks falls back to the gather walk by
    itself and equals the oracle; asked for the staged walk it raises."""
    ctx = _ctx(sa, 'spadl_k3')
    X, kinds = ctx['X'], ctx['kinds']
    s = _spread_f_splits(ctx, 2000, 40) + bm.b_splits(kinds, 60, 40)
    L = _learner(sa, ctx, bm.model_from_splits(bm.shuffled(s, 41), X.shape[1], 41, per_tree=11))
    te = L['te']
    n_cond, n_nodes, lds = _staged_size(sa, ctx, te)
    assert len(te.nodes) > 2048 and lds > LDS_LIMIT, (len(te.nodes), lds)
    for lay in ('tiled', 'plain'):
        _assert_close(te.predict_blocks(ctx['blocks'][lay]), L['ref32'], 1e-6, f'gather fallback, {lay} blocks')
    with pytest.raises(ValueError):
        te.predict_blocks(ctx['blocks']['tiled'], method='staged')
    with pytest.raises(ValueError):
        sa['trees'].predict_pair_conditions(ctx['ab'], ctx['plan'], [te])
