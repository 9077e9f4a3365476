"""Float-derived decisions against the reference at their thresholds.

Three one-line float64 rules in the kernels decide an id, a count or a whole output row, and the
inputs of tests/threshold_cases.py sit ON them:

* the dribble rule ``d2 >= min2 && d2 <= max2 && dt < max_dt`` with the separately rounded
  ``d2 = dx*dx + dy*dy`` (csrc/sa_atomic.hip ``dribble_after``; what ``-ffp-contract=off`` in
  socceraction_amd/build.py is for);
* the xT binning ``clip(int64(x / 105 * l), 0, l - 1)`` in its two arithmetic forms (csrc/sa_common.h
  ``flat_index`` by a division, ``flat_index_q`` by ``bin_quot``'s reciprocal and two FMAs) at
  every device site that bins a coordinate;
* the formula's same-phase rule ``abs(t - t_prev) > 10`` (csrc/sa_vaep.hip), which Atomic-VAEP's
  formula does not have.

Every device result is compared with ``oracle/`` and with the reference's own outputs
(tests/golden/make_golden_thresholds.py), never with another device path.  Bars: ids, counts,
cells, rows and dtypes bit-exact; xT rates bit-exact (surfaces of small integers: every rate is
an exact integer difference that names the cell pair); formula values bit-exact, float32 and
float64 (golden_io.assert_same_floats; one wrong decision moves a value by at least 0.1); the
interpolated xT rates within golden_io.assert_close.  The unmarked
tests hold the inputs to a coverage floor, so a later edit of the value sets cannot hollow the
device tests out, and the oracle to the goldens.

That the device tests bite was checked once with eight mutated builds of the library, each run
against this module in a process of its own (of the 53 device cases, the number that failed):
``-ffp-contract=off`` removed 18, ``d2 > min2`` 22, ``d2 < max2`` 18, ``dt <= max_dt`` 10,
``fabs(...) >= 10.0`` 13, ``flat_index`` as ``x * (l / FIELD_L)`` 12, ``bin_quot`` without its
correction 10, ``cell_index`` without the ``inr`` test 12.  The unmutated library passes all of
them; the device cases take about 4 s together on one MI355X.
"""
import os

import numpy as np
import pandas as pd
import pytest

import threshold_cases as tc
from golden_io import GOLDEN, assert_close, assert_frame_same, assert_same_floats, dribbles_frame, load
from oracle import atomic_convert_oracle as co
from oracle import vaep_oracle as vo
from oracle import xt_oracle as xo
from xt_count_checks import ref_counts as _ref_counts, same_counts as _same_counts

gpu = pytest.mark.gpu

XT_COLS = ('start_x', 'start_y', 'end_x', 'end_y', 'type_id', 'result_id')
SPADL_COLS = ('period_id', 'time_seconds', 'team_id', 'start_x', 'start_y', 'end_x', 'end_y',
              'type_id', 'result_id', 'bodypart_id')
VALUES = ('offensive_value', 'defensive_value', 'vaep_value')
ALL_GRIDS = tc.GRIDS16 + tc.GRIDS32


def _npz(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# =============================================================================== CPU: the inputs
@pytest.mark.parametrize('rule', [(3.0, 60.0, 10.0), (1.5, 40.0, 7.5)])
def test_dribble_frame_meets_the_coverage_floor(rule):
    """Per distance threshold: >= 50 pairs on which a fused multiply-add (either operand order,
    evaluated exactly with fractions.Fraction) decides differently from the unfused sum, and >= 10
    pairs with d2 exactly on it; every duration case is present with an exact difference; the
    frame is long enough to put a threshold pair across every multiple of 256 rows up to 2048."""
    mn, mx, md = rule
    f = tc.dribble_frame(min_len=mn, max_len=mx, max_dt=md)
    n = len(f['type_id'])
    assert n >= 2049
    assert (f['start_x'] == 0).all() and (f['start_y'] == 0).all()
    dx, dy, dt = tc.dribble_pairs(f)
    d2 = dx * dx + dy * dy
    same = (f['team_id'][:-1] == f['team_id'][1:]) & (f['period_id'][:-1] == f['period_id'][1:])
    mid = (d2 > 1.5 * mn ** 2) & (d2 < mx ** 2 / 1.5)   # the duration cases: only dt decides
    on = mid.copy()
    for T, lower in ((mn ** 2, True), (mx ** 2, False)):
        near = np.abs(d2 - T) <= 8 * np.spacing(T)
        flips = tc.fused_flips(dx[near], dy[near], T, lower)
        assert int((flips & same[near]).sum()) >= 50, (T, int(flips.sum()))
        assert int(((d2 == T) & same).sum()) >= 10, T
        on |= near
    up, dn = np.nextafter(md, np.inf), np.nextafter(md, -np.inf)
    for v in (md, up, dn, -md, 0.0, -1e6, 1e6):
        assert ((dt == v) & same & mid).any(), v
    assert on.all()   # every pair is a threshold case, so one straddles every block boundary:
    for m in (128, 256, 512, 1024, 2048):
        assert mid[m - 1] and same[m - 1], m   # a duration case across rows m - 1, m
    assert int((~same).sum()) >= 10
    # per-game action ids in increasing key order: the fast placement
    key = f['game_id'] * 10 ** 9 + f['period_id'] * 10 ** 6 + f['action_id']
    assert (np.diff(key) > 0).all()


def _union_values():
    for l, w in ALL_GRIDS + (tc.NODE_GRID,):
        yield tc.FIELD_L, l, tc.edge_values(tc.FIELD_L, l)
        yield tc.FIELD_W, w, tc.edge_values(tc.FIELD_W, w)


def test_binning_values_meet_the_coverage_floor():
    """Each plausible wrong way to write the binning disagrees with xt_oracle.cell_indexes on at
    least 5 of the values, over all grids together (one grid may score zero for one formula)."""
    miss = {name: 0 for name in tc.WRONG_BINNINGS}
    for b, l, v in _union_values():
        ref = xo.cell_indexes(v, v, l, l)[0] if b == tc.FIELD_L else xo.cell_indexes(v, v, l, l)[1]
        assert ref.min() == 0 and ref.max() == l - 1
        for name, fn in tc.WRONG_BINNINGS.items():
            miss[name] += int((fn(v, b, l) != ref).sum())
    assert all(c >= 5 for c in miss.values()), miss
    # the batches carry every value on both the start and the end coordinate
    for l, w in ((16, 12), (120, 68)):
        d = tc.binning_batch(l, w)
        for c, b, k in (('start_x', 105.0, l), ('end_x', 105.0, l), ('start_y', 68.0, w), ('end_y', 68.0, w)):
            assert set(tc.edge_values(b, k).tolist()) <= set(d[c].tolist())
        assert np.isfinite(np.r_[d['start_x'], d['start_y'], d['end_x'], d['end_y']]).all()
        assert set(d['type_id'].tolist()) == set(tc.BIN_TYPES) and set(d['result_id'].tolist()) == {0, 1}


def test_samephase_batches_sit_on_the_threshold():
    up, dn = np.nextafter(10.0, np.inf), np.nextafter(10.0, -np.inf)
    for n in tc.SAMEPHASE_N:
        d = tc.samephase_batch(n)
        off = d['game_off']
        assert len(d['type_id']) == n and off[0] == 0 and off[-1] == n
        assert len(off) - 1 >= (2 if n >= 2 else 1) and (np.diff(off) > 0).all()
        df = tc.samephase_diffs(d)
        assert len(df) == n - (len(off) - 1)
        assert (np.abs(df - 10.0) < 2e-3).all()
        assert ((d['ps'] > 0.1) & (d['ps'] < 0.9) & (d['pc'] > 0.1) & (d['pc'] < 0.9)).all()
        if n >= 127:
            for v in (10.0, up, dn, 9.999, 10.001):
                assert (df == v).any(), (n, v)
            t = d['time_seconds']
            assert ((t[1:] - t[:-1]) == -10.0).any() and ((t[1:] - t[:-1]) == 10.0).any()
            assert {5, 6, 11, 12} <= set(d['type_id'].tolist())


# =============================================================================== CPU: the oracle
def test_golden_inputs_are_the_builders():
    """The goldens were made from the builders as they are now."""
    g = load('dribbles', 'thresholds')
    f = tc.dribble_frame(per_threshold=230)
    df = dribbles_frame(g, 'in_')
    for c in tc.DRIBBLE_COLS:
        np.testing.assert_array_equal(df[c].to_numpy(), f[c], err_msg=c)
    g = _npz('xt_edges.npz')
    for l, w in tc.GOLDEN_GRIDS:
        d = tc.binning_batch(l, w)
        for c in XT_COLS:
            np.testing.assert_array_equal(g[f'g{l}x{w}_in_{c}'], d[c], err_msg=c)
    g = _npz('formula_samephase.npz')
    d = tc.samephase_batch(600)
    for c in SPADL_COLS:
        np.testing.assert_array_equal(g['in_' + c], d[c], err_msg=c)
    np.testing.assert_array_equal(g['ps'], d['ps'])


def _xt_case(g, l, w):
    tag = f'g{l}x{w}_'
    d = {c: g[tag + 'in_' + c] for c in ('game_id', 'period_id', 'time_seconds', 'team_id', 'bodypart_id') + XT_COLS}
    d['game_off'], d['home_team_id'] = g[tag + 'game_off'], g[tag + 'home_team_id']
    return tag, d


@pytest.mark.parametrize('l,w', tc.GOLDEN_GRIDS)
def test_xt_oracle_reproduces_the_edge_golden(l, w):
    """xt_oracle's cell indexes, counts and transition entries == the reference's
    (_get_cell_indexes, _count, move_transition_matrix) on the edge values, exactly."""
    tag, d = _xt_case(_npz('xt_edges.npz'), l, w)
    g = _npz('xt_edges.npz')
    for side in ('start', 'end'):
        xi, yj = xo.cell_indexes(d[side + '_x'], d[side + '_y'], l, w)
        np.testing.assert_array_equal(xi, g[tag + side + '_xi'])
        np.testing.assert_array_equal(yj, g[tag + side + '_yj'])
    ref = _ref_counts(d, l, w)   # what the device tests compare with
    for name in ('shot', 'goal', 'move'):
        np.testing.assert_array_equal(ref[name], g[tag + name].reshape(-1))
    idx, c = ref['trans']
    np.testing.assert_array_equal(idx, g[tag + 'trans_idx'])
    start = g[tag + 'move'].reshape(-1)[idx // (l * w)]
    np.testing.assert_array_equal(c / start, g[tag + 'trans_val'])


def test_formula_oracle_reproduces_the_samephase_golden():
    g = _npz('formula_samephase.npz')
    cols = {c: g['in_' + c] for c in SPADL_COLS}
    for tag, dt in (('64', np.float64), ('32', np.float32)):
        v = vo.formula(cols, g['ps'].astype(dt), g['pc'].astype(dt), seg_off=g['game_off'])
        for c in VALUES:
            assert v[c].dtype == dt
            assert_same_floats(v[c], g[f'{c}_{tag}'], c)
    # the rule took both branches on the threshold pairs
    t = g['in_time_seconds']
    assert (np.abs(np.diff(t)) == 10.0).any() and (np.abs(np.diff(t)) > 10.0).any()


def test_dribble_oracle_reproduces_the_threshold_golden():
    g = load('dribbles', 'thresholds')
    df = dribbles_frame(g, 'in_')
    ref = dribbles_frame(g, 'out_')
    _frame_vs_oracle(ref, co.add_dribbles({c: df[c].to_numpy() for c in co.COLS}), 'golden', dtypes=False)
    assert len(ref) > len(df)


def _frame_vs_oracle(got: pd.DataFrame, ref: dict, name: str, dtypes: bool = True):
    """Every column of a frame bit for bit against the oracle's columns (and their dtypes)."""
    assert len(got) == len(ref['type_id']), (name, len(got), len(ref['type_id']))
    for c in co.COLS:
        if c == 'original_event_id':
            miss = pd.isna(ref[c])
            np.testing.assert_array_equal(got[c].isna().to_numpy(), miss, err_msg=name)
            np.testing.assert_array_equal(got[c].to_numpy()[~miss].astype(str), ref[c][~miss].astype(str))
            continue
        a, b = got[c].to_numpy(), np.asarray(ref[c])
        if dtypes:
            assert a.dtype == b.dtype, (name, c, a.dtype, b.dtype)
        np.testing.assert_array_equal(a, b, err_msg=f'{name} {c}')


# =============================================================================== GPU
@pytest.fixture(scope='module')
def sa():
    import torch
    from socceraction_amd import _native, batch, catalog, ops
    from socceraction_amd.atomic.spadl import base as atomic_base
    from socceraction_amd.spadl import base
    _native.load_library()
    return dict(torch=torch, native=_native, batch=batch, catalog=catalog, ops=ops, base=base,
                atomic_base=atomic_base)


# ------------------------------------------------------------------------------- A. dribbles
_FRAMES = {}


def _dribble_case(rule, layout):
    """The frame of a rule (built once) in a layout, with the oracle's output of the whole frame."""
    key = (rule, layout)
    if key not in _FRAMES:
        f = tc.dribble_frame(min_len=rule[0], max_len=rule[1], max_dt=rule[2])
        if layout == 'shuffled':
            f = tc.dribble_shuffled(f)
        for v in f.values():
            v.setflags(write=False)
        _FRAMES[key] = f
    return _FRAMES[key]


DEFAULT_RULE = (3.0, 60.0, 10.0)


@gpu
@pytest.mark.parametrize('n', tc.DRIBBLE_PREFIXES + (None,))
@pytest.mark.parametrize('layout', ['fast', 'shuffled'])
def test_dribble_thresholds_vs_oracle(sa, layout, n):
    """_add_dribbles of the threshold frame and its prefixes == the oracle: every column and
    dtype bit for bit, per-game action ids (fast placement) and shuffled rows (lexsort)."""
    f = _dribble_case(DEFAULT_RULE, layout)
    if n is not None:
        f = tc.dribble_prefix(f, n)
    df = pd.DataFrame({c: f[c] for c in tc.DRIBBLE_COLS})
    ref = co.add_dribbles(f)
    got = sa['base']._add_dribbles(df)
    _frame_vs_oracle(got, ref, f'{layout} n={n}')
    if n is None:
        assert 200 < len(got) - len(df) < len(df) - 200   # both outcomes, in numbers


@gpu
@pytest.mark.parametrize('layout', ['fast', 'shuffled'])
def test_dribble_module_thresholds_vs_oracle(sa, layout):
    """The thresholds are module globals read at call time (not a baked-in 9 / 3600 / 10): a
    frame built on 1.5 m / 40 m / 7.5 s against the oracle with the same rule."""
    sb = sa['base']
    rule = (1.5, 40.0, 7.5)
    f = _dribble_case(rule, layout)
    df = pd.DataFrame({c: f[c] for c in tc.DRIBBLE_COLS})
    old = sb.min_dribble_length, sb.max_dribble_length, sb.max_dribble_duration
    try:
        sb.min_dribble_length, sb.max_dribble_length, sb.max_dribble_duration = rule
        got = sb._add_dribbles(df)
    finally:
        sb.min_dribble_length, sb.max_dribble_length, sb.max_dribble_duration = old
    _frame_vs_oracle(got, co.add_dribbles(f, *rule), f'rule {rule} {layout}')
    assert len(got) != len(co.add_dribbles(f)['type_id'])  # the default rule decides otherwise


@gpu
def test_dribble_thresholds_golden(sa):
    """== the reference's own output (tests/golden/dribbles_thresholds.npz)."""
    g = load('dribbles', 'thresholds')
    df = dribbles_frame(g, 'in_')
    assert_frame_same(sa['base']._add_dribbles(df.copy()), dribbles_frame(g, 'out_'), 'thresholds')


@gpu
def test_dribble_thresholds_device_frame(sa):
    """add_dribbles_device on a SpadlFrame directly: the inserted rows (``src`` < 0) are the
    oracle's, each right after its parent, and every device column holds the oracle's values."""
    torch = sa['torch']
    f = _dribble_case(DEFAULT_RULE, 'fast')
    df = pd.DataFrame({c: f[c] for c in tc.DRIBBLE_COLS})
    frame = sa['atomic_base'].SpadlFrame.from_frame(df, sort=False)
    out = sa['base'].add_dribbles_device(frame, f['action_id'])
    torch.cuda.synchronize()
    ref = co.add_dribbles(f)
    m = len(ref['type_id'])
    assert out.n == m and out.n_dribbles == m - len(df)
    drib = pd.isna(ref['original_event_id'])
    src = out.cols['src'][:m].cpu().numpy()
    np.testing.assert_array_equal(src < 0, drib)
    np.testing.assert_array_equal(src[~drib], np.arange(len(df)))
    pos = np.flatnonzero(drib)
    np.testing.assert_array_equal(~src[pos], src[pos + 1])   # inserted before its successor
    for c in ('time_seconds', 'start_x', 'start_y', 'end_x', 'end_y', 'period_id', 'type_id',
              'result_id', 'bodypart_id'):
        got = out.cols[c][:m].cpu().numpy()
        np.testing.assert_array_equal(got, np.asarray(ref[c]).astype(got.dtype), err_msg=c)
    for c, key in (('game_id', 'game'), ('team_id', 'team'), ('player_id', 'player')):
        got = frame.uniques[key].to_numpy()[out.cols[key][:m].cpu().numpy()]
        np.testing.assert_array_equal(got, ref[c], err_msg=c)


# ------------------------------------------------------------------------------- B. binning
def _batch(sa, d):
    return sa['batch'].ActionBatch.from_columns(d)


def _same_rate(got, ref, what):
    """The same NaN rows and bitwise-equal values."""
    a = got.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(a), np.isnan(ref), err_msg=what)
    np.testing.assert_array_equal(a[~np.isnan(ref)], ref[~np.isnan(ref)], err_msg=what)


def _decode_cells(sa, cells, n, l, w):
    """(class, start cell, end cell, success) of every action from its cell code (csrc/sa_common.h
    xt_cell_code / xt_cell_code16); -1 where the code holds no such cell."""
    c = sa['ops'].xt_cell_codes(cells, n, l, w).cpu().numpy()
    if l * w <= sa['native'].SA_XT_CELLS16_MAX_C:
        c = c.view(np.uint16).astype(np.int64)
        shot0, miss0 = 202 << 8, (202 << 8) + 512
        cls = np.where(c < shot0, 2, np.where(c < miss0, 1, np.where(c < miss0 + 256, 2, 0)))
        assert ((c < miss0 + 256) | (c == 0xFFFF)).all()   # no non-finite coordinate
        cs = np.where(c < shot0, c >> 8, np.where(c < miss0, (c - shot0) >> 1, np.where(cls == 2, c - miss0, -1)))
        ce = np.where(c < shot0, c & 0xFF, -1)
        succ = np.where(c < shot0, 1, np.where(c < miss0, (c - shot0) & 1, 0))
        return cls, cs, ce, succ
    c = c.view(np.uint32).astype(np.int64)
    cls = (c >> 24) & 3
    assert ((c >> 27) == 0).all()
    return cls, np.where(cls != 0, c & 0xFFF, -1), np.where(cls == 2, (c >> 12) & 0xFFF, -1), (c >> 26) & 1


def _check_cells(sa, cells, d, l, w, what):
    n = len(d['type_id'])
    t, r = d['type_id'], d['result_id']
    cls, cs, ce, succ = _decode_cells(sa, cells, n, l, w)
    want_cls = np.where(t == 11, 1, np.where((t == 0) | (t == 21) | (t == 1), 2, 0))
    np.testing.assert_array_equal(cls, want_cls, err_msg=what)
    s = xo.flat_indexes(d['start_x'], d['start_y'], l, w)
    e = xo.flat_indexes(d['end_x'], d['end_y'], l, w)
    np.testing.assert_array_equal(cs[cls != 0], s[cls != 0], err_msg=f'{what} start cells')
    ends = ce >= 0   # 32-bit codes: every move; 16-bit codes: successful moves
    assert (ends == ((cls == 2) & ((r == 1) | (l * w > sa['native'].SA_XT_CELLS16_MAX_C)))).all(), what
    np.testing.assert_array_equal(ce[ends], e[ends], err_msg=f'{what} end cells')
    np.testing.assert_array_equal(succ[cls != 0] == 1, r[cls != 0] == 1, err_msg=what)


@gpu
@pytest.mark.parametrize('l,w', ALL_GRIDS)
def test_binning_edges_vs_oracle(sa, l, w):
    """Counts, cell codes and rates of coordinates on the cell edges +-2 ulp, outside the pitch
    and past the int64 range == xt_oracle, exactly, at every device site that bins: the
    coordinate count (+ its rate codes), the band-owned bucket count (binning quotients), the
    cell codes of sa_xt_cells and of the feature pass and step (16-bit codes up to 202 cells,
    32-bit up to 4096), and the rates on coordinates, rate codes and cell codes."""
    torch, ops, N = sa['torch'], sa['ops'], sa['native']
    d = tc.binning_batch(l, w)
    ab = _batch(sa, d)
    n, C = ab.n, l * w
    ref = _ref_counts(d, l, w)
    assert (ops.xt_band_shape(l, w) is None) == (C <= 202)   # the bucket count from 203 cells
    codes = ops.xt_rate_codes_buffer(n, ab.device)
    _same_counts(sa, ops.xt_count(ab, l, w), ref, 'xt_count')
    _same_counts(sa, ops.xt_count(ab, l, w, codes=codes), ref, 'xt_count + codes')
    _same_counts(sa, ops.xt_count_many([ab], l, w), ref, 'xt_count_many')
    # a surface whose value at cell c is c + 1: every rate names its cell pair
    surf = np.arange(1, C + 1, dtype=np.float64).reshape(w, l)
    grid = torch.from_numpy(surf).to(ab.device)
    want = xo.rate(d, surf)
    assert (~np.isnan(want)).sum() > n // 4
    for what, (r, e) in (('xt_rate', ops.xt_rate(ab, grid, l, w)),
                         ('xt_rate_codes', ops.xt_rate_codes(codes, n, grid))):
        _same_rate(r, want, what)
        assert int(e.item()) == 0, what
    if C > N.SA_XT_CELLS_MAX_C:
        with pytest.raises(ValueError):
            ops.xt_cells(ab, l, w)
        return
    cells = ops.xt_cells(ab, l, w)
    _check_cells(sa, cells, d, l, w, 'xt_cells')
    _same_counts(sa, ops.xt_count_cells(cells, n, l, w), ref, 'xt_cells + xt_count_cells')
    r, e = ops.xt_rate_cells(cells, n, l, w, grid)
    _same_rate(r, want, 'xt_rate_cells')
    assert int(e.item()) == 0
    # the feature pass's cell codes (register-window path k = 3 and generic path k = 5), the step's
    for k in (3, 5):
        fb = ops.alloc_feature_blocks(sa['catalog'].build_plan(vo.SPADL_DEFAULT, k), n, ab.device, 1024, 128)
        c2 = ops.xt_cells_buffer(n, ab.device)
        ops.features_into(ab.struct(), fb, xt_cells=(l, w, c2))
        _check_cells(sa, c2, d, l, w, f'feature pass k={k}')
        _same_counts(sa, ops.xt_count_cells(c2, n, l, w), ref, f'feature pass k={k} + xt_count_cells')
    fb = ops.alloc_feature_blocks(ops.build_plan(vo.SPADL_DEFAULT, 3, False), n, ab.device, 1024, 128)
    ps = torch.full((n,), 0.5, dtype=torch.float64, device=ab.device)
    lab, val = ops.labels_formula(ab, ps, ps)
    c3 = ops.xt_cells_buffer(n, ab.device)
    ops.step_into(ab.struct(), fb, ps, ps, 10, lab, val, xt_cells=(l, w, c3))
    _check_cells(sa, c3, d, l, w, 'step')
    _same_counts(sa, ops.xt_count_cells(c3, n, l, w), ref, 'step + xt_count_cells')


@gpu
def test_binning_edges_node_grid_vs_oracle(sa):
    """The interpolated rate's 1050 x 680 node grid on its own edge values: sa_xt_rate on the
    coordinates, sa_xt_rate_interp, and the interp codes the band-owned count of the 105 x 68 fit
    writes (binning quotients) + sa_xt_rate_interp_codes, against xt_oracle exactly.  The surface
    is 2 x 2 with node axes chosen so that node (row r, column h) interpolates to exactly
    h + 2048 r (every factor a dyadic rational, every product and sum exact), so the rates are
    exact integers that name the node pair; the library's own axes and a random 105 x 68 surface
    are held to the oracle's interpolation within the suite's float bar."""
    torch, ops = sa['torch'], sa['ops']
    L, W = tc.NODE_GRID
    d = tc.binning_batch(L, W)
    ab = _batch(sa, d)
    n = ab.n
    nodes = np.arange(L, dtype=np.float64)[None, :] + 2048.0 * np.arange(W, dtype=np.float64)[:, None]
    want = xo.rate(d, nodes)
    assert (~np.isnan(want)).sum() > n // 4 and len(np.unique(want[~np.isnan(want)])) > 1000
    r, e = ops.xt_rate(ab, torch.from_numpy(nodes).to(ab.device), L, W)
    _same_rate(r, want, 'xt_rate on the node grid')
    assert int(e.item()) == 0
    ic = ops.xt_interp_codes_buffer(n, ab.device)
    acc = ops.xt_count_many([ab], 105, 68, interp_codes=[ic])
    _same_counts(sa, acc, _ref_counts(d, 105, 68), 'xt_count_many + interp codes')
    xT = torch.tensor([[0.0, 2048.0], [2048.0 * 1024.0, 2048.0 * 1024.0 + 2048.0]], dtype=torch.float64,
                      device=ab.device)
    axes = torch.from_numpy(np.r_[0.0, 2048.0, 0.0, 1024.0, np.arange(L, dtype=np.float64),
                                  np.arange(W, dtype=np.float64)]).to(ab.device)
    for what, (r, e) in (('xt_rate_interp', ops.xt_rate_interp(ab, xT, 2, 2, axes=axes)),
                         ('xt_rate_interp_codes', ops.xt_rate_interp_codes(ic, n, xT, 2, 2, axes=axes))):
        _same_rate(r, want, what)
        assert int(e.item()) == 0, what
    surf = np.random.default_rng(3).random((68, 105))
    want = xo.rate(d, surf, use_interpolation=True)
    xs = torch.from_numpy(surf).to(ab.device)
    for what, (r, e) in (('xt_rate_interp', ops.xt_rate_interp(ab, xs, 105, 68)),
                         ('xt_rate_interp_codes', ops.xt_rate_interp_codes(ic, n, xs, 105, 68))):
        assert_close(r.cpu().numpy(), want, what)


@gpu
@pytest.mark.parametrize('l,w', tc.GOLDEN_GRIDS)
def test_binning_edges_golden(sa, l, w):
    """Device cells, counts and transition probabilities == the reference's own
    (tests/golden/xt_edges.npz)."""
    torch, ops = sa['torch'], sa['ops']
    g = _npz('xt_edges.npz')
    tag, d = _xt_case(g, l, w)
    ab = _batch(sa, d)
    flat = {s: (w - 1 - g[tag + s + '_yj']) * l + g[tag + s + '_xi'] for s in ('start', 'end')}
    if l * w <= sa['native'].SA_XT_CELLS_MAX_C:
        cls, cs, ce, _ = _decode_cells(sa, ops.xt_cells(ab, l, w), ab.n, l, w)
        np.testing.assert_array_equal(cs[cls != 0], flat['start'][cls != 0])
        np.testing.assert_array_equal(ce[ce >= 0], flat['end'][ce >= 0])
    else:   # the cells through the rate of a surface that names them
        surf = np.arange(1, l * w + 1, dtype=np.float64).reshape(w, l)
        r, _ = ops.xt_rate(ab, torch.from_numpy(surf).to(ab.device), l, w)
        r = r.cpu().numpy()
        ok = ~np.isnan(r)
        np.testing.assert_array_equal(r[ok], (flat['end'] - flat['start'])[ok].astype(np.float64))
    for acc in (ops.xt_count(ab, l, w), ops.xt_count_many([ab], l, w)):
        for name in ('shot', 'goal', 'move'):
            np.testing.assert_array_equal(getattr(acc, name).cpu().numpy(), g[tag + name].reshape(-1))
        nz = torch.nonzero(acc.trans).reshape(-1)
        np.testing.assert_array_equal(nz.cpu().numpy(), g[tag + 'trans_idx'])
        start = acc.move[nz // (l * w)].cpu().numpy()
        np.testing.assert_array_equal(acc.trans[nz].cpu().numpy() / start, g[tag + 'trans_val'])


# ------------------------------------------------------------------------------- C. same phase
def _formula_ref(d, dt, atomic=False):
    cols = {c: d[c] for c in d if c not in ('game_off', 'home_team_id', 'ps', 'pc')}
    return vo.formula(cols, d['ps'].astype(dt), d['pc'].astype(dt), atomic=atomic, seg_off=d['game_off'])


def _same_values(v, ref, n, dt, what):
    v = v.cpu().numpy()[:, :n]
    for r, c in enumerate(VALUES):
        assert v[r].dtype == dt
        # a few IEEE operations in the reference's order, f32 and f64 alike: bit-exact
        assert_same_floats(v[r], ref[c], f'{what} {c}')


@gpu
@pytest.mark.parametrize('n', tc.SAMEPHASE_N)
def test_samephase_rule_vs_oracle(sa, n):
    """formula and labels_formula (float64 and float32 probabilities) and the fused step on
    batches whose every time difference inside a segment sits on the rule's 10 s == the oracle;
    the labels of the fused launches too."""
    torch, ops = sa['torch'], sa['ops']
    d = tc.samephase_batch(n)
    ab = _batch(sa, d)
    lab_ref = vo.labels({c: d[c] for c in SPADL_COLS}, seg_off=d['game_off'])
    for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        ref = _formula_ref(d, dt)
        ps = torch.from_numpy(d['ps'].astype(dt)).to(ab.device)
        pc = torch.from_numpy(d['pc'].astype(dt)).to(ab.device)
        assert ps.dtype == tdt
        _same_values(ops.formula(ab, ps, pc), ref, n, dt, 'formula')
        lab, val = ops.labels_formula(ab, ps, pc)
        _same_values(val, ref, n, dt, 'labels_formula')
        for c in ('scores', 'concedes', 'goal_from_shot'):
            np.testing.assert_array_equal(getattr(lab, c)[:n].cpu().numpy().astype(bool), lab_ref[c], err_msg=c)
    ps = torch.from_numpy(d['ps']).to(ab.device)
    pc = torch.from_numpy(d['pc']).to(ab.device)
    ref = _formula_ref(d, np.float64)
    for k in (1, 3):
        out = ops.alloc_feature_blocks(ops.build_plan(vo.SPADL_DEFAULT, k, False), n, ab.device, 1024, 128)
        lab, val = ops.labels_formula(ab, ps, pc)   # right-shaped buffers
        for t in (lab.scores, lab.concedes, lab.goal_from_shot):
            t.fill_(7)
        val.fill_(float('nan'))
        ops.step_into(ab.struct(), out, ps, pc, 10, lab, val)
        _same_values(val, ref, n, np.float64, f'step k={k}')
        for c in ('scores', 'concedes', 'goal_from_shot'):
            np.testing.assert_array_equal(getattr(lab, c)[:n].cpu().numpy().astype(bool), lab_ref[c], err_msg=c)


@gpu
@pytest.mark.parametrize('chunk', [512, 1024])
def test_samephase_rule_chunked_step_vs_oracle(sa, chunk):
    """The chunked step with chunks that end on threshold pairs (every pair is one): the row
    before a chunk's first row comes from the previous launch's range."""
    import copy
    torch, ops = sa['torch'], sa['ops']
    n = 2049
    d = tc.samephase_batch(n)
    ab = _batch(sa, d)
    plan = ops.build_plan(vo.SPADL_DEFAULT, 3, False)
    num = copy.copy(plan)   # the chunked step is the numeric pass only
    num.struct = copy.deepcopy(plan.struct)
    for x in range(len(num.struct.bool_col)):
        num.struct.bool_col[x] = -1
    blk = ops.alloc_feature_blocks(plan, n, ab.device, 1024, 128)
    view = ops.FeatureBlocks(num, n, blk.Rb, blk.Rn, blk.bool_block, blk.f64_block, blk.i64_block)
    ps = torch.from_numpy(d['ps']).to(ab.device)
    pc = torch.from_numpy(d['pc']).to(ab.device)
    lab, val = ops.labels_formula(ab, ps, pc)
    for t in (lab.scores, lab.concedes, lab.goal_from_shot):
        t.fill_(7)
    val.fill_(float('nan'))
    ops.step_into(ab.struct(), view, ps, pc, 10, lab, val, chunk_rows=chunk)
    _same_values(val, _formula_ref(d, np.float64), n, np.float64, f'chunked step {chunk}')
    lab_ref = vo.labels({c: d[c] for c in SPADL_COLS}, seg_off=d['game_off'])
    for c in ('scores', 'concedes', 'goal_from_shot'):
        np.testing.assert_array_equal(getattr(lab, c)[:n].cpu().numpy().astype(bool), lab_ref[c], err_msg=c)


@gpu
def test_samephase_rule_golden(sa):
    """== the reference's own vaep.formula.value (tests/golden/formula_samephase.npz)."""
    torch, ops = sa['torch'], sa['ops']
    g = _npz('formula_samephase.npz')
    d = {c: g['in_' + c] for c in SPADL_COLS}
    d.update(game_off=g['game_off'], home_team_id=g['home_team_id'])
    ab = _batch(sa, d)
    for tag, dt in (('64', np.float64), ('32', np.float32)):
        ps = torch.from_numpy(g['ps'].astype(dt)).to(ab.device)
        pc = torch.from_numpy(g['pc'].astype(dt)).to(ab.device)
        ref = {c: g[f'{c}_{tag}'] for c in VALUES}
        _same_values(ops.formula(ab, ps, pc), ref, ab.n, dt, 'formula')
        _same_values(ops.labels_formula(ab, ps, pc)[1], ref, ab.n, dt, 'labels_formula')


@gpu
@pytest.mark.parametrize('n', [129, 2049])
def test_atomic_formula_has_no_samephase_rule(sa, n):
    """The reference's atomic formula has the rule commented out: on the same times nothing is
    zeroed -- the values are the oracle's, and every row more than 10 s after a non-goal
    predecessor still subtracts that row's probability (>= 0.1)."""
    torch, ops = sa['torch'], sa['ops']
    d = tc.samephase_batch(n)
    rng = np.random.default_rng(n)
    a = {c: d[c] for c in ('game_id', 'period_id', 'time_seconds', 'team_id', 'bodypart_id', 'game_off',
                           'home_team_id', 'ps', 'pc')}
    a.update(x=d['start_x'], y=d['start_y'], dx=d['end_x'] - d['start_x'], dy=d['end_y'] - d['start_y'],
             type_id=rng.choice([0, 11, 21, 23, 27, 28], n, p=[0.4, 0.1, 0.2, 0.2, 0.05, 0.05]).astype(np.int64))
    ab = sa['batch'].ActionBatch.from_columns(a, atomic=True)
    off = d['game_off']
    prev = np.maximum(np.arange(n) - 1, off[np.searchsorted(off, np.arange(n), 'right') - 1])
    late = (np.abs(a['time_seconds'] - a['time_seconds'][prev]) >= 10.0) & ~np.isin(a['type_id'][prev], [27, 28])
    late &= prev != np.arange(n)
    assert late.sum() > n // 3
    for dt in (np.float64, np.float32):
        ref = _formula_ref(a, dt, atomic=True)
        ps = torch.from_numpy(a['ps'].astype(dt)).to(ab.device)
        pc = torch.from_numpy(a['pc'].astype(dt)).to(ab.device)
        for what, v in (('formula', ops.formula(ab, ps, pc)), ('labels_formula', ops.labels_formula(ab, ps, pc)[1])):
            _same_values(v, ref, n, dt, f'atomic {what}')
            h = v.cpu().numpy()[:, :n].astype(np.float64)
            assert (a['ps'].astype(dt)[late] - h[0][late] >= 0.0999).all(), what   # prev_s kept
            assert (h[1][late] + a['pc'].astype(dt)[late] >= 0.0999).all(), what   # prev_c kept
