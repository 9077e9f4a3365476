"""Every feature, label and formula kernel variant of csrc/sa_vaep.hip against the oracle (or the
reference's goldens) at segment edges: the batch of tests/window_cases.py puts segment starts on
every residue of a lane and on both sides of every 128-, 512- and 1024-row boundary, with
segments shorter than, equal to and longer than every window depth and look-ahead used here.
tests/test_windows_host.py asserts those conditions on the inputs.

No row and no column is left out.  Ids, one-hots, bitmaps, labels and goal scores are bit-exact;
so are the f64 feature columns that are not angles and the f64 and f32 formula
(golden_io.assert_same_floats); the angle columns lie within value_cases.ANGLE_ULPS ulps of the
200-bit value (one more against a golden of the reference).

The instantiations ``launch_features`` can reach, SPADL and atomic each -- its flag dispatch
excludes every other combination at compile time (EXPLICIT never with BITS or WIDE; TAIL, N32 and
COND only windowed with KF = 3 and one at a time; TAIL only SPADL), so no other kernel exists --
and the test here that checks them against the oracle or the reference:

==========================================================  =====================================
``bool_colgroup_kernel<A, EXPLICIT, BITS, WIDE>``
----------------------------------------------------------  -------------------------------------
windowed, k <= 9                                            test_feature_blocks_vs_oracle
windowed, WIDE (k >= 10)                                    test_feature_blocks_vs_oracle
BITS, k <= 9                                                test_bool_bitmaps_vs_oracle (3, 9)
BITS, WIDE                                                  test_bool_bitmaps_vs_oracle (10, 12, 17)
EXPLICIT                                                    test_explicit_frames_*
``num_features_kernel<A, EXPLICIT, KF, TAIL, N32, COND>``
----------------------------------------------------------  -------------------------------------
KF = 3 (k <= 3)                                             test_feature_blocks_vs_oracle
KF = 0 (k >= 4)                                             test_feature_blocks_vs_oracle
EXPLICIT                                                    test_explicit_frames_*, the public
                                                            transformers on 9 and 17 frames
TAIL (SPADL)                                                test_step_vs_oracle
N32                                                         test_float32_and_condition_forms
``num_cond_lds_kernel<A>`` (COND, tables staged in LDS)     test_float32_and_condition_forms
==========================================================  =====================================

Not here: COND with its tables in global memory needs thousands of numeric conditions, which
tests/test_gpu_tree_boundaries.py::test_condition_tables_in_global_memory checks against the
oracle; the chunked TAIL launches are a benchmark probe that tests/test_gpu_parity.py compares
with the step checked here.  There is no atomic TAIL kernel: ``sa_vaep_step_f64`` gives atomic
actions the separate launches, which test_step_vs_oracle checks through the same call.
"""
import numpy as np
import pytest

import value_cases as vc
import window_cases as wc
from golden_io import assert_same_floats
from oracle import vaep_oracle as vo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

PACKAGES = [False, True]
LAYOUTS = ((None, None), (wc.BOOL_TILE, wc.SEG_BLOCK))  # plain, tiled (1024 / 128)
VALUES = ('offensive_value', 'defensive_value', 'vaep_value')
LABELS = ('scores', 'concedes', 'goal_from_shot')
_DTYPES = {'b': np.bool_, 'f': np.float64, 'i': np.int64}


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, batch, catalog, ops, trees
    _native.load_library()
    return dict(batch=batch, catalog=catalog, ops=ops, trees=trees)


def _xfns(atomic):
    return vo.ATOMIC_DEFAULT if atomic else vo.SPADL_DEFAULT


_BATCHES = {}
_REFS = {}
_LABELS = {}


def _batch(sa, atomic, strings=False):
    """The edge batch on the device: from flat columns, or from the string-team DataFrame."""
    key = (atomic, strings)
    if key not in _BATCHES:
        B = sa['batch']
        if strings:
            df, homes = wc.frame(atomic)
            ab = B.ActionBatch.from_frame(df, atomic=atomic, home_team_id=homes, segments='game')
        else:
            ab = B.ActionBatch.from_columns({c: v.copy() for c, v in wc.batch(atomic).items()},
                                            atomic=atomic)  # the cached batch is read-only
        d = wc.batch(atomic)
        assert ab.n == int(d['game_off'][-1]) and ab.n_segments == len(d['game_off']) - 1
        _BATCHES[key] = ab
    return _BATCHES[key]


def _stack(cols, exact):
    """Oracle columns -> (names, kinds, {kind: [n_cols, n] matrix}, exact angles) in the oracle's
    order; ``exact`` = the 200-bit angle columns by name, or None when the columns are a golden."""
    mats = {}
    for kind in 'bfi':
        sel = [v for _, kk, v in cols if kk == kind]
        mats[kind] = np.stack(sel).astype(_DTYPES[kind]) if sel else None
    return [c[0] for c in cols], [c[1] for c in cols], mats, exact


def _frames_ref(frames, atomic, seg_off=None):
    """The oracle's features of a list of game-state frames and their 200-bit angles."""
    return _stack(vo.features_frames(frames, _xfns(atomic), atomic, seg_off=seg_off),
                  vc.exact_angles_frames(frames, atomic))


def _ref(atomic, k):
    """The oracle's features of the edge batch at depth k: computed once, never modified."""
    if (atomic, k) not in _REFS:
        d = wc.batch(atomic)
        W = vo.windows(wc.cols_of(d, atomic), k, atomic, d['game_off'], d['home_team_id'])
        _REFS[atomic, k] = _frames_ref(W, atomic, d['game_off'])
    return _REFS[atomic, k]


def _ref_labels(atomic, nr):
    if (atomic, nr) not in _LABELS:
        d = wc.batch(atomic)
        _LABELS[atomic, nr] = vo.labels(wc.cols_of(d, atomic), atomic=atomic, nr_actions=nr,
                                        seg_off=d['game_off'])
    return _LABELS[atomic, nr]


def _check_blocks(fb, ref, tag, kinds='bfi'):
    """Every column of the blocks ``kinds`` of ``fb``, every row, against stacked oracle columns."""
    names, rkinds, mats, exact = ref
    assert fb.plan.names == names, tag
    assert [kk for _, kk, _ in fb.plan.order] == rkinds, tag
    for kind in kinds:
        idx = [col for _, kk, col in fb.plan.order if kk == kind]
        if mats[kind] is None:
            assert not idx
            continue
        got = fb.block(kind)[idx].cpu().numpy()
        assert got.shape == mats[kind].shape, (tag, kind)
        if kind == 'f':
            fnames = [nm for nm, kk in zip(names, rkinds) if kk == 'f']
            if exact is None:
                vc.golden_angle_columns(fnames, got, mats[kind], f'{tag} f64 block')
            else:
                vc.check_float_columns(fnames, got, mats[kind], exact, f'{tag} f64 block')
        else:
            np.testing.assert_array_equal(got.astype(np.int64), mats[kind].astype(np.int64),
                                          err_msg=f'{tag} {kind} block')


def _check_bits(fb, ref, n, tag):
    """The bitmaps of ``fb`` unpacked == the oracle's bool columns; rows >= n are clear."""
    bits = fb.bool_bits.cpu().numpy().view(np.uint8)
    unpacked = np.unpackbits(bits, axis=1, bitorder='little')
    idx = [col for _, kk, col in fb.plan.order if kk == 'b']
    np.testing.assert_array_equal(unpacked[idx, :n].astype(bool), ref[2]['b'], err_msg=tag)
    assert not unpacked[:, n:].any(), tag


def _check_labels(lb, ref, n, tag, names=LABELS):
    for c in names:
        got = getattr(lb, c)[:n].cpu().numpy()
        assert set(np.unique(got).tolist()) <= {0, 1}, (tag, c)
        np.testing.assert_array_equal(got.astype(bool), ref[c], err_msg=f'{tag} {c}')


def _check_values(v, ref, n, dtype, tag):
    v = v.cpu().numpy()[:, :n]
    for r, c in enumerate(VALUES):
        assert ref[c].dtype == dtype
        # the reference's IEEE operations in its order, f32 and f64 alike: bit-exact, -0.0 included
        assert_same_floats(v[r], ref[c], f'{tag} {c}')


def _probs(sa, atomic, dtype):
    """(numpy ps, pc, the oracle's formula, aligned device ps, pc) of the edge batch."""
    d = wc.batch(atomic)
    ab = _batch(sa, atomic)
    ps, pc = wc.probabilities(ab.n, dtype)
    fo = vo.formula(wc.cols_of(d, atomic), ps, pc, atomic=atomic, seg_off=d['game_off'])
    return ps, pc, fo, torch.from_numpy(ps).to(ab.device), torch.from_numpy(pc).to(ab.device)


# ------------------------------------------------------------------ bool and numeric blocks
@pytest.mark.parametrize('k', wc.KS)
@pytest.mark.parametrize('atomic', PACKAGES)
def test_feature_blocks_vs_oracle(sa, atomic, k):
    """sa_vaep_features on the edge batch == the oracle, SPADL and atomic, at every depth where
    the passes change: the register windows (k <= 3), the per-window row loads of the numeric pass
    (k >= 4), the last halo-resident depth of the bool pass (k = 9), its per-action gathers
    (k >= 10) and distances past the 4-bit field (k >= 17); plain and tiled layouts; the batch
    built from flat columns and from the DataFrame with string team ids."""
    ops = sa['ops']
    ref = _ref(atomic, k)
    for strings in (False, True):
        ab = _batch(sa, atomic, strings)
        for Rb, Rn in LAYOUTS:
            fb = ops.features(ab, _xfns(atomic), k, bool_tile=Rb, num_tile=Rn)
            if Rb is not None:
                assert fb.bool_block.shape[0] == -(-ab.n // Rb) > 1
                assert fb.f64_block.shape[0] == -(-ab.n // Rn) > 1
            _check_blocks(fb, ref, f'atomic={atomic} k={k} strings={strings} tiles={Rb}/{Rn}')


# ------------------------------------------------------------------ bitmaps
@pytest.mark.parametrize('k', wc.BITMAP_KS)
@pytest.mark.parametrize('atomic', PACKAGES)
def test_bool_bitmaps_vs_oracle(sa, atomic, k):
    """sa_vaep_features_bits (the BITS forms of the bool pass, WIDE from k = 10): the unpacked
    bits == the oracle's bool columns, rows >= n are clear, and the numeric blocks are the ones
    of the plain call, which equal the oracle."""
    ops = sa['ops']
    ab = _batch(sa, atomic)
    ref = _ref(atomic, k)
    assert ab.n % 64
    got = ops.features(ab, _xfns(atomic), k, num_tile=wc.SEG_BLOCK, bool_bits=True)
    assert got.bool_block is None and got.bool_bits.shape[0] == got.plan.n_bool
    _check_bits(got, ref, ab.n, f'atomic={atomic} k={k} bitmaps')
    _check_blocks(got, ref, f'atomic={atomic} k={k} bitmap form', kinds='fi')
    plain = ops.features(ab, _xfns(atomic), k, num_tile=wc.SEG_BLOCK)
    for kind in 'fi':
        assert torch.equal(got.block(kind), plain.block(kind)), kind


# ------------------------------------------------------------------ float32 and condition forms
@pytest.mark.parametrize('atomic', PACKAGES)
def test_float32_and_condition_forms(sa, atomic):
    """k = 3 on the edge batch: the bitmap form's blocks == the oracle; ``num32=True`` == the
    ORACLE's f64 / i64 columns cast to float32 (angles: the float32 bracket of the 200-bit value
    +- ANGLE_ULPS float64 ulps) and, second, the device's own f64 / i64 blocks cast down, with the
    same bitmaps; and trees.predict_pair_conditions
    (the COND numeric pass + the staged walk over condition bitmaps) of two small xgboost-shaped
    learners == each learner's staged walk over the checked blocks, bit for bit."""
    ops, trees = sa['ops'], sa['trees']
    ab = _batch(sa, atomic)
    ref = _ref(atomic, 3)
    chk = ops.features(ab, _xfns(atomic), 3, num_tile=wc.SEG_BLOCK, bool_bits=True)
    _check_bits(chk, ref, ab.n, f'atomic={atomic} bitmaps')
    _check_blocks(chk, ref, f'atomic={atomic} bitmap form', kinds='fi')
    got = ops.features(ab, _xfns(atomic), 3, num_tile=wc.SEG_BLOCK, bool_bits=True, num32=True)
    assert got.num32 and not chk.num32
    assert torch.equal(got.bool_bits, chk.bool_bits)
    names, rkinds, mats, exact = ref
    for kind in 'fi':
        assert got.block(kind).dtype == torch.float32
        idx = [col for _, kk, col in got.plan.order if kk == kind]
        g32 = got.block(kind)[idx].cpu().numpy()
        want = mats[kind].astype(np.float32)
        if kind == 'f':
            vc.check_float_columns([nm for nm, kk in zip(names, rkinds) if kk == 'f'], g32, want,
                                   exact, f'atomic={atomic} float32 block')
        else:
            assert_same_floats(g32, want, f'atomic={atomic} float32 integer columns')
        assert torch.equal(got.block(kind), chk.block(kind).to(torch.float32)), kind
    kinds = [kk for _, kk, _ in chk.plan.order]
    models = [trees.TreeEnsemble.from_model(trees.synthetic_xgboost_json(
        len(kinds), n_trees=12, depth=3, seed=sd, feature_kinds=kinds)) for sd in (51, 52)]
    pair = trees.predict_pair_conditions(ab, chk.plan, models)
    for m, p in zip(models, pair):
        want = m.predict_blocks(chk, method='staged')
        assert torch.equal(p, want)
        assert float(want.min()) < float(want.max())


# ------------------------------------------------------------------ labels
@pytest.mark.parametrize('atomic', PACKAGES)
def test_labels_vs_oracle(sa, atomic):
    """sa_vaep_labels and sa_vaep_labels_formula == the oracle at every nr_actions around the
    step's limit (11 -> 12) and the change of algorithm in labels_rows (17 -> 18), on a batch in
    which every seventh game has three teams (the full-compare branch on valid rows)."""
    ops = sa['ops']
    ab = _batch(sa, atomic)
    n = ab.n
    _, _, fo, tps, tpc = _probs(sa, atomic, np.float64)
    for nr in wc.NR_ACTIONS:
        ref = _ref_labels(atomic, nr)
        _check_labels(ops.labels(ab, nr_actions=nr), ref, n, f'labels atomic={atomic} nr={nr}')
        lf, vf = ops.labels_formula(ab, tps, tpc, nr_actions=nr)
        _check_labels(lf, ref, n, f'labels_formula atomic={atomic} nr={nr}')
        _check_values(vf, fo, n, np.float64, f'labels_formula atomic={atomic} nr={nr}')


# ------------------------------------------------------------------ fused step
@pytest.mark.parametrize('k', wc.STEP_KS)
@pytest.mark.parametrize('atomic', PACKAGES)
def test_step_vs_oracle(sa, atomic, k):
    """sa_vaep_step_f64 (SPADL: labels + f64 formula inside the numeric pass, TAIL; atomic: the
    separate launches behind the same entry point) == the oracle directly: features, labels and
    formula, with probabilities and without, both layouts, nr_actions up to the step's limit; the
    xT cell codes == sa_xt_cells."""
    ops = sa['ops']
    ab = _batch(sa, atomic)
    n = ab.n
    ref = _ref(atomic, k)
    _, _, fo, tps, tpc = _probs(sa, atomic, np.float64)
    plan = ops.build_plan(_xfns(atomic), k, atomic)
    cells_ref = None if atomic else ops.xt_cell_codes(ops.xt_cells(ab, 16, 12), n, 16, 12)
    ld = -(-n // wc.LANE_ACTS) * wc.LANE_ACTS
    for Rb, Rn in LAYOUTS:
        for nr in wc.STEP_NR:
            lref = _ref_labels(atomic, nr)
            for with_p in (True, False):
                tag = f'step atomic={atomic} k={k} nr={nr} tiles={Rb}/{Rn} probabilities={with_p}'
                out = ops.alloc_feature_blocks(plan, n, ab.device, Rb, Rn)
                buf = torch.full((3, ld), 7, dtype=torch.uint8, device=ab.device)
                lab = ops.LabelBlocks(n, buf[0], buf[1], buf[2])
                val = torch.full((3, ld), float('nan'), dtype=torch.float64, device=ab.device) \
                    if with_p else None
                cells = None if atomic else ops.xt_cells_buffer(n, ab.device)
                ops.step_into(ab.struct(), out, tps if with_p else None, tpc if with_p else None,
                              nr, lab, val, xt_cells=None if atomic else (16, 12, cells))
                _check_blocks(out, ref, tag)
                _check_labels(lab, lref, n, tag)
                if with_p:
                    _check_values(val, fo, n, np.float64, tag)
                if not atomic:
                    assert torch.equal(ops.xt_cell_codes(cells, n, 16, 12), cells_ref), tag


# ------------------------------------------------------------------ formula alignment
def _misaligned(t):
    """The same values as a contiguous view that is element- but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:]
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size() and t.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('atomic', PACKAGES)
def test_formula_scalar_path(sa, atomic, dtype):
    """Probabilities that are not 16-byte aligned (``vec_ok`` false: the scalar loads of
    formula_vals) through sa_vaep_formula, sa_vaep_labels_formula and, in f64, the fused
    step == the oracle, and == the aligned call bit for bit."""
    ops = sa['ops']
    ab = _batch(sa, atomic)
    n = ab.n
    _, _, fo, tps, tpc = _probs(sa, atomic, dtype)
    ups, upc = _misaligned(tps), _misaligned(tpc)
    tag = f'atomic={atomic} {np.dtype(dtype).name}'
    a = ops.formula(ab, tps, tpc)
    for ps, pc in ((ups, upc), (ups, tpc), (tps, upc)):
        u = ops.formula(ab, ps, pc)
        _check_values(u, fo, n, dtype, f'formula {tag}')
        assert torch.equal(u[:, :n], a[:, :n])
    _check_values(a, fo, n, dtype, f'formula aligned {tag}')
    for nr in (10, wc.LABELS_WINDOW + 1):
        lref = _ref_labels(atomic, nr)
        la, va = ops.labels_formula(ab, tps, tpc, nr_actions=nr)
        lu, vu = ops.labels_formula(ab, ups, upc, nr_actions=nr)
        _check_labels(lu, lref, n, f'labels_formula {tag} nr={nr}')
        _check_values(vu, fo, n, dtype, f'labels_formula {tag} nr={nr}')
        assert torch.equal(vu[:, :n], va[:, :n])
        for c in LABELS:
            assert torch.equal(getattr(lu, c)[:n], getattr(la, c)[:n])
    if dtype != np.float64:
        return  # the fused step takes f64 probabilities only
    plan = ops.build_plan(_xfns(atomic), 3, atomic)
    ld = -(-n // wc.LANE_ACTS) * wc.LANE_ACTS
    vals = []
    for ps, pc in ((tps, tpc), (ups, upc)):
        out = ops.alloc_feature_blocks(plan, n, ab.device, wc.BOOL_TILE, wc.SEG_BLOCK)
        buf = torch.full((3, ld), 7, dtype=torch.uint8, device=ab.device)
        lab = ops.LabelBlocks(n, buf[0], buf[1], buf[2])
        val = torch.full((3, ld), float('nan'), dtype=torch.float64, device=ab.device)
        ops.step_into(ab.struct(), out, ps, pc, 10, lab, val)
        _check_blocks(out, _ref(atomic, 3), f'step {tag}')
        _check_labels(lab, _ref_labels(atomic, 10), n, f'step {tag}')
        _check_values(val, fo, n, dtype, f'step {tag}')
        vals.append(val)
    assert torch.equal(vals[0][:, :n], vals[1][:, :n])


# ------------------------------------------------------------------ explicit frames
@pytest.mark.parametrize('atomic', PACKAGES)
def test_explicit_frames_goldens(sa, atomic):
    """ops.features_explicit on the golden frames (frames that are no shifts of one another) ==
    the reference's own transformers on them, as built and after its play_left_to_right."""
    B, ops = sa['batch'], sa['ops']
    g = wc.explicit_golden(atomic)
    for tag in ('plain', 'ltr'):
        frames = wc.golden_frames(g, tag, atomic)
        fb = ops.features_explicit(B.frames_batches(frames, atomic=atomic), _xfns(atomic))
        names, kinds = list(g[f'{tag}_names_all']), list(g[f'{tag}_kinds_all'])
        mats = {}
        for kind in 'bfi':
            m = g[f'{tag}_feat_{kind}']
            mats[kind] = np.ascontiguousarray(m.T.astype(_DTYPES[kind])) if m.shape[1] else None
        # the golden's blocks hold each kind's columns in frame order: so does _stack
        order = {kind: [nm for nm, kk in zip(names, kinds) if kk == kind] for kind in 'bfi'}
        for kind in 'bfi':
            assert order[kind] == list(g[f'{tag}_names_{kind}'])
        _check_blocks(fb, (names, kinds, mats, None), f'explicit golden atomic={atomic} {tag}')


@pytest.mark.parametrize('k', wc.EXPLICIT_KS)
@pytest.mark.parametrize('atomic', PACKAGES)
def test_explicit_frames_vs_oracle(sa, atomic, k):
    """The EXPLICIT instantiations on permuted frames (frame i's team, time and coordinates differ
    from frame 0's at almost every row) == oracle.features_frames, at lengths around a lane and
    past one bool tile, up to the most frames one launch takes."""
    B, ops = sa['batch'], sa['ops']
    for n in wc.EXPLICIT_NS:
        frames = wc.permuted_frames(n, k, atomic)
        ref = _frames_ref(wc.frame_cols(frames, atomic), atomic)
        fb = ops.features_explicit(B.frames_batches(frames, atomic=atomic), _xfns(atomic))
        assert fb.n == n
        _check_blocks(fb, ref, f'explicit atomic={atomic} k={k} n={n}')


@pytest.mark.parametrize('k,n', list(zip(wc.GROUPED_KS, (wc.EXPLICIT_NS[-1], wc.EXPLICIT_NS[3]))))
@pytest.mark.parametrize('atomic', PACKAGES)
def test_public_transformers_on_long_frame_lists(sa, atomic, k, n):
    """The public ``features.*`` transformers on permuted lists of more than SA_MAX_FRAMES frames
    (groups of frames per launch; a0 plus groups of the rest for team, time_delta and
    space_delta), concatenated over ``xfns_default`` == the oracle: names, dtypes and values."""
    import pandas as pd
    if atomic:
        from socceraction_amd.atomic.vaep import base, features as fs
    else:
        from socceraction_amd.vaep import base, features as fs
    assert [f.__name__ for f in base.xfns_default] == _xfns(atomic)
    frames = wc.permuted_frames(n, k, atomic)
    X = pd.concat([fn(frames) for fn in base.xfns_default], axis=1)
    ref = vo.features_frames(wc.frame_cols(frames, atomic), _xfns(atomic), atomic)
    assert list(X.columns) == [c[0] for c in ref]
    assert len(X) == n and X.index.equals(frames[0].index)
    for name, kind, v in ref:
        assert X[name].dtype == _DTYPES[kind], name
        if kind != 'f':
            np.testing.assert_array_equal(X[name].to_numpy(), v.astype(_DTYPES[kind]), err_msg=name)
    fnames = [name for name, kind, _ in ref if kind == 'f']
    vc.check_float_columns(fnames, np.stack([X[name].to_numpy() for name in fnames]),
                           np.stack([v for _, kind, v in ref if kind == 'f']),
                           vc.exact_angles_frames(wc.frame_cols(frames, atomic), atomic),
                           f'public transformers atomic={atomic} k={k}')
    for name in ('time', 'team', 'goalscore'):  # one transformer alone keeps its own columns
        one = getattr(fs, name)(frames)
        assert list(one.columns) == [c[0] for c in vo.features_frames(
            wc.frame_cols(frames, atomic), [name], atomic)]
