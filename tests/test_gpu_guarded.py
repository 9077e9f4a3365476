"""Every kernel family held to its own bytes (tests/guarded.py): each family's existing edge
inputs, every device input alone between two guard bands of poison, every allocation of the
call under test served poisoned and guarded, under the two fills ``0xFF`` (NaN / -1 / 255) and
``0x5A`` (huge finite / large positive / 90).

Every case asserts

a. the family's existing assertion against its reference (the helpers of the family's own test
   module are called as they stand), under both fills;
b. fill independence: the result bytes are the same under both fills, regions whose contents
   are contract included (the zero padding rows of ``select_rows``, the clear tail bits of
   bitmaps, whole accumulator buffers);
c. every guard band intact, for the allocations of the calls and for the rehomed inputs, checked
   when each call returns and again when the case ends (a consumer may stray into its producer);
d. the rehomed inputs unchanged, byte for byte;
e. at least one allocation intercepted in each guarded call.

What is produced under a fill is fed to its consumers under the same fill, each consumer held to
its own reference: blocks -> tree walks and select_rows (test_vaep_kernels, test_tree_inference,
test_select_rows); blocks and labels -> logistic moments, the learners' probabilities -> formula,
binary scores and grouped sums (test_chained_consumers).  What a producer leaves unwritten is live
poison for its consumer.  Where a builder's row count is even the case also
runs with the last row dropped, so end-of-column vector loads meet an odd n.

Each family's cases are a module-level generator ``cases_<family>(sa, ...)`` that yields
``(family, case)``; ``test_<family>`` runs every yielded ``case(run)`` through :func:`both_fills`,
and tests/test_gpu_streams.py drives the same closures through another runner.  The closures read
the generator's loop variables, so a consumer runs each case before it asks for the next.

Regions WITHOUT a contract -- compared up to ``n`` only; the chained consumers are the proof that
nothing reads them:

==========================================  =====================================================
region                                      why it has no contract
==========================================  =====================================================
rows >= n of the last tile of a byte,       the kernels write whole tiles where that is cheaper and
f64 / i64 / f32 feature block               leave the rest; every consumer takes ``n`` with the block
rows n .. ld - 1 of label, value, rate,     ``ld`` rounds the pitch to 16 rows for aligned stores;
cell-code and operand-code buffers, rows    the public views end at ``n`` (``out.n``)
>= ``out.n`` of converted columns
heat-map rows past ``n_iter``               ``XTSolution.heatmaps`` is the slice that was written
dense C x C transition table after          ``dense=False`` writes only the rows of bands holding
``xt_count_many(..., dense=False)``         a count >= 65535; ``acc.dense`` is False and every
                                            reader of the table refuses it (``require_dense``)
alignment gaps inside ``XTCounts.buf``      the parts are carved at 256-byte offsets and an
(so ``head`` of a fresh overwriting         overwriting count zeroes the error word only; no count
accumulator)                                or flag lives in the gaps
==========================================  =====================================================
"""
import copy
import dataclasses

import numpy as np
import pytest

import guarded as gd

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

COUNTS = {}  # family -> guarded allocations intercepted


@pytest.fixture(scope='module', autouse=True)
def interception_counts():
    """For the record (run with ``-s``): the guarded allocations per family of the cases that ran.
    Property (e) itself is asserted per call in :meth:`Run.call`."""
    yield
    if COUNTS:
        print('\nguarded allocations intercepted per family (both fills): '
              + ', '.join(f'{k}: {v}' for k, v in sorted(COUNTS.items())))


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, batch, catalog, linear, ops, synthetic, trees
    _native.load_library()
    return dict(native=_native, batch=batch, catalog=catalog, ops=ops, trees=trees, linear=linear,
                synthetic=synthetic, torch=torch)


class Run:
    """One pass of a case under one fill: the guarded calls, the rehomed inputs, the results
    whose bytes must not depend on the fill."""

    def __init__(self, family, fill):
        self.family, self.fill = family, fill
        self.arenas, self.handles, self.out = [], [], {}

    def call(self, fn, *args, **kw):
        """``fn(*args, **kw)`` with every allocation guarded and poisoned (c, e)."""
        with gd.guarded_allocations(self.fill) as arena:
            res = fn(*args, **kw)
        what = getattr(fn, '__qualname__', repr(fn))
        assert arena.count >= 1, f'{what}: no allocation was intercepted'
        COUNTS[self.family] = COUNTS.get(self.family, 0) + arena.count
        self.arenas.append(arena)
        return res

    def own(self, handle):
        self.handles.append(handle)
        return handle

    def home(self, a):
        """A host array or device tensor as a rehomed device input."""
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        arena = self.own(gd.Arena(self.fill))
        return arena.rehome(t.cuda())

    def batch(self, B, d, atomic=False, flip=True):
        ab = B.ActionBatch.from_columns({c: np.array(v) for c, v in d.items()}, atomic=atomic, flip=flip)
        self.own(gd.rehome_batch(ab, self.fill))
        return ab

    def keep(self, name, t):
        """A result whose bytes must be the same under both fills (b)."""
        if isinstance(t, torch.Tensor) and t.numel() * t.element_size() > 1 << 24:  # compared on the device
            t = t.detach().contiguous()
            self.out[name] = (str(t.dtype), tuple(t.shape), t.view(-1).view(torch.uint8))
            return
        if isinstance(t, torch.Tensor):
            t = t.detach().contiguous().cpu().numpy()
        self.out[name] = (str(np.asarray(t).dtype), np.asarray(t).shape, np.ascontiguousarray(t).tobytes())

    def keep_frame(self, name, df):
        """Every column of a host frame (object columns as strings)."""
        for c in df.columns:
            v = df[c].to_numpy()
            self.keep(f'{name} {c}', v.astype(str) if v.dtype == object else v)
        self.keep(f'{name} index', np.asarray(df.index))

    def finish(self):
        for a in self.arenas + self.handles:  # (c), (d): once more, after every consumer ran
            a.check()
        return self.out


def both_fills(family, case):
    """``case(run)`` under the two fills; the kept results are the same bytes."""
    outs = []
    for fill in gd.FILLS:
        run = Run(family, fill)
        case(run)
        outs.append(run.finish())
    a, b = outs
    assert list(a) == list(b) and a, family
    for k in a:
        assert a[k][:2] == b[k][:2], (family, k, a[k][:2], b[k][:2])
        if isinstance(a[k][2], torch.Tensor):
            if torch.equal(a[k][2], b[k][2]):
                continue
            x, y = (o[k][2].cpu().numpy() for o in outs)
        elif a[k][2] != b[k][2]:
            x, y = (np.frombuffer(o[k][2], np.uint8) for o in outs)
        else:
            continue
        at = int(np.flatnonzero(x != y)[0])
        raise AssertionError(f'{family}: {k} {a[k][0]} {a[k][1]} depends on the fill: '
                             f'{int((x != y).sum())} bytes differ, the first at byte {at}')


def drop_last(d, rows_key='type_id'):
    """Flat columns with the last row dropped (the last segment is longer than one row)."""
    n = len(d[rows_key])
    off = np.array(d['game_off'])
    assert off[-1] == n and off[-1] - off[-2] > 1
    out = {c: (v[:n - 1] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for c, v in d.items()}
    off[-1] = n - 1
    out['game_off'] = off
    return out


# =============================================================================== VAEP kernels
def _cut_ref(ref, n):
    """A stacked feature reference restricted to the first n rows (features look backwards)."""
    names, kinds, mats, exact = ref
    return (names, kinds, {k: (None if m is None else m[:, :n]) for k, m in mats.items()},
            None if exact is None else {k: v[:n] for k, v in exact.items()})


def cases_vaep_kernels(sa, atomic, drop):
    """sa_vaep.hip on the segment-edge batch of tests/window_cases.py (7190 rows; 7189 with the
    last row dropped): features in byte, bitmap and float32 forms at k = 3 and at ``BOOL_HALO + 2``
    (the wide bool pass), labels and labels + formula at nr_actions 10 and ``LABELS_WINDOW``, the
    formula in f64 and f32, the fused step at k = 3
    -- each against the oracle through the helpers of tests/test_gpu_windows.py.  The bitmap-form
    blocks then feed a small xgboost-shaped learner (staged walk, gather walk, condition bitmaps).
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import test_gpu_windows as tw
    import window_cases as wc
    from oracle import vaep_oracle as vo
    B, ops, trees = sa['batch'], sa['ops'], sa['trees']
    full = wc.batch(atomic)
    assert len(full['type_id']) % 2 == 0
    d = drop_last(full) if drop else full
    n = len(d['type_id'])
    xf = tw._xfns(atomic)
    refs = {k: _cut_ref(tw._ref(atomic, k), n) for k in (3, wc.BOOL_HALO + 2)}
    cols = wc.cols_of(d, atomic)
    lrefs = {nr: vo.labels(cols, atomic=atomic, nr_actions=nr, seg_off=d['game_off']) for nr in (10, wc.LABELS_WINDOW)}
    probs = {dt: wc.probabilities(n, dt) for dt in (np.float64, np.float32)}
    fos = {dt: vo.formula(cols, *probs[dt], atomic=atomic, seg_off=d['game_off']) for dt in probs}
    ld = -(-n // wc.LANE_ACTS) * wc.LANE_ACTS
    model = None

    def case(run):
        nonlocal model
        tag = f'atomic={atomic} n={n} fill={run.fill:#x}'
        ab = run.batch(B, d, atomic)
        assert ab.n == n
        for k, ref in refs.items():
            Rb, Rn = (wc.BOOL_TILE, wc.SEG_BLOCK) if k == 3 else (None, None)
            fb = run.call(ops.features, ab, xf, k, bool_tile=Rb, num_tile=Rn)
            tw._check_blocks(fb, ref, f'{tag} k={k} byte form')
            for kind in 'bfi':
                run.keep(f'k{k} {kind} block', fb.block(kind))
            bits = run.call(ops.features, ab, xf, k, num_tile=wc.SEG_BLOCK, bool_bits=True)
            tw._check_bits(bits, ref, n, f'{tag} k={k} bitmaps')
            tw._check_blocks(bits, ref, f'{tag} k={k} bitmap form', kinds='fi')
            run.keep(f'k{k} bitmaps', bits.bool_bits)  # whole words: the tail bits are clear by contract
            for kind in 'fi':
                assert torch.equal(bits.block(kind), fb.block(kind)), (tag, k, kind)
            if k == 3:
                b32 = run.call(ops.features, ab, xf, 3, num_tile=wc.SEG_BLOCK, bool_bits=True, num32=True)
                assert torch.equal(b32.bool_bits, bits.bool_bits), tag
                for kind in 'fi':
                    assert torch.equal(b32.block(kind), bits.block(kind).to(torch.float32)), (tag, kind)
                    run.keep(f'k3 {kind} float32', b32.block(kind))
                # consumers of the blocks made under this fill
                kinds = [kk for _, kk, _ in bits.plan.order]
                if model is None:
                    model = trees.synthetic_xgboost_json(len(kinds), n_trees=12, depth=3, seed=51, feature_kinds=kinds)
                te = trees.TreeEnsemble.from_model(model)
                want = te.predict_blocks(fb, method='gather')  # the checked byte-form blocks
                te.predict_blocks(copy.copy(bits), method='staged')  # builds the cached staged tables
                run.own(gd.rehome_model(te, ab.device, run.fill))
                for blocks, method in ((bits, 'staged'), (b32, 'staged'), (bits, 'gather'), (fb, 'staged')):
                    got = run.call(te.predict_blocks, copy.copy(blocks), method=method)
                    assert torch.equal(got, want), (tag, method)
                pair = run.call(trees.predict_pair_conditions, ab, bits.plan, [te])
                assert torch.equal(pair[0], want) and float(want.min()) < float(want.max()), tag
                run.keep('learner on the blocks', want)
        for nr, lref in lrefs.items():
            lb = run.call(ops.labels, ab, nr_actions=nr)
            tw._check_labels(lb, lref, n, f'{tag} labels nr={nr}')
            tps, tpc = (run.home(p) for p in probs[np.float64])
            lf, vf = run.call(ops.labels_formula, ab, tps, tpc, nr_actions=nr)
            tw._check_labels(lf, lref, n, f'{tag} labels_formula nr={nr}')
            tw._check_values(vf, fos[np.float64], n, np.float64, f'{tag} labels_formula nr={nr}')
            for c in tw.LABELS:
                run.keep(f'nr{nr} {c}', getattr(lb, c)[:n])
                assert torch.equal(getattr(lf, c)[:n], getattr(lb, c)[:n]), (tag, c)
            run.keep(f'nr{nr} values', vf[:, :n])
        for dt in probs:
            tps, tpc = (run.home(p) for p in probs[dt])
            v = run.call(ops.formula, ab, tps, tpc)
            tw._check_values(v, fos[dt], n, dt, f'{tag} formula {np.dtype(dt).name}')
            run.keep(f'formula {np.dtype(dt).name}', v[:, :n])
        # the fused step: its buffers are the caller's, so the caller's are the guarded ones

        def step():
            plan = ops.build_plan(xf, 3, atomic)
            out = ops.alloc_feature_blocks(plan, n, ab.device, wc.BOOL_TILE, wc.SEG_BLOCK)
            buf = torch.empty((3, ld), dtype=torch.uint8, device=ab.device)
            lab = ops.LabelBlocks(n, buf[0], buf[1], buf[2])
            val = torch.empty((3, ld), dtype=torch.float64, device=ab.device)
            cells = None if atomic else ops.xt_cells_buffer(n, ab.device)
            ops.step_into(ab.struct(), out, tps, tpc, 10, lab, val, xt_cells=None if atomic else (16, 12, cells))
            return out, lab, val, cells
        tps, tpc = (run.home(p) for p in probs[np.float64])
        out, lab, val, cells = run.call(step)
        tw._check_blocks(out, refs[3], f'{tag} step')
        tw._check_labels(lab, lrefs[10], n, f'{tag} step')
        tw._check_values(val, fos[np.float64], n, np.float64, f'{tag} step')
        for kind in 'bfi':
            run.keep(f'step {kind} block', out.block(kind))
        run.keep('step values', val[:, :n])
        if not atomic:
            codes = ops.xt_cell_codes(cells, n, 16, 12)
            assert torch.equal(codes, ops.xt_cell_codes(run.call(ops.xt_cells, ab, 16, 12), n, 16, 12)), tag
            run.keep('step cell codes', codes)

    yield 'vaep', case


@pytest.mark.parametrize('drop', [0, 1], ids=['n_even', 'n_odd'])
@pytest.mark.parametrize('atomic', [False, True], ids=['spadl', 'atomic'])
def test_vaep_kernels(sa, atomic, drop):
    for family, case in cases_vaep_kernels(sa, atomic, drop):
        both_fills(family, case)


def cases_vaep_explicit_frames(sa, atomic):
    """The EXPLICIT instantiations: SA_MAX_FRAMES permuted frames of 1041 rows (one bool tile,
    one lane and one row), every frame's columns rehomed.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import test_gpu_windows as tw
    import window_cases as wc
    B, ops, N = sa['batch'], sa['ops'], sa['native']
    n, k = wc.EXPLICIT_NS[-1], N.SA_MAX_FRAMES
    assert n % 2 == 1
    frames = wc.permuted_frames(n, k, atomic)
    ref = tw._frames_ref(wc.frame_cols(frames, atomic), atomic)

    def case(run):
        abs_ = B.frames_batches(frames, atomic=atomic)
        for ab in abs_:
            run.own(gd.rehome_batch(ab, run.fill))
        fb = run.call(ops.features_explicit, abs_, tw._xfns(atomic))
        assert fb.n == n
        tw._check_blocks(fb, ref, f'explicit atomic={atomic} fill={run.fill:#x}')
        for kind in 'bfi':
            run.keep(f'{kind} block', fb.block(kind))

    yield 'vaep explicit', case


@pytest.mark.parametrize('atomic', [False, True], ids=['spadl', 'atomic'])
def test_vaep_explicit_frames(sa, atomic):
    for family, case in cases_vaep_explicit_frames(sa, atomic):
        both_fills(family, case)


# =============================================================================== producers into consumers
def cases_chained_consumers(sa, atomic, drop):
    """What a producer leaves unwritten is live poison for its consumer.  On the segment-edge
    batch, everything made under the fill: the k = 3 bitmap-form blocks and the labels feed the
    logistic moments (limb sums at beta = 0 == the oracle's integers over the oracle's own feature
    columns, the angle columns left out: they are held to ulps, not bits); the blocks feed two
    xgboost-shaped learners whose float32 probabilities feed the f32 formula (== the oracle's
    formula of those probabilities, bit for bit), the binary scores against the device labels
    (counts, Brier limbs and U2 == the integer restatements of tests/test_gpu_metrics.py) and,
    with the formula's values, the grouped sums by action type (== the integer restatement of
    tests/test_gpu_ratings.py).
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import linear_reference as lr
    import test_gpu_metrics as tm
    import test_gpu_ratings as tg
    import test_gpu_windows as tw
    import value_cases as vc
    import window_cases as wc
    from oracle import vaep_oracle as vo
    from test_ratings_host import py_quantize
    B, ops, trees, lin = sa['batch'], sa['ops'], sa['trees'], sa['linear']
    full = wc.batch(atomic)
    d = drop_last(full) if drop else full
    n = len(d['type_id'])
    cols = wc.cols_of(d, atomic)
    names, kinds, mats, _ = _cut_ref(tw._ref(atomic, 3), n)
    lref = vo.labels(cols, atomic=atomic, nr_actions=10, seg_off=d['game_off'])
    y = lref['scores'].astype(np.uint8)
    # the model's columns: 30 bool, the first 11 float columns that are no angles, 5 integer ones
    at, column = {'b': 0, 'f': 0, 'i': 0}, {}
    for nm, kk in zip(names, kinds):
        column[nm] = mats[kk][at[kk]].astype(np.float64)
        at[kk] += 1
    pick = [nm for nm, kk in zip(names, kinds) if kk == 'b'][:30] + \
        [nm for nm, kk in zip(names, kinds) if kk == 'f' and not vc.is_angle(nm)][:11] + \
        [nm for nm, kk in zip(names, kinds) if kk == 'i'][:5]
    X = np.column_stack([column[nm] for nm in pick])
    G = wc.N_TYPES[atomic]
    keys = np.asarray(d['type_id']).astype(np.int32)
    models = [trees.synthetic_xgboost_json(len(kinds), n_trees=12, depth=3, seed=sd, feature_kinds=kinds)
              for sd in (51, 52)]
    host = {}

    def case(run):
        tag = f'atomic={atomic} n={n} fill={run.fill:#x}'
        ab = run.batch(B, d, atomic)
        bits = run.call(ops.features, ab, tw._xfns(atomic), 3, num_tile=wc.SEG_BLOCK, bool_bits=True)
        lb = run.call(ops.labels, ab, nr_actions=10)
        tw._check_labels(lb, lref, n, tag)
        # features + labels -> logistic moments
        _, kc = lin.model_slots(bits, pick)
        col_exp = run.call(lin.column_exps, bits, kc, None)
        limbs, err = run.call(lin.moments_limbs, bits, kc, np.zeros(len(pick) + 1), lb.scores, None, col_exp, 1, 0)
        assert int(err.item()) == 0, tag
        if 'limbs' not in host:
            host['limbs'] = lr.moments_limbs_at_zero(X, y, None, lr.item_exps(col_exp, 1))
        assert limbs.cpu().numpy().tolist() == host['limbs'], tag
        run.keep('moment limbs', limbs)
        # features -> learners -> probabilities
        ps, pc = (run.call(trees.TreeEnsemble.from_model(m).predict_blocks, copy.copy(bits), method='staged')
                  for m in models)
        assert ps.dtype == torch.float32 and float(ps.min()) < float(ps.max())
        hps, hpc = ps.cpu().numpy(), pc.cpu().numpy()
        run.keep('p_scores', ps)
        run.keep('p_concedes', pc)
        # probabilities -> formula
        v = run.call(ops.formula, ab, ps, pc)
        fo = vo.formula(cols, hps, hpc, atomic=atomic, seg_off=d['game_off'])
        tw._check_values(v, fo, n, np.float32, f'{tag} formula of the learners')
        run.keep('values', v[:, :n])
        # probabilities + labels -> binary scores
        acc = run.call(ops.binary_metrics, lb.scores[:n], ps)
        h = acc.buf.cpu().tolist()
        dd = hps.astype(np.float64) - y
        key = hps.tobytes() + hpc.tobytes()  # the second fill gives the same probabilities: restated once
        if host.get('key') != key:
            host.update(key=key, brier=np.array([py_quantize(x, tm.BRIER_EXP) for x in (dd * dd).tolist()],
                                                np.int64).sum(axis=0),
                        vl=np.array([[py_quantize(x, 2) for x in fo[c].astype(np.float64).tolist()]
                                     for c in tw.VALUES], np.int64))
        brier, vl = host['brier'], host['vl']
        assert h[8] == 0 and h[:2] == [n, int(y.sum())] and h[2:5] == brier.tolist(), tag
        assert h[9] == tm.u2_reference(y, hps), tag
        want = tm.ref_log_loss(y, hps)
        assert abs(acc.finalize()['log_loss'] - want) <= 1e-12 * want, tag
        run.keep('scores', acc.buf)
        # values -> grouped sums by action type
        E = [2, 2, 2]
        sums = run.call(ops.group_sums, run.home(keys), [v[r, :n] for r in range(3)], G, scale_exp=E)
        sums.check_errors()
        want_l, want_c = tg.reference(keys, vl, 3, G)
        assert torch.equal(sums.limbs.cpu(), torch.from_numpy(want_l)), tag
        assert torch.equal(sums.count.cpu(), torch.from_numpy(want_c)), tag
        run.keep('group sums', sums.buf)

    yield 'chained', case


@pytest.mark.parametrize('drop', [0, 1], ids=['n_even', 'n_odd'])
@pytest.mark.parametrize('atomic', [False, True], ids=['spadl', 'atomic'])
def test_chained_consumers(sa, atomic, drop):
    for family, case in cases_chained_consumers(sa, atomic, drop):
        both_fills(family, case)


# =============================================================================== tree inference
def _rehome_cond_cache(run, te):
    """The device tables ``trees._conditions_prep`` cached on the first learner, rehomed."""
    cache = te._cond_cache
    arena = run.own(gd.Arena(run.fill))
    for k in ('fstart', 'istart', 'thr', 'dl'):
        cache[k] = arena.rehome(cache[k])
    cache['walks'] = [tuple(arena.rehome(t) if isinstance(t, torch.Tensor) else t for t in w)
                      for w in cache['walks']]


def cases_tree_inference(sa, config, drop):
    """sa_trees.hip and the condition passes on the boundary models of
    tests/tree_boundary_models.py (thresholds ON the batch, NaN coordinates, depths 1..5): the
    feature blocks are made under the fill, the model tables are rehomed, and the gather and the
    staged walks over tiled, plain and bitmap blocks and predict_pair_conditions equal the oracle
    at the bars of tests/test_gpu_tree_boundaries.py (float32 rtol 1e-6, float64 rtol 1e-12), on
    the whole batch and on the batch cut one row short (segments end at the cut).
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import test_gpu_tree_boundaries as tb
    import tree_boundary_models as bm
    from oracle import tree_oracle as to
    B, ops, trees = sa['batch'], sa['ops'], sa['trees']
    sa_tb = dict(batch=B, ops=ops, trees=trees, native=sa['native'])
    ctx = tb._ctx(sa_tb, config)
    atomic, k, xfns = tb.CONFIGS[config]
    n = ctx['ab'].n - drop  # the whole batch, or cut one row short: an even and an odd n
    d = tb._cut(ctx['d'], n) if drop else ctx['d']
    learners = [tb._boundary(sa_tb, ctx, t) for t in (37, 9)]
    L = learners[0]
    ref64 = to.predict_flat(L['model'].flat_le, L['model'].base_le, ctx['X'], False, np.float64)

    def case(run):
        tag = f'{config} n={n} fill={run.fill:#x}'
        ab = run.batch(B, d, atomic)
        assert ab.n == n
        blocks = {'plain': run.call(ops.features, ab, xfns, k),
                  'tiled': run.call(ops.features, ab, xfns, k, bool_tile=1024, num_tile=128),
                  'bits': run.call(ops.features, ab, xfns, k, num_tile=128, bool_bits=True),
                  'bits32': run.call(ops.features, ab, xfns, k, num_tile=128, bool_bits=True, num32=True)}
        for tname, ens, ref, rtol in (('xgboost', trees.TreeEnsemble.from_model(L['model'].json), L['ref32'], 1e-6),
                                      ('sklearn-rule', bm.ensemble_le(trees, L['model']), ref64, 1e-12)):
            lays = ['tiled', 'plain', 'bits'] + (['bits32'] if ens.f32 else [])
            for lay in lays:  # the first prediction of each kind builds the cached tables
                ens.predict_blocks(copy.copy(blocks[lay]), method='staged')
            run.own(gd.rehome_model(ens, ab.device, run.fill))
            for lay in lays:
                got = run.call(ens.predict_blocks, copy.copy(blocks[lay]), method='staged')
                tb._assert_close(got, ref[:n], rtol, f'{tag} {tname} staged {lay}')
                run.keep(f'{tname} staged {lay}', got)
            for lay in ('tiled', 'plain', 'bits'):
                got = run.call(ens.predict_blocks, copy.copy(blocks[lay]), method='gather')
                tb._assert_close(got, ref[:n], rtol, f'{tag} {tname} gather {lay}')
                run.keep(f'{tname} gather {lay}', got)
        tes = [trees.TreeEnsemble.from_model(q['model'].json) for q in learners]
        trees.predict_pair_conditions(ab, ctx['plan'], tes)  # builds the cached tables
        for te in tes:
            run.own(gd.rehome_model(te, ab.device, run.fill))
        _rehome_cond_cache(run, tes[0])
        pair = run.call(trees.predict_pair_conditions, ab, ctx['plan'], tes)
        for q, (lrn, got) in enumerate(zip(learners, pair)):
            tb._assert_close(got, lrn['ref32'][:n], 1e-6, f'{tag} conditions, learner {q}')
            run.keep(f'conditions learner {q}', got)

    yield 'trees', case


@pytest.mark.parametrize('drop', [0, 1], ids=['n', 'n_minus_1'])
@pytest.mark.parametrize('config', ['spadl_k3', 'atomic_k3'])
def test_tree_inference(sa, config, drop):
    for family, case in cases_tree_inference(sa, config, drop):
        both_fills(family, case)


# =============================================================================== select, top-k, sums, metrics, moments
def cases_select_rows(sa, variant):
    """sa_select.hip on the source of tests/test_gpu_select.py made under the fill: the row lists
    ``edges``, ``repeats``, ``m65`` and ``m0`` equal the numpy restatement byte for byte, zero
    padding rows ``m .. ld - 1`` and clear tail bits included; the selected blocks then feed the
    staged tree walk.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import test_gpu_select as ts
    from oracle import vaep_oracle as vo
    B, ops, syn, trees = sa['batch'], sa['ops'], sa['synthetic'], sa['trees']
    atomic = variant == 'atomic'
    d0 = syn.atomic_games(1, seed=5, mean_actions=1000.0) if atomic else syn.spadl_games(2, seed=5, mean_actions=500.0)
    n0 = len(d0['type_id'])
    xf = vo.ATOMIC_DEFAULT if atomic else vo.SPADL_DEFAULT
    for d in ([d0] if n0 % 2 else [d0, drop_last(d0)]):
        n = len(d['type_id'])

        def case(run):
            ab = run.batch(B, d, atomic)
            fb = run.call(ops.features, ab, xf, 3, num_tile=ts.TILE, bool_bits=True, num32=variant == 'f32')
            size = fb.f64_block.element_size()
            ts._int_view(fb.f64_block)[0, 0, 0] = ts.NAN_BITS[size]
            fb.f64_block[(n - 1) // ts.TILE, 1, (n - 1) % ts.TILE] = -0.0
            # the restatement reads whole tiles: the rows past n of the last tile are not part of it
            host = dict(f=fb.f64_block.cpu().numpy(), i=fb.i64_block.cpu().numpy(), bits=fb.bool_bits.cpu().numpy())
            run.own(gd.rehome_blocks(fb, run.fill))
            src = dict(fb=fb, n=n, host=host, frame=None)
            lists = ts._row_lists(n)
            kinds = [kk for _, kk, _ in fb.plan.order]
            te = trees.TreeEnsemble.from_model(trees.synthetic_xgboost_json(len(kinds), n_trees=12, depth=3, seed=52,
                                                                            feature_kinds=kinds))
            whole = te.predict_blocks(copy.copy(fb), method='staged')
            for which in ('edges', 'repeats', 'm65', 'm0'):
                rows = lists[which]
                got = run.call(ops.select_rows, fb, run.home(rows.astype(np.int64)))
                ts._check(src, got, rows)
                run.keep(f'{which} f', got.f64_block)
                run.keep(f'{which} i', got.i64_block)
                run.keep(f'{which} bits', got.bool_bits)
                if len(rows):
                    p = run.call(te.predict_blocks, got, method='staged')
                    assert torch.equal(p, whole[torch.from_numpy(rows.astype(np.int64)).cuda()]), which

        yield 'select', case


@pytest.mark.parametrize('variant', ['f64', 'f32', 'atomic'])
def test_select_rows(sa, variant):
    for family, case in cases_select_rows(sa, variant):
        both_fills(family, case)


def cases_top_rows(sa, f32):
    """sa_topk.hip: the tie-heavy pool column of 2 * CHUNK + 2 rows (and of one row fewer) with a
    keep mask, k = 7 and CHUNK + 3, both directions, against tests/top_rows_reference.py.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import test_gpu_top_rows as tt
    import top_rows_reference as tr
    ops = sa['ops']
    v0, keep0 = tr.pool_column(2 * tr.CHUNK + 2, f32)
    for v, keep in ((v0, keep0), (v0[:-1], keep0[:-1])):
        def case(run):
            dv, dkeep = run.home(v), run.home(keep)
            for k in (7, tr.CHUNK + 3):
                for largest in (True, False):
                    for mask, dmask in ((keep, dkeep), (None, None)):
                        rows, vals = run.call(tt.check, ops, v, k, mask, largest, dv=dv, dkeep=dmask)
                        run.keep(f'k={k} largest={largest} keep={mask is not None} rows', rows)
                        run.keep(f'k={k} largest={largest} keep={mask is not None} vals', vals)

        yield 'top-k', case


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_top_rows(sa, f32):
    for family, case in cases_top_rows(sa, f32):
        both_fills(family, case)


def cases_group_sums(sa, V, f32):
    """sa_group.hip at G = 40 (the ``skipped`` key pattern of tests/test_gpu_ratings.py: 40 groups,
    a fifth of the rows skipped) at 65 rows, one chunk and one row, and 5000 / 4999 rows: limbs
    and counts equal the integer restatement, finalize() the Python-integer rounding; the whole
    accumulator buffer is the same under both fills.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import test_gpu_ratings as tg
    ops = sa['ops']
    v, limbs = tg.values(f32)
    for n in (65, tg.CHUNK + 1, 5000, 4999):
        keys, G = tg.key_pattern('skipped', n, np.random.default_rng([n, V]))
        assert G == 40
        want_l, want_c = tg.reference(keys, limbs, V, G)

        def case(run):
            dk = run.home(keys)
            cols = [run.home(v[c, :n]) for c in range(V)]
            acc = run.call(ops.group_sums, dk, cols, G, scale_exp=tg.EXPS[:V])
            acc.check_errors()
            assert torch.equal(acc.limbs.cpu(), torch.from_numpy(want_l)), n
            assert torch.equal(acc.count.cpu(), torch.from_numpy(want_c)), n
            fin = run.call(acc.finalize)
            tg.check_finalize(acc, tg.EXPS[:V])
            run.keep('buf', acc.buf)
            run.keep('finalize', fin)

        yield 'group sums', case


@pytest.mark.parametrize('V,f32', [(8, False), (3, True)], ids=['8xf64', '3xf32'])
def test_group_sums(sa, V, f32):
    for family, case in cases_group_sums(sa, V, f32):
        both_fills(family, case)


def cases_binary_metrics(sa, f32):
    """sa_metrics.hip: the sums at one chunk and one row (4097) against the integer restatement
    and scikit-learn, and the exact AUROC count with 1025 minority keys of either class (one more
    than the LDS sample holds) at 5000 and 4999 rows.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import test_gpu_metrics as tm
    ops = sa['ops']
    y, p, limbs = tm.rows(f32)
    n = tm.CHUNK + 1

    def sums(run):
        acc = run.call(lambda: tm.new_acc(ops).add(run.home(y[:n]), run.home(p[:n])))
        h = acc.buf.cpu().numpy()
        assert h[8] == 0 and h[9] == 0 and h[:2].tolist() == [n, int(y[:n].sum())]
        assert h[2:5].tolist() == limbs[:n].sum(axis=0).tolist()
        res = acc.finalize()
        assert res['brier'] == tm.py_finalize(*h[2:5].tolist(), tm.BRIER_EXP) / n
        want = tm.ref_log_loss(y[:n], p[:n])
        assert abs(res['log_loss'] - want) <= 1e-12 * want
        run.keep('sums', acc.buf)

    yield 'metrics', sums
    for name in (f'm={tm.SAMPLE + 1}', f'm={tm.SAMPLE + 1}_negatives'):
        y0, p0 = tm.auc_case(name, f32)
        assert len(y0) % 2 == 0
        for ya, pa in ((y0, p0), (y0[:-1], p0[:-1])):
            def auc(run):
                acc = run.call(ops.binary_metrics, run.home(ya), run.home(pa))
                h = acc.buf.cpu().tolist()
                m, n_pos = len(ya), int(ya.sum())
                assert h[8] == 0 and h[:2] == [m, n_pos] and h[9] == tm.u2_reference(ya, pa), name
                res = acc.finalize()
                assert res['auroc'] == h[9] / (2 * n_pos * (m - n_pos))
                assert tm.ulps(res['auroc'], tm.roc_auc_score(ya, pa.astype(np.float64))) <= 2
                run.keep('auc', acc.buf)

            yield 'metrics', auc


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_binary_metrics(sa, f32):
    for family, case in cases_binary_metrics(sa, f32):
        both_fills(family, case)


def cases_logistic_moments(sa, cols):
    """sa_linear.hip on the blocks of tests/test_gpu_linear.py (129 rows in tiles of 16, poison in
    the tiles' padding and set tail bits) rehomed: the limb sums at beta = 0 equal the oracle's
    integers, the moments at a non-zero beta lie within that file's 1e-12 of each entry's sum of
    |terms|, and predict_blocks of a model with that beta (the kernel's last rows end inside a
    tile and a bitmap word) lies within that file's 4 ulps of the oracle's sigmoid in f64 and f32.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import linear_reference as lr
    import test_gpu_linear as tl
    lin = sa['linear']
    n = 129
    names = tl.SETS[cols]
    X, y, mask = tl._matrix(names, slice(0, n)), tl.Y[:n], tl._mask(n)
    shared = tl._blocks(sa, n)
    beta = tl._tail_beta(X)
    zero = np.zeros(len(names) + 1)
    rg, rH, rf, ag, aH, af = lr.moments(X, y, beta, mask, with_abs=True)
    want_p = lr.sigmoid_of(X, beta)
    assert want_p.min() < 0.01 and want_p.max() > 0.99  # both tails of the sigmoid

    def case(run):
        blocks = dataclasses.replace(shared)
        run.own(gd.rehome_blocks(blocks, run.fill))
        _, kc = lin.model_slots(blocks, names)
        dmask, dy = run.home(mask), run.home(y)
        col_exp = run.call(lin.column_exps, blocks, kc, dmask)
        tl._check_exps(X, mask, col_exp)
        limbs, err = run.call(lin.moments_limbs, blocks, kc, zero, dy, dmask, col_exp, 1, 0)
        assert int(err.item()) == 0
        got = limbs.cpu().numpy()
        assert got.shape == (lin.n_items(len(names)), 3)
        assert got.tolist() == lr.moments_limbs_at_zero(X, y, mask, lr.item_exps(col_exp, 1))
        run.keep('limbs at zero', limbs)
        loss_exp = lin.loss_exponent(beta, col_exp)
        limbs, err = run.call(lin.moments_limbs, blocks, kc, beta, dy, dmask, col_exp, loss_exp, 0)
        assert int(err.item()) == 0
        g, H, f = lin.finalize(limbs.cpu().numpy(), col_exp, loss_exp)
        assert (np.abs(g - rg) <= 1e-12 * ag).all() and (np.abs(H - rH) <= 1e-12 * aH).all()
        assert abs(f - rf) <= 1e-12 * af and np.array_equal(H, H.T)
        run.keep('limbs at beta', limbs)
        # sa_logit_predict of a model with that beta: 4 ulps of the oracle's sigmoid, as
        # tests/test_gpu_linear.py::test_predict_blocks
        model = lin.DeviceLogisticRegression()
        model.feature_names_in_ = np.array(names, dtype=object)
        model.coef_, model.intercept_ = beta[:-1].reshape(1, -1), beta[-1:]
        for dt, ndt in ((torch.float64, np.float64), (torch.float32, np.float32)):
            p = run.call(model.predict_blocks, blocks, dtype=dt)
            got = p.cpu().numpy()
            assert got.dtype == ndt and got.shape == (n,)
            assert tl._ulps(got, want_p.astype(ndt)).max() <= 4, ndt
            run.keep(f'predict {np.dtype(ndt).name}', p)

    yield 'logistic moments', case


@pytest.mark.parametrize('cols', ['xg46', 'vaep568'])
def test_logistic_moments(sa, cols):
    for family, case in cases_logistic_moments(sa, cols):
        both_fills(family, case)


# =============================================================================== xT
def _same_rate(got, ref, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    np.testing.assert_array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)], err_msg=what)


_XT = {}


def _xt_games(sa):
    if 'd' not in _XT:
        d = sa['synthetic'].spadl_games(30)
        _XT['d'] = d
        _XT['variants'] = [d] if len(d['type_id']) % 2 else [d, drop_last(d)]
    return _XT['variants']


def cases_xt_small_grids(sa, l, w):
    """sa_xt.hip on 30 synthetic games: count == xt_oracle's counts; the solve in both summation
    orders == xt_oracle.solve (bit for bit up to 1024 cells and in the reference's order; the
    reordered sums of the 1200-cell grid within the 1e-12 of tests/test_gpu_xt_large.py, same
    iteration count); the rate of the surface == xt_oracle.rate.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    from oracle import xt_oracle as xo
    from xt_count_checks import ref_counts, same_counts
    B, ops = sa['batch'], sa['ops']
    C = l * w
    for d in _xt_games(sa):
        ref = ref_counts(d, l, w)
        fit = xo.solve(xo.counts(d, l, w), l, w)
        rated = xo.rate(d, fit['xT'])

        def case(run):
            tag = f'{l}x{w} n={len(d["type_id"])} fill={run.fill:#x}'
            ab = run.batch(B, d)
            acc = run.call(ops.xt_count, ab, l, w)
            same_counts(sa, acc, ref, f'{tag} xt_count')
            run.keep('counts', acc.head)
            run.keep('transitions', acc.trans)
            for exact in (False, True):
                sol = run.call(ops.xt_solve, acc, exact_order=exact)
                assert sol.n_iter + 1 == len(fit['heatmaps']), tag
                m = sol.mats.cpu().numpy()
                for q, name in enumerate(('scoring_prob', 'shot_prob', 'move_prob')):
                    np.testing.assert_array_equal(m[q].reshape(w, l), fit[name], err_msg=f'{tag} {name}')
                heat = sol.heatmaps.cpu().numpy().reshape(-1, w, l)
                if exact or C <= 1024:
                    np.testing.assert_array_equal(heat, fit['heatmaps'], err_msg=tag)
                    np.testing.assert_array_equal(m[3].reshape(w, l), fit['xT'], err_msg=tag)
                else:
                    assert np.all(np.abs(heat - fit['heatmaps']) <= 1e-12 * np.abs(fit['heatmaps']) + 1e-300), tag
                if sol.trans_t is not None:
                    np.testing.assert_array_equal(sol.trans_t.cpu().numpy().T, fit['transition'], err_msg=tag)
                    run.keep(f'exact={exact} transition', sol.trans_t)
                run.keep(f'exact={exact} mats', sol.mats)
                run.keep(f'exact={exact} heatmaps', sol.heatmaps)
                if exact:
                    surface = sol.mats[3].reshape(w, l)
            got, err = run.call(ops.xt_rate, ab, surface, l, w)
            assert int(err.item()) == 0
            _same_rate(got.cpu().numpy(), rated, f'{tag} xt_rate')
            run.keep('rate', got)
            if C <= sa['native'].SA_XT_CELLS_MAX_C:
                cells = run.call(ops.xt_cells, ab, l, w)
                same_counts(sa, run.call(ops.xt_count_cells, cells, ab.n, l, w), ref, f'{tag} xt_count_cells')
                got, err = run.call(ops.xt_rate_cells, cells, ab.n, l, w, surface)
                _same_rate(got.cpu().numpy(), rated, f'{tag} xt_rate_cells')
                run.keep('rate from cells', got)
            if C <= 65535:
                codes = run.call(ops.xt_rate_codes_buffer, ab.n, ab.device)
                same_counts(sa, run.call(ops.xt_count, ab, l, w, codes=codes), ref, f'{tag} xt_count + codes')
                got, err = run.call(ops.xt_rate_codes, codes, ab.n, surface)
                _same_rate(got.cpu().numpy(), rated, f'{tag} xt_rate_codes')
                run.keep('rate from codes', got)

        yield 'xT small grids', case


@pytest.mark.parametrize('l,w', [(16, 12), (30, 20), (40, 30)])
def test_xt_small_grids(sa, l, w):
    for family, case in cases_xt_small_grids(sa, l, w):
        both_fills(family, case)


def cases_xt_large_grid(sa):
    """sa_xt_large.hip at 105 x 68: the band count with interpolated-rate operands and without
    the dense table (every buffer of the fit poisoned, the accumulator's counts included: the
    overwriting count never reads them), its compact rows == xt_oracle's counts; the solve in both
    orders against the sparse restatement of xt_oracle.solve (tests/xt_dispatch_cases.py); the
    interpolated rate from coordinates, from the operand codes and fused behind the solve ==
    xt_oracle.rate; at 120 x 68 the rate kernel that does not stage its tables in LDS.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import xt_dispatch_cases as dc
    from golden_io import assert_close
    from oracle import xt_oracle as xo
    from xt_count_checks import ref_counts
    B, ops = sa['batch'], sa['ops']
    l, w = 105, 68
    C = l * w
    for d in _xt_games(sa):
        n = len(d['type_id'])
        ref = ref_counts(d, l, w)
        idx, cnt = ref['trans']
        system = dict(shot=ref['shot'], goal=ref['goal'], move=ref['move'], rows=idx // C, cols=idx % C, vals=cnt)
        fit = dc.solve_sparse(system)
        surface = fit['xT'].reshape(w, l)
        rated = xo.rate(d, surface, use_interpolation=True)
        xs120 = np.random.default_rng(120).random((68, 120))
        rated120 = xo.rate(d, xs120, use_interpolation=True)

        def case(run):
            tag = f'105x68 n={n} fill={run.fill:#x}'
            ab = run.batch(B, d)
            ic = run.call(ops.xt_interp_codes_buffer, n, ab.device)
            acc = run.call(ops.xt_count_many, [ab], l, w, interp_codes=[ic], dense=False)
            assert not acc.dense and acc.compact is not None and int(acc.err.item()) == 0
            for name in ('shot', 'goal', 'move'):
                np.testing.assert_array_equal(getattr(acc, name).cpu().numpy(), ref[name], err_msg=f'{tag} {name}')
            gi, gc = ops.xt_transition_entries(acc)  # torch indexing only: nothing to guard
            np.testing.assert_array_equal(gi.cpu().numpy(), idx, err_msg=tag)
            np.testing.assert_array_equal(gc.cpu().numpy(), cnt, err_msg=tag)
            # (not ``acc.head``: the fresh overwriting accumulator zeroes its error word only, and
            # head spans the alignment gap behind the three vectors)
            run.keep('counts', torch.stack([acc.shot, acc.goal, acc.move]))
            run.keep('error word', acc.err)
            run.keep('row lengths', acc.compact[1])
            run.keep('operand codes', ic[:n])
            exact = run.call(ops.xt_solve, acc, transition=False, exact_order=True)
            assert exact.path == 'sequential' and exact.n_iter == fit['n_iter'], tag
            m = exact.mats.cpu().numpy()
            for q, name in enumerate(('scoring_prob', 'shot_prob', 'move_prob', 'xT')):
                np.testing.assert_array_equal(m[q], fit[name], err_msg=f'{tag} {name}')
            np.testing.assert_array_equal(exact.heatmaps.cpu().numpy(), fit['heatmaps'], err_msg=tag)
            fast = run.call(ops.xt_solve, acc, transition=False)
            assert fast.n_iter == fit['n_iter'], tag
            h = fast.heatmaps.cpu().numpy()
            assert np.all(np.abs(h - fit['heatmaps']) <= 1e-12 * np.abs(fit['heatmaps']) + 1e-300), tag
            for nm, sol in (('exact', exact), ('fast', fast)):
                run.keep(f'{nm} mats', sol.mats)
                run.keep(f'{nm} heatmaps', sol.heatmaps)
            xT = exact.mats[3].reshape(w, l)
            got, err = run.call(ops.xt_rate_interp, ab, xT, l, w)
            assert int(err.item()) == 0
            assert_close(got.cpu().numpy(), rated, f'{tag} xt_rate_interp')
            run.keep('rate', got)
            got2, err = run.call(ops.xt_rate_interp_codes, ic, n, xT, l, w)
            assert int(err.item()) == 0 and torch.equal(got2.view(torch.int64), got.view(torch.int64)), tag
            sol2, outs, err = run.call(ops.xt_fit_rate_interp_codes, acc, [ic], [n], exact_order=True)
            assert int(err.item()) == 0 and sol2.n_iter == exact.n_iter
            assert torch.equal(sol2.mats, exact.mats) and torch.equal(sol2.heatmaps, exact.heatmaps), tag
            assert torch.equal(outs[0].view(torch.int64), got.view(torch.int64)), tag
            grid = run.call(ops.xt_interp_grid, xT, l, w)
            got3, err = run.call(ops.xt_rate, ab, grid, 1050, 680)
            assert torch.equal(got3.view(torch.int64), got.view(torch.int64)), tag  # as xt_rate_interp's docstring says
            run.keep('interpolated grid', grid)
            got, err = run.call(ops.xt_rate_interp, ab, run.home(xs120), 120, 68)
            assert int(err.item()) == 0
            assert_close(got.cpu().numpy(), rated120, f'{tag} xt_rate_interp 120x68')
            run.keep('rate 120x68', got)

        yield 'xT large grid', case


def test_xt_large_grid(sa):
    for family, case in cases_xt_large_grid(sa):
        both_fills(family, case)


# =============================================================================== convert, dribbles
def _rehome_cols(run, cols):
    arena = run.own(gd.Arena(run.fill))
    for k in list(cols):
        cols[k] = arena.rehome(cols[k])


def cases_atomic_scan_tile(sa, what):
    """sa_atomic.hip one block past the scan's first tile (SA_ATOMIC_SCAN_TILE * 256 + 1 rows, odd):
    the device expansion of the rehomed frame, every output column and the row count against the
    oracle's output for the 30-game base, as tests/test_gpu_convert.py and test_gpu_dribbles.py
    compare it; the output columns are carved from one poisoned buffer and are the same bytes
    under both fills.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import convert_cases as cc
    import test_gpu_convert as tc
    import test_gpu_dribbles as td
    from oracle import atomic_convert_oracle as co
    from socceraction_amd.atomic.spadl import base as cb
    from socceraction_amd.spadl import base as sb
    N = sa['native']
    n = N.SA_ATOMIC_SCAN_TILE * N.SA_ATOMIC_BLOCK_ROWS + 1
    assert N.lib().sa_atomic_scratch_bytes(n) == (N.SA_ATOMIC_SCAN_TILE + 1 + 2) * 8
    t = cc.tiled(cc.tile_base(), n, co.convert_to_atomic if what == 'convert' else co.add_dribbles)
    if what == 'dribbles':
        for ref in (t.full, t.part):
            ref['src'] = cc.dribble_src(ref)

    def case(run):
        frame = cb.SpadlFrame.from_columns(t.cols)
        assert frame.n == n and 'order' not in frame.cols and (what != 'convert' or frame.keys is None)
        frame.cols['event'].copy_(torch.arange(n, dtype=torch.int32, device=frame.buffer.device))
        _rehome_cols(run, frame.cols)
        if what == 'convert':
            out = run.call(cb.convert_device, frame)
            cc.assert_tiled_on_device(t, out.cols, out.n, frame.uniques, tc.ATOMIC_DEVICE_COLS)
        else:
            out = run.call(sb.add_dribbles_device, frame, t.cols['action_id'])
            assert out.n_dribbles == out.n - n > 0
            cc.assert_tiled_on_device(t, out.cols, out.n, frame.uniques, td.SPADL_DEVICE_COLS)
        run.keep('rows out', np.int64(out.n))
        for c in sorted(out.cols):
            run.keep(c, out.cols[c][:out.n])

    yield 'convert / dribbles', case


@pytest.mark.parametrize('what', ['convert', 'dribbles'])
def test_atomic_scan_tile(sa, what):
    for family, case in cases_atomic_scan_tile(sa, what):
        both_fills(family, case)


def cases_convert_group_shapes(sa, layout):
    """convert_to_atomic on the enumeration of every group shape (tests/convert_cases.py: 152,352
    rows; one fewer; repeated keys through the general path) == the four-pass restatement, floats
    bit for bit, with every allocation of the public function poisoned and guarded.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import convert_cases as cc
    import pandas as pd
    import test_gpu_convert as tc
    from oracle import atomic_convert_oracle as co
    from socceraction_amd.atomic import spadl as aspadl
    f = cc.enum_frame()
    assert len(f['type_id']) % 2 == 0
    if layout == 'as_built_odd':
        f = {c: v[:-1] for c, v in f.items()}
    elif layout == 'duplicated_keys':
        f = cc.duplicated_keys(f)
    ref = co.convert_to_atomic(f)

    def case(run):
        out = run.call(aspadl.convert_to_atomic, pd.DataFrame(f))
        tc._assert_exact(tc._cols(out), ref, layout)
        run.keep_frame('atomic', out)

    yield 'convert / dribbles', case


@pytest.mark.parametrize('layout', ['as_built', 'as_built_odd', 'duplicated_keys'])
def test_convert_group_shapes(sa, layout):
    for family, case in cases_convert_group_shapes(sa, layout):
        both_fills(family, case)


def cases_add_dribbles_group_shapes(sa, layout):
    """_add_dribbles on the same enumeration == the restatement, every column bit for bit.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import convert_cases as cc
    import pandas as pd
    import test_gpu_dribbles as td
    from socceraction_amd.spadl import base as sb
    f = cc.enum_frame()
    if layout == 'per_game_ids_odd':
        f = {c: v[:-1] for c, v in f.items()}
    elif layout == 'global_ids':
        f = dict(f, action_id=np.arange(len(f['type_id']), dtype=np.int64))
    df = pd.DataFrame(f)

    def case(run):
        got = run.call(sb._add_dribbles, df.copy())
        assert len(got) > len(df) + 1000
        td._vs_oracle_exact(got, df, layout)
        run.keep_frame('with dribbles', got)

    yield 'convert / dribbles', case


@pytest.mark.parametrize('layout', ['per_game_ids', 'per_game_ids_odd', 'global_ids'])
def test_add_dribbles_group_shapes(sa, layout):
    for family, case in cases_add_dribbles_group_shapes(sa, layout):
        both_fills(family, case)


# =============================================================================== the learner
_TABLE = {}


def _table():
    """The 3,000-row table of tests/boost_shard_cases.py with its restated cuts and bins."""
    if not _TABLE:
        import boost_reference as br
        import boost_shard_cases as C
        X, y = C.table()
        cols = [X[c].to_numpy() for c in X.columns]
        cuts = [br.cuts_of(c, c.dtype == np.bool_) for c in cols]
        _TABLE.update(X=X, y=y, cols=cols, cuts=cuts,
                      B=np.stack([br.bins_of(br.cast32(c), k) for c, k in zip(cols, cuts)]))
    return _TABLE


def _binned(run, boost, X, y, rows=None):
    """The table binned under the fill, its device tensors rehomed, and the padded label column."""
    data = run.call(boost.bin_host, X, None, rows)
    arena = run.own(gd.Arena(run.fill))
    data.bits, data.bins = (None if t is None else arena.rehome(t) for t in (data.bits, data.bins))
    for k, t in list(data.dev.items()):
        if isinstance(t, torch.Tensor):
            data.dev[k] = arena.rehome(t)
    yh = np.zeros(data.ld, np.uint8)
    yh[:data.n] = y
    return data, run.home(yh)


def _keep_fit(run, clf):
    run.keep('trees', clf.trees_.view(np.uint8))
    run.keep('margin', clf.margin_)
    run.keep('p', clf.p_)
    run.keep('recorded p', clf.record_['p'])
    run.keep('recorded margin', clf.record_['margin'])


def cases_learner_plain_fit(sa):
    """sa_boost.hip: five rounds of depth 3 on the table, replayed round by round against
    tests/boost_reference.py (tests/test_gpu_boost.py::_replay: node tables and margins as bytes).
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import boost_reference as br
    import boost_shard_cases as C
    import test_gpu_boost as tgb
    from socceraction_amd import boost
    T = _table()
    params = {**br.DEFAULTS, **C.PLAIN['d3']}

    def case(run):
        data, yd = _binned(run, boost, T['X'], T['y'])
        clf = boost.DeviceGBTClassifier(record=True, **C.PLAIN['d3'])
        run.call(clf.fit_binned, data, yd)
        assert tgb._replay(clf, params, T['B'], T['y'], T['cuts']) >= params['n_estimators']
        _keep_fit(run, clf)

    yield 'learner', case


def test_learner_plain_fit(sa):
    for family, case in cases_learner_plain_fit(sa):
        both_fills(family, case)


def cases_learner_tuned_fit(sa):
    """Weights (the last row's lifts the quantisation shift), row and column samples and the L1
    penalty against tests/boost_sample_reference.py, as tests/test_gpu_boost_shard.py replays them.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import boost_reference as br
    import boost_sample_reference as bsr
    import boost_shard_cases as C
    from socceraction_amd import boost
    T = _table()
    params = {**bsr.DEFAULTS, **C.TUNED}
    y, w = T['y'], C.weights(T['y'])
    we = bsr.effective_weight(w, y, params['scale_pos_weight'])
    e = bsr.shift_of(we.max())
    keys = np.arange(C.N, dtype=np.int64)

    def case(run):
        data, yd = _binned(run, boost, T['X'], y)
        wh, _ = boost.check_weights(w, C.N, y, params['scale_pos_weight'])
        arena = run.own(gd.Arena(run.fill))
        wd = arena.rehome(boost.weights_to_device(wh, data.device))
        clf = boost.TunedGBTClassifier(record=True, **C.TUNED)
        run.call(clf.fit_binned, data, yd, sample_weight=wd)
        assert int(clf.quant_shift_) == e
        P, M = clf.record_['p'].cpu().numpy(), clf.record_['margin'].cpu().numpy()
        F, m = len(T['cuts']), np.full(C.N, br.base_margin(0.5), np.float32)
        for a, b in zip(clf.cuts_, T['cuts']):
            np.testing.assert_array_equal(a, b)
        for t in range(params['n_estimators']):
            np.testing.assert_allclose(P[t], br.probability(m), rtol=1e-6, atol=0)
            rows, cols = bsr.round_inputs(params, t, F, keys)
            gq, hq = bsr.quantise(P[t], y, we, e, rows)
            tab, node = bsr.build_tree(T['B'], gq, hq, T['cuts'], params, e, cols)
            assert tab.tobytes() == clf.trees_[t].tobytes(), t
            m = br.update_margin(m, tab, node)
            assert m.tobytes() == M[t].tobytes(), t
        assert (clf.trees_['feature'] >= 0).sum() >= params['n_estimators']
        _keep_fit(run, clf)

    yield 'learner', case


def test_learner_tuned_fit(sa):
    for family, case in cases_learner_tuned_fit(sa):
        both_fills(family, case)


def cases_learner_early_stopping(sa):
    """Early stopping by the log loss of held-out rows (the split of the two-rank case of
    tests/boost_shard_cases.py, on one device) against tests/boost_stop_reference.py: every
    round's tree, the metric integers within 1e-12, the stopping round, the kept model.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import boost_reference as br
    import boost_shard_cases as C
    import boost_stop_reference as bst
    from socceraction_amd import boost
    T = _table()
    y = T['y']
    train, ev = np.zeros(C.N, bool), []
    for (a, _), (tr, e) in zip(C.bounds(C.SHARDS[2]), C.stop_rows(y, C.SHARDS[2])):
        train[a + tr] = True
        ev.append(a + e)
    ev = np.concatenate(ev)
    tr_idx = np.flatnonzero(train)
    cuts = [br.cuts_of(c[train], c.dtype == np.bool_) for c in T['cols']]
    B = np.stack([br.bins_of(br.cast32(c), k) for c, k in zip(T['cols'], cuts)])
    params = {**br.DEFAULTS, **C.STOP}
    X32 = np.stack([br.cast32(c) for c in T['cols']], 1)
    alone = bst.fit(B, y, cuts, train, ev, 'logloss', C.STOP_ROUNDS, **C.STOP)

    def case(run):
        data, yd = _binned(run, boost, T['X'], y, rows=tr_idx)
        for a, b in zip(data.cuts, cuts):
            np.testing.assert_array_equal(a, b)
        clf = boost.DeviceGBTClassifier(record=True, early_stopping_rounds=C.STOP_ROUNDS, eval_metric='logloss',
                                        **C.STOP)
        run.call(clf.fit_binned, data, yd, rows=run.home(tr_idx), eval_rows=run.home(ev))
        best, ran = int(clf.best_iteration), int(clf.n_rounds_run_)
        series = [int(v) for v in clf.eval_sums_]
        P, EP = clf.record_['p'].cpu().numpy(), clf.record_['eval_p'].cpu().numpy()
        assert P.shape == (ran, C.N) and EP.shape == (ran, len(ev)) and len(series) == ran
        tabs = []
        for t in range(ran):
            gq, hq = br.quantise(P[t], y)
            tabs.append(br.build_tree(B, gq, hq, cuts, params, active=train)[0])
            want = bst.logloss_integer(y[ev], EP[t])
            assert abs(series[t] - want) <= 1e-12 * want, t
            assert clf.evals_result_['validation_0']['logloss'][t] == bst.metric_score(series[t], 'logloss', y[ev])
        assert (best, ran) == bst.stopping(series, C.STOP_ROUNDS, False)
        assert ran < C.STOP['n_estimators'] and ran == best + C.STOP_ROUNDS + 1
        assert len(clf.trees_) == best + 1
        for t in range(best + 1):
            assert tabs[t].tobytes() == clf.trees_[t].tobytes(), t
        np.testing.assert_allclose(EP[best], br.predict(clf.trees_, X32[ev]), rtol=1e-6, atol=0)
        assert (alone['best_iteration'], alone['rounds_run']) == (best, ran)
        run.keep('trees', clf.trees_.view(np.uint8))
        run.keep('recorded p', clf.record_['p'])
        run.keep('held-out p', clf.record_['eval_p'])
        run.keep('metric integers', np.array([str(v) for v in series]))

    yield 'learner', case


def test_learner_early_stopping(sa):
    for family, case in cases_learner_early_stopping(sa):
        both_fills(family, case)


# =============================================================================== pandas boundary, public path
def cases_pandas_boundary(sa, atomic, chunks):
    """pipeline.value_frames through compute_batch on the edge frame of tests/boundary_cases.py
    (string team ids, absent homes) at one-game chunks and at the default chunk size: features,
    labels and the f64 formula against the oracle as tests/test_gpu_boundary.py checks them, with
    every slot, staging buffer and batch of the pipeline poisoned (the pinned ones too).
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import boundary_cases as bc
    import test_gpu_boundary as tbd
    import window_cases as wc
    d = wc.batch(atomic)
    n = int(d['game_off'][-1])
    games, actions = bc.edge(atomic)
    ref, lab = tbd._edge_refs(atomic)
    ps, pc, fo = tbd._formula(d, atomic, np.float64)
    kw = dict(chunk_rows=bc.edge_chunk_rows(n)[0]) if chunks == 'one_game' else {}

    def case(run):
        model = tbd._model(atomic)
        out = run.call(model.compute_batch, games, actions, ps, pc, **kw)
        tbd._check_all(out, ref, lab, fo, n, atomic, np.float64, f'atomic={atomic} {chunks} fill={run.fill:#x}')
        for name, frame in zip(('features', 'labels', 'values'), out):
            run.keep_frame(name, frame)

    yield 'pandas boundary', case


@pytest.mark.parametrize('chunks', ['one_game', 'default'])
@pytest.mark.parametrize('atomic', [False, True], ids=['spadl', 'atomic'])
def test_pandas_boundary(sa, atomic, chunks):
    for family, case in cases_pandas_boundary(sa, atomic, chunks):
        both_fills(family, case)


def cases_public_path(sa):
    """fit_batch -> rate_batch -> score_batch -> rate_players -> top_actions on the nine small
    games of tests/boost_shard_cases.py, every call under the fill: each result is byte for byte
    the unguarded call's (the paths the other cases of this module and the existing suite hold
    to their oracles), and the same under both fills.
    Yields ``(family, case)``: run each case before asking for the next (module docstring)."""
    import json

    import boost_shard_cases as C
    from socceraction_amd.vaep import VAEP
    games, actions = C.games()

    def public(call):
        model = call(VAEP().fit_batch, games, actions, tree_params=C.BATCH)
        return dict(values=call(model.rate_batch, games, actions),
                    scores=call(model.score_batch, games, actions),
                    players=call(model.rate_players, games, actions),
                    top=call(model.top_actions, games, actions, k=7))

    plain = public(lambda fn, *a, **kw: fn(*a, **kw))
    assert len(plain['values']) == len(actions) and np.isfinite(plain['values']['vaep_value']).all()
    assert int(plain['players']['count'].sum()) == len(actions) and len(plain['top']) == 7
    for col in ('scores', 'concedes'):
        assert 0 < plain['scores'][col]['log_loss'] < 1

    def case(run):
        got = public(run.call)
        assert got['scores'] == plain['scores']
        for k in ('values', 'players', 'top'):
            assert list(got[k].columns) == list(plain[k].columns) and got[k].index.equals(plain[k].index), k
            for c in got[k].columns:
                a, b = got[k][c].to_numpy(), plain[k][c].to_numpy()
                assert (a.tobytes() == b.tobytes()) if a.dtype != object else (a == b).all(), (k, c)
            run.keep_frame(k, got[k])
        run.keep('scores', np.array(json.dumps(got['scores'], sort_keys=True)))

    yield 'public path', case


def test_public_path(sa):
    for family, case in cases_public_path(sa):
        both_fills(family, case)
