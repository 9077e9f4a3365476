"""The xT count, solve and rate kernels against the oracle on both sides of every dispatch edge.

The library picks its xT kernels from the cell count C = l * w, the action count and pointer
alignment.  tests/xt_dispatch_cases.py lists a grid on each side of every such edge (and
tests/test_xt_dispatch_host.py proves, by a sweep of C = 1 .. 46340 through ``sa_xt_count_mode``
and ``sa_xt_band_shape``, that none is missing); here each of them runs on the device:

* counts of coordinates on every cell edge +-2 ulp (threshold_cases.binning_batch) == xt_oracle,
  exactly, through every count entry point, with the mode of every grid asserted -- a threshold
  that moves fails here instead of silently un-covering a kernel;
* action counts around each count kernel's own chunking (one action, one workgroup's share +-1,
  one more than the grid covers in a pass), and a full 32768-action workgroup into ONE packed
  u16 transition bin of XC_SMALL, low and high half-word;
* the solve of systems written directly (xt_dispatch_cases.system: a row without transitions, a
  cell without shots, a 0 / 0 cell) == xt_oracle.solve bit for bit on the register and the
  one-workgroup kernel, == the sparse restatement of it above 1024 cells;
* the rate and band-count kernels' scalar loads (columns that start 8 bytes / 1 byte off
  alignment) and the persistent rate kernel's unrolled pass.

Every device result is compared with ``oracle/`` (or xt_dispatch_cases.solve_sparse, itself held
to the oracle on the CPU); a second device path is only ever an additional comparison.

That these tests bite was checked once with mutated builds of the library (value-changing edits
only), each run against this module in a process of its own; the unmutated library passes all 79
cases, in about 6 s together on one MI355X (no case above 0.4 s):

* ``row_payoff`` without its scalar tail: test_small_solve_vs_oracle fails at 193, 199, 1001 and
  1023 cells (1024 and the register kernel's grids pass);
* XC_SMALL's high half-word flushed to ``trans[2k]``: every XC_SMALL count fails -- the grids of
  195, 196 and 199 cells, the shared run at 194, all eight test_small_count_action_edges cases
  and the two odd-index cases of test_small_count_full_workgroup_into_one_bin;
* the scalar branch of ``xt_rate_kernel``, of ``xt_rate_interp_kernel`` and of
  ``rate_interp_pair`` with the end coordinates swapped, and the scalar branch of
  ``xt_keys_kernel`` reading every result as a failure: test_unaligned_columns_take_the_scalar_loads
  fails, at the rate, the interpolated rate and the band count respectively;
* the unrolled pass of ``xt_rate_interp_lds_kernel`` taking its second action's end x from the
  first: test_interp_rate_unrolled_pass_and_tail fails;
* count_mode's XC_WIDE budget at 149 KiB (194 cells turn to XC_SMALL): the CPU sweep and the
  table row of tests/test_xt_dispatch_host.py fail, as the mode assertion here would.
"""
import ctypes

import numpy as np
import pytest

import threshold_cases as tc
import xt_dispatch_cases as dc
from golden_io import assert_close
from oracle import xt_oracle as xo
from xt_count_checks import ref_counts, same_counts, same_counts_gathered

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROW_COLS = ('start_x', 'start_y', 'end_x', 'end_y', 'type_id', 'result_id', 'period_id', 'time_seconds',
            'team_id', 'bodypart_id')


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, batch, ops
    _native.load_library()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return dict(torch=torch, native=_native, batch=batch, ops=ops, cus=cus)


def _batch(sa, d):
    return sa['batch'].ActionBatch.from_columns(d)


def _tile(d, n):
    """The first n rows of the batch repeated for ever, as one game."""
    out = {c: np.resize(d[c], n) for c in ROW_COLS}
    out.update(game_off=np.array([0, n], np.int64), home_team_id=np.zeros(1, np.int64))
    return out


def _mode(sa, l, w, n, shared=False):
    return sa['native'].lib().sa_xt_count_mode(l, w, n, dc.SHARED if shared else 0)


# =============================================================================== counts
@pytest.mark.parametrize('l,w,mode', dc.COUNT_GRIDS)
def test_count_on_both_sides_of_every_edge(sa, l, w, mode):
    """Every count entry point on the grid's own edge values == xt_oracle's counts exactly, and
    the grid takes the count pass the table says."""
    ops, N = sa['ops'], sa['native']
    C = l * w
    if C == dc.MAX_CELLS and torch.cuda.mem_get_info()[0] < 32 << 30:
        pytest.skip('the 8.6 GB table of 46340 cells needs 32 GB of free device memory')
    d = tc.binning_batch(l, w)
    ab = _batch(sa, d)
    n = ab.n
    assert _mode(sa, l, w, n) == mode
    ref = ref_counts(d, l, w)
    assert len(ref['trans'][0]) > 30 and ref['shot'].sum() > 20
    check = same_counts if C <= 12000 else same_counts_gathered   # no search of a 0.58 / 8.6 GB table
    acc = ops.xt_count(ab, l, w)
    check(sa, acc, ref, 'xt_count')
    del acc
    if C <= 65535:
        acc = ops.xt_count(ab, l, w, codes=ops.xt_rate_codes_buffer(n, ab.device))
        check(sa, acc, ref, 'xt_count + codes')
        del acc
    acc = ops.xt_count_many([ab], l, w)
    check(sa, acc, ref, 'xt_count_many')
    del acc
    assert (ops.xt_band_shape(l, w) is None) == (C <= N.SA_XT_CELLS16_MAX_C or C > 12000)
    if C <= 199:
        assert _mode(sa, l, w, n, shared=True) == dc.SMALL
        check(sa, ops.xt_count(ab, l, w, shared=True), ref, 'xt_count shared')
    if C <= N.SA_XT_CELLS_MAX_C:
        cells = ops.xt_cells(ab, l, w)
        check(sa, ops.xt_count_cells(cells, n, l, w), ref, 'xt_cells + xt_count_cells')
        if C <= 199:
            check(sa, ops.xt_count_cells(cells, n, l, w, shared=True), ref, 'xt_count_cells shared')


def _count_n(sa, l, w, n, mode, cells=True):
    """The grid's edge batch tiled to n actions through the coordinate count (and the cell-code
    count) == the oracle's counts of those n actions."""
    ops = sa['ops']
    d = _tile(tc.binning_batch(l, w), n)
    ab = _batch(sa, d)
    assert ab.n == n and _mode(sa, l, w, n) == mode
    ref = ref_counts(d, l, w)
    check = same_counts if l * w <= 12000 else same_counts_gathered
    check(sa, ops.xt_count(ab, l, w), ref, f'xt_count n={n}')
    if cells:
        check(sa, ops.xt_count_cells(ops.xt_cells(ab, l, w), n, l, w), ref, f'xt_count_cells n={n}')


@pytest.mark.parametrize('n', [1, 3, 5, 4095, 4096, 4097, None])
def test_wide_count_action_edges(sa, n):
    """XC_WIDE (97 x 2): fewer actions than one pass of a thread, one workgroup's 4096 +-1, and
    one action more than 4096 per CU (every CU's chunk uneven)."""
    _count_n(sa, 97, 2, sa['cus'] * 4096 + 1 if n is None else n, dc.WIDE)


@pytest.mark.parametrize('l,w', [(199, 1), (14, 14)])
@pytest.mark.parametrize('n', [32767, 32768, 32769, 65537])
def test_small_count_action_edges(sa, l, w, n):
    """XC_SMALL without the shared flag (an odd and an even C * C in the packed table): one
    workgroup's 32768 actions +-1 and a third workgroup of one action."""
    _count_n(sa, l, w, n, dc.SMALL)


@pytest.mark.parametrize('l,w', [(199, 1), (14, 14)])
@pytest.mark.parametrize('step', [0, 1])
def test_small_count_full_workgroup_into_one_bin(sa, l, w, step):
    """32768 identical successful passes: one workgroup adds 32768 (< 65535: exact) to ONE packed
    u16 transition bin.  ``step`` moves the end cell by one, so the two cases are the low half
    of a word (an even flat index s * C + e) and the high half."""
    ops = sa['ops']
    C, n = l * w, 32768
    cx, cy = xo.centres(tc.FIELD_L, l), xo.centres(tc.FIELD_W, w)
    sx, sy, ex, ey = cx[l // 2], cy[w // 2], cx[l // 2 + step], cy[w // 2]
    s, e = int(xo.flat_indexes(sx, sy, l, w)), int(xo.flat_indexes(ex, ey, l, w))
    assert e == s + step
    one = dict(start_x=[sx], start_y=[sy], end_x=[ex], end_y=[ey], type_id=[0], result_id=[1], period_id=[1],
               time_seconds=[0.0], team_id=[0], bodypart_id=[0])
    d = _tile({k: np.asarray(v) for k, v in one.items()}, n)
    ab = _batch(sa, d)
    assert _mode(sa, l, w, n) == dc.SMALL
    ref = ref_counts(d, l, w)
    assert ref['trans'][0].tolist() == [s * C + e] and ref['trans'][1].tolist() == [n] and ref['move'][s] == n
    same_counts(sa, ops.xt_count(ab, l, w), ref, 'one bin')
    same_counts(sa, ops.xt_count_cells(ops.xt_cells(ab, l, w), n, l, w), ref, 'one bin, cell codes')


@pytest.mark.parametrize('n', [1, 1023, 4 * 4096 * 256 + 1027])
def test_global_count_action_edges(sa, n):
    """XC_GLOBAL (1091 x 11 = 12001 cells): one action, four workgroups with the last thread
    idle, and the second grid-stride pass of the capped 4096-workgroup launch (4 actions per
    thread per pass) with a ragged end."""
    _count_n(sa, 1091, 11, n, dc.GLOBAL, cells=False)


# =============================================================================== solve
def _counts(sa, s, l, w):
    """A system as the XTCounts a count pass would have left."""
    acc = sa['ops'].xt_zero_counts(l, w, torch.device('cuda'))
    dev = acc.shot.device
    for k in ('shot', 'goal', 'move'):
        getattr(acc, k).copy_(torch.from_numpy(s[k]))
    acc.trans[torch.from_numpy(s['rows'] * (l * w) + s['cols']).to(dev)] = \
        torch.from_numpy(s['vals'].astype(np.int32)).to(dev)
    return acc


@pytest.mark.parametrize('l,w', dc.SOLVE_SMALL)
def test_small_solve_vs_oracle(sa, l, w):
    """sa_xt_solve and sa_xt_solve_async on the register kernel (<= 192 cells: a partly
    filled second column part, partly filled waves) and the one-workgroup kernel (193 - 1024:
    its scalar tail where C % 8 != 0, the full 1024-thread workgroup) == xt_oracle.solve bit
    for bit: matrices, transposed transition matrix, every iterate, the surface, n_iter."""
    ops = sa['ops']
    C = l * w
    for seed in (1, 2):
        s = dc.system(C, seed)
        ref = xo.solve(dc.dense_counts(s), l, w)
        acc = _counts(sa, s, l, w)
        sol = ops.xt_solve(acc)
        a = ops.xt_solve_async(acc)
        torch.cuda.synchronize()
        n_async = int(a.n_iter.item())
        for what, mats, tt, heat, n in (('solve', sol.mats, sol.trans_t, sol.heatmaps, sol.n_iter),
                                        ('async', a.mats, a.trans_t, a.heatmaps[:max(n_async, 0) + 1], n_async)):
            m = mats.cpu().numpy()
            assert n + 1 == len(ref['heatmaps']), (what, seed, n)
            for k, name in enumerate(('scoring_prob', 'shot_prob', 'move_prob', 'xT')):
                np.testing.assert_array_equal(m[k].reshape(w, l), ref[name], err_msg=f'{what} {name}')
            np.testing.assert_array_equal(tt.cpu().numpy().T, ref['transition'], err_msg=what)
            np.testing.assert_array_equal(heat.cpu().numpy().reshape(-1, w, l), ref['heatmaps'], err_msg=what)
        assert sol.path == 'sequential'
        if C > 2:
            assert sol.n_iter >= 3   # the sums matter


@pytest.mark.parametrize('l,w', dc.SOLVE_LARGE)
def test_large_solve_vs_sparse_oracle(sa, l, w):
    """Above 1024 cells, in the reference's order: the compact rows at both ends of their range
    (1025, 9472) and the dense count-row loop (9473, 12001) == xt_dispatch_cases.solve_sparse bit
    for bit.  The default solve: the same matrices and iteration count, iterates within the 1e-12
    relative of test_xt_large_grid_vs_oracle where the reordered sums ran -- and they have to
    run on the compact grids: the systems keep every convergence decision clear of that solve's
    error bound (xt_dispatch_cases.decision_clearance), so 'inside-bound' would be a fault."""
    ops, N = sa['ops'], sa['native']
    C = l * w
    s = dc.system(C, dc.LARGE_SEED[C])
    ref = dc.solve_sparse(s)
    assert ref['n_iter'] >= 10 and N.SA_XT_COMPACT_MAX_C == dc.COMPACT_MAX_C
    acc = _counts(sa, s, l, w)
    exact = ops.xt_solve(acc, transition=False, exact_order=True)
    assert exact.path == 'sequential' and exact.trans_t is None
    m = exact.mats.cpu().numpy()
    for k, name in enumerate(('scoring_prob', 'shot_prob', 'move_prob', 'xT')):
        np.testing.assert_array_equal(m[k], ref[name], err_msg=name)
    assert exact.n_iter == ref['n_iter']
    np.testing.assert_array_equal(exact.heatmaps.cpu().numpy(), ref['heatmaps'])
    fast = ops.xt_solve(acc, transition=False)
    assert fast.n_iter == ref['n_iter']
    np.testing.assert_array_equal(fast.mats[:3].cpu().numpy(), m[:3])
    h = fast.heatmaps.cpu().numpy()
    if C <= N.SA_XT_COMPACT_MAX_C:   # no decision of this system comes near the solve's error bound
        assert dc.decision_clearance(ref['heatmaps'], C) > 2.0
        assert fast.path in ('reordered', 'unavailable')
    else:
        assert fast.path == 'sequential'
    if fast.path == 'reordered':
        assert np.all(np.abs(h - ref['heatmaps']) <= 1e-12 * np.abs(ref['heatmaps']))
        assert np.all(np.abs(fast.mats[3].cpu().numpy() - ref['xT']) <= 1e-12 * np.abs(ref['xT']))
    else:
        np.testing.assert_array_equal(h, ref['heatmaps'])
        np.testing.assert_array_equal(fast.mats[3].cpu().numpy(), ref['xT'])


# =============================================================================== coordinate loaders
def _rows(sa, ab, first, n):
    """sa_actions of rows [first, first + n) of a batch: the columns the xT passes read, each
    pointer moved by ``first`` elements (8 bytes per coordinate, 1 byte per id), one segment."""
    N = sa['native']
    s = N.SaActions()
    s.n, s.n_segments, s.n_frames, s.atomic = n, 1, 1, 0
    off = torch.tensor([0, n], dtype=torch.int64, device=ab.device)
    s.seg_off = off.data_ptr()
    fr = s.frames[0]
    for k in ('c0', 'c1', 'c2', 'c3'):
        setattr(fr, k, ab.cols[k].data_ptr() + 8 * first)
    for k in ('type_id', 'result_id'):
        setattr(fr, k, ab.cols[k].data_ptr() + first)
    return s, off


def _rate(sa, s, n, out, grid, L, W):
    from socceraction_amd.batch import stream_handle
    N = sa['native']
    err = torch.zeros(1, dtype=torch.int32, device=out.device)
    N.check(N.lib().sa_xt_rate(ctypes.byref(s), grid.data_ptr(), L, W, out.data_ptr(), err.data_ptr(),
                               stream_handle()))
    return err


def _rate_interp(sa, s, out_ptr, xT, l, w, axes, dev, L=1050, W=680):
    from socceraction_amd.batch import stream_handle
    N = sa['native']
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    p = axes.data_ptr()
    N.check(N.lib().sa_xt_rate_interp(ctypes.byref(s), xT.data_ptr(), p, p + 8 * l, l, w, p + 8 * (l + w), L,
                                      p + 8 * (l + w + L), W, out_ptr, err.data_ptr(), stream_handle()))
    return err


def _same_rate(got, ref, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    np.testing.assert_array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)], err_msg=what)


@pytest.mark.parametrize('drop', [0, 1])
def test_unaligned_columns_take_the_scalar_loads(sa, drop):
    """Rows 1 .. n of a batch through pointers that start one element in (coordinates 8 bytes,
    ids 1 byte, ``out`` 8 bytes off 16-byte alignment), n - 1 even and odd: sa_xt_rate,
    sa_xt_rate_interp on 105 x 68 (surface and tables in LDS) and on 120 x 68 (they exceed it:
    the plain kernel) and the band count's key kernel give what the aligned call gives on those
    rows, bit for bit, and what xt_oracle gives."""
    ops = sa['ops']
    from socceraction_amd.batch import stream_handle
    N = sa['native']
    l, w = 105, 68
    full = tc.binning_batch(l, w)
    n0 = len(full['type_id']) - drop
    d = _tile(full, n0)
    ab = _batch(sa, d)
    dev = ab.device
    n = n0 - 1
    assert n % 2 == drop
    tail = {c: d[c][1:] for c in ROW_COLS}
    s, keep = _rows(sa, ab, 1, n)
    for k in ('c0', 'c1', 'c2', 'c3'):
        assert getattr(s.frames[0], k) % 16 == 8
    assert s.frames[0].type_id % 2 == 1 and s.frames[0].result_id % 2 == 1

    def shifted():
        buf = torch.full((n0 + 2,), -7.0, dtype=torch.float64, device=dev)
        assert buf.data_ptr() % 16 == 0
        return buf, buf[1:]

    # sa_xt_rate on a surface whose value at cell c is c + 1: every rate names its cell pair
    surf = np.arange(1, l * w + 1, dtype=np.float64).reshape(w, l)
    grid = torch.from_numpy(surf).to(dev)
    buf, out = shifted()
    err = _rate(sa, s, n, out, grid, l, w)
    aligned, e0 = ops.xt_rate(ab, grid, l, w)
    got = out[:n].cpu().numpy()
    _same_rate(got, aligned.cpu().numpy()[1:], 'xt_rate vs aligned')
    _same_rate(got, xo.rate(tail, surf), 'xt_rate vs oracle')
    assert int(err.item()) == 0 and int(e0.item()) == 0
    assert float(buf[0]) == -7.0 and float(buf[n + 1]) == -7.0   # nothing written outside rows 1 .. n
    # the interpolated rate, LDS kernel and plain kernel
    for gl, gw in ((105, 68), (120, 68)):
        lds = 8 * (gl * gw + 1050 + 680) + 4 * (1050 + 680)
        assert (lds <= 78 * 1024) == ((gl, gw) == (105, 68))
        xs = np.random.default_rng(gl).random((gw, gl))
        xT = torch.from_numpy(xs).to(dev)
        axes = ops.xt_interp_axes(gl, gw, dev)
        buf, out = shifted()
        err = _rate_interp(sa, s, out.data_ptr(), xT, gl, gw, axes, dev)
        aligned, e0 = ops.xt_rate_interp(ab, xT, gl, gw, axes=axes)
        got = out[:n].cpu().numpy()
        _same_rate(got, aligned.cpu().numpy()[1:], f'xt_rate_interp {gl} x {gw} vs aligned')
        assert_close(got, xo.rate(tail, xs, use_interpolation=True), f'xt_rate_interp {gl} x {gw} vs oracle')
        assert int(err.item()) == 0 and int(e0.item()) == 0
        assert float(buf[0]) == -7.0 and float(buf[n + 1]) == -7.0
    # the band count from unaligned coordinates
    assert _mode(sa, l, w, n) == dc.BANDS
    acc = ops.xt_zero_counts(l, w, dev)
    N.check(N.lib().sa_xt_count(ctypes.byref(s), l, w, acc.shot.data_ptr(), acc.goal.data_ptr(), acc.move.data_ptr(),
                                acc.trans.data_ptr(), acc.err.data_ptr(), None, 0, stream_handle()))
    same_counts(sa, acc, ref_counts(tail, l, w), 'band count, unaligned')
    del keep


def test_interp_rate_unrolled_pass_and_tail(sa):
    """One aligned interpolated rate long enough for the persistent kernel's unrolled pass (more
    than two pairs per thread of the capped grid) plus a tail of three actions: every row equals
    the same row rated in aligned slices of 2^20 actions (which the capped grid covers in one
    pass, so the plain pair path rates them), and the rows, a small batch repeated, repeat."""
    ops = sa['ops']
    l, w = 105, 68
    n = 2 * sa['cus'] * 4 * 1024 * 2 + 3
    base = tc.binning_batch(l, w)
    n0 = len(base['type_id'])
    ab = _batch(sa, _tile(base, n))
    dev = ab.device
    xs = np.random.default_rng(11).random((w, l))
    xT = torch.from_numpy(xs).to(dev)
    axes = ops.xt_interp_axes(l, w, dev)
    out, err = ops.xt_rate_interp(ab, xT, l, w, axes=axes)
    assert int(err.item()) == 0
    step = 1 << 20
    parts = torch.empty(n, dtype=torch.float64, device=dev)
    for first in range(0, n, step):
        m = min(step, n - first)
        s, keep = _rows(sa, ab, first, m)
        e = _rate_interp(sa, s, parts.data_ptr() + 8 * first, xT, l, w, axes, dev)
        assert int(e.item()) == 0
        del keep
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int64)  # noqa: E731  (NaN rows compare by their bits)
    assert torch.equal(bits(out), bits(parts))
    q = n // n0
    assert torch.equal(bits(out[:q * n0]).view(q, n0), bits(out[:n0]).expand(q, n0))
    assert torch.equal(bits(out[q * n0:]), bits(out[:n - q * n0]))
    assert_close(out[:n0].cpu().numpy(), xo.rate(base, xs, use_interpolation=True), 'first copy vs oracle')
