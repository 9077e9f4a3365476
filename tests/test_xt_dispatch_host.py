"""CPU checks behind tests/test_gpu_xt_dispatch.py: the count pass's choice of kernel
(``sa_xt_count_mode``, host only) and the band shape over every cell count the library takes,
the coverage of tests/xt_dispatch_cases.py's grids, and its sparse solve against
``xt_oracle.solve``.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import threshold_cases as tc
import xt_dispatch_cases as dc
from oracle import xt_oracle as xo


@pytest.fixture(scope='module')
def lib():
    from socceraction_amd import _native, build
    build.build(force=False, verbose=False)
    return _native.load_library()


def _shape(lib, l, w):
    r, nb = ctypes.c_int32(0), ctypes.c_int32(0)
    if lib.sa_xt_band_shape(l, w, ctypes.byref(r), ctypes.byref(nb)) != 0:
        return None
    return r.value, nb.value


def test_mode_values_match_the_header():
    from socceraction_amd import _native
    for name in ('GLOBAL', 'VEC', 'SMALL', 'WIDE', 'BANDS'):
        assert getattr(dc, name) == getattr(_native, 'SA_XT_COUNT_MODE_' + name), name
    assert dc.SHARED == _native.SA_XT_COUNT_SHARED


@pytest.mark.parametrize('l,w,mode', dc.COUNT_GRIDS)
def test_count_mode_of_every_table_grid(lib, l, w, mode):
    """Each row's mode as the table states it, with and without SA_XT_COUNT_SHARED (which only
    turns XC_WIDE into XC_SMALL), whatever the action count below 2^31."""
    C = l * w
    assert mode == dc.expected_mode(C, False)
    for n in (0, 1, 32768, 2 ** 31 - 1):
        assert lib.sa_xt_count_mode(l, w, n, 0) == mode, (C, n)
        assert lib.sa_xt_count_mode(l, w, n, dc.SHARED) == (dc.SMALL if mode == dc.WIDE else mode), (C, n)
    # past the band count's 32-bit positions: XC_VEC while its three C-vectors fit 120 KiB
    if mode == dc.BANDS:
        assert lib.sa_xt_count_mode(l, w, 2 ** 31, 0) == (dc.VEC if C <= 10240 else dc.GLOBAL)


def test_count_mode_rejects_bad_arguments(lib):
    from socceraction_amd import _native
    for l, w, n in ((0, 1, 1), (1, 0, 1), (331, 141, 1), (-3, -4, 1), (16, 12, -1)):
        assert lib.sa_xt_count_mode(l, w, n, 0) == _native.SA_EINVAL, (l, w, n)


def test_every_dispatch_edge_has_a_grid_on_both_sides(lib):
    """C = 1 .. 46340 through sa_xt_count_mode and sa_xt_band_shape: the mode is the one the
    LDS budgets give, R and the band count are consistent, and wherever the mode (shared or
    not) or R changes, C - 1 and C are both cell counts of a grid the suite counts on the
    device: this table's or threshold_cases.GRIDS16 / GRIDS32."""
    pinned = {l * w for l, w, _ in dc.COUNT_GRIDS} | {l * w for l, w in tc.GRIDS16 + tc.GRIDS32}
    prev, edges = None, []
    for C in range(1, dc.MAX_CELLS + 1):
        mode, shared = lib.sa_xt_count_mode(C, 1, 1, 0), lib.sa_xt_count_mode(C, 1, 1, dc.SHARED)
        assert mode == dc.expected_mode(C, False) and shared == dc.expected_mode(C, True), C
        shape = _shape(lib, C, 1)
        assert (shape is not None) == (C <= 12000), C
        if shape is not None:
            r, nb = shape
            assert 1 <= r <= 8 and nb == -(-C // r) and nb <= 4000, (C, shape)
        state = (mode, shared, shape[0] if mode == dc.BANDS else 0)
        if prev is not None and state != prev:
            edges.append(C)
        prev = state
    assert edges == [195, 200, 512, 768, 1024, 1280, 1536, 1792, 2048, 4830, 5518, 6438, 7726, 9662, 12001]
    for C in edges:
        assert C - 1 in pinned and C in pinned, C
    assert dc.MAX_CELLS in pinned   # the int32 indexing limit itself
    assert _shape(lib, 331, 140) is None and lib.sa_xt_count_mode(331, 140, 1, 0) == dc.GLOBAL


def test_solve_grids_sit_on_the_kernels_shapes():
    """The register kernel's parts (96 columns) and waves (32 rows), the one-workgroup kernel's
    ends and its scalar tail (C % 8 != 0), the compact form's limits and the dense loop."""
    reg = [l * w for l, w in dc.SOLVE_REG]
    one = [l * w for l, w in dc.SOLVE_ONE_WG]
    assert reg == [1, 2, 7, 31, 32, 33, 95, 96, 97, 191, 192]
    assert one == [193, 199, 1001, 1023, 1024] and sum(c % 8 != 0 for c in one) == 4
    assert [l * w for l, w in dc.SOLVE_LARGE] == [1025, 9472, 9473, 12001]
    for l, w in dc.SOLVE_SMALL + dc.SOLVE_LARGE:   # w = 1 where C is prime
        C = l * w
        if all(C % p for p in range(2, int(C ** 0.5) + 1)) and C > 1:
            assert w == 1, (l, w)


@pytest.mark.parametrize('C', sorted({l * w for l, w in dc.SOLVE_SMALL + dc.SOLVE_LARGE}))
def test_systems_hold_the_awkward_cells(C):
    s = dc.system(C, 3)
    shot, goal, move = s['shot'], s['goal'], s['move']
    rowsum = np.bincount(s['rows'], weights=s['vals'], minlength=C).astype(np.int64)
    assert (s['vals'] >= 1).all() and (goal >= 0).all() and (goal <= shot).all()
    assert (move >= rowsum).all()
    assert (np.diff(s['rows'] * C + s['cols']) > 0).all() and s['cols'].max() < C
    assert np.array_equal(dc.system(C, 3)['vals'], s['vals'])   # deterministic
    empty, noshot, nothing = s['special']
    if C >= 3:
        assert len({empty, noshot, nothing}) == 3
        assert rowsum[empty] == 0 and move[empty] > 0 and shot[empty] > 0
        assert shot[noshot] == 0 and move[noshot] > 0 and rowsum[noshot] > 0
    if C >= 2:
        assert shot[nothing] == 0 and move[nothing] == 0 and rowsum[nothing] == 0
        assert (rowsum == 0).sum() >= 1 and (shot == 0).sum() >= min(2, C - 1)
    assert (rowsum > 0).sum() >= max(1, C - 2)


@pytest.mark.parametrize('C', dc.HOST_SOLVE_C)
def test_sparse_solve_equals_the_oracle(C):
    """solve_sparse == xt_oracle.solve bit for bit: matrices, every iterate, the surface and the
    iteration count; the systems take more than two iterations, so the sums matter."""
    for seed in (1, 2):
        s = dc.system(C, seed)
        got = dc.solve_sparse(s)
        ref = xo.solve(dc.dense_counts(s), C, 1)
        for k in ('scoring_prob', 'shot_prob', 'move_prob', 'xT'):
            np.testing.assert_array_equal(got[k], ref[k].reshape(-1), err_msg=k)
        assert got['n_iter'] + 1 == len(ref['heatmaps'])
        np.testing.assert_array_equal(got['heatmaps'], ref['heatmaps'].reshape(-1, C))
        assert np.isfinite(got['heatmaps']).all() and (got['heatmaps'] >= 0).all()
        if C > 2:
            assert 3 <= got['n_iter'] <= 200, (C, seed, got['n_iter'])


@pytest.mark.parametrize('C', sorted(dc.LARGE_SEED))
def test_large_systems_keep_clear_of_the_reordered_bound(C):
    """The compact grids' systems leave the reordered solve no decision inside its error bound
    (so the device test may insist on 'reordered'), with the lowest seed that does; every large
    system iterates long enough for the row sums to matter."""
    assert sorted(dc.LARGE_SEED) == [l * w for l, w in dc.SOLVE_LARGE]
    ref = dc.solve_sparse(dc.system(C, dc.LARGE_SEED[C]))
    assert ref['n_iter'] >= 10
    if C <= dc.COMPACT_MAX_C:
        assert dc.decision_clearance(ref['heatmaps'], C) > 2.0
        for seed in range(1, dc.LARGE_SEED[C]):
            assert dc.decision_clearance(dc.solve_sparse(dc.system(C, seed))['heatmaps'], C) <= 2.0, seed
