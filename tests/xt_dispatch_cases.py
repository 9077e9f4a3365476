"""Grids and systems that sit on the xT kernels' dispatch edges (pure numpy, no device).

The xT half of the library picks its kernels from the cell count C = l * w:

* the count pass (``count_mode``, csrc/sa_xt.hip; ``sa_xt_count_mode`` reports it): XC_WIDE up to
  194 cells, XC_SMALL up to 199 (and for every C <= 199 under SA_XT_COUNT_SHARED), the band-owned
  count for 200 - 12000 cells with R = 1 .. 8 start cells per band (``sa_xt_band_shape``), and
  XC_GLOBAL above -- :data:`COUNT_GRIDS` puts a grid on both sides of every C at which the mode
  or R changes;
* the solve (``launch_small_solve`` / ``solve_hooked``): the register kernel up to 192 cells (two
  column parts of 96, 32 rows per wave), one workgroup up to 1024, the compact rows up to 9472
  and the dense count rows above -- :data:`SOLVE_SMALL` / :data:`SOLVE_LARGE`.

:func:`system` writes counts directly (no actions), so the awkward cells are there on purpose:
a row without transitions, a cell without shots and a cell with neither shots nor moves (the
0 / 0 of the reference's ``_safe_divide``).  :func:`solve_sparse` restates ``xt_oracle.solve``
over each row's non-zero terms only, which is what lets it run at 12001 cells;
tests/test_xt_dispatch_host.py holds it to ``xt_oracle.solve`` bit for bit where the dense
oracle is affordable.  tests/test_gpu_xt_dispatch.py runs all of it on the device.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

# sa_xt_count_mode's values (include/socceraction_amd.h SA_XT_COUNT_MODE_*)
GLOBAL, VEC, SMALL, WIDE, BANDS = 0, 1, 2, 3, 4
SHARED = 1  # SA_XT_COUNT_SHARED
MAX_CELLS = 46340  # check_grid: the int32 indexing limit of the C x C table

# (l, w, mode without SA_XT_COUNT_SHARED): both neighbours of every C at which the count's mode
# or the band shape's R changes (194|195 WIDE -> SMALL, 199|200 SMALL -> bands, R at 512, 768,
# 1024, 1280, 1536, 1792, 2048, 4830, 5518, 6438, 7726, 9662, 12000|12001 bands -> GLOBAL), 196
# (an even C*C in the packed XC_SMALL table; 195 and 199 are odd), 202|203 (where
# ops.xt_count_many turns to the bucketed count and the cell codes to 32 bits) and the largest
# grid check_grid takes
COUNT_GRIDS: Tuple[Tuple[int, int, int], ...] = (
    (97, 2, WIDE), (15, 13, SMALL), (14, 14, SMALL), (199, 1, SMALL), (20, 10, BANDS),
    (101, 2, BANDS), (29, 7, BANDS), (73, 7, BANDS), (32, 16, BANDS), (59, 13, BANDS),
    (32, 24, BANDS), (33, 31, BANDS), (32, 32, BANDS), (1279, 1, BANDS), (40, 32, BANDS),
    (307, 5, BANDS), (48, 32, BANDS), (199, 9, BANDS), (56, 32, BANDS), (89, 23, BANDS),
    (64, 32, BANDS), (439, 11, BANDS), (70, 69, BANDS), (613, 9, BANDS), (89, 62, BANDS),
    (157, 41, BANDS), (111, 58, BANDS), (103, 75, BANDS), (3863, 2, BANDS), (9661, 1, BANDS),
    (4831, 2, BANDS), (120, 100, BANDS), (1091, 11, GLOBAL), (331, 140, GLOBAL),
)


def expected_mode(C: int, shared: bool) -> int:
    """The count pass of a C-cell grid (fewer than 2^31 actions), from the LDS budgets the
    kernels are written for: XC_WIDE's 3C + C*C u32 bins in 150 KiB, XC_SMALL's 3C u32 bins +
    C*C u16 bins in 80 KiB, the band count's at most 4000 bands of at most 3 rows at its top."""
    if (3 * C + C * C) * 4 <= 150 * 1024 and not shared:
        return WIDE
    if (3 * C + (C * C + 1) // 2) * 4 <= 80 * 1024:
        return SMALL
    return BANDS if C <= 12000 else GLOBAL


# the solve's kernels: (l, w) with l * w the cell counts the kernels' shapes turn on; w = 1 where
# C is prime
SOLVE_REG = ((1, 1), (2, 1), (7, 1), (31, 1), (8, 4), (11, 3), (19, 5), (12, 8), (97, 1), (191, 1), (16, 12))
SOLVE_ONE_WG = ((193, 1), (199, 1), (13, 77), (33, 31), (32, 32))
SOLVE_SMALL = SOLVE_REG + SOLVE_ONE_WG
SOLVE_LARGE = ((1025, 1), (9472, 1), (9473, 1), (1091, 11))
HOST_SOLVE_C = (1, 2, 7, 97, 193, 199, 1023, 1024)  # solve_sparse == xt_oracle.solve, bit for bit
# the seed of each large grid's system: for the compact grids the lowest whose reference iterates
# keep every convergence decision clear of the reordered solve's error bound
# (:func:`decision_clearance` > 2), so that solve may not hand the grid back as 'inside-bound'
LARGE_SEED = {1025: 1, 9472: 4, 9473: 1, 12001: 1}
COMPACT_MAX_C = 9472  # SA_XT_COMPACT_MAX_C


def system(C: int, seed: int) -> Dict[str, np.ndarray]:
    """Counts of a C-cell grid written directly: ``shot``, ``goal``, ``move`` int64 [C] and the
    non-zero transition counts as ``rows``, ``cols``, ``vals`` (int64, row-major order).  A row
    holds up to 12 geometric counts at random columns, ``move`` is at least the row's sum.  From
    3 cells on, three distinct special cells (``special``): one with moves and shots but no
    transitions, one with ``shot == 0``, one with ``shot == move == 0`` (and so no transitions).
    Two cells: cell 1 is all three (nothing at all), cell 0 moves to both.  One cell: a
    self-transition."""
    rng = np.random.default_rng([seed, C])
    K = min(C, 12)
    cols = rng.integers(0, C, (C, K))
    cols[np.arange(K)[None, :] >= rng.integers(1, K + 1, C)[:, None]] = C   # 1 .. K entries per row
    cols.sort(axis=1)
    keep = cols < C
    keep[:, 1:] &= cols[:, 1:] != cols[:, :-1]
    vals = rng.geometric(0.25, (C, K)).astype(np.int64)
    shot = rng.integers(1, 6, C)
    if C >= 3:
        empty, noshot, nothing = (int(c) for c in rng.choice(C, 3, replace=False))
    else:
        empty, noshot, nothing = C - 1, C - 1, C - 1
    if C >= 2:
        keep[empty] = False
        keep[nothing] = False
        shot[noshot] = 0
        shot[nothing] = 0
    rows = np.broadcast_to(np.arange(C)[:, None], (C, K))[keep].astype(np.int64)
    move = np.bincount(rows, weights=vals[keep], minlength=C).astype(np.int64) + rng.integers(0, 3, C)
    if C >= 2:
        move[empty] = 5
        move[nothing] = 0
    goal = rng.integers(0, shot + 1)
    return dict(shot=shot.astype(np.int64), goal=goal.astype(np.int64), move=move, rows=rows,
                cols=cols[keep].astype(np.int64), vals=vals[keep],
                special=np.array([empty, noshot, nothing], np.int64))


def dense_counts(s: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A system as ``xt_oracle.solve`` takes it (``start = move``, the dense C x C table)."""
    C = len(s['shot'])
    trans = np.zeros((C, C), np.int64)
    trans[s['rows'], s['cols']] = s['vals']
    return dict(shot=s['shot'], goal=s['goal'], move=s['move'], start=s['move'], trans=trans)


def _safe_divide(a, b):
    return np.divide(a, b, out=np.zeros_like(a), where=b != 0)


def solve_sparse(s: Dict[str, np.ndarray], eps: float = 1e-5, max_iter: int = 1000) -> Dict[str, np.ndarray]:
    """``xt_oracle.solve`` of a system over each row's non-zero terms only, in column order.
    The oracle adds T[r, c] * x[c] for c = 0 .. C - 1 into a sum that starts at +0; a zero entry
    adds +0 * x[c] = +0 (x is finite and non-negative), which leaves the non-negative sum as it
    is, so dropping those terms changes no bit.  Rows are padded to the longest with
    (value +0, column 0), which add +0 in the same way.  Everything flat, [C]; ``n_iter`` = the
    iterations run (``len(heatmaps) - 1``)."""
    shot, goal, move = (s[k].astype(np.float64) for k in ('shot', 'goal', 'move'))
    C = len(shot)
    scoring = _safe_divide(goal, shot)
    total = move + shot
    pshot, pmove = _safe_divide(shot, total), _safe_divide(move, total)
    rows, cols = s['rows'], s['cols']
    assert (np.diff(rows * C + cols) > 0).all()   # row-major, one entry per cell pair
    t = s['vals'] / move[rows]                    # int64 / float64, as the oracle's tc[nz] / start[rows]
    length = np.bincount(rows, minlength=C)
    first = np.cumsum(length) - length
    k = np.arange(len(rows)) - first[rows]        # the entry's place in its row
    K = int(length.max()) if len(rows) else 0
    val = np.zeros((C, K))
    col = np.zeros((C, K), np.int64)
    val[rows, k] = t
    col[rows, k] = cols
    gs = scoring * pshot
    x = np.zeros(C)
    heat = [x.copy()]
    while True:
        tot = np.zeros(C)
        for j in range(K):
            tot += val[:, j] * x[col[:, j]]
        new = gs + pmove * tot
        diff = new - x
        x = new
        heat.append(x.copy())
        if not np.any(diff > eps):
            break
        assert len(heat) <= max_iter, 'no convergence'
    return dict(scoring_prob=scoring, shot_prob=pshot, move_prob=pmove, xT=x, heatmaps=np.stack(heat),
                n_iter=len(heat) - 1)


def decision_clearance(heat: np.ndarray, C: int, eps: float = 1e-5) -> float:
    """How far the reference's iterates keep ``diff > eps`` from the error bound under which the
    reordered large-grid solve (xt_solve_reordered_kernel, csrc/sa_xt_large.hip) decides: the
    least ``|diff - eps| / margin`` over every cell and iteration, with that kernel's margin
    ``e_t (x_new + x_old) + 8 u (|diff| + eps)``, ``e_t = (e_{t-1} + (2 C + 16) u)(1 + 2^-20)``,
    ``u = 2^-53``.  The kernel's own iterates are within ``e_t`` (relative) of these, so its
    ``diff`` is within one margin of the reference's: above 2 no decision of the kernel can fall
    inside its bound, and it has to finish as 'reordered'."""
    u = 2.0 ** -53
    delta, bound, least = (2.0 * C + 16.0) * u, 0.0, np.inf
    for old, new in zip(heat[:-1], heat[1:]):
        bound = (bound + delta) * (1.0 + 2.0 ** -20)
        d = new - old
        margin = bound * (new + old) * (1.0 + 2.0 ** -20) + 8.0 * u * (np.abs(d) + eps)
        least = min(least, float((np.abs(d - eps) / margin).min()))
    return least
