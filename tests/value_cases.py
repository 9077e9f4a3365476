"""One deterministic value batch for the float outputs of csrc/sa_vaep.hip (pure numpy / mpmath,
no device): the f64 numeric feature block, its float32 form and the f64 / f32 VAEP formula.

With ``-ffp-contract=off`` every f64 feature column but the four angle families is a short
sequence of IEEE ``+ - * / sqrt fabs`` and casts in the reference's order, so it must equal numpy
bit for bit (``golden_io.assert_same_floats``).  The angle families (:data:`ANGLE_FAMILIES`) call
``atan`` / ``atan2``, where two honest libms may differ: they are held to :data:`ANGLE_ULPS` units
in the last place of the 200-bit value (``golden_io.assert_within_ulps``), ``atan`` taken at the
rounded quotient ``dy / dx`` both sides compute, ``atan2`` at ``(dy, dx)``.

:func:`batch` is :data:`N_ROWS` rows (odd: the numeric pass's two-row lane has a tail; more than
4 x 512: several numeric workgroups, more than one 1,024-row tile) in five segments:

* ordinary rows: half on the 0.01 m grid real data uses, half full-precision uniform over the
  pitch; atomic ``dx, dy`` from normal(0, 15) / normal(0, 10), half rounded to 0.01;
  ``time_seconds`` in whole milliseconds (fractional parts that are not dyadic), ``period_id``
  1..5, ids uniform over their ranges; two teams per segment in random order, the home id
  alternating between them;
* the special rows of :func:`specials` (each with its reason): every one is followed by two
  ordinary rows of its segment, so at k = 3 it is seen as window 0, 1 and 2.  The block of specials
  occurs twice, as segments 1 and 3: teams (away, home, away) put the special row under the flip
  in windows 0 and 2 of the first copy, teams (home, away, home) in window 1 of the second, so
  every special value meets every window under both flip states.

Not reachable: a subnormal ``105 - x`` or ``34 - y``.  The difference of two doubles is a
multiple of the smaller one's ulp, so ``105 - x`` is 0, at least 2^-46, or (x tiny) 105 itself.  The
specials hold the smallest differences there are (one ulp either side of 105 and 34) and
subnormal coordinates, whose own differences (``movement``, ``space_delta``) are subnormal and
whose squares underflow.

tests/test_values_host.py holds the conditions the device tests (tests/test_gpu_values.py) rest
on.

The angle bound.  Measured on an MI355X against the 200-bit value over this batch and the batch
of tests/window_cases.py (k = 3, SPADL and atomic, every angle column):

* ``atan``: 1.381 ulp, at dy / dx = 6.397208044491698 / 6.370353985048553
  (``start_angle_to_goal_a2``, window batch row 774; 1.267 ulp on this batch);
* ``atan2``: 1.421 ulp, at (dy, dx) = (13.023474093627161, 10.399450239684835)
  (``mov_angle_a0``, window batch row 5887; 1.321 ulp on this batch);
* no value farther than 2 ulps, no NaN or sign mismatch, on 111,492 angle values;

so :data:`ANGLE_ULPS` = 3: that maximum rounded up to a whole ulp, plus 1 (the batches sample the
input range, they do not exhaust it).  numpy's own maxima on the same inputs: ``arctan`` 0.554 ulp,
``arctan2`` 0.749 ulp (tests/test_values_host.py holds them to 1 ulp on this batch).
"""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Sequence, Tuple

import mpmath
import numpy as np
import pandas as pd

from golden_io import assert_same_floats, assert_within_ulps
from oracle import vaep_oracle as vo

ANGLE_ULPS = 3
PREC = 200                         # bits of the reference angles
N_ROWS = 2101
FIELD_L, GOAL_Y = 105.0, 34.0
TINY = 5e-324
ANGLE_FAMILIES = ('start_angle_to_goal_a', 'end_angle_to_goal_a', 'angle_to_goal_a', 'mov_angle_a')
# columns whose sum of squares a contracting build would fuse (SPADL, atomic)
LENGTH_COLUMNS = {False: ('start_dist_to_goal', 'end_dist_to_goal', 'movement', 'mov_a0i'),
                  True: ('dist_to_goal', 'mov_d')}
SPADL_COLS = ('period_id', 'time_seconds', 'team_id', 'start_x', 'start_y', 'end_x', 'end_y',
              'type_id', 'result_id', 'bodypart_id')
ATOMIC_COLS = ('period_id', 'time_seconds', 'team_id', 'x', 'y', 'dx', 'dy', 'type_id',
               'bodypart_id')
COORDS = {False: ('start_x', 'start_y', 'end_x', 'end_y'), True: ('x', 'y', 'dx', 'dy')}
N_TYPES = {False: 23, True: 33}
VALUES = ('offensive_value', 'defensive_value', 'vaep_value')
GOLDEN_ORDINARY = 300              # ordinary rows of the golden game (tests/golden/make_golden.py)


def is_angle(name: str) -> bool:
    return name.startswith(ANGLE_FAMILIES)


def _up(v: float) -> float:
    return float(np.nextafter(v, np.inf))


def _dn(v: float) -> float:
    return float(np.nextafter(v, -np.inf))


# (x, y, why): positions, used as SPADL start and end points and as atomic locations
POSITIONS: List[Tuple[float, float, str]] = [
    (105.0, 34.0, 'the goal point: dx = dy = 0, 0 / 0 -> NaN -> nan_to_num 0, distance 0'),
    (105.0, 0.0, 'the goal line: dx = 0, dy / 0 = inf, angle pi / 2'),
    (105.0, 68.0, 'the goal line, far post side'),
    (52.5, 34.0, 'the goal axis: dy = 0, angle +0'),
    (110.0, 34.0, 'beyond the goal line on the axis: fabs folds it back'),
    (-3.0, 70.0, 'outside the pitch on both axes (beyond the line once flipped)'),
    (_up(105.0), 20.25, 'one ulp past 105: the smallest negative 105 - x'),
    (_dn(105.0), 20.25, 'one ulp short of 105: the smallest positive 105 - x, a huge quotient'),
    (60.5, _up(34.0), 'one ulp past 34: the smallest 34 - y, an angle of about 1e-16'),
    (60.5, _dn(34.0), 'one ulp short of 34'),
    (_dn(105.0), _dn(34.0), 'both differences the smallest there are'),
    (0.0, 0.0, 'own corner: flips onto the goal line (105, 68)'),
    (0.0, 68.0, 'own corner: flips onto the goal line (105, 0)'),
    (-0.0, -0.0, 'negative zeros: the location columns keep the sign, the flip loses it'),
    (1e200, 20.25, 'dx * dx overflows to inf: distance inf, angle about 1e-199'),
    (TINY, 1e-310, 'subnormal coordinates: flip to (105, 68) exactly'),
]
# (dx, dy, why): atomic movements
MOVEMENTS: List[Tuple[float, float, str]] = [
    (0.0, 0.0, 'no movement: totald = 0, direction keeps dx, dy; dy == 0 override'),
    (-0.0, -0.0, 'signed zeros: direction keeps -0.0, the flip turns them to +0.0'),
    (-1.0, 0.0, 'arctan2(0, -1) = pi, overridden to 0 by dy == 0'),
    (-1.0, -0.0, 'arctan2(-0, -1) = -pi, overridden to 0 by dy == 0 (-0.0 == 0)'),
    (-1.0, TINY, 'dy subnormal, not zero: no override, the angle is pi'),
    (0.0, 1.0, 'dx = 0: pi / 2'),
    (0.0, -1.0, 'dx = 0: -pi / 2'),
    (float('nan'), 0.0, 'NaN dx with dy == 0: angle 0, mov_d NaN, direction keeps (NaN, 0)'),
    (1.0, float('nan'), 'NaN dy: everything NaN but direction dx = 1 (totald > 0 is False)'),
    (1e200, 1e200, 'the sum of squares is inf: direction = d / inf = 0'),
    (1e-200, 1e-200, 'the sum of squares underflows to 0: direction keeps dx, dy'),
    (3.0, 4.0, 'the 3-4-5 triple: exact'),
]
_BASE = {False: (40.25, 30.5, 70.75, 20.125), True: (60.5, 30.25, 3.25, -1.5)}


@lru_cache(maxsize=None)
def specials(atomic: bool) -> Tuple[Tuple[Tuple[float, float, float, float], str], ...]:
    """The special rows as ((c0, c1, c2, c3), why) over the columns ``COORDS[atomic]``."""
    base = _BASE[atomic]
    out = []
    for p, (x, y, why) in enumerate(POSITIONS):
        if atomic:
            out.append(((x, y, base[2], base[3]), why))
        else:  # start = position p, end = the next one: each is a start once and an end once
            ex, ey, _ = POSITIONS[(p + 1) % len(POSITIONS)]
            out.append(((x, y, ex, ey), 'start: ' + why))
    if atomic:
        for c in (0, 1):
            v = list(base)
            v[c] = float('nan')
            out.append((tuple(v), f'NaN in {COORDS[True][c]} alone'))
        out.append(((float('inf'), base[1], base[2], base[3]), '+inf in x'))
        for dx, dy, why in MOVEMENTS:  # NaN in dx alone and in dy alone are among them
            out.append(((base[0], base[1], dx, dy), why))
    else:
        for c in range(4):
            v = list(base)
            v[c] = float('nan')
            out.append((tuple(v), f'NaN in {COORDS[False][c]} alone'))
        out.append(((base[0], base[1], float('inf'), base[3]), '+inf in end_x'))
        out.append(((TINY, 1e-310, 3 * TINY, 3e-310),
                    'subnormal movement: dx, dy subnormal, their squares underflow, movement 0'))
    return tuple(out)


def _ordinary(rng: np.random.Generator, m: int, atomic: bool) -> List[np.ndarray]:
    """Coordinates of m ordinary rows: half on the 0.01 grid, half full precision."""
    x, y = rng.uniform(0, 105, m), rng.uniform(0, 68, m)
    if atomic:
        c2, c3 = rng.normal(0, 15, m), rng.normal(0, 10, m)
    else:
        c2, c3 = rng.uniform(0, 105, m), rng.uniform(0, 68, m)
    grid = rng.random(m) < 0.5
    grid2 = rng.random(m) < 0.5 if atomic else grid
    return [np.where(grid, np.round(x, 2), x), np.where(grid, np.round(y, 2), y),
            np.where(grid2, np.round(c2, 2), c2), np.where(grid2, np.round(c3, 2), c3)]


def _segment_sizes(atomic: bool) -> np.ndarray:
    block = 3 * len(specials(atomic))
    rest = N_ROWS - 2 * block
    a, b = rest // 3 + 5, rest // 3 - 11
    return np.array([a, block, b, block, rest - a - b], np.int64)


def special_rows(atomic: bool) -> np.ndarray:
    """[2, n_specials] row indexes of the special rows: copy 0 (segment 1), copy 1 (segment 3)."""
    sz = _segment_sizes(atomic)
    off = np.concatenate([[0], np.cumsum(sz)])
    step = 3 * np.arange(len(specials(atomic)))
    return np.stack([off[1] + step, off[3] + step])


@lru_cache(maxsize=None)
def batch(atomic: bool, seed: int = 7) -> Dict[str, np.ndarray]:
    """The value batch as flat columns plus ``game_off`` and ``home_team_id`` (the shape
    ``ActionBatch.from_columns`` takes).  Cached: treat it as read-only."""
    rng = np.random.default_rng([seed, int(atomic)])
    sz = _segment_sizes(atomic)
    off = np.concatenate([[0], np.cumsum(sz)]).astype(np.int64)
    n, ng = int(off[-1]), len(sz)
    g = np.repeat(np.arange(ng), sz)
    d: Dict[str, np.ndarray] = dict(
        type_id=rng.integers(0, N_TYPES[atomic], n), bodypart_id=rng.integers(0, 4, n),
        period_id=rng.integers(1, 6, n),
        time_seconds=np.cumsum(rng.integers(300, 14000, n)) / 1000.0)
    if not atomic:
        d['result_id'] = rng.integers(0, 6, n)
    coords = _ordinary(rng, n, atomic)
    side = rng.integers(0, 2, n)
    sp = specials(atomic)
    for copy, rows in enumerate(special_rows(atomic)):
        for r, (vals, _) in zip(rows, sp):
            for c in range(4):
                coords[c][r] = vals[c]
            # copy 0: (away, home, away); copy 1: (home, away, home); the segment's home ends in 0
            side[r:r + 3] = (1, 0, 1) if copy == 0 else (0, 1, 0)
    d['team_id'] = (10 * g + side).astype(np.int64)
    for name, v in zip(COORDS[atomic], coords):
        d[name] = v
    gi = np.arange(ng)
    d['home_team_id'] = (10 * gi + np.where(gi % 2 == 1, 0, (gi // 2) % 2)).astype(np.int64)
    d['game_off'] = off
    d['game_id'] = g.astype(np.int64)
    for v in d.values():
        v.setflags(write=False)
    return d


def cols_of(d: Dict[str, np.ndarray], atomic: bool) -> Dict[str, np.ndarray]:
    """The oracle's input columns of a batch."""
    return {c: d[c] for c in (ATOMIC_COLS if atomic else SPADL_COLS)}


@lru_cache(maxsize=None)
def golden_game(atomic: bool) -> pd.DataFrame:
    """One game for the reference itself (tests/golden/make_golden.py's ``values`` cases) and for
    the public ``compute_features``: segment 1 of :func:`batch` (every special row with its two
    followers, specials flipped in windows 0 and 2) followed by segment 3 (flipped in window 1)
    and :data:`GOLDEN_ORDINARY` ordinary rows, as a reference-shaped DataFrame whose two team ids
    are 0 (home) and 1."""
    d = batch(atomic)
    off = d['game_off']
    rows = np.r_[off[1]:off[2], off[3]:off[4], off[0]:off[0] + GOLDEN_ORDINARY]
    n = len(rows)
    out = dict(game_id=np.full(n, 7, np.int64), original_event_id=np.array([None] * n, object),
               action_id=np.arange(n, dtype=np.int64))
    for c in (ATOMIC_COLS if atomic else SPADL_COLS):
        out[c] = d[c][rows].copy()
    out['team_id'] = out['team_id'] % 10
    out['player_id'] = np.zeros(n, np.int64)
    order = ['game_id', 'original_event_id', 'action_id', 'period_id', 'time_seconds', 'team_id',
             'player_id'] + [c for c in (ATOMIC_COLS if atomic else SPADL_COLS)
                             if c not in ('period_id', 'time_seconds', 'team_id')]
    return pd.DataFrame({c: out[c] for c in order})


GOLDEN_HOME = 0


def permuted_frames(k: int, atomic: bool, seed: int = 3) -> List[pd.DataFrame]:
    """k game-state frames for explicit-frame mode, in the shape of
    ``window_cases.permuted_frames``: frame 0 holds every row of :func:`batch` (one segment, raw
    team ids), frame i the same rows under its own seeded permutation."""
    d = batch(atomic)
    n = N_ROWS
    cols = dict(game_id=np.full(n, 7, np.int64), original_event_id=np.array([None] * n, object),
                action_id=np.arange(n, dtype=np.int64))
    for c in (ATOMIC_COLS if atomic else SPADL_COLS):
        cols[c] = d[c].copy()
    cols['player_id'] = np.zeros(n, np.int64)
    f0 = pd.DataFrame(cols)
    rng = np.random.default_rng([seed, k, int(atomic)])
    return [f0] + [f0.iloc[rng.permutation(n)].reset_index(drop=True) for _ in range(1, k)]


def probabilities(n: int, dtype, seed: int = 9) -> Tuple[np.ndarray, np.ndarray]:
    """Full-precision uniform doubles over [0, 1) with a dozen rows of 0, 1, the smallest
    subnormal and 1 - 2^-53 from row 5 on; ``dtype=float32`` is the same draw cast down."""
    rng = np.random.default_rng([seed, n])
    ps, pc = rng.random(n), rng.random(n)
    edge = np.array([0.0, 1.0, TINY, 1.0 - 2.0 ** -53])
    m = min(12, max(n - 5, 0))
    ps[5:5 + m] = edge[np.arange(m) % 4]
    pc[5:5 + m] = edge[(np.arange(m) // 4 + np.arange(m)) % 4]
    return ps.astype(dtype), pc.astype(dtype)


# ------------------------------------------------------------------------------- exact angles
_ATAN: Dict[float, object] = {}
_ATAN2: Dict[Tuple[float, float], object] = {}


def exact_atan_of_quotient(dy: np.ndarray, dx: np.ndarray) -> np.ndarray:
    """nan_to_num(arctan(q)) at the rounded quotient q = dy / dx, to :data:`PREC` bits."""
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.asarray(dy, np.float64) / np.asarray(dx, np.float64)
    out = np.empty(q.shape, object)
    with mpmath.workprec(PREC):
        for j, v in enumerate(q.tolist()):
            if v not in _ATAN:  # a NaN key never matches: recomputed, which is cheap
                _ATAN[v] = mpmath.mpf(0) if v != v else mpmath.atan(mpmath.mpf(v))
            out[j] = _ATAN[v]
    return out


def exact_atan2(dy: np.ndarray, dx: np.ndarray) -> np.ndarray:
    """arctan2(dy, dx) with the reference's ``dy == 0 -> 0`` override, to :data:`PREC` bits; NaN
    where either argument is NaN and dy is not 0."""
    out = np.empty(len(dy), object)
    with mpmath.workprec(PREC):
        for j, (y, x) in enumerate(zip(np.asarray(dy, np.float64).tolist(),
                                       np.asarray(dx, np.float64).tolist())):
            key = (y, x)
            if key not in _ATAN2:
                if y == 0:
                    _ATAN2[key] = mpmath.mpf(0)
                elif y != y or x != x:
                    _ATAN2[key] = mpmath.mpf('nan')
                else:
                    _ATAN2[key] = mpmath.atan2(mpmath.mpf(y), mpmath.mpf(x))
            out[j] = _ATAN2[key]
    return out


def exact_angles_frames(frames: Sequence[Dict[str, np.ndarray]], atomic: bool) -> Dict[str, np.ndarray]:
    """The 200-bit value of every angle column of a list of game-state frames (as
    ``oracle.features_frames`` sees them), by column name."""
    out = {}
    for i, a in enumerate(frames):
        pairs = (('angle_to_goal', 'x', 'y'),) if atomic else (
            ('start_angle_to_goal', 'start_x', 'start_y'), ('end_angle_to_goal', 'end_x', 'end_y'))
        for name, cx, cy in pairs:
            dx = np.abs(FIELD_L - np.asarray(a[cx], np.float64))
            dy = np.abs(GOAL_Y - np.asarray(a[cy], np.float64))
            out[f'{name}_a{i}'] = exact_atan_of_quotient(dy, dx)
        if atomic:
            out[f'mov_angle_a{i}'] = exact_atan2(a['dy'], a['dx'])
    return out


def exact_angles(cols: Dict[str, np.ndarray], k: int, atomic: bool, seg_off=None,
                 home=None) -> Dict[str, np.ndarray]:
    """:func:`exact_angles_frames` of the windows the oracle builds from a batch."""
    return exact_angles_frames(vo.windows(cols, k, atomic, seg_off, home), atomic)


def check_float_columns(names: Sequence[str], got, ref, exact: Dict[str, np.ndarray], tag: str,
                        bound: float = ANGLE_ULPS) -> float:
    """The float feature columns ``names`` (rows of the matrices ``got`` and ``ref``, float64 or
    float32 alike): angle columns within ``bound`` ulps of ``exact[name]``, every other column
    equal to the reference bit for bit.  Returns the largest angle distance seen."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert len(names) == len(got) == len(ref), tag
    worst = 0.0
    plain = [j for j, nm in enumerate(names) if not is_angle(nm)]
    for j, nm in enumerate(names):
        if is_angle(nm):
            worst = max(worst, assert_within_ulps(got[j], exact[nm], bound, f'{tag} {nm}'))
    try:
        assert_same_floats(got[plain], ref[plain], tag)
    except AssertionError:  # name the first column that differs
        for j in plain:
            assert_same_floats(got[j], ref[j], f'{tag} {names[j]}')
        raise
    return worst


def golden_angle_columns(names: Sequence[str], got, ref, tag: str) -> float:
    """Against numpy's own values (a golden of the reference, or the oracle where the 200-bit
    value would cost too much): angle columns within ``ANGLE_ULPS + 1`` ulps of that value (itself
    within 1 ulp of exact, tests/test_values_host.py), every other column bit for bit."""
    exact = {nm: (ref[j], ref[j]) for j, nm in enumerate(names) if is_angle(nm)}
    return check_float_columns(names, got, ref, exact, tag, ANGLE_ULPS + 1)
