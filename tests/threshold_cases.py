"""Inputs that sit ON the float64 thresholds behind discrete outputs (pure numpy, no device).

Three families, each decided in the kernels by one float64 comparison:

* the dribble rule (``dribble_after``, csrc/sa_atomic.hip; reference spadl/base.py:54-93):
  ``d2 = dx*dx + dy*dy``, ``d2 >= min2 && d2 <= max2 && dt < max_dt`` -- :func:`dribble_frame`;
* the xT binning (``flat_index`` / ``flat_index_q``, csrc/sa_common.h; reference
  xthreat.py:25-37): ``clip(int64(x / 105 * l), 0, l - 1)`` -- :func:`edge_values`,
  :func:`binning_batch`, with the plausible wrong formulas in :data:`WRONG_BINNINGS`;
* the formula's same-phase rule (csrc/sa_vaep.hip; reference vaep/formula.py:51):
  ``abs(t - t_prev) > 10`` -- :func:`samephase_batch`.

tests/test_gpu_thresholds.py runs them on the device, tests/golden/make_golden_thresholds.py runs
the reference on them.  Every builder is deterministic (seeded).
"""
from __future__ import annotations

from fractions import Fraction
from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

FIELD_L, FIELD_W = 105.0, 68.0

# ------------------------------------------------------------------------------- dribbles
DRIBBLE_COLS = ('game_id', 'original_event_id', 'action_id', 'period_id', 'time_seconds', 'team_id',
                'player_id', 'start_x', 'start_y', 'end_x', 'end_y', 'type_id', 'result_id',
                'bodypart_id')
DRIBBLE_PREFIXES = (1, 2, 3, 127, 128, 129, 1023, 1024, 1025)


def _ulps(v: np.ndarray, k: int) -> np.ndarray:
    """v moved by k units in the last place (k in -2..2)."""
    v = np.asarray(v, np.float64).copy()
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def fused_d2(dx: np.ndarray, dy: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``fma(dx, dx, dy*dy)`` and ``fma(dy, dy, dx*dx)``, each rounded once from the exact value
    (fractions.Fraction; float(Fraction) is correctly rounded): what a build that contracts
    ``dx*dx + dy*dy`` would compute."""
    a = np.empty(len(dx))
    b = np.empty(len(dx))
    for i, (x, y) in enumerate(zip(dx.tolist(), dy.tolist())):
        a[i] = float(Fraction(x) * Fraction(x) + Fraction(y * y))
        b[i] = float(Fraction(y) * Fraction(y) + Fraction(x * x))
    return a, b


def _decide(d2: np.ndarray, T: float, lower: bool) -> np.ndarray:
    return d2 >= T if lower else d2 <= T


def fused_flips(dx, dy, T: float, lower: bool) -> np.ndarray:
    """Pairs whose threshold decision differs between the unfused sum and either fused form."""
    d2 = dx * dx + dy * dy
    a, b = fused_d2(dx, dy)
    ref = _decide(d2, T, lower)
    return (_decide(a, T, lower) != ref) | (_decide(b, T, lower) != ref)


@lru_cache(maxsize=None)
def _circle_pairs(r: float, lower: bool, count: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """``count`` (dx, dy) on the circle of radius r: dx over (0.05 r, 0.99 r), dy the
    neighbours (0, +-1, +-2 ulp) of sqrt(T - dx*dx), T = r*r as the host squares it.  Kept:
    every candidate on which a fused build decides differently (up to half), every candidate
    with d2 == T exactly (up to a quarter), the rest as they come; then the exact cases."""
    T = float(r) ** 2
    rng = np.random.default_rng([seed, int(lower)])
    base = rng.uniform(0.05 * r, 0.99 * r, 3000)
    dx = np.repeat(base, 5)
    dy0 = np.sqrt(T - base * base)
    dy = np.stack([_ulps(dy0, k) for k in (0, 1, -1, 2, -2)], axis=1).reshape(-1)
    d2 = dx * dx + dy * dy
    flips = fused_flips(dx, dy, T, lower)
    exact = (d2 == T) & ~flips
    rest = ~flips & ~exact
    pick = np.r_[np.flatnonzero(flips)[:count // 2], np.flatnonzero(exact)[:count // 4]]
    pick = np.r_[pick, np.flatnonzero(rest)[:max(count - len(pick) - 6, 0)]]
    # the exact cases: axis points and the 3-4-5 triple scaled to r (1.8 / 2.4, 36 / 48)
    ex = np.array([r, 0.0, 0.6 * r, 0.8 * r, 3 * r / 5, 4 * r / 5])
    ey = np.array([0.0, r, 0.8 * r, 0.6 * r, 4 * r / 5, 3 * r / 5])
    return np.r_[dx[pick], ex], np.r_[dy[pick], ey]


def _dt_sequence(max_dt: float) -> List[float]:
    """Times whose consecutive differences are exact: +-max_dt, +-both neighbours, 0, a large
    positive and a large negative one (which qualifies), +-9.999 / +-10.001 (scaled)."""
    up, dn = float(np.nextafter(max_dt, np.inf)), float(np.nextafter(max_dt, -np.inf))
    return [0.0, max_dt, 0.0, up, 0.0, dn, 0.0, 0.0, 1e6, 0.0, max_dt * 0.9999, 0.0, max_dt * 1.0001, 0.0]


def dribble_frame(per_threshold: int = 1050, min_len: float = 3.0, max_len: float = 60.0,
                  max_dt: float = 10.0, seed: int = 11) -> Dict[str, np.ndarray]:
    """A SPADL frame (two games, per-game action ids: the fast placement) in which every
    consecutive pair is a threshold case.  Every row starts at (0, 0) and ends at (dx, dy), so the
    rule's ``end - next start`` is exact and d2 is the separately rounded dx*dx + dy*dy of the
    row's own end point.  Distance rows step the time by 1; the time-threshold rows (d2 = 25 or,
    scaled, the middle of the distance window) are inserted across rows 128, 256, 512, 1024 and
    2048 and at the end.  Every 47th row belongs to the other team; each game turns to period 2
    once; the game boundary separates two pairs of teams."""
    ax, ay = _circle_pairs(float(min_len), True, per_threshold, seed)
    bx, by = _circle_pairs(float(max_len), False, per_threshold, seed)
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(ax) + len(bx))
    ex = np.r_[ax, bx][order]
    ey = np.r_[ay, by][order]
    mid = 0.5 * (float(min_len) + float(max_len)) if (min_len, max_len) != (3.0, 60.0) else 5.0
    tx, ty = 0.6 * mid, 0.8 * mid   # d2 well inside the window: only dt decides
    seq = _dt_sequence(float(max_dt))
    rows_x: List[float] = []
    rows_y: List[float] = []
    times: List[float] = []
    marks = [m - len(seq) // 2 for m in (128, 256, 512, 1024, 2048)]
    t = 0.0
    for j in range(len(ex)):
        if marks and len(rows_x) >= marks[0]:
            marks.pop(0)
            rows_x += [tx] * len(seq)
            rows_y += [ty] * len(seq)
            times += seq
            t = seq[-1]
        t += 1.0
        rows_x.append(float(ex[j]))
        rows_y.append(float(ey[j]))
        times.append(t)
    rows_x += [tx] * len(seq)
    rows_y += [ty] * len(seq)
    times += seq
    n = len(times)
    idx = np.arange(n)
    half = n // 2 + 3
    game = np.where(idx < half, 7, 9).astype(np.int64)
    pos = np.where(idx < half, idx, idx - half).astype(np.int64)
    size = np.where(idx < half, half, n - half)
    team = np.where(idx % 47 == 46, 1, 0) + np.where(idx < half, 10, 20)
    return {
        'game_id': game,
        'original_event_id': np.array([f'ev{i}' for i in range(n)], dtype=object),
        'action_id': pos,
        'period_id': np.where(pos * 2 < size, 1, 2).astype(np.int64),
        'time_seconds': np.array(times, np.float64),
        'team_id': team.astype(np.int64),
        'player_id': (team * 100 + idx % 11).astype(np.int64),
        'start_x': np.zeros(n), 'start_y': np.zeros(n),
        'end_x': np.array(rows_x, np.float64), 'end_y': np.array(rows_y, np.float64),
        'type_id': (idx % 3).astype(np.int64),
        'result_id': (idx % 2).astype(np.int64),
        'bodypart_id': (idx % 4).astype(np.int64),
    }


def dribble_prefix(f: Dict[str, np.ndarray], n: int) -> Dict[str, np.ndarray]:
    return {c: v[:n] for c, v in f.items()}


def dribble_shuffled(f: Dict[str, np.ndarray], seed: int = 3) -> Dict[str, np.ndarray]:
    """The same rows in a seeded random order (keys no longer increasing: lexsort placement).
    All starts are (0, 0), so every pair still has its row's own d2."""
    p = np.random.default_rng(seed).permutation(len(f['type_id']))
    return {c: v[p] for c, v in f.items()}


def dribble_pairs(f: Dict[str, np.ndarray]):
    """(dx, dy, dt) of every consecutive pair, as the rule computes them."""
    dx = f['end_x'][:-1] - f['start_x'][1:]
    dy = f['end_y'][:-1] - f['start_y'][1:]
    return dx, dy, f['time_seconds'][1:] - f['time_seconds'][:-1]


# ------------------------------------------------------------------------------- xT binning
GRIDS16 = ((16, 12), (15, 14))                       # <= 202 cells: the 16-bit cell code
GRIDS32 = ((30, 20), (40, 30), (64, 64), (75, 68), (100, 68), (105, 68), (120, 68))
NODE_GRID = (1050, 680)                              # the interpolated rate's node grid
GOLDEN_GRIDS = ((16, 12), (105, 68))
BIN_TYPES = (0, 1, 21, 11, 7)                        # pass, cross, dribble, shot, one uncounted
TWO63 = 9.223372036854775808e18


def _crossing(b: float, l: int) -> Tuple[float, float]:
    """The two doubles on either side of the point where x / b * l reaches 2^63."""
    x = TWO63 / l * b
    while x / b * l >= TWO63:
        x = float(np.nextafter(x, -np.inf))
    while x / b * l < TWO63:
        x = float(np.nextafter(x, np.inf))
    return float(np.nextafter(x, -np.inf)), x


def edge_values(b: float, l: int) -> np.ndarray:
    """The coordinates of one axis (extent b, l cells) that tell the binning formulas apart: both
    roundings of every cell edge with their +-1 and +-2 ulp neighbours, signed zero, denormals,
    negatives, the far edge and beyond, and the finite values whose int64 cast overflows."""
    i = np.arange(l + 1, dtype=np.float64)
    edges = np.r_[b * i / l, i * (b / l)]
    v = [_ulps(edges, k) for k in (0, 1, -1, 2, -2)]
    lo, hi = _crossing(b, l)
    tiny = 5e-324
    v.append(np.array([-0.0, tiny, -tiny, -1e-300, -1.0, b, float(np.nextafter(b, np.inf)),
                       float(np.nextafter(b, -np.inf)), 2 * b, 1e18, lo, hi, 1e300]))
    return np.concatenate(v)


def binning_batch(l: int, w: int, seed: int = 5, n_games: int = 2) -> Dict[str, np.ndarray]:
    """SPADL columns whose x (y) coordinates are the edge values of the l (w) axis, start and end
    in independent seeded orders; types cycle over pass, cross, dribble, shot and one uncounted
    type, results over success and fail; ``n_games`` segments."""
    xv, yv = edge_values(FIELD_L, l), edge_values(FIELD_W, w)
    n = max(len(xv), len(yv))
    rng = np.random.default_rng([seed, l, w])
    cols = {}
    for name, v in (('start_x', xv), ('start_y', yv), ('end_x', xv), ('end_y', yv)):
        cols[name] = np.resize(v, n)[rng.permutation(n)]
    idx = np.arange(n)
    off = np.linspace(0, n, n_games + 1).astype(np.int64)
    seg = np.searchsorted(off, idx, 'right') - 1
    cols.update(
        game_id=(seg + 1).astype(np.int64), period_id=np.ones(n, np.int64),
        time_seconds=idx.astype(np.float64), team_id=(seg * 2 + idx % 2).astype(np.int64),
        type_id=np.array(BIN_TYPES, np.int64)[idx % len(BIN_TYPES)],
        result_id=((idx // len(BIN_TYPES)) % 2).astype(np.int64),
        bodypart_id=np.zeros(n, np.int64), game_off=off,
        home_team_id=(np.arange(n_games) * 2).astype(np.int64))
    return cols


def _cast_clip(v: np.ndarray, l: int, overflow_to_last: bool = False) -> np.ndarray:
    """numpy's float64 -> int64 cast as on x86 (NaN / out of range -> INT64_MIN), then clip."""
    v = np.asarray(v, np.float64)
    out = np.full(v.shape, l - 1 if overflow_to_last else 0, np.int64)
    ok = (v >= -TWO63) & (v < TWO63)
    out[ok] = np.clip(v[ok].astype(np.int64), 0, l - 1)
    out[v < -TWO63] = 0
    return out


def _f32(x, b, l):
    with np.errstate(over='ignore'):
        return (np.asarray(x, np.float64).astype(np.float32) / np.float32(b) * np.float32(l)).astype(np.float64)


# name -> (x, b, l) -> cell index: the wrong ways to write cell_index(x / b * l)
WRONG_BINNINGS = {
    'x * (l / b)': lambda x, b, l: _cast_clip(x * (l / b), l),
    'x * (1 / b) * l': lambda x, b, l: _cast_clip(x * (1.0 / b) * l, l),
    'x * l / b': lambda x, b, l: _cast_clip(x * l / b, l),
    'floor(x / (b / l))': lambda x, b, l: _cast_clip(np.floor(x / (b / l)), l),
    'float32': lambda x, b, l: _cast_clip(_f32(x, b, l), l),
    '>= 2^63 to l - 1': lambda x, b, l: _cast_clip(x / b * l, l, overflow_to_last=True),
}


# ------------------------------------------------------------------------------- same phase
SAMEPHASE_N = (1, 2, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 2049)


def samephase_walk() -> List[float]:
    """A closed walk of times whose every step (the wrap-around included) sits at the rule's
    threshold: |t - t_prev| is exactly 10, one of its two neighbours (or the next ones out),
    9.999 / 10.001 or the float sum 5 + 5.000000000000001, each reached with either sign (time
    going backwards: 0 -> v -> 0), and differences from a non-zero time that round onto or next
    to 10 (10 -> a -> a + 10 -> a -> 10)."""
    up, dn = float(np.nextafter(10.0, np.inf)), float(np.nextafter(10.0, -np.inf))
    walk = []
    for v in (10.0, up, dn, 9.999, 10.001, 5 + 5.000000000000001, float(np.nextafter(up, np.inf)),
              float(np.nextafter(dn, -np.inf))):
        walk += [0.0, v]
    walk += [0.0, 10.0]
    for a in (1e-9, 2.0 ** -30, 1e-15, 3e-16, 2.0 ** -52):
        walk += [a, a + 10.0, a, 10.0]
    return walk  # ... -> 10 -> (wrap) 0


def samephase_batch(n: int, seed: int = 17) -> Dict[str, np.ndarray]:
    """SPADL columns of n rows whose times follow :func:`samephase_walk` inside every segment
    (each from its own seeded offset), so every consecutive pair inside a segment is a threshold
    case.  Two segments from n = 2, three from n = 600; previous-goal, penalty and corner rows
    are sprinkled in; probabilities ``ps`` / ``pc`` uniform in (0.1, 0.9), so one wrong decision
    moves a value by at least 0.1."""
    rng = np.random.default_rng([seed, n])
    walk = np.array(samephase_walk())
    if n >= 600:
        off = [0, n // 3 + 1, (2 * n) // 3 + 2, n]
    elif n >= 2:
        off = [0, (n + 1) // 2, n]
    else:
        off = [0, n]
    off = np.array(off, np.int64)
    t = np.zeros(n)
    for s, e in zip(off[:-1], off[1:]):
        t[s:e] = walk[(int(rng.integers(0, len(walk))) + np.arange(e - s)) % len(walk)]
    idx = np.arange(n)
    seg = np.searchsorted(off, idx, 'right') - 1
    type_id = np.zeros(n, np.int64)
    result_id = (rng.random(n) < 0.8).astype(np.int64)
    u = rng.random(n)
    type_id[u < 0.06] = 11
    type_id[(u >= 0.06) & (u < 0.09)] = 12
    type_id[(u >= 0.09) & (u < 0.12)] = 5
    type_id[(u >= 0.12) & (u < 0.14)] = 6
    type_id[(u >= 0.14) & (u < 0.16)] = 13
    return dict(
        game_id=(seg + 1).astype(np.int64), period_id=np.ones(n, np.int64), time_seconds=t,
        team_id=(seg * 2 + (rng.random(n) < 0.5)).astype(np.int64),
        start_x=np.round(rng.uniform(0, FIELD_L, n), 4), start_y=np.round(rng.uniform(0, FIELD_W, n), 4),
        end_x=np.round(rng.uniform(0, FIELD_L, n), 4), end_y=np.round(rng.uniform(0, FIELD_W, n), 4),
        type_id=type_id, result_id=result_id, bodypart_id=np.zeros(n, np.int64), game_off=off,
        home_team_id=(np.arange(len(off) - 1) * 2).astype(np.int64),
        ps=rng.uniform(0.1, 0.9, n), pc=rng.uniform(0.1, 0.9, n))


def samephase_diffs(d: Dict[str, np.ndarray]) -> np.ndarray:
    """|t_j - t_{j-1}| of the pairs inside a segment."""
    t = d['time_seconds']
    inside = np.ones(len(t), bool)
    inside[d['game_off'][:-1][d['game_off'][:-1] < len(t)]] = False
    return np.abs(t[1:] - t[:-1])[inside[1:]]
