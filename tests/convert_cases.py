"""Inputs for the two count -> scan -> emit operators of csrc/sa_atomic.hip (pure numpy; only
:func:`assert_tiled_on_device` touches a device, and imports torch itself).

SPADL -> Atomic-SPADL conversion expands input row r into ``r, x4?, x3?, dA?, e1?, dB?`` (card,
goal / owngoal / out after a shot, dribble, receival / interception / out / offside, dribble after
that one); ``_add_dribbles`` expands it into ``r, dribble?``.  Both count the output rows of every
block of SA_ATOMIC_BLOCK_ROWS input rows, scan the block totals in tiles of SA_ATOMIC_SCAN_TILE
and write each block's rows from LDS.  The builders here make the inputs at which that can go
wrong and synthetic games never arrive:

* :func:`enum_frame` -- every combination of the facts the rules read, as two-row runs, so that
  every reachable group shape (:data:`REACHABLE_SHAPES`) occurs;
* :func:`dense_frame` / :func:`sparse_frame` -- blocks in which every row expands to the maximum,
  or none does;
* :func:`tiled` -- a small base repeated to any length with the expected output assembled from
  the oracle's output for the base alone, for sizes past one scan tile.

A frame is a dict of equal-length numpy columns named as in ``oracle.atomic_convert_oracle.COLS``.
Every builder is deterministic.  tests/test_convert_host.py holds the conditions the device
tests rely on; tests/golden/make_golden_convert.py and make_golden_dribbles.py run the reference
on a reduced enumeration.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

COLS = ('game_id', 'original_event_id', 'action_id', 'period_id', 'time_seconds', 'team_id',
        'player_id', 'start_x', 'start_y', 'end_x', 'end_y', 'type_id', 'result_id',
        'bodypart_id')
ALL_TYPES = tuple(range(23))
# the reduced enumeration the reference runs on (tests/golden/*_enum.npz): a pass, a throw-in, a
# corner, a goalkick, an interception, two shots, a foul, a dribble and a bad touch, each followed
# by a pass, a throw-in, a corner, a goalkick, an interception, a shot, a foul, a dribble, a
# tackle and a short corner
GOLDEN_TYPES = (0, 2, 5, 22, 10, 11, 13, 8, 21, 19)
GOLDEN_SUCCESSORS = (0, 2, 5, 22, 10, 11, 8, 21, 9, 6)
DISTANCES = (1.0, 10.0, 70.0)  # below, inside and above the 3..60 m dribble window
MAX_INSERTED = 3

# Atomic-SPADL names of the inserted rows (atomic/spadl/config.py:25-36)
INSERTED = {21: 'dribble', 23: 'receival', 10: 'interception', 25: 'out', 26: 'offside',
            27: 'goal', 28: 'owngoal', 29: 'yellow', 30: 'red'}


def _reachable() -> Tuple[Tuple[str, ...], ...]:
    """The non-empty group shapes the reference's rules allow, in emission order.

    A card needs result 4 / 5, a goal result 1 on a shot, an owngoal result 3, offside result 2:
    one result excludes the others.  A pass-like row with a successor in its game and period that
    is not interception-like gets e1 (receival, interception, out or offside), then possibly a
    dribble from e1; it is no shot, so of x3 only the owngoal remains.  Any other row may get x3
    (goal / owngoal, or out before a corner or goalkick, which needs the successor directly
    behind: no dribble between) and a dribble.  The out after a shot and the out after a pass
    carry one name (one Atomic-SPADL type), so "out" and "card, out" arise both ways and are
    listed once."""
    shapes: List[Tuple[str, ...]] = []
    for card in ((), ('yellow',), ('red',)):
        for x3 in ((), ('goal',), ('owngoal',), ('out',)):
            if card and x3 in (('goal',), ('owngoal',)):
                continue
            for tail in ((), ('dribble',)):                       # no e1
                if x3 == ('out',) and tail:
                    continue
                shapes.append(card + x3 + tail)
            if x3 in (('goal',), ('out',)):
                continue                                          # e1: pass-like, no shot
            for e1 in ('receival', 'interception', 'out', 'offside'):
                if e1 == 'offside' and (card or x3):
                    continue
                for tail in ((), ('dribble',)):
                    shapes.append(card + x3 + (e1,) + tail)
    return tuple(dict.fromkeys(s for s in shapes if s))


REACHABLE_SHAPES = _reachable()


def _pairs(first: np.ndarray, second: np.ndarray) -> np.ndarray:
    return np.stack([first, second], axis=1).reshape(-1)


def enum_frame(types: Sequence[int] = ALL_TYPES,
               successors: Sequence[int] = ALL_TYPES) -> Dict[str, np.ndarray]:
    """One two-row run per combination of: the row's type x its result 0..5 x the successor's
    type x same / other team x the successor's start 1, 10 or 70 m from the row's end x same /
    next period x same / next game.

    Run c has its own game (two when the successor is in the next one) and its own two teams, so
    nothing reaches across runs and the keys (game, period, action_id) increase strictly; action
    ids restart in every game.  The successor follows after 2 s, in every 7th run after 12 s (too
    late for a dribble from the row, not from the receival at the midpoint) and in every 11th of
    the rest after 24 s (too late for both); 7 and 11 share no factor with the enumeration's
    sizes, so every combination meets every gap.  The second row's result cycles through 0..5
    too; being the last row of its game and followed by another team it can only get a card, a
    goal or an owngoal.  Periods stay in 1..5, coordinates on the pitch, event ids are unique.

    On all 23 x 23 types the oracle's output holds every shape of :data:`REACHABLE_SHAPES` and no
    other, with at most :data:`MAX_INSERTED` inserted rows per input row.  Without a card:
    dribble; goal; goal dribble; owngoal; owngoal dribble; out; E; E dribble; owngoal E; owngoal E
    dribble; offside; offside dribble -- E one of receival, interception, out.  After a yellow or
    a red card: nothing; dribble; out; E; E dribble."""
    types = np.asarray(types, np.int64)
    successors = np.asarray(successors, np.int64)
    shape = (len(types), 6, len(successors), 2, len(DISTANCES), 2, 2)
    ti, res, si, other_team, dist, next_period, next_game = (a.reshape(-1) for a in np.indices(shape))
    n_runs = len(ti)
    c = np.arange(n_runs, dtype=np.int64)
    gap = np.where(c % 7 == 0, 12.0, np.where(c % 11 == 0, 24.0, 2.0))
    game = 10 + 2 * c
    period = 1 + (c // 5) % 4
    team = 1000 + 2 * c
    t = 60.25 + (c % 50)
    ex = 20.3 + 0.01 * (c % 13)
    ey = 30.7 + 0.01 * (c % 17)
    sx2 = ex + np.asarray(DISTANCES)[dist]
    sy2 = ey + 0.25
    team2 = team + other_team
    n = 2 * n_runs
    return {
        'game_id': _pairs(game, game + next_game),
        'original_event_id': np.array([f'e{i}' for i in range(n)], dtype=object),
        'action_id': _pairs(np.zeros(n_runs, np.int64), 1 - next_game),
        'period_id': _pairs(period, period + next_period),
        'time_seconds': _pairs(t, t + gap),
        'team_id': _pairs(team, team2),
        'player_id': _pairs(team * 10 + 1, team2 * 10 + 2),
        'start_x': _pairs(ex - 8.0 - 0.5 * (c % 3), sx2),
        'start_y': _pairs(ey + 2.5, sy2),
        'end_x': _pairs(ex, sx2 + 3.5),
        'end_y': _pairs(ey, sy2 - 1.25),
        'type_id': _pairs(types[ti], successors[si]),
        'result_id': _pairs(res, (c // 3) % 6),
        'bodypart_id': _pairs(c % 4, (c // 4) % 4),
    }


def _single_game(n: int, **cols) -> Dict[str, np.ndarray]:
    idx = np.arange(n, dtype=np.int64)
    out = {
        'game_id': np.full(n, 3, np.int64),
        'original_event_id': np.array([f'e{i}' for i in range(n)], dtype=object),
        'action_id': idx,
        'period_id': np.ones(n, np.int64),
        'time_seconds': 2.0 * idx,
        'start_x': np.full(n, 40.0), 'start_y': 30.0 + 0.5 * (idx % 7),
        'end_x': np.full(n, 50.0), 'end_y': 30.0 + 0.5 * (idx % 7),
        'bodypart_id': idx % 4,
    }
    out.update(cols)
    out['player_id'] = out['team_id'] * 100 + idx % 11
    return {c: out[c] for c in COLS}


def dense_frame(n: int) -> Dict[str, np.ndarray]:
    """n passes of one team in one period, each with a yellow card, each 2 s and 10 m (end to next
    start) before the next: every row but the last becomes pass, yellow card, receival, dribble,
    the last one pass, yellow card -- 4n - 2 rows, the most a block can hold; ``_add_dribbles``
    inserts n - 1 dribbles."""
    return _single_game(n, team_id=np.full(n, 5, np.int64), type_id=np.zeros(n, np.int64),
                        result_id=np.full(n, 4, np.int64))


def sparse_frame(n: int) -> Dict[str, np.ndarray]:
    """n successful take-ons, tackles, dribbles and bad touches by alternating teams: no row
    expands, in either operator."""
    idx = np.arange(n, dtype=np.int64)
    return _single_game(n, team_id=5 + idx % 2, type_id=np.array([7, 9, 21, 19])[idx % 4],
                        result_id=np.ones(n, np.int64))


def prefix(f: Dict[str, np.ndarray], n: int) -> Dict[str, np.ndarray]:
    return {c: v[:n] for c, v in f.items()}


def shuffled(f: Dict[str, np.ndarray], seed: int = 3) -> Dict[str, np.ndarray]:
    """The same rows in a seeded random order (the ``order`` path / lexsort placement)."""
    p = np.random.default_rng(seed).permutation(len(f['type_id']))
    return {c: v[p] for c, v in f.items()}


def shuffled_runs(f: Dict[str, np.ndarray], seed: int = 4) -> Dict[str, np.ndarray]:
    """The two-row runs of an :func:`enum_frame` in a seeded random order, each run's rows still
    next to each other: the keys are out of order, yet every row keeps its input-order successor
    (a full shuffle leaves hardly a pair of neighbours in one game or team, so what reads the
    input order -- the receival rule, ``_add_dribbles`` -- inserts next to nothing)."""
    p = np.random.default_rng(seed).permutation(len(f['type_id']) // 2)
    p = np.stack([2 * p, 2 * p + 1], axis=1).reshape(-1)
    return {c: v[p] for c, v in f.items()}


def duplicated_keys(f: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """``action_id // 3``: keys repeat, so conversion takes the general path."""
    return dict(f, action_id=f['action_id'] // 3)


def group_shapes(f: Dict[str, np.ndarray], out: Dict[str, np.ndarray]) -> List[Tuple[str, ...]]:
    """The shape of every input row's group in a conversion output: the names of the rows between
    the first output row with the input row's event id and the first with the next one's (a card,
    goal or receival carries its parent's event id, a dribble none).  ``f`` is in key order with
    unique event ids."""
    index = {e: i for i, e in enumerate(f['original_event_id'])}
    assert len(index) == len(f['type_id'])
    owner = np.array([-1 if e is None else index[e] for e in out['original_event_id']], np.int64)
    assert owner[0] == 0 and (np.diff(owner[owner >= 0]) >= 0).all()  # the groups are in order
    owner = np.maximum.accumulate(owner)            # a dribble belongs to the row before it
    start = np.searchsorted(owner, np.arange(len(index) + 1), 'left')
    assert (np.diff(start) >= 1).all()
    types = np.asarray(out['type_id'])
    shapes: List[Tuple[str, ...]] = [()] * len(index)
    for i in np.flatnonzero(np.diff(start) > 1):
        shapes[i] = tuple(INSERTED[int(t)] for t in types[start[i] + 1:start[i + 1]])
    return shapes


# ------------------------------------------------------------------------------- tiling
ID_COLS = ('game_id', 'team_id', 'player_id')


def tile_base(n_games: int = 30, seed: int = 41) -> Dict[str, np.ndarray]:
    """Synthetic games (socceraction_amd.synthetic) with a tenth of the results redrawn from 0..5
    and a twentieth of the types from 0..22, so that cards, owngoals and offsides meet every type;
    global action ids."""
    from socceraction_amd import synthetic
    d = synthetic.spadl_games(n_games, seed=seed)
    n = len(d['type_id'])
    rng = np.random.default_rng([seed, 1])
    res = d['result_id'].copy()
    m = rng.random(n) < 0.1
    res[m] = rng.integers(0, 6, int(m.sum()))
    typ = d['type_id'].copy()
    m = rng.random(n) < 0.05
    typ[m] = rng.integers(0, 23, int(m.sum()))
    out = {c: d[c] for c in COLS if c in d}
    out.update(type_id=typ, result_id=res, action_id=np.arange(n, dtype=np.int64),
               player_id=(d['team_id'] * 100 + d['pos'] % 11).astype(np.int64),
               original_event_id=np.arange(n, dtype=np.int64))
    return {c: out[c] for c in COLS}


def event_index(col: np.ndarray) -> np.ndarray:
    """An event id column of integers and None as int64, None -> -1."""
    col = np.asarray(col)
    if col.dtype != object:
        return col.astype(np.int64)
    return np.array([-1 if e is None else e for e in col], np.int64)


@dataclass
class Tiled:
    """``cols``: the first n rows of the base repeated, copy k with k * ``shift[c]`` added to id
    column c and k * ``base_len`` to the (integer) event ids, action ids 0..n-1.  ``full`` /
    ``part``: the oracle's output for the base and for its first ``rest`` rows (None when n is a
    multiple of the base), event ids as int64 with -1 = missing."""

    cols: Dict[str, np.ndarray]
    base_len: int
    copies: int
    rest: int
    shift: Dict[str, int]
    full: Dict[str, np.ndarray]
    part: Optional[Dict[str, np.ndarray]]

    def shifted(self, out: Dict[str, np.ndarray], k: int) -> Dict[str, np.ndarray]:
        res = dict(out)
        for c in ID_COLS:
            res[c] = out[c] + k * self.shift[c]
        ev = out['original_event_id']
        res['original_event_id'] = np.where(ev >= 0, ev + k * self.base_len, -1)
        return res

    def expected(self) -> Dict[str, np.ndarray]:
        """The whole expected output (host memory: for small n)."""
        parts = [self.shifted(self.full, k) for k in range(self.copies)]
        if self.part is not None:
            parts.append(self.shifted(self.part, self.copies))
        res = {c: np.concatenate([p[c] for p in parts]) for c in self.full}
        res['action_id'] = np.arange(len(res['type_id']), dtype=np.int64)
        return res


def dribble_src(out: Dict[str, np.ndarray]) -> np.ndarray:
    """``src`` of an ``add_dribbles`` output whose input had event ids 0..n-1 and every dribble
    directly before its successor: the input row, or ~successor for a dribble (event -1)."""
    ev = out['original_event_id']
    assert ev[-1] >= 0
    return np.where(ev >= 0, ev, ~np.r_[ev[1:], 0])


def assert_tiled_on_device(t: Tiled, got, n_out: int, uniques, names: Dict[str, str]) -> None:
    """Compare device columns with a tiled expectation without copying them back: ``got[names[c]]``
    (torch tensors, codes as in the frame whose ``uniques`` decode them; event codes are the event
    ids) against column c of ``t.full`` for every whole copy -- one [copies, rows] comparison per
    column after adding the copy's offsets -- and of ``t.part`` for the rest.  Floats are compared
    as bit patterns."""
    import torch
    lf = len(t.full['type_id'])
    lp = len(t.part['type_id']) if t.part is not None else 0
    assert n_out == t.copies * lf + lp, (n_out, t.copies, lf, lp)
    key = {'game_id': 'game', 'team_id': 'team', 'player_id': 'player'}
    for c, name in names.items():
        col = got[name][:n_out]
        dev = col.device
        for exp, lo, hi, k0 in ((t.full, 0, t.copies * lf, 0), (t.part, t.copies * lf, n_out, t.copies)):
            if exp is None or hi == lo:
                continue
            e = torch.from_numpy(np.ascontiguousarray(exp[c])).to(dev)[None, :]
            g = col[lo:hi]
            if e.dtype == torch.float64:
                assert g.dtype == torch.float64, c
                g, e = g.view(torch.int64), e.view(torch.int64)
            g = g.reshape(-1, e.shape[1]).long()
            k = k0 + torch.arange(g.shape[0], device=dev, dtype=torch.int64)[:, None]
            if c in ID_COLS:
                ids = torch.from_numpy(uniques[key[c]].to_numpy().astype(np.int64)).to(dev)
                assert bool(((g >= 0) & (g < len(ids))).all()), f'{c}: a code outside the frame\'s'
                g = ids[g]
                e = e + k * t.shift[c]
            elif c == 'original_event_id':
                e = torch.where(e >= 0, e + k * t.base_len, e)
            elif c == 'src':
                e = torch.where(e >= 0, e + k * t.base_len, e - k * t.base_len)
            bad = g != e
            if bool(bad.any()):
                i = int(bad.reshape(-1).nonzero()[0])
                raise AssertionError(f'{c}: {int(bad.sum())} rows differ, first at output row {lo + i} '
                                     f'(copy {k0 + i // e.shape[1]}, row {i % e.shape[1]} of its output)')


def tiled(base: Dict[str, np.ndarray], n: int,
          oracle: Callable[[Dict[str, np.ndarray]], Dict[str, np.ndarray]]) -> Tiled:
    """The first n rows of ``base`` repeated (see :class:`Tiled`) and what ``oracle`` -- the
    oracle's ``convert_to_atomic`` or ``add_dribbles`` -- makes of them, assembled from its output
    for the base alone.  The identity holds when the copies share no game and no team: the last
    row of a copy then gets from the next copy's first row what it gets from no row at all (a
    receival or an out needs the same game, a dribble the same team), which is also why a
    truncated last copy is the oracle's output for that prefix.  ``base`` is in key order;
    tests/test_convert_host.py checks the identity against the oracle run on the whole."""
    L = len(base['type_id'])
    base = dict(base, original_event_id=np.arange(L, dtype=np.int64),
                action_id=np.arange(L, dtype=np.int64))
    copies, rest = divmod(n, L)
    shift = {c: int(base[c].max()) + 1 for c in ID_COLS}
    assert all(int(base[c].min()) >= 0 for c in ID_COLS)
    reps = copies + (rest > 0)
    k = np.repeat(np.arange(reps, dtype=np.int64), L)[:n]
    cols = {}
    for c in COLS:
        v = np.tile(base[c], reps)[:n]
        if c in ID_COLS:
            v = v + k * shift[c]
        elif c == 'original_event_id':
            v = v + k * L
        cols[c] = v
    cols['action_id'] = np.arange(n, dtype=np.int64)

    def run(f):
        out = oracle(f)
        return dict(out, original_event_id=event_index(out['original_event_id']))

    return Tiled(cols, L, copies, rest, shift, run(base), run(prefix(base, rest)) if rest else None)
