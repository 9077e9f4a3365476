"""Deterministic inputs for the layer that hands device results to the user: the bitmap kernel
``sa_pack_bits`` (csrc/sa_store.hip), the pipelined pandas boundary ``pipeline.value_frames`` and
the Parquet writers of ``store.py`` (pure numpy / pandas, no device).

* :func:`pack_source`: a tiled byte block whose true values are ANY non-zero byte and whose rows
  at or beyond ``n`` are all 0xFF (the rest of the last 16-row group, of the last tile and any
  spare tile), with numpy's little-endian bitmap of it.  :data:`PACK_NS` puts ``n`` on both
  sides of a bitmap byte, of a 16-row group and of one 256-thread workgroup (4096 rows).
* :func:`games_of` / the edge batch of tests/window_cases.py as ``(games, actions)`` frames with
  string team ids: game starts on every residue mod 8, games of 1 to 1025 rows.
* :func:`unaligned`: frames whose every interior game start is off a 4-row boundary, so that
  no cut ``pipeline._chunks`` can choose is aligned: the pitched copies of the 1-byte bool and
  label blocks then start at addresses that are no multiple of 4.
* :func:`defective`: the edge frame with a defect in its LAST game, behind a long game that is
  a chunk of its own, for the failure path of the chunk loop.

tests/test_boundary_host.py holds the conditions the device tests (tests/test_gpu_pack_bits.py,
tests/test_gpu_boundary.py) rest on.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np
import pandas as pd

import window_cases as wc

# ------------------------------------------------------------------ sa_pack_bits
PACK_BYTES = (0, 0, 0, 1, 2, 0x10, 0x80, 0xFF)   # any non-zero byte is true
PACK_FILL = 0xFF                                  # every source row at or beyond n
PACK_GROUP = 16                                   # rows per thread: one 16-byte load, 2 bitmap bytes
PACK_THREADS = 256                                # threads per workgroup (PB_THREADS)
PACK_NS = (1, 8, 9, 15, 16, 17, 4095, 4096, 4097, 4113)
PACK_CS = (1, 7)
PLAN_WIDTH_N = 33                                 # the row count of the one plan-wide case
GUARD = 0xA5                                      # prefill of an output buffer the test owns
GUARD_BYTES = 64                                  # after the last column


def groups(n: int) -> int:
    return -(-n // PACK_GROUP)


def roundup16(n: int) -> int:
    return groups(n) * PACK_GROUP


def pack_layouts(n: int) -> List[Tuple[str, int, int]]:
    """(tag, tile_rows, tiles): one tile; every 16-row group its own tile; tiles of 48 rows; tiles
    of 1024 rows with one spare tile after the last used one."""
    return [('one tile', roundup16(n), 1), ('tiles of 16', 16, groups(n)),
            ('tiles of 48', 48, -(-n // 48)), ('tiles of 1024 + spare', 1024, -(-n // 1024) + 1)]


def pack_source(n: int, C: int, tile_rows: int, tiles: int, seed: int = 11) -> Tuple[np.ndarray, np.ndarray]:
    """(block ``[tiles, C, tile_rows]`` uint8, reference ``[C, 2 * groups(n)]`` uint8): the
    block's rows < n drawn from :data:`PACK_BYTES`, every other row :data:`PACK_FILL`; the
    reference is ``np.packbits(bitorder='little')`` of ``byte != 0`` padded with zero bits."""
    assert tile_rows % PACK_GROUP == 0 and tiles * tile_rows >= roundup16(n)
    rng = np.random.default_rng([seed, n, C, tile_rows])
    flat = np.full((C, tiles * tile_rows), PACK_FILL, np.uint8)
    flat[:, :n] = rng.choice(np.array(PACK_BYTES, np.uint8), (C, n))
    block = np.ascontiguousarray(flat.reshape(C, tiles, tile_rows).transpose(1, 0, 2))
    ref = np.zeros((C, 2 * groups(n)), np.uint8)
    packed = np.packbits(flat[:, :n] != 0, axis=1, bitorder='little')
    ref[:, :packed.shape[1]] = packed
    return block, ref


# ------------------------------------------------------------------ the edge batch as frames
CHUNK_ROWS = (1, 64, 700)          # then n + 1 (the ramp alone: n / 4, n / 2, the rest) and 4 n + 4
EDGE_CHUNKS = (47, 36, 7, 3, 1)    # pipeline._chunks of the edge batch at edge_chunk_rows(n)


def edge_chunk_rows(n: int) -> Tuple[int, ...]:
    """``chunk_rows`` of the edge-batch cases: one chunk only from 4 n + 4 on, since the first
    chunk of the ramp is a quarter of ``chunk_rows``."""
    return CHUNK_ROWS + (n + 1, 4 * n + 4)


PARTS = 3                          # part files of the Parquet tests
ROW_GROUP = 64                     # rows per row group there


def games_of(homes, ids=None) -> pd.DataFrame:
    ids = np.arange(len(homes), dtype=np.int64) if ids is None else ids
    return pd.DataFrame({'game_id': ids, 'home_team_id': list(homes)})


def edge(atomic: bool, seed: int = 1) -> Tuple[pd.DataFrame, pd.DataFrame]:
    """(games, actions) of the edge batch: string team ids, a third of the homes absent."""
    df, homes = wc.frame(atomic, seed)
    return games_of(homes), df


def part_bounds(off: np.ndarray, parts: int) -> List[int]:
    """The key ranges ``FeatureStore.put_many`` gives each part file (contiguous keys of about
    equal row counts)."""
    nk = len(off) - 1
    cuts = np.searchsorted(off, np.linspace(0, off[-1], parts + 1)[1:-1])
    return [0] + sorted(set(int(c) for c in cuts if 0 < c < nk)) + [nk]


# ------------------------------------------------------------------ unaligned cuts
UNALIGNED_FIRST = (1, 2, 3)
UNALIGNED_MIDDLE = (4, 8, 12, 4, 16, 4, 20, 8, 4, 4, 64, 4, 8, 132) + (4,) * 26
UNALIGNED_LAST = 5
UNALIGNED_CHUNK_ROWS = (1, 16, 100)
UNALIGNED_CHUNKS = (42, 18, 7)     # at a first game of 3 rows (at 1: every game a chunk of its own)


def _frames(lengths, atomic: bool, seed: int) -> Tuple[pd.DataFrame, pd.DataFrame, Dict[str, np.ndarray]]:
    """Games of the given lengths (``window_cases._game``: three team ids each) as (games,
    actions, the oracle's input: columns, ``game_off``, ``home_team_id``).  Game i's home is
    team 100, 101, 102 or (every fourth game) one no row carries."""
    parts = []
    for i, m in enumerate(lengths):
        g = wc._game(int(m), atomic, seed + i)
        g['game_id'] = np.int64(1000 + i)
        parts.append(g)
    actions = pd.concat(parts, ignore_index=True)
    homes = np.array([100 + (i % 4 if i % 4 < 3 else 5) for i in range(len(lengths))], np.int64)
    games = games_of(homes, 1000 + np.arange(len(lengths), dtype=np.int64))
    d = {c: actions[c].to_numpy() for c in (wc.ATOMIC_COLS if atomic else wc.SPADL_COLS)}
    d['game_off'] = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    d['home_team_id'] = homes
    return games, actions, d


@lru_cache(maxsize=None)
def unaligned(first: int, atomic: bool):
    """(games, actions, oracle input) of a frame whose interior game starts are all off a
    multiple of 4 rows and whose row count is no multiple of 16.  Cached: read-only."""
    return _frames((first,) + UNALIGNED_MIDDLE + (UNALIGNED_LAST,), atomic, 200 + 50 * first)


@lru_cache(maxsize=None)
def degenerate(n: int, atomic: bool):
    """(games, actions, oracle input) of one game of n rows (n = 0: the empty frame with the
    columns and dtypes of the others)."""
    games, actions, d = _frames((max(n, 1),), atomic, 77)
    if n == 0:
        actions = actions.iloc[:0].reset_index(drop=True)
        d = {c: v[:0] for c, v in d.items() if c not in ('game_off', 'home_team_id')}
        d.update(game_off=np.zeros(1, np.int64), home_team_id=np.zeros(0, np.int64))
    return games, actions, d


# ------------------------------------------------------------------ a defect in the last game
# the long game is the chunk right before the defective one: its copy out (about 515 bytes per
# row) is the one still running when the last game's validation raises
LONG_GAME_ROWS = 1 << 17
DEFECTS = ('type_id out of range', 'NaN type_id', 'missing team_id')


def defective(defect: str, atomic: bool = False, long_rows: int = None) -> Tuple[pd.DataFrame, pd.DataFrame]:
    """(games, actions): the edge frame, a long game added before its last game (ending on a
    multiple of 4 rows, so ``_chunks`` keeps it a chunk of its own), and ``defect`` in one row of
    the last game."""
    long_rows = LONG_GAME_ROWS if long_rows is None else long_rows
    games, df = edge(atomic)
    last = int(df['game_id'].iloc[-1])
    head, tail = df[df['game_id'] != last], df[df['game_id'] == last].copy()
    parts = [head]
    if long_rows:
        m = long_rows + (-(len(head) + long_rows)) % 4
        g = wc._game(m, atomic, 5)[list(df.columns)]
        g['game_id'] = np.int64(last + 1)
        g['team_id'] = ['team-%d' % t for t in g['team_id']]
        parts.append(g)
        games = pd.concat([games, games_of(['team-100'], np.array([last + 1], np.int64))],
                          ignore_index=True)
    row = tail.index[len(tail) // 2]
    if defect == 'type_id out of range':
        tail.loc[row, 'type_id'] = 99
    elif defect == 'NaN type_id':
        parts = [p.astype({'type_id': np.float64}) for p in parts]
        tail = tail.astype({'type_id': np.float64})
        tail.loc[row, 'type_id'] = np.nan
    elif defect == 'missing team_id':
        tail.loc[row, 'team_id'] = None
    else:
        raise ValueError(defect)
    return games, pd.concat(parts + [tail], ignore_index=True)
