"""GPU parity of ``_add_dribbles`` (reference spadl/base.py:54-93).

Against the reference's own outputs (tests/golden/dribbles_*.npz, made by
tests/golden/make_golden_dribbles.py: whole DataFrames, dtypes included) and, at larger sizes,
against the numpy restatement (oracle/atomic_convert_oracle.py ``add_dribbles``). Bar: every
column bit-exact (the kernel performs the reference's own f64 midpoint), same dtypes.
"""
import numpy as np
import pandas as pd
import pytest

import convert_cases as cc
from golden_io import assert_frame_same, cases, dribbles_frame, load

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from socceraction_amd._native import SA_ATOMIC_BLOCK_ROWS as B, SA_ATOMIC_SCAN_TILE as T  # noqa: E402

# the frame's last row on either side of the first and the second block edge
BLOCK_EDGES = (B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1)
# (rows, blocks): one block into the scan's second tile, one into its third
SCAN_SIZES = ((T * B + 1, T + 1), (2 * T * B + 77, 2 * T + 1))


@pytest.fixture(scope='module')
def sb():
    from socceraction_amd import _native
    from socceraction_amd.spadl import base
    _native.load_library()
    return base


@pytest.mark.parametrize('name', cases('dribbles'))
def test_add_dribbles_goldens(sb, name):
    g = load('dribbles', name)
    df = dribbles_frame(g, 'in_')
    ref = dribbles_frame(g, 'out_')
    assert_frame_same(sb._add_dribbles(df.copy()), ref, name)


def _synthetic(n_games, seed):
    from socceraction_amd import synthetic
    d = synthetic.spadl_games(n_games, seed=seed)
    df = synthetic.to_frame(d)
    df['original_event_id'] = [f'ev{i}' for i in range(len(df))]
    df['action_id'] = df.groupby('game_id').cumcount().astype(np.int64)
    return df


def _vs_oracle(got: pd.DataFrame, df: pd.DataFrame, name: str):
    from oracle import atomic_convert_oracle as co
    ref = co.add_dribbles({c: df[c].to_numpy() for c in co.COLS})
    assert len(got) == len(ref['type_id']), name
    for c in co.COLS:
        if c == 'original_event_id':
            np.testing.assert_array_equal(got[c].isna().to_numpy(), pd.isna(ref[c]), err_msg=name)
            continue
        np.testing.assert_array_equal(got[c].to_numpy(), np.asarray(ref[c]), err_msg=f'{name} {c}')


def test_add_dribbles_vs_oracle_300_games(sb):
    """~480k actions (per-game action ids: the game boundaries are checked for cross-game
    dribbles, which would take the general placement path)."""
    df = _synthetic(300, 95)
    got = sb._add_dribbles(df)
    _vs_oracle(got, df, 'synthetic-300')
    assert len(got) > len(df)


def test_add_dribbles_general_placement(sb):
    """Shuffled rows (stable lexsort placement) and global action ids (fast layout) agree
    with the oracle."""
    df = _synthetic(4, 96)
    rng = np.random.default_rng(0)
    shuffled = df.iloc[rng.permutation(len(df))].reset_index(drop=True)
    _vs_oracle(sb._add_dribbles(shuffled), shuffled, 'shuffled')
    glob = df.copy()
    glob['action_id'] = np.arange(len(glob), dtype=np.int64)
    _vs_oracle(sb._add_dribbles(glob), glob, 'global-ids')


def _vs_oracle_exact(got: pd.DataFrame, df: pd.DataFrame, name: str):
    """_vs_oracle, and every float column bit for bit."""
    from oracle import atomic_convert_oracle as co
    _vs_oracle(got, df, name)
    ref = co.add_dribbles({c: df[c].to_numpy() for c in co.COLS})
    for c in ('time_seconds', 'start_x', 'start_y', 'end_x', 'end_y'):
        np.testing.assert_array_equal(got[c].to_numpy().view(np.int64),
                                      np.asarray(ref[c], np.float64).view(np.int64),
                                      err_msg=f'{name} {c}')


@pytest.fixture(scope='module')
def enum():
    return cc.enum_frame()


@pytest.mark.parametrize('layout', ['per_game_ids', 'global_ids', 'shuffled', 'shuffled_runs'])
def test_add_dribbles_enumeration_vs_oracle(sb, enum, layout):
    """Every combination of (type, result, successor type, team, distance, period, game)
    (tests/convert_cases.py) == the restatement: with action ids restarting in every game (a
    dribble into the next game sorts behind that game's first row: lexsort placement), with
    global ids (the fast layout), with the rows shuffled (hardly two neighbours of one team left: the
    rows sorted back) and with the runs shuffled (every dribble, placed by the
    lexsort)."""
    f = enum
    if layout == 'global_ids':
        f = dict(f, action_id=np.arange(len(f['type_id']), dtype=np.int64))
    elif layout == 'shuffled':
        f = cc.shuffled(f)
    elif layout == 'shuffled_runs':
        f = cc.shuffled_runs(f)
    df = pd.DataFrame(f)
    got = sb._add_dribbles(df)
    if layout != 'shuffled':
        assert len(got) > len(df) + 1000
    _vs_oracle_exact(got, df, layout)


@pytest.mark.parametrize('n', BLOCK_EDGES)
@pytest.mark.parametrize('kind', ['dense', 'sparse'])
def test_add_dribbles_full_and_empty_blocks(sb, kind, n):
    """Blocks in which every row gets a dribble (2n - 1 rows out) or none does, with the frame's
    last row (no successor) on either side of a block edge."""
    df = pd.DataFrame(cc.dense_frame(n) if kind == 'dense' else cc.sparse_frame(n))
    got = sb._add_dribbles(df)
    assert len(got) == (2 * n - 1 if kind == 'dense' else n)
    _vs_oracle_exact(got, df, f'{kind}-{n}')


SPADL_DEVICE_COLS = {'game_id': 'game', 'original_event_id': 'event', 'period_id': 'period_id',
                     'time_seconds': 'time_seconds', 'team_id': 'team', 'player_id': 'player',
                     'start_x': 'start_x', 'start_y': 'start_y', 'end_x': 'end_x', 'end_y': 'end_y',
                     'type_id': 'type_id', 'result_id': 'result_id', 'bodypart_id': 'bodypart_id',
                     'src': 'src'}


@pytest.mark.parametrize('n, n_blocks', SCAN_SIZES)
def test_add_dribbles_scan_tiles(sb, n, n_blocks):
    """The scan of the block totals one block into its second tile and into its third: a 30-game
    base repeated to n rows with global action ids (the fast layout), every output column, ``src``
    and the row count against the oracle's output for the base, compared on the device."""
    from oracle import atomic_convert_oracle as co
    from socceraction_amd import _native
    from socceraction_amd.atomic.spadl import base as cb
    assert _native.lib().sa_atomic_scratch_bytes(n) == (n_blocks + 2) * 8  # the library's n_blocks
    t = cc.tiled(cc.tile_base(), n, co.add_dribbles)
    assert t.part is not None
    for ref in (t.full, t.part):
        ref['src'] = cc.dribble_src(ref)
    frame = cb.SpadlFrame.from_columns(t.cols)
    assert frame.n == n and 'order' not in frame.cols
    # from_columns has no event ids: give every row its own (the code is the id)
    frame.cols['event'].copy_(torch.arange(n, dtype=torch.int32, device=frame.buffer.device))
    out = sb.add_dribbles_device(frame, t.cols['action_id'])
    assert out.n_dribbles == out.n - n > 0
    cc.assert_tiled_on_device(t, out.cols, out.n, frame.uniques, SPADL_DEVICE_COLS)


def test_add_dribbles_thresholds_are_module_globals(sb):
    """The reference reads min/max_dribble_length and max_dribble_duration at call time."""
    from oracle import atomic_convert_oracle as co
    df = _synthetic(2, 97)
    base_n = len(sb._add_dribbles(df))
    old = sb.min_dribble_length, sb.max_dribble_length, sb.max_dribble_duration
    try:
        sb.min_dribble_length, sb.max_dribble_length, sb.max_dribble_duration = 1.0, 200.0, 100.0
        wide = sb._add_dribbles(df)
    finally:
        sb.min_dribble_length, sb.max_dribble_length, sb.max_dribble_duration = old
    assert len(wide) > base_n
    f = {c: df[c].to_numpy() for c in co.COLS}
    nx_team = np.r_[f['team_id'][1:], 0]
    dx = f['end_x'] - np.r_[f['start_x'][1:], 0.0]
    dy = f['end_y'] - np.r_[f['start_y'][1:], 0.0]
    dt = np.r_[f['time_seconds'][1:], 0.0] - f['time_seconds']
    d2 = dx ** 2 + dy ** 2
    same = (f['team_id'] == nx_team) & (f['period_id'] == np.r_[f['period_id'][1:], 0])
    expect = int((same & (d2 >= 1.0) & (d2 <= 40000.0) & (dt < 100.0)).sum())
    assert len(wide) - len(df) == expect


def test_add_dribbles_full_size(sb):
    """cfg2 size (10k games, ~16M actions) on device: n_out = n + dribbles; inputs keep their
    order; each dribble sits between its parent and successor with the reference's values."""
    from socceraction_amd import synthetic
    from socceraction_amd.atomic.spadl import base as cb
    d = synthetic.spadl_games(10000)
    df = synthetic.to_frame(d)
    df['original_event_id'] = None
    df['action_id'] = np.arange(len(df), dtype=np.int64)
    frame = cb.SpadlFrame.from_frame(df, sort=False)
    out = sb.add_dribbles_device(frame, df['action_id'].to_numpy())
    torch.cuda.synchronize()
    src = out.cols['src'][:out.n].cpu().numpy()
    orig = src >= 0
    np.testing.assert_array_equal(src[orig], np.arange(len(df)))
    pos = np.flatnonzero(~orig)
    assert len(pos) == out.n_dribbles > 0
    np.testing.assert_array_equal(src[pos - 1], ~src[pos] - 1)   # parent right before
    t = out.cols['time_seconds'][:out.n].cpu().numpy()
    ts = df['time_seconds'].to_numpy()
    q = ~src[pos]
    np.testing.assert_array_equal(t[pos], (ts[q - 1] + ts[q]) / 2)
    ty = out.cols['type_id'][:out.n].cpu().numpy()
    assert (ty[pos] == 21).all()
