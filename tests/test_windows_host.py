"""The conditions tests/test_gpu_windows.py relies on, asserted on the inputs alone (no device):
the edge batch of tests/window_cases.py puts segment starts where the kernels of csrc/sa_vaep.hip
cut a batch, and the oracle's outputs on it leave no column, label or branch constant."""
import numpy as np
import pytest

import window_cases as wc
from oracle import vaep_oracle as vo

PACKAGES = [False, True]


@pytest.mark.parametrize('atomic', PACKAGES)
def test_segment_starts_meet_every_boundary(atomic):
    d = wc.batch(atomic)
    off = d['game_off']
    n = int(off[-1])
    starts = off[:-1]
    assert 4000 < n < 10000 and len(starts) > 170
    assert (np.diff(off) >= 1).all()
    assert set(starts % wc.LANE_ACTS) == set(range(wc.LANE_ACTS))
    for q in (wc.SEG_BLOCK, wc.BLOCK_ACTS, wc.BOOL_TILE):
        assert {q - 1, 0, 1} <= set((starts % q).tolist()), q
    for q in (wc.LANE_ACTS, wc.SEG_BLOCK, wc.BLOCK_ACTS, wc.BOOL_TILE):
        assert n % q, q
    sizes = set(np.diff(off).tolist())
    for big in (2 * wc.LANE_ACTS, wc.SEG_BLOCK, wc.BLOCK_ACTS, wc.BOOL_TILE):
        assert {big - 1, big, big + 1} <= sizes
    # a segment shorter than, equal to and longer than every window depth and look-ahead in use
    for k in set(wc.KS) | set(wc.BITMAP_KS) | set(wc.NR_ACTIONS) | set(wc.STEP_NR):
        assert k in sizes and max(sizes) > k and (k == 1 or min(sizes) < k), k


@pytest.mark.parametrize('atomic', PACKAGES)
def test_columns_cover_their_ranges(atomic):
    d = wc.batch(atomic)
    off = d['game_off']
    n = int(off[-1])
    assert set(d['type_id'].tolist()) == set(range(wc.N_TYPES[atomic]))
    assert set(d['bodypart_id'].tolist()) == set(range(4))
    assert set(d['period_id'].tolist()) == set(range(1, 6))
    if not atomic:
        assert set(d['result_id'].tolist()) == set(range(6))
    t = d['time_seconds']
    gaps = np.diff(t)
    assert (gaps > 0).all() and (gaps < 10).any() and (gaps == 10).any() and (gaps > 10).any()
    assert (t * 2 == np.round(t * 2)).all() and t[-1] < 2.0 ** 40  # exact differences
    # teams: two per game, three in every seventh (long enough); a third of the homes absent
    g = np.repeat(np.arange(len(off) - 1), np.diff(off))
    per_game = np.array([len(set(d['team_id'][off[i]:off[i + 1]].tolist())) for i in range(len(off) - 1)])
    assert per_game.max() == 3 and (per_game[np.diff(off) >= 3] >= 2).mean() > 0.9
    assert (per_game[np.arange(len(per_game)) % wc.THIRD_TEAM_EVERY != 3] <= 2).all()
    assert (per_game == 3).sum() >= 15
    away = d['team_id'] != d['home_team_id'][g]
    absent = np.array([d['home_team_id'][i] not in d['team_id'][off[i]:off[i + 1]]
                       for i in range(len(off) - 1)])
    assert absent[np.arange(len(absent)) % wc.ABSENT_HOME_EVERY == 2].all()
    assert 1 / wc.ABSENT_HOME_EVERY <= absent.mean() < 0.5  # short games may miss their home too
    assert away[np.repeat(absent, np.diff(off))].all() and not away.all()
    # a third team code inside the 32-row window of a lane whose own rows are valid
    t3 = np.flatnonzero(d['team_id'] % 10 == 2)
    assert len(t3) > 50
    # the string-team frame factorises to the same equalities, the absent homes to -1
    from socceraction_amd.batch import encode_teams
    df, homes = wc.frame(atomic)
    codes, hc = encode_teams(df['team_id'].to_numpy(), homes)
    assert len(df) == n and ((hc == -1) == absent).all()
    np.testing.assert_array_equal(codes[1:] == codes[:-1], d['team_id'][1:] == d['team_id'][:-1])
    np.testing.assert_array_equal(codes != np.repeat(hc, np.diff(off)), away)


@pytest.mark.parametrize('atomic', PACKAGES)
@pytest.mark.parametrize('k', wc.HOST_KS)
def test_no_bool_feature_is_constant(atomic, k):
    d = wc.batch(atomic)
    xfns = vo.ATOMIC_DEFAULT if atomic else vo.SPADL_DEFAULT
    ref = vo.features(wc.cols_of(d, atomic), k, xfns, atomic=atomic, seg_off=d['game_off'],
                      home=d['home_team_id'])
    const = [nm for nm, kind, v in ref if kind == 'b' and (v.all() or not v.any())]
    assert not const, const
    assert sum(kind == 'b' for _, kind, _ in ref) > 30 * k


@pytest.mark.parametrize('atomic', PACKAGES)
def test_every_label_holds_both_values(atomic):
    d = wc.batch(atomic)
    cols = wc.cols_of(d, atomic)
    for nr in sorted(set(wc.NR_ACTIONS) | set(wc.STEP_NR)):
        lab = vo.labels(cols, atomic=atomic, nr_actions=nr, seg_off=d['game_off'])
        for c, v in lab.items():
            assert v.any() and not v.all(), (c, nr)
        if atomic:
            assert lab['goal_from_shot'].sum() >= 50
    if atomic:  # shot -> goal pairs that straddle a segment end are no goal from a shot
        t, off = d['type_id'], d['game_off']
        ends = off[1:-1]
        straddle = ends[(t[ends - 1] == 11) & (t[ends] == 27)]
        assert len(straddle) >= 10
        assert not vo.labels(cols, atomic=True, seg_off=off)['goal_from_shot'][straddle - 1].any()


@pytest.mark.parametrize('atomic', PACKAGES)
def test_permuted_frames_are_no_shifts(atomic):
    n = wc.EXPLICIT_NS[-1]
    frames = wc.permuted_frames(n, 3, atomic)
    t = [f['time_seconds'].to_numpy() for f in frames]
    for f in frames:
        assert f.index.equals(frames[0].index) and len(f) == n
    for i in (1, 2):
        assert sorted(t[i].tolist()) == t[0].tolist() and (t[i] != t[0]).mean() > 0.9
        shifted = t[0][np.maximum(np.arange(n) - i, 0)]
        assert (t[i] != shifted).mean() > 0.9
        for c in ('team_id', 'type_id'):
            assert (frames[i][c].to_numpy() != frames[0][c].to_numpy()).any()
