"""The conditions tests/test_gpu_pack_bits.py and tests/test_gpu_boundary.py rest on, asserted on
the inputs of tests/boundary_cases.py alone, and the host-side refusals of the same layer: calls
of ``sa_pack_bits`` that launch nothing, a ``game_id`` listed twice in ``games``, and a
``game_id`` that heads two runs of rows in front of the Parquet writers.  No device."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import boundary_cases as bc
import window_cases as wc

PACKAGES = [False, True]


# ------------------------------------------------------------------ sa_pack_bits inputs
def test_pack_sources_hold_what_the_device_cases_claim():
    per_wg = bc.PACK_THREADS * bc.PACK_GROUP
    assert per_wg == 4096
    assert {bc.groups(n) for n in bc.PACK_NS} >= {1, 2, bc.PACK_THREADS, bc.PACK_THREADS + 1,
                                                 bc.PACK_THREADS + 2}
    assert {n % 16 for n in bc.PACK_NS} >= {0, 1, 8, 9, 15}
    assert set(bc.PACK_BYTES) - {0, 1} and not all(b & 1 for b in bc.PACK_BYTES if b)
    for n in bc.PACK_NS:
        layouts = bc.pack_layouts(n)
        assert [t for t, _, _ in layouts] == ['one tile', 'tiles of 16', 'tiles of 48',
                                              'tiles of 1024 + spare']
        for tag, R, tiles in layouts:
            blk, ref = bc.pack_source(n, 7, R, tiles)
            assert blk.shape == (tiles, 7, R) and blk.dtype == np.uint8 and R % 16 == 0
            flat = blk.transpose(1, 0, 2).reshape(7, -1)
            assert flat.shape[1] >= bc.roundup16(n) and (flat[:, n:] == bc.PACK_FILL).all()
            if n >= 4095:  # every source byte occurs; bytes a `& 1` test would get wrong
                assert set(np.unique(flat[:, :n]).tolist()) == set(bc.PACK_BYTES)
                assert ((flat[:, :n] != 0) != ((flat[:, :n] & 1) != 0)).mean() > 0.2
            assert ref.shape == (7, 2 * bc.groups(n))
            np.testing.assert_array_equal(
                np.unpackbits(ref, axis=1, bitorder='little')[:, :n], flat[:, :n] != 0)
            assert not np.unpackbits(ref, axis=1, bitorder='little')[:, n:].any()
            if 0 < n % 16 <= 8:  # the byte only the tail mask clears
                assert -(-n // 8) == ref.shape[1] - 1 and not ref[:, -1].any()
        assert layouts[3][2] * 1024 >= bc.roundup16(n) + 1024   # a whole spare tile
        assert layouts[1][2] == bc.groups(n)
    for n in (4097, 4113):  # a second workgroup in x, holding one and two groups
        assert -(-bc.groups(n) // bc.PACK_THREADS) == 2
        assert bc.groups(n) - bc.PACK_THREADS == (1 if n == 4097 else 2)
    stride = 2 * bc.groups(4113) + 6
    assert stride % 2 == 0 and stride % 64


def test_pack_bits_refuses_bad_calls_before_any_launch():
    """Every refusal of sa_pack_bits comes before its launch, so it can be asked for here; n == 0
    and zero columns are SA_OK with null pointers."""
    from socceraction_amd import _native
    lib = _native.load_library()
    n = 100
    need = 2 * bc.groups(n)

    def call(n=n, C=7, R=112, data=256, bits=512, stride=need, blk=True):
        b = _native.SaBlock()
        b.data, b.n_cols, b.tile_rows = data, C, R
        return lib.sa_pack_bits(ctypes.byref(b) if blk else None, n, bits, stride, None)

    refused = dict(null_descriptor=dict(blk=False), negative_n=dict(n=-1), tile_of_8=dict(R=8),
                   tile_of_24=dict(R=24), block_8_mod_16=dict(data=264), odd_stride=dict(stride=need + 1),
                   stride_2_short=dict(stride=need - 2), odd_bits=dict(bits=513),
                   too_many_columns=dict(C=65536), negative_columns=dict(C=-1),
                   null_block=dict(data=None), null_bits=dict(bits=None))
    for tag, kw in refused.items():
        assert call(**kw) == _native.SA_EINVAL, tag
        assert lib.sa_last_error(), tag
        with pytest.raises(ValueError):
            _native.check(_native.SA_EINVAL)
    assert call(n=0, data=None, bits=None, stride=0) == _native.SA_OK
    assert call(C=0, data=None, bits=None, stride=0) == _native.SA_OK


def test_an_empty_batch_is_not_refused_for_its_null_columns():
    """The columns of an empty batch have no address.  ``sa_vaep_features`` checks the columns
    of a batch that has rows only, so the empty frame reaches the entry point's own ``n == 0``
    return (``compute_features_batch`` and ``store_features_batch`` of no action)."""
    from socceraction_amd import _native
    lib = _native.load_library()
    plan = _native.SaFeaturePlan()
    for n, named in ((1, True), (0, False)):
        s = _native.SaActions()
        s.n, s.n_segments, s.n_frames, s.seg_off = n, 1, 1, 256
        rc = lib.sa_vaep_features(ctypes.byref(s), ctypes.byref(plan), None, None, None, 0, 0, None, None)
        assert rc == _native.SA_EINVAL   # a plan of depth 0: refused later, nothing is ever launched
        assert (b'null column' in lib.sa_last_error()) == named


# ------------------------------------------------------------------ the edge batch under _chunks
@pytest.mark.parametrize('atomic', PACKAGES)
def test_edge_batch_chunks(atomic):
    """The chunkings the device cases name: 47, 36, 7, 3 (``chunk_rows = n + 1``: the ramp's
    quarter, half and the rest) and 1 chunks of 3 to 4,740 rows, both slots reused up to 23 times;
    the cuts at 64 and 700 rows are all aligned (a mutation that rounds the 1-byte copies' first
    row down to a multiple of 4 does not show there)."""
    from socceraction_amd import pipeline
    d = wc.batch(atomic)
    off = d['game_off']
    n = int(off[-1])
    assert (n, len(off) - 1) == (7190, 186)
    counts, rows = [], []
    for chunk in bc.edge_chunk_rows(n):
        cuts = pipeline._chunks(off, chunk)
        assert cuts[0][0] == 0 and cuts[-1][1] == len(off) - 1
        assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        counts.append(len(cuts))
        if chunk in bc.CHUNK_ROWS:
            rows += [int(off[s1] - off[s0]) for s0, s1 in cuts]
    assert tuple(counts) == bc.EDGE_CHUNKS
    assert min(rows) == 3 and max(rows) == 4740
    assert (max(counts) - 1) // 2 == 23
    for chunk in (64, 700):
        assert all(off[s0] % 4 == 0 for s0, _ in pipeline._chunks(off, chunk))
    games, actions = bc.edge(atomic)
    assert len(actions) == n and actions['team_id'].map(type).eq(str).all()
    assert games['game_id'].is_unique and len(games) == len(off) - 1
    assert (~games['home_team_id'].isin(actions['team_id'])).mean() >= 1 / 3


@pytest.mark.parametrize('atomic', PACKAGES)
@pytest.mark.parametrize('first', bc.UNALIGNED_FIRST)
def test_unaligned_frames_leave_no_aligned_cut(first, atomic):
    from socceraction_amd import pipeline
    from socceraction_amd.batch import segment_offsets
    games, actions, d = bc.unaligned(first, atomic)
    off = d['game_off']
    n = len(actions)
    np.testing.assert_array_equal(segment_offsets(actions['game_id'].to_numpy()), off)
    assert len(off) - 1 == 42 and n == off[-1] and n % 16
    assert (off[1:-1] % 4 != 0).all()
    assert all(m % 4 == 0 for m in bc.UNALIGNED_MIDDLE) and len(bc.UNALIGNED_MIDDLE) == 40
    assert max(bc.UNALIGNED_MIDDLE) > max(bc.UNALIGNED_CHUNK_ROWS)   # a game longer than chunk_rows
    counts = []
    for chunk in bc.UNALIGNED_CHUNK_ROWS:
        cuts = pipeline._chunks(off, chunk)
        assert cuts[0][0] == 0 and cuts[-1][1] == 42 and len(cuts) >= 3
        assert all(off[s0] % 4 for s0, _ in cuts[1:]), chunk
        if chunk == 1:  # copies a few bytes wide, and one-row chunks when the first game has one
            assert min(int(off[s1] - off[s0]) for s0, s1 in cuts) == min(first, 4)
        counts.append(len(cuts))
    if first == 3:
        assert tuple(counts) == bc.UNALIGNED_CHUNKS
    assert games['game_id'].tolist() == actions['game_id'].drop_duplicates().tolist()
    per_game = actions.groupby('game_id')['team_id'].nunique()
    assert per_game.max() == 3


@pytest.mark.parametrize('atomic', PACKAGES)
def test_degenerate_frames(atomic):
    for n in (40, 1, 0):
        games, actions, d = bc.degenerate(n, atomic)
        assert len(actions) == n == int(d['game_off'][-1]) and len(games) == 1
        assert list(actions.columns) == list(bc.degenerate(40, atomic)[1].columns)
        assert (actions.dtypes == bc.degenerate(40, atomic)[1].dtypes).all()


def test_defective_frames():
    """The defect sits in the last game, which is the last chunk; the chunk before it holds the
    long game; every earlier game is the edge batch's."""
    from socceraction_amd import pipeline
    from socceraction_amd.batch import encode_columns, encode_teams, segment_offsets
    good = bc.edge(False)[1]
    for defect in bc.DEFECTS:
        games, actions = bc.defective(defect)
        off = segment_offsets(actions['game_id'].to_numpy())
        assert games['game_id'].is_unique and set(actions['game_id']) == set(games['game_id'])
        cuts = pipeline._chunks(off, 64)
        assert len(cuts) > 30 and cuts[-1] == (len(off) - 2, len(off) - 1)
        s0, s1 = cuts[-2]
        assert off[s1] - off[s0] >= bc.LONG_GAME_ROWS and off[s1] % 4 == 0
        m = int(off[-1] - off[-2])
        pd.testing.assert_frame_equal(
            actions.iloc[:100].astype(good.dtypes.to_dict()), good.iloc[:100])
        ok = actions.iloc[:int(off[-2])]
        encode_columns(ok.iloc[-500:], False)
        encode_teams(ok['team_id'].to_numpy()[-500:])
        with pytest.raises(ValueError):
            bad = actions.iloc[-m:]
            encode_columns(bad, False)
            encode_teams(bad['team_id'].to_numpy())
    assert bc.defective(bc.DEFECTS[0], long_rows=0)[1].shape == good.shape


# ------------------------------------------------------------------ a game_id twice in games
@pytest.mark.parametrize('atomic', PACKAGES)
def test_from_frame_refuses_a_repeated_game_id(atomic):
    """``home_team_id.loc[gids]`` returns one home per MATCH: four homes for three games, and
    every game after the repeated one flipped by the wrong team.  It raises, naming the id,
    before the batch is built (no device is needed to get there)."""
    from socceraction_amd.batch import ActionBatch
    games, actions, _ = bc.unaligned(3, atomic)
    three = actions[actions['game_id'].isin(games['game_id'][:3])]
    twice = pd.concat([games.iloc[:2], games.iloc[1:3]], ignore_index=True)
    home_of = twice.set_index('game_id')['home_team_id']
    assert len(home_of.loc[games['game_id'][:3].to_numpy()]) == 4
    with pytest.raises(ValueError, match=f"game_id {games['game_id'][1]} occurs more than once"):
        ActionBatch.from_frame(three, atomic=atomic, home_team_id=home_of, segments='game')


# ------------------------------------------------------------------ the Parquet inputs
@pytest.mark.parametrize('atomic', PACKAGES)
def test_store_keys_meet_every_bitmap_and_row_group_edge(atomic):
    off = wc.batch(atomic)['game_off']
    bounds = bc.part_bounds(off, bc.PARTS)
    assert len(bounds) == bc.PARTS + 1 and all(b > a for a, b in zip(bounds, bounds[1:]))
    residues, spans, shared = set(), [], 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        start = off[a:b] - off[a]          # each key's first row in its part file
        end = off[a + 1:b + 1] - off[a]
        residues |= set((start % 8).tolist())
        first, last = start // bc.ROW_GROUP, (end - 1) // bc.ROW_GROUP
        spans += (last - first + 1).tolist()
        shared += sum(np.bincount(first)[g] > 1 for g in set(first.tolist()))
    assert residues == set(range(8))
    assert sum(s >= 3 for s in spans) >= 8 and max(spans) >= 16
    assert shared >= 20
    assert (np.diff(off) == 1).sum() >= 10   # one-row games


def test_store_writers_refuse_a_game_that_heads_two_runs(tmp_path):
    """One key per game: a second run of the same ``game_id`` would overwrite the first one's rows
    in the index.  Both writers raise before a batch is built or anything is written."""
    pytest.importorskip('pyarrow')
    from socceraction_amd import store
    from socceraction_amd.vaep import VAEP
    games, actions, d = bc.unaligned(3, False)
    off = d['game_off']
    again = pd.concat([actions.iloc[:off[3]], actions.iloc[off[1]:off[2]], actions.iloc[off[3]:]],
                      ignore_index=True)
    gid = int(actions['game_id'].iloc[off[1]])
    for write in (store.store_features_batch, store.store_labels_batch):
        p = tmp_path / write.__name__
        with store.FeatureStore(str(p), mode='w') as st:
            with pytest.raises(ValueError, match=f'game_id {gid} heads more than one run'):
                write(VAEP(), games, again, st)
            assert len(st) == 0 and st.keys() == []
        assert [f.name for f in p.iterdir()] == []
