"""Conditions on the inputs of tests/convert_cases.py that the device tests of the convert and
dribble expansions rely on, held on the CPU against oracle/atomic_convert_oracle.py: the
enumeration covers every reachable group shape, the dense and sparse frames expand to the counts
that fill or empty a block, and a tiled frame's expected output, assembled from the oracle's
output for the base, is the oracle's output for the whole."""
import collections
import os

import numpy as np
import pytest

import convert_cases as cc
from oracle import atomic_convert_oracle as co
from socceraction_amd._native import SA_ATOMIC_BLOCK_ROWS as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_native_constants_match_the_header():
    """_native mirrors the two launch constants of include/socceraction_amd.h that the device
    tests size their inputs by."""
    from socceraction_amd import _native
    with open(os.path.join(ROOT, 'include', 'socceraction_amd.h')) as f:
        src = f.read()
    for name in ('SA_ATOMIC_BLOCK_ROWS', 'SA_ATOMIC_SCAN_TILE'):
        line = [ln for ln in src.splitlines() if ln.startswith(f'#define {name} ')]
        assert len(line) == 1, name
        assert int(line[0].split()[2]) == getattr(_native, name), name


def _strictly_increasing_keys(f):
    d_g, d_p, d_a = np.diff(f['game_id']), np.diff(f['period_id']), np.diff(f['action_id'])
    return bool(((d_g > 0) | ((d_g == 0) & ((d_p > 0) | ((d_p == 0) & (d_a > 0))))).all())


@pytest.fixture(scope='module')
def full_enum():
    f = cc.enum_frame()
    return f, co.convert_to_atomic(f)


def test_enum_frame_is_a_valid_sorted_frame(full_enum):
    f, _ = full_enum
    n = len(f['type_id'])
    assert n == 2 * 23 * 6 * 23 * 2 * 3 * 2 * 2
    assert _strictly_increasing_keys(f)
    assert f['period_id'].min() == 1 and f['period_id'].max() == 5
    assert len(set(f['original_event_id'])) == n
    for c, hi in (('start_x', 105), ('end_x', 105), ('start_y', 68), ('end_y', 68)):
        assert f[c].min() >= 0 and f[c].max() <= hi, c
    gap = (f['time_seconds'][1::2] - f['time_seconds'][0::2])
    assert (gap > 10).sum() > 1000 and (gap < 10).sum() > 1000  # the duration rule, both ways


def test_enum_coverage_floor(full_enum):
    """Every reachable group shape occurs at least 8 times in the oracle's output of the full
    enumeration, no other shape occurs, and no row gets more than 3 inserted rows."""
    f, out = full_enum
    count = collections.Counter(cc.group_shapes(f, out))
    assert sum(count.values()) == len(f['type_id'])
    unlisted = set(count) - set(cc.REACHABLE_SHAPES) - {()}
    assert not unlisted, unlisted
    rare = {s: count[s] for s in cc.REACHABLE_SHAPES if count[s] < 8}
    assert not rare, rare
    assert max(map(len, count)) == cc.MAX_INSERTED
    # the shapes no synthetic game holds: a card on a pass-like row, before e1 and its dribble
    for card in ('yellow', 'red'):
        for e1 in ('receival', 'interception', 'out'):
            assert count[(card, e1, 'dribble')] >= 8 and count[(card, e1)] >= 8


def test_golden_enumeration_holds_every_shape():
    """The reduced enumeration the reference ran on (tests/golden/*_enum.npz) misses no shape."""
    g = cc.enum_frame(cc.GOLDEN_TYPES, cc.GOLDEN_SUCCESSORS)
    count = collections.Counter(cc.group_shapes(g, co.convert_to_atomic(g)))
    assert set(count) - {()} == set(cc.REACHABLE_SHAPES)


@pytest.mark.parametrize('n', [1, 2, B - 1, B, B + 1, 4 * B - 24])
def test_dense_and_sparse_counts(n):
    dense, sparse = cc.dense_frame(n), cc.sparse_frame(n)
    assert _strictly_increasing_keys(dense) and _strictly_increasing_keys(sparse)
    out = co.convert_to_atomic(dense)
    assert len(out['type_id']) == 4 * n - 2
    want = np.resize([0, 29, 23, 21], 4 * n)[:4 * n - 2]  # pass, yellow card, receival, dribble
    np.testing.assert_array_equal(out['type_id'], want)
    drib = co.add_dribbles(dense)
    assert len(drib['type_id']) == 2 * n - 1
    np.testing.assert_array_equal(drib['type_id'], np.resize([0, 21], 2 * n - 1))
    assert len(co.convert_to_atomic(sparse)['type_id']) == n
    assert len(co.add_dribbles(sparse)['type_id']) == n


@pytest.mark.parametrize('op', ['convert_to_atomic', 'add_dribbles'])
def test_tiled_identity(op):
    """tiled(base, 3 copies + 7001 rows): the output assembled from oracle(base) per copy and
    oracle(base[:7001]) equals the oracle run on the whole, every column."""
    oracle = getattr(co, op)
    base = cc.tile_base()
    L = len(base['type_id'])
    assert np.gcd(L, B) == 1  # the copies meet the blocks of SA_ATOMIC_BLOCK_ROWS rows at every phase
    t = cc.tiled(base, 3 * L + 7001, oracle)
    assert (t.copies, t.rest) == (3, 7001) and _strictly_increasing_keys(t.cols)
    assert len(t.cols['type_id']) == 3 * L + 7001
    for c in cc.ID_COLS:  # the copies share no game, team or player
        ids = [set(t.cols[c][k * L:(k + 1) * L]) for k in range(4)]
        assert not any(ids[a] & ids[b] for a in range(4) for b in range(a))
    exp = t.expected()
    whole = oracle(t.cols)
    assert set(exp) == set(whole)
    assert len(exp['type_id']) > len(t.cols['type_id'])
    for c in whole:
        w = cc.event_index(whole[c]) if c == 'original_event_id' else np.asarray(whole[c])
        assert w.dtype == exp[c].dtype or c == 'original_event_id', c
        np.testing.assert_array_equal(w, exp[c], err_msg=c)
