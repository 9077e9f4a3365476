"""The grouped sums' fixed-point format and host layers, without a GPU: csrc/sa_fixed.h (through
scripts/fixed_sum_host.cc, plain g++) against a Python-integer restatement, the C ABI's argument
checks, the table's all-reduce over gloo and the host-side key factorisation."""
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAC = 95


# ----------------------------------------------------------------------------- restatement
def py_quantize(v: float, E: int):
    """Signed limbs of trunc(v * 2^(95 - E)) in Python integers (NaN: nothing)."""
    if math.isnan(v):
        return (0, 0, 0)
    q = int(abs(Fraction(v)) * Fraction(2) ** (FRAC - E))  # int() truncates
    s = -1 if math.copysign(1.0, v) < 0 else 1
    return tuple(s * ((q >> (32 * i)) & 0xFFFFFFFF) for i in range(3))


def py_finalize(l0: int, l1: int, l2: int, E: int) -> float:
    """(l2 * 2^64 + l1 * 2^32 + l0) * 2^(E - 95): int / int division rounds once, half to even."""
    return float(Fraction(l0 + (l1 << 32) + (l2 << 64)) * Fraction(2) ** (E - FRAC))


def py_group_sums(keys, vals, G: int, E: int):
    """(limbs [G][3], count [G], err) by sa_group_sums' rules for one column."""
    limbs = [[0, 0, 0] for _ in range(G)]
    count = [0] * G
    err = 0
    for k, v in zip(keys.tolist(), vals.tolist()):
        if k == -1:
            continue
        if not 0 <= k < G:
            err |= 1
        elif math.isinf(v):
            err |= 2
        elif abs(v) >= 2.0 ** E:
            err |= 4
        else:
            for i, m in enumerate(py_quantize(v, E)):
                limbs[k][i] += m
            count[k] += 1
    return limbs, count, err


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('fixed_sum') / 'fixed_sum_host')
    subprocess.run(['g++', '-O1', '-std=c++17', '-Wall', '-Werror',
                    os.path.join(ROOT, 'scripts', 'fixed_sum_host.cc'), '-o', exe], check=True)
    return exe


def run_sum(exe, tmp_path, keys, vals, G, E):
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        f.write(struct.pack('<iiqq', 0, E, len(vals), G))
        f.write(np.ascontiguousarray(vals, '<f8').tobytes())
        f.write(np.ascontiguousarray(keys, '<i4').tobytes())
    subprocess.run([exe, src, dst], check=True)
    raw = open(dst, 'rb').read()
    assert len(raw) == 8 * (3 * G + G + 1 + G)
    a = np.frombuffer(raw, '<i8')
    return (a[:3 * G].reshape(G, 3), a[3 * G:4 * G], int(a[4 * G]),
            np.frombuffer(raw, '<f8')[4 * G + 1:])


def run_finalize(exe, tmp_path, limbs, E):
    src, dst = str(tmp_path / 'fin.bin'), str(tmp_path / 'fout.bin')
    with open(src, 'wb') as f:
        f.write(struct.pack('<iiqq', 1, E, len(limbs), 0))
        f.write(np.ascontiguousarray(limbs, '<i8').tobytes())
    subprocess.run([exe, src, dst], check=True)
    return np.fromfile(dst, '<f8')


def format_inputs(E: int, big_group: bool):
    """keys, values: group 0 has one row, the last group 1e5 rows (``big_group``), the rest are
    the special values, spread over a few groups."""
    rng = np.random.default_rng([E + 1000, 3])
    top = 2.0 ** E
    res = 2.0 ** (E - FRAC)
    n = 4000
    # random doubles across exponents: from far below the resolution up to just below 2^E
    v = rng.uniform(0.5, 1.0, n) * 2.0 ** rng.integers(E - 130, E + 1, n) * rng.choice([-1.0, 1.0], n)
    special = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308 / 3, np.nextafter(top, 0.0),
               -np.nextafter(top, 0.0), np.nextafter(res, 0.0), -np.nextafter(res, 0.0), res, -res,
               np.nextafter(res, np.inf), res * 1.5, top / 2, -top / 2, float('nan')]
    pairs = rng.uniform(-1, 1, 300) * top / 4
    cancel = np.stack([pairs, -pairs], axis=1).reshape(-1)  # every group's pair cancels exactly
    with np.errstate(over='ignore'):  # E = 900: beyond float32, dropped on the next line
        f32 = (rng.standard_normal(500) * top / 8).astype(np.float32).astype(np.float64)
    f32 = f32[np.abs(f32) < top]
    vals = np.concatenate([[top / 3], v, special, cancel, f32])
    keys = np.concatenate([[0], rng.integers(1, 6, n), rng.integers(1, 6, len(special)),
                           np.full(len(cancel), 6), rng.integers(1, 6, len(f32))])
    G = 7
    if big_group:
        bv = rng.beta(0.5, 30, 100000) - rng.beta(0.5, 60, 100000)  # VAEP-like
        vals = np.concatenate([vals, bv * top / 4])
        keys = np.concatenate([keys, np.full(100000, 7)])
        G = 8
    p = rng.permutation(len(vals))
    return keys[p].astype(np.int32), vals[p], G


@pytest.mark.parametrize('E', [2, 1, 0, 37, -900, 900])
def test_fixed_point_format_matches_python_integers(host_program, tmp_path, E):
    """sa_fixed.h's quantise + finalise == the Python-integer restatement, bit for bit."""
    keys, vals, G = format_inputs(E, big_group=(E == 2))
    limbs, count, err, sums = run_sum(host_program, tmp_path, keys, vals, G, E)
    rl, rc, re_ = py_group_sums(keys, vals, G, E)
    assert err == re_ == 0
    assert limbs.tolist() == rl
    assert count.tolist() == rc and rc[0] == 1 and (E != 2 or rc[7] == 100000)
    want = np.array([py_finalize(*l, E) for l in rl])
    assert sums.view(np.int64).tolist() == want.view(np.int64).tolist()
    assert limbs[6].tolist() == [0, 0, 0] and sums[6] == 0.0 and not np.signbit(sums[6])


def test_fixed_point_special_rows(host_program, tmp_path):
    """inf, |v| >= 2^E and bad keys flag their bit and add nothing; NaN and key -1 as pandas."""
    E = 1
    vals = np.array([0.5, np.inf, 0.25, 2.0, -np.inf, np.nan, 0.125, 1.0, -2.0, 0.0625, 1.75])
    keys = np.array([0, 0, 1, 1, 2, 2, -1, 3, 0, -2, 2], np.int32)
    limbs, count, err, sums = run_sum(host_program, tmp_path, keys, vals, 3, E)
    rl, rc, re_ = py_group_sums(keys, vals, 3, E)
    assert err == re_ == 7
    assert limbs.tolist() == rl and count.tolist() == rc == [1, 1, 2]
    assert sums.tolist() == [0.5, 0.25, 1.75]


def test_finalize_rounds_ties_to_even(host_program, tmp_path):
    """Totals exactly on a rounding tie and one unit either side, built directly from limbs;
    random (also non-canonical) limb triples."""
    rng = np.random.default_rng(12)
    totals = []
    for M in (1 << 52, (1 << 52) + 1, (1 << 53) - 1, (1 << 53) - 2, 0x12345678ABCDEF | (1 << 52)):
        for s in (1, 2, 10, 11, 12, 31, 32, 33, 43, 44, 63, 64, 65, 66, 72):
            tie = (M << s) + (1 << (s - 1))
            totals += [tie - 1, tie, tie + 1, -(tie - 1), -tie, -(tie + 1)]
    totals += [0, 1, -1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 125) + (1 << 72), -(1 << 125)]
    limbs = []
    for S in totals:
        a = abs(S)
        sg = -1 if S < 0 else 1
        limbs.append([sg * (a & 0xFFFFFFFF), sg * ((a >> 32) & 0xFFFFFFFF), sg * (a >> 64)])
    limbs += rng.integers(-(1 << 61), 1 << 61, (500, 3)).tolist()
    limbs += [[-5, 1, 0], [(1 << 61), -(1 << 29), 0], [-(1 << 32), 1, 0], [3, -(1 << 32), 1]]
    for E in (1, 2, -900, 900):
        got = run_finalize(host_program, tmp_path, np.array(limbs, np.int64), E)
        want = np.array([py_finalize(*l, E) for l in limbs])
        assert got.view(np.int64).tolist() == want.view(np.int64).tolist(), E
    # the tie itself goes to the even mantissa: a tie above an odd 53-bit integer rounds up
    M, s = (1 << 52) + 1, 12
    assert py_finalize(((M << s) + (1 << (s - 1))) & 0xFFFFFFFF, ((M << s) + (1 << (s - 1))) >> 32, 0,
                       FRAC) == float((M + 1) << s)


def test_header_sums_vaep_like_values_to_fsum(host_program, tmp_path):
    """The format is wide enough that VAEP-like values (E = 1) lose nothing: the header's sum of
    3000 of them, through the host program, is math.fsum exactly."""
    rng = np.random.default_rng(5)
    v = rng.beta(0.5, 30, 3000) - rng.beta(0.5, 60, 3000)
    limbs, count, err, sums = run_sum(host_program, tmp_path, np.zeros(3000, np.int32), v, 1, 1)
    assert err == 0 and count.tolist() == [3000]
    assert sums.tolist() == [math.fsum(v.tolist())]


# ----------------------------------------------------------------------------- C ABI
def test_group_entry_points_validate_without_a_gpu():
    """sa_group_sums / sa_group_finalize return SA_EINVAL for every invalid argument before any
    HIP call; n == 0 is a successful no-op."""
    import ctypes

    from socceraction_amd import _native
    lib = _native.load_library()
    fake = ctypes.c_void_p(256)  # never dereferenced on the host
    cols = (ctypes.c_void_p * 8)(*[256] * 8)
    exps = (ctypes.c_int32 * 8)(*[2] * 8)
    good = dict(key=fake, cols=cols, n_cols=3, f32=0, n=10, n_groups=5, scale_exp=exps, limbs=fake,
                count=fake, err=fake, stream=None)
    order = list(good)

    def sums(**kw):
        a = dict(good, **kw)
        return lib.sa_group_sums(*[a[k] for k in order])

    none_cols = ctypes.POINTER(ctypes.c_void_p)()
    none_exps = ctypes.POINTER(ctypes.c_int32)()
    hole = (ctypes.c_void_p * 8)(*[256, None, 256, 256, 256, 256, 256, 256])
    bad = [dict(key=None), dict(cols=none_cols), dict(cols=hole), dict(scale_exp=none_exps),
           dict(limbs=None), dict(count=None), dict(err=None), dict(n_cols=0), dict(n_cols=9),
           dict(n=-1), dict(n_groups=0), dict(n_groups=-3),
           dict(scale_exp=(ctypes.c_int32 * 8)(2, -901, 2)), dict(scale_exp=(ctypes.c_int32 * 8)(901, 2, 2))]
    for kw in bad:
        assert sums(**kw) == _native.SA_EINVAL, kw
        assert b'sa_group_sums' in lib.sa_last_error(), kw
        with pytest.raises(ValueError):
            _native.check(_native.SA_EINVAL)
    assert sums(n=0) == _native.SA_OK
    assert sums(n=0, scale_exp=(ctypes.c_int32 * 8)(-900, 900, 0)) == _native.SA_OK
    assert sums(n=0, n_cols=9) == _native.SA_EINVAL  # checked before the no-op

    fgood = dict(limbs=fake, n_groups=5, n_cols=3, scale_exp=exps, out=fake, stream=None)
    forder = list(fgood)
    for kw in [dict(limbs=None), dict(out=None), dict(scale_exp=none_exps), dict(n_cols=0), dict(n_cols=9),
               dict(n_groups=0), dict(scale_exp=(ctypes.c_int32 * 8)(2, 2, 901)),
               dict(scale_exp=(ctypes.c_int32 * 8)(-901, 2, 2))]:
        a = dict(fgood, **kw)
        assert lib.sa_group_finalize(*[a[k] for k in forder]) == _native.SA_EINVAL, kw
        assert b'sa_group_finalize' in lib.sa_last_error(), kw
    assert _native.SA_GROUP_LDS_SLOTS == 256 and _native.SA_GROUP_MAX_COLS == 8


def test_native_constants_match_the_header():
    from socceraction_amd import _native
    with open(os.path.join(ROOT, 'include', 'socceraction_amd.h')) as f:
        src = f.read()
    for name in ('SA_GROUP_MAX_COLS', 'SA_GROUP_LDS_SLOTS', 'SA_GROUP_CHUNK_ROWS', 'SA_GROUP_HASH_MUL',
                 'SA_GROUP_ERR_KEY', 'SA_GROUP_ERR_NONFINITE', 'SA_GROUP_ERR_RANGE', 'SA_GROUP_WG_PER_CU'):
        line = [ln for ln in src.splitlines() if ln.startswith(f'#define {name} ')]
        assert len(line) == 1, name
        assert int(line[0].split()[2].rstrip('u')) == getattr(_native, name), name


def test_python_layer_argument_checks():
    import torch

    from socceraction_amd import ops
    k = torch.zeros(4, dtype=torch.int32)
    c = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.group_sums(k, [c] * 9, 3, scale_exp=[1] * 9)
    with pytest.raises(TypeError):
        ops.group_sums(k.long(), [c], 3, scale_exp=[1])
    with pytest.raises(TypeError):
        ops.group_sums(k, [c, c.float()], 3, scale_exp=[1, 1])
    with pytest.raises(ValueError):
        ops.group_sums(k, [c[:3]], 3, scale_exp=[1])
    with pytest.raises(ValueError):
        ops.group_sums(k, [c], 3, scale_exp=[901])
    acc = ops.group_sums_zero(3, 1, [1], 'cpu')
    assert acc.limbs.shape == (3, 1, 3) and acc.count.shape == (3,) and acc.err.shape == (1,)
    assert acc.buf.dtype == torch.int64 and acc.buf.is_contiguous()
    with pytest.raises(ValueError):  # another shape than the table was started with
        ops.group_sums(k, [c], 4, scale_exp=[1], acc=acc)
    with pytest.raises(ValueError, match='scale_exp'):  # this call's values overflow acc's scale
        ops.group_sums(k, [c + 3.0], 3, acc=acc)
    acc.rows = ops.GROUP_MAX_ROWS - 3
    with pytest.raises(ValueError, match='2\\*\\*30'):  # the capacity bound counts rows
        ops.group_sums(k, [c], 3, scale_exp=[1], acc=acc)
    acc.buf[-2] = 4
    with pytest.raises(ValueError, match='scale_exp'):
        acc.check_errors()
    acc.zero_()
    acc.check_errors()
    assert acc.rows == 0


# ----------------------------------------------------------------------------- all-reduce
def _gloo_group_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist

    from socceraction_amd import ops, shard
    dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world)
    acc = ops.group_sums_zero(11, 3, [2, 2, 1], 'cpu')  # the device layout, on the host for gloo
    g = torch.Generator().manual_seed(100 + rank)
    acc.limbs.copy_(torch.randint(-(1 << 61), 1 << 61, acc.limbs.shape, generator=g))
    acc.count.copy_(torch.randint(0, 1 << 29, acc.count.shape, generator=g))
    acc.err.fill_(1 if rank == 0 else 5)
    acc.rows = 1000 + rank
    mine = acc.buf.clone()
    shard.allreduce_group_sums(acc)  # ONE all-reduce
    q.put((rank, mine.numpy(), acc.buf.numpy().copy(), int(acc.err.item()), acc.rows))
    dist.destroy_process_group()


def test_group_sums_allreduce_gloo_world2():
    """shard.allreduce_group_sums over gloo, world 2: every rank ends with the integer sum of the
    two buffers, the OR of the error bits and the total row count."""
    import multiprocessing as mp
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_group_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = res[0][1][:-2] + res[1][1][:-2]  # limbs and counts
    for _, _, after, err, rows in res:
        assert (after[:-2] == want).all()
        assert err == 5 and rows == 2001
        assert after[-2] == 5 and after[-1] == 0


# ----------------------------------------------------------------------------- host layers
def test_factorize_matches_groupby_order():
    from socceraction_amd import ratings
    rng = np.random.default_rng(3)
    df = pd.DataFrame({'game_id': rng.integers(0, 5, 400), 'player_id': rng.integers(0, 30, 400).astype(float),
                       'x': rng.random(400)})
    df.loc[rng.random(400) < 0.1, 'player_id'] = np.nan
    for by in ('player_id', ['game_id', 'player_id'], ['player_id', 'game_id']):
        codes, keys = ratings.factorize(df, by)
        ref = df.assign(count=1).groupby(by).sum().reset_index()
        names = [by] if isinstance(by, str) else by
        pd.testing.assert_frame_equal(keys, ref[names])
        assert codes.dtype == np.int32 and ((codes == -1) == df.player_id.isna().to_numpy()).all()
        got = np.bincount(codes[codes >= 0], minlength=len(keys))
        assert (got == ref['count'].to_numpy()).all()
    # an explicit vocabulary: sorted, a superset of the observed keys; unknown keys raise
    codes, keys = ratings.factorize(df, 'game_id', groups=[7, 4, 3, 2, 1, 0])
    assert keys.game_id.tolist() == [0, 1, 2, 3, 4, 7] and (codes == df.game_id.to_numpy()).all()
    with pytest.raises(ValueError):
        ratings.factorize(df, 'game_id', groups=[0, 1])


def test_per_90_is_the_notebook_normalisation():
    from socceraction_amd import ratings
    table = pd.DataFrame({'player_id': [1, 2, 3], 'vaep_value': [1.0, 2.0, 3.0],
                          'offensive_value': [0.5, 1.0, 1.5], 'defensive_value': [0.5, 1.0, 1.5],
                          'count': [10, 20, 30]})
    pg = pd.DataFrame({'player_id': [1, 1, 2, 3, 3], 'minutes_played': [90, 90, 200, 90, 100]})
    out = ratings.per_90(table, pg)
    assert out.player_id.tolist() == [2, 3]  # player 1 has exactly 180 minutes: not more than
    assert out.vaep_rating.tolist() == [2.0 * 90 / 200, 3.0 * 90 / 190]
    assert out.offensive_rating.tolist() == [1.0 * 90 / 200, 1.5 * 90 / 190]
    assert list(out.columns) == ['player_id', 'vaep_value', 'offensive_value', 'defensive_value', 'count',
                                 'minutes_played', 'vaep_rating', 'offensive_rating', 'defensive_rating']
