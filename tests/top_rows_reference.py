"""The contract of the filtered top-k (ops.top_rows, include/socceraction_amd.h "filtered top-k of
a column") restated in numpy -- the order key and one lexsort over the eligible rows -- and the
case builders its host and device tests share."""
import numpy as np
import pandas as pd

CHUNK = 4096     # SA_TOP_CHUNK_ROWS
MAX_K = 65536    # SA_TOP_MAX_K
POOL = 17        # distinct values of the tie-heavy columns


def order_key(v: np.ndarray) -> np.ndarray:
    """The unsigned key of the values' width whose order is the numeric order: the bit pattern with
    -0.0 folded onto +0.0, complemented when negative, else with the sign bit set."""
    v = np.ascontiguousarray(v)
    ut = np.uint32 if v.dtype == np.float32 else np.uint64
    assert v.dtype in (np.float32, np.float64)
    sign = ut(1) << ut(v.dtype.itemsize * 8 - 1)
    b = v.view(ut).copy()
    b[b == sign] = 0
    return np.where(b & sign != 0, ~b, b | sign).astype(ut)


def top_rows(v: np.ndarray, k: int, keep=None, largest: bool = True):
    """(rows int64, vals): the eligible rows (kept, not NaN) by key -- descending for largest --
    then by row number, cut at k."""
    v = np.ascontiguousarray(v)
    ok = ~np.isnan(v)
    if keep is not None:
        ok &= np.asarray(keep).astype(bool)
    rows = np.flatnonzero(ok).astype(np.int64)
    key = order_key(v[rows])
    order = np.lexsort((rows, ~key if largest else key))
    rows = rows[order[:k]]
    return rows, v[rows]


def pandas_top_rows(v: np.ndarray, k: int, keep=None, largest: bool = True):
    """The issue's expression, verbatim."""
    s = pd.Series(v)
    if keep is not None:
        s = s[np.asarray(keep).astype(bool)]
    s = s.dropna()
    expected = s.sort_values(ascending=not largest, kind='stable').head(k)
    return expected.index.to_numpy().astype(np.int64), expected.to_numpy()


def bits(v: np.ndarray) -> np.ndarray:
    v = np.ascontiguousarray(v)
    return v.view(np.int32 if v.dtype == np.float32 else np.int64)


def dtype_of(f32: bool):
    return np.float32 if f32 else np.float64


# ----------------------------------------------------------------------------- case builders
SHAPE_NS = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


def shape_ks(n: int):
    return sorted({k for k in (1, 2, n - 1, n, n + 5) if 1 <= k <= MAX_K})


def pool_column(n: int, f32: bool, seed: int = 0):
    """n values drawn from POOL distinct numbers (both signs, both zeros), and a random keep."""
    rng = np.random.default_rng([41, n, int(f32), seed])
    pool = np.concatenate([rng.normal(0, 0.05, POOL - 2), [0.0, -0.0]]).astype(dtype_of(f32))
    assert len(np.unique(bits(pool))) == POOL
    v = pool[rng.integers(0, POOL, n)]
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    return v, keep


def special_column(f32: bool):
    """+-0.0 interleaved, +- the smallest subnormal, +-inf, NaN of both signs and two payloads,
    +- the largest finite value and three nextafter neighbours."""
    dt = dtype_of(f32)
    fi = np.finfo(dt)
    tiny = fi.smallest_subnormal
    one = dt(1)
    up = np.nextafter(one, dt(2))
    down = np.nextafter(one, dt(0))
    it, ut = (np.int32, np.uint32) if f32 else (np.int64, np.uint64)
    nan_bits = np.array([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFA00123] if f32 else
                        [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFF4000000000123], ut)
    nans = nan_bits.view(dt)
    assert np.isnan(nans).all()
    v = np.array([0.0, -0.0, tiny, -0.0, 0.0, -tiny, np.inf, 0.0, -np.inf, -0.0, fi.max, -fi.max,
                  one, up, down, -0.0, 0.0, up, one], dt)
    v = np.concatenate([v[:5], nans[:2], v[5:12], nans[2:], v[12:]])
    assert np.signbit(v[v == 0]).any() and (~np.signbit(v[v == 0])).any()
    return v


def all_equal_column(f32: bool):
    return np.full(3 * CHUNK + 1, 0.125, dtype_of(f32))


def last_digit_column(f32: bool, count: int = 300):
    """Keys that differ only in the last digit: base + i ulps, shuffled."""
    dt = dtype_of(f32)
    it = np.int32 if f32 else np.int64
    base = np.array([0.0371], dt).view(it)[0] & ~it(0x1FF)  # the low 9 bits clear: count <= 512 stays inside them
    assert count <= 512
    v = (base + np.arange(count, dtype=it)).view(dt)
    return v[np.random.default_rng(5).permutation(count)]


def first_digit_column(f32: bool):
    """Keys that differ only in the first digit: powers of two of both signs, shuffled.  The
    first 11 bits of a float64 hold the sign and the exponent's upper 10 bits: its exponents go
    in steps of 2."""
    dt = dtype_of(f32)
    e = np.arange(-100, 101, 4 if f32 else 2)
    v = np.concatenate([np.ldexp(1.0, e), -np.ldexp(1.0, e)]).astype(dt)
    assert np.isfinite(v).all() and (v != 0).all()
    return v[np.random.default_rng(6).permutation(len(v))]


def host_cases(f32: bool):
    """(name, values, keep or None, ks) of every builder, at sizes a host test sorts quickly."""
    out = []
    for n in SHAPE_NS:
        v, keep = pool_column(n, f32)
        out.append((f'pool{n}', v, None, shape_ks(n)))
        out.append((f'pool{n}_keep', v, keep, shape_ks(n)))
    s = special_column(f32)
    out.append(('special', s, None, list(range(1, len(s) + 2))))
    out.append(('all_equal', all_equal_column(f32), None, [5, CHUNK + 3]))
    ld = last_digit_column(f32)
    out.append(('last_digit', ld, None, [len(ld) // 2]))
    fd = first_digit_column(f32)
    out.append(('first_digit', fd, None, [len(fd) // 2]))
    return out
