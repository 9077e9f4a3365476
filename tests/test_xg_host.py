"""CPU-only tests of the expected-goals path: the model's feature names and shot types, the numpy
restatement of the row-selection contract on hand-made inputs, and ``sa_select_rows``' argument
checks, which come before any HIP call.  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest

import select_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_feature_names_are_the_notebooks_46():
    from socceraction_amd import xg
    with open(os.path.join(ROOT, 'tests', 'golden', 'xg_feature_names.json')) as f:
        want = json.load(f)
    assert len(want) == 46
    assert xg.feature_names() == want
    assert xg.feature_names(xg.XFNS, xg.NB_PREV_ACTIONS) == want
    assert xg.NB_PREV_ACTIONS == 2 and [f.__name__ for f in xg.XFNS] == [
        'actiontype_onehot', 'bodypart_onehot', 'startlocation', 'movement', 'space_delta', 'startpolar', 'team']
    assert xg.ExpectedGoals()._columns() == want
    assert xg.TREE_PARAMS == dict(n_estimators=100, max_depth=6, learning_rate=0.3)


def test_shot_types_are_the_three_shot_actions():
    from socceraction_amd import xg
    from socceraction_amd.spadl import config
    assert sorted(xg.SHOT_TYPES) == sorted(config.actiontypes.index(t) for t in ('shot', 'shot_penalty', 'shot_freekick'))
    assert config.results[xg.SUCCESS] == 'success'


def test_unfitted_and_unsupported_models_raise():
    from sklearn.exceptions import NotFittedError

    from socceraction_amd import xg
    model = xg.ExpectedGoals()
    for call in (lambda: model.rate_batch(None, None), lambda: model.rate(None, None),
                 lambda: model.score_batch(None, None), model.to_xgboost_json):
        with pytest.raises(NotFittedError):
            call()
    with pytest.raises(ValueError, match='learner'):
        model.fit_batch(None, None, learner='xgboost')
    with pytest.raises(ValueError, match='built-in'):
        xg.ExpectedGoals(xfns=[lambda gs: None]).fit_batch(None, [])


# ----------------------------------------------------------------------------- the restatement
def _bitmaps(values):
    """[C, n] bools -> [C, words] int64 bitmaps."""
    values = np.asarray(values, bool)
    words = max(1, (values.shape[1] + 63) // 64)
    padded = np.zeros((values.shape[0], words * 64), np.uint8)
    padded[:, :values.shape[1]] = values
    return np.packbits(padded, axis=1, bitorder='little').view(np.int64)


def _bit(bits, c, q):
    return (int(bits[c, q // 64]) >> (q % 64)) & 1


def test_restated_bitmaps_on_hand_made_rows():
    n = 130  # three source words, the last one partly used
    vals = np.zeros((2, n), bool)
    vals[0, [0, 63, 64, 127, 129]] = True   # bits 0 and 63 of words 0 and 1, the last row
    vals[1] = np.arange(n) % 3 == 0
    bits = _bitmaps(vals)
    assert bits.shape == (2, 3)
    assert bits[0, 0] == np.int64(1) | np.int64(-2 ** 63) and bits[0, 2] == 2
    # descending, with repeats, across word edges
    rows = [129, 129, 128, 127, 64, 63, 0, 0, 1]
    out = sr.select_bits(bits, n, rows)
    assert out.shape == (2, 1) and out.dtype == np.int64
    for c in range(2):
        assert [_bit(out, c, q) for q in range(len(rows))] == [int(vals[c, r]) for r in rows]
        assert int(out[c, 0]) >> len(rows) == 0  # every tail bit is zero
    # 65 rows: a second word with one live bit
    rows = np.arange(n - 1, n - 66, -1)
    out = sr.select_bits(bits, n, rows)
    assert out.shape == (2, 2)
    assert [_bit(out, 1, q) for q in range(65)] == [int(vals[1, r]) for r in rows]
    assert int(out[1, 1]) in (0, 1) and int(out[0, 1]) in (0, 1)
    # all rows ascending is the identity; none gives one zero word per column
    np.testing.assert_array_equal(sr.select_bits(bits, n, np.arange(n)), bits)
    np.testing.assert_array_equal(sr.select_bits(bits, n, []), np.zeros((2, 1), np.int64))
    # no bool column: the one placeholder row, zero
    np.testing.assert_array_equal(sr.select_bits(np.zeros((0, 3), np.int64), n, [5, 4]), np.zeros((1, 1), np.int64))


@pytest.mark.parametrize('dtype', [np.float64, np.int64, np.float32])
def test_restated_blocks_on_hand_made_rows(dtype):
    n, R, C = 40, 16, 3
    flat = (np.arange(C * n).reshape(C, n) * 3 - 7).astype(dtype)
    if dtype != np.int64:
        u = {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]
        flat.view(u)[1, 17] = {4: 0x7FC12345, 8: 0x7FF8000000ABCDEF}[np.dtype(dtype).itemsize]  # a NaN with a payload
        flat[2, 16] = -0.0
    tiled = np.zeros((3, C, R), dtype)
    for t in range(3):
        w = min(R, n - t * R)
        tiled[t, :, :w] = flat[:, t * R:t * R + w]
    np.testing.assert_array_equal(sr.untile(tiled, n).view(np.uint8), flat.view(np.uint8))
    rows = [39, 17, 16, 15, 0, 17, 17]
    out = sr.select_block(tiled, n, rows)
    assert out.shape == (1, C, 16) and out.dtype == np.dtype(dtype)
    assert out[0, :, :len(rows)].tobytes() == np.ascontiguousarray(flat[:, rows]).tobytes()
    assert not out.view(np.uint8)[0, :, len(rows) * out.itemsize:].any()  # the padding is zero bytes
    assert sr.select_block(tiled, n, np.arange(17)).shape == (1, C, 32)
    assert sr.ld(0) == 16 and sr.ld(16) == 16 and sr.ld(129) == 144


# ----------------------------------------------------------------------------- the C entry point
def test_select_rows_rejects_bad_arguments_without_a_gpu():
    """Every argument check of sa_select_rows comes before any HIP call (SA_EINVAL)."""
    from socceraction_amd import _native
    lib = _native.load_library()
    fake = ctypes.c_void_p(256)  # never dereferenced on the host

    def blk(cols, tile=128, data=fake):
        b = _native.SaBlock()
        b.data, b.n_cols, b.tile_rows = data, cols, tile
        return b

    def call(f=None, i=None, f32=0, bits=fake, words_in=16, n_bool=5, n=1000, rows=fake, m=100, f_out=fake,
             i_out=fake, ld=112, bits_out=fake, words_out=2):
        f = blk(3) if f is None else f
        i = blk(2) if i is None else i
        return lib.sa_select_rows(ctypes.byref(f), ctypes.byref(i), f32, bits, words_in, n_bool, n, rows, m, f_out,
                                  i_out, ld, bits_out, words_out, None)

    einval = lambda rc, word: rc == _native.SA_EINVAL and word in lib.sa_last_error()  # noqa: E731
    assert einval(lib.sa_select_rows(None, None, 0, fake, 16, 5, 1000, fake, 100, fake, fake, 112, fake, 2, None),
                  b'null block descriptor')
    # negative sizes
    for kw in (dict(n=-1), dict(m=-1), dict(n_bool=-1), dict(words_in=-1), dict(words_out=-1), dict(ld=-16),
               dict(f=blk(-1)), dict(i=blk(-1))):
        assert einval(call(**kw), b'negative'), kw
    # null pointers with rows to select
    assert einval(call(rows=None), b'null row list')
    assert einval(call(f=blk(3, data=None)), b'null numeric block')
    assert einval(call(i=blk(2, data=None)), b'null numeric block')
    assert einval(call(f_out=None), b'null numeric block')
    assert einval(call(i_out=None), b'null numeric block')
    assert einval(call(bits=None), b'null bitmap')
    assert einval(call(bits_out=None), b'null bitmap')
    # tiles that are not a multiple of 16 rows
    for tile in (0, 8, 24, 130):
        assert einval(call(f=blk(3, tile=tile)), b'multiples of 16'), tile
        assert einval(call(i=blk(2, tile=tile)), b'multiples of 16'), tile
    # source bitmaps shorter than the table, outputs shorter than the selection
    assert einval(call(words_in=15), b'words_in * 64 < n')
    assert einval(call(words_out=1), b'fewer than m rows')
    assert einval(call(ld=96), b'output tile')
    assert einval(call(ld=104), b'output tile')
    assert einval(call(n=0, words_in=0), b'empty table')
    # nothing to do: SA_OK with no launch, whatever the pointers
    assert call(m=0, rows=None, bits=None, f_out=None, i_out=None, bits_out=None) == _native.SA_OK
    assert call(f=blk(0, data=None), i=blk(0, data=None), n_bool=0, rows=None, bits=None) == _native.SA_OK
    with pytest.raises(ValueError):
        _native.check(call(rows=None))
