"""``sa_pack_bits`` (csrc/sa_store.hip) against ``np.packbits(..., bitorder='little')`` on the
sources of tests/boundary_cases.py: true values are any non-zero byte, every source row at or
beyond ``n`` is 0xFF, ``n`` lies on both sides of a bitmap byte, of a 16-row group and of one
workgroup, and the tiles are one, one per group, 48 rows, and 1024 rows with a spare.

Through ``store.pack_bits`` all ``2 * ceil(n / 16)`` bytes of every column are compared (the
second byte of the last pair is the one the tail mask clears).  Through the C entry point the
output is a buffer the test owns, prefilled with 0xA5, with a column stride that is even but no
multiple of 64: the bytes between the columns and after the last one must keep the prefill.
tests/test_boundary_host.py asserts the conditions on the sources and the refused calls."""
import ctypes

import numpy as np
import pytest

import boundary_cases as bc
from oracle import vaep_oracle as vo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, catalog, store
    _native.load_library()
    return dict(native=_native, catalog=catalog, store=store)


def _through_wrapper(sa, blk, R, n, ref, tag):
    bits = sa['store'].pack_bits(torch.from_numpy(blk).cuda(), R, n)
    assert bits.shape[0] == blk.shape[1] and bits.shape[1] >= ref.shape[1], tag
    np.testing.assert_array_equal(bits.cpu().numpy()[:, :ref.shape[1]], ref, err_msg=tag)


def _through_entry_point(sa, blk, R, n, ref, tag, shift=0):
    """sa_pack_bits into a guarded buffer at ``shift`` bytes past a 16-byte boundary."""
    native = sa['native']
    C, need = blk.shape[1], ref.shape[1]
    stride = need + 6
    assert stride % 2 == 0 and stride % 64 and shift % 2 == 0
    src = torch.from_numpy(blk).cuda()
    buf = torch.full((shift + C * stride + bc.GUARD_BYTES,), bc.GUARD, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    b = native.SaBlock()
    b.data, b.n_cols, b.tile_rows = src.data_ptr(), C, R
    native.check(native.lib().sa_pack_bits(ctypes.byref(b), n, buf.data_ptr() + shift, stride,
                                           torch.cuda.current_stream().cuda_stream))
    out = buf.cpu().numpy()
    assert (out[:shift] == bc.GUARD).all(), tag
    cols = out[shift:shift + C * stride].reshape(C, stride)
    np.testing.assert_array_equal(cols[:, :need], ref, err_msg=tag)
    assert (cols[:, need:] == bc.GUARD).all(), f'{tag}: bytes between the columns'
    assert (out[shift + C * stride:] == bc.GUARD).all(), f'{tag}: bytes after the last column'


@pytest.mark.parametrize('n', bc.PACK_NS)
def test_pack_bits_vs_numpy(sa, n):
    for C in bc.PACK_CS:
        for layout, R, tiles in bc.pack_layouts(n):
            blk, ref = bc.pack_source(n, C, R, tiles)
            tag = f'n={n} C={C} {layout}'
            _through_wrapper(sa, blk, R, n, ref, tag)
            _through_entry_point(sa, blk, R, n, ref, tag + ' (entry point)')


def test_pack_bits_at_an_address_2_mod_16(sa):
    """The 2-byte stores of a column need an even address, nothing more."""
    for n in (17, 4097):
        layout, R, tiles = bc.pack_layouts(n)[2]
        blk, ref = bc.pack_source(n, 7, R, tiles)
        _through_entry_point(sa, blk, R, n, ref, f'n={n} {layout} bits at 2 mod 16', shift=2)


def test_pack_bits_as_wide_as_the_default_plan(sa):
    """One grid row per bool column of the default SPADL plan at k = 3."""
    C = sa['catalog'].build_plan(vo.SPADL_DEFAULT, 3, False).n_bool
    assert C > 100
    n = bc.PLAN_WIDTH_N
    for layout, R, tiles in bc.pack_layouts(n):
        blk, ref = bc.pack_source(n, C, R, tiles)
        _through_wrapper(sa, blk, R, n, ref, f'C={C} {layout}')
        _through_entry_point(sa, blk, R, n, ref, f'C={C} {layout} (entry point)')
