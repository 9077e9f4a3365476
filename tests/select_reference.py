"""Numpy restatement of the row-selection contract (``sa_select_rows``, include/socceraction_amd.h);
TEST INFRASTRUCTURE ONLY.  Written from the contract, not from the kernels: fancy indexing on
unpacked bits and untiled blocks, repacked with ``bitorder='little'``.
"""
from __future__ import annotations

import numpy as np


def ld(m: int) -> int:
    """Rows of the one output tile: m rounded up to 16, at least 16."""
    return max(16, (m + 15) // 16 * 16)


def select_bits(bits, n: int, rows) -> np.ndarray:
    """Bitmaps ``[C, words_in]`` int64 (bit i of word w = row 64w + i) of n rows -> the bitmaps
    ``[max(C, 1), max(1, ceil(m / 64))]`` of the listed rows: bit i of word j = the source bit of
    row ``rows[64j + i]``, every bit at or beyond m zero."""
    bits = np.ascontiguousarray(bits, np.int64)
    rows = np.asarray(rows, np.int64).ravel()
    m = len(rows)
    assert bits.shape[1] * 64 >= n and (m == 0 or (rows.min() >= 0 and rows.max() < n))
    un = np.unpackbits(bits.view(np.uint8), axis=1, bitorder='little')  # [C, words_in * 64]
    words = max(1, (m + 63) // 64)
    picked = np.zeros((max(bits.shape[0], 1), words * 64), np.uint8)
    picked[:bits.shape[0], :m] = un[:, rows]
    return np.packbits(picked, axis=1, bitorder='little').view(np.int64)


def untile(block, n: int) -> np.ndarray:
    """A tiled block ``[tiles, C, R]`` as ``[C, n]``."""
    block = np.asarray(block)
    return block.transpose(1, 0, 2).reshape(block.shape[1], -1)[:, :n]


def select_block(block, n: int, rows) -> np.ndarray:
    """A tiled numeric block ``[tiles, C, R]`` of n rows -> the one-tile block ``[1, C, ld(m)]`` of
    the listed rows: element bits unchanged, elements ``m .. ld(m) - 1`` zero.  Works on the
    integer view of the elements, so NaN payloads and -0.0 are carried as they are."""
    block = np.asarray(block)
    iview = block.view({4: np.uint32, 8: np.uint64}[block.dtype.itemsize])
    rows = np.asarray(rows, np.int64).ravel()
    m = len(rows)
    out = np.zeros((1, block.shape[1], ld(m)), iview.dtype)
    out[0, :, :m] = untile(iview, n)[:, rows]
    return out.view(block.dtype)
