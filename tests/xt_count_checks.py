"""The oracle's xT counts in sparse form and their comparison with a device count, shared by
tests/test_gpu_thresholds.py and tests/test_gpu_xt_dispatch.py.  The C x C transition table is
compared through its non-zero entries, so grids of thousands of cells need no dense reference;
:func:`same_counts_gathered` does the same for tables too large to search for non-zeros."""
import numpy as np

from oracle import xt_oracle as xo


def sparse_trans(d, l, w):
    """The successful-move transition counts as (sorted flat s * C + e, count), from the
    oracle's binning."""
    t, r = d['type_id'], d['result_id']
    mv = ((t == 0) | (t == 21) | (t == 1)) & (r == 1)
    s = xo.flat_indexes(d['start_x'][mv], d['start_y'][mv], l, w)
    e = xo.flat_indexes(d['end_x'][mv], d['end_y'][mv], l, w)
    return np.unique(s.astype(np.int64) * (l * w) + e, return_counts=True)


def ref_counts(d, l, w):
    """The oracle's counts with the C x C transition counts as their non-zero entries (up to 1024
    cells straight from xt_oracle.counts; above, from its binning without the dense table)."""
    t, r = d['type_id'], d['result_id']
    out = {}
    for name, m in (('shot', t == 11), ('goal', (t == 11) & (r == 1)), ('move', (t == 0) | (t == 21) | (t == 1))):
        out[name] = xo.count(d['start_x'][m], d['start_y'][m], l, w).astype(np.int64).reshape(-1)
    out['trans'] = sparse_trans(d, l, w)
    if l * w <= 1024:
        cnt = xo.counts(d, l, w)
        for name in ('shot', 'goal', 'move'):
            np.testing.assert_array_equal(cnt[name].reshape(-1), out[name])
        nz = np.flatnonzero(cnt['trans'])
        np.testing.assert_array_equal(nz, out['trans'][0])
        np.testing.assert_array_equal(cnt['trans'].reshape(-1)[nz], out['trans'][1])
    return out


def scaled(ref, k):
    """The counts of a batch repeated k times."""
    return dict(shot=ref['shot'] * k, goal=ref['goal'] * k, move=ref['move'] * k,
                trans=(ref['trans'][0], ref['trans'][1] * k))


def same_counts(sa, acc, ref, what):
    torch = sa['torch']
    for name in ('shot', 'goal', 'move'):
        np.testing.assert_array_equal(getattr(acc, name).cpu().numpy(), ref[name], err_msg=f'{what} {name}')
    nz = torch.nonzero(acc.trans).reshape(-1)
    np.testing.assert_array_equal(nz.cpu().numpy(), ref['trans'][0], err_msg=f'{what} transition cells')
    np.testing.assert_array_equal(acc.trans[nz].cpu().numpy(), ref['trans'][1], err_msg=f'{what} transitions')
    assert int(acc.err.item()) == 0, what   # every coordinate is finite: the reference does not raise


def same_counts_gathered(sa, acc, ref, what, row_block=2048):
    """:func:`same_counts` without a search of the table (0.58 GB at 12001 cells, 8.6 GB at
    46340): the expected entries are gathered and compared, and the table's total, summed in
    int64 by row blocks, is the expected total -- so nothing else is non-zero (no count is
    negative: a wrong cell would need a wrong negative one to cancel it)."""
    torch = sa['torch']
    for name in ('shot', 'goal', 'move'):
        np.testing.assert_array_equal(getattr(acc, name).cpu().numpy(), ref[name], err_msg=f'{what} {name}')
    idx, cnt = ref['trans']
    got = acc.trans[torch.from_numpy(idx).to(acc.trans.device)].cpu().numpy()
    np.testing.assert_array_equal(got, cnt, err_msg=f'{what} transitions')
    C = acc.C
    table = acc.trans.view(C, C)
    total, low = 0, 0
    for r0 in range(0, C, row_block):
        blk = table[r0:r0 + row_block]
        total += int(blk.sum(dtype=torch.int64).item())
        low = min(low, int(blk.min().item()))
    assert total == int(cnt.sum()) and low == 0, (what, total, int(cnt.sum()), low)
    assert int(acc.err.item()) == 0, what
