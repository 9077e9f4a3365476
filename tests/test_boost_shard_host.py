"""The host side of the sharded device learner, without a GPU: the
exchange layout as a pure function of the cut counts and feature kinds, the ranks' parts of the
global cut sample, the sharded cuts over gloo on host frames, and the argument checks of the two
exchange entries."""
import ctypes
import datetime

import numpy as np
import pandas as pd
import pytest

import boost_reference as br

from socceraction_amd import boost


# ----------------------------------------------------------------------------- the layout
def _layout_case(counts, kinds):
    cut_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return boost.exchange_layout(cut_start, np.array(kinds, bool)), cut_start


def test_exchange_layout_of_the_edge_features():
    # a 0-cut numeric, a 1-cut bool, a 254-cut numeric (bins 0..254 and 255: all 256), a bool, a 4-cut numeric
    lay, _ = _layout_case([0, 1, 254, 1, 4], [0, 1, 0, 1, 0])
    assert (lay.n_bool, lay.n_num, lay.n_features) == (2, 2 + 256 + 6, 5)
    assert lay.pairs.dtype == np.int32
    want = [1 * 256 + 1, 3 * 256 + 1]                 # the bools' bin 1, model order
    want += [0 * 256 + 0, 0 * 256 + 255]              # no cut: bin 0 and the missing bin
    want += list(range(2 * 256, 2 * 256 + 256))       # 254 cuts: every bin
    want += [4 * 256 + b for b in (0, 1, 2, 3, 4, 255)]
    assert lay.pairs.tolist() == want
    assert [lay.words(k) for k in (1, 2, 4, 32)] == [2 + 2 * 266, 4 * 266, 8 * 266, 64 * 266]


@pytest.mark.parametrize('nodes', [1, 4, 32])
def test_exchange_layout_is_a_bijection_onto_the_used_entries(nodes):
    rng = np.random.default_rng(nodes)
    kinds = rng.random(40) < 0.6
    counts = np.where(kinds, 1, rng.integers(0, 255, 40))
    counts[np.flatnonzero(~kinds)[:2]] = (0, 254)
    lay, cut_start = _layout_case(counts, kinds)
    F = len(kinds)
    used = np.zeros((nodes, F, 256), bool)  # what the histogram kernels and the split search can touch
    for f in range(F):
        if kinds[f]:
            used[:, f, 1] = True  # (bin 0 is derived after the sum)
        else:
            used[:, f, :counts[f] + 1] = True
            used[:, f, 255] = True
    at = lay.dense_pairs(nodes)
    assert len(at) == len(set(at.tolist())) == used.sum() == nodes * (lay.n_bool + lay.n_num)
    assert used.reshape(-1)[at].all()
    assert 2 * len(at) + 2 * (nodes == 1) == lay.words(nodes)
    # payload order: every node's bool pairs, then every node's numeric pairs, model order inside
    node, rest = at // (F * 256), at % (F * 256)
    nb = nodes * lay.n_bool
    assert (node[:nb] == np.repeat(np.arange(nodes), lay.n_bool)).all()
    assert (node[nb:] == np.repeat(np.arange(nodes), lay.n_num)).all()
    assert (rest[:nb].reshape(nodes, -1) == lay.pairs[:lay.n_bool]).all()
    assert (np.diff(rest[nb:].reshape(nodes, -1), axis=1) > 0).all()


def test_exchange_layout_refuses_bad_tables():
    with pytest.raises(ValueError):
        boost.exchange_layout([0, 1], [True, False])
    with pytest.raises(ValueError):
        boost.exchange_layout([0, 255], [False])


def test_vaep_payload_is_a_tenth_of_the_dense_level():
    """515 bools and 53 numeric features of at most 254 cuts: at most 515 + 53 * 256 pairs per node."""
    lay, _ = _layout_case([1] * 515 + [254] * 53, [1] * 515 + [0] * 53)
    assert lay.n_bool + lay.n_num == 515 + 53 * 256
    assert lay.words(32) * 8 < 0.1 * 32 * 568 * 256 * 16


# ----------------------------------------------------------------------------- the global cut sample
@pytest.mark.parametrize('counts', [(1027, 0, 64, 1909), (70000, 3), (0, 0, 5), (65536, 65536), (1,)])
def test_ranks_picks_are_the_global_sample(counts):
    off = np.concatenate([[0], np.cumsum(counts)])
    picks = [boost.shard_sample_rows(counts, r) for r in range(len(counts))]
    for r, p in enumerate(picks):
        assert p.dtype == np.int64 and (p >= 0).all() and (p < max(counts[r], 1)).all() and (np.diff(p) > 0).all()
        assert counts[r] or not len(p)
    union = np.concatenate([p + off[r] for r, p in enumerate(picks)])
    np.testing.assert_array_equal(union, boost.sample_rows(sum(counts)))
    np.testing.assert_array_equal(union, br.sample_rows(sum(counts)))


def _frame(n=2500):
    rng = np.random.default_rng(21)
    a = rng.integers(0, 12, n).astype(np.float64)
    a[rng.random(n) < 0.2] = np.nan
    return pd.DataFrame({'nan': a, 'flag': rng.random(n) < 0.3, 'wide': rng.standard_normal(n),
                         'const': np.full(n, 7, np.int64), 'ints': rng.integers(-5, 400, n)})


_SPLITS = {2: (1100, 1400), 3: (900, 0, 1600)}


def _cuts_worker(rank, world, port, q):
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    off = np.concatenate([[0], np.cumsum(_SPLITS[world])])
    X = _frame().iloc[off[rank]:off[rank + 1]].reset_index(drop=True)
    rows = np.flatnonzero(np.arange(len(X)) % 5 != 0)  # the training rows of this rank
    q.put((rank, boost.make_cuts(X, process_group=dist.group.WORLD),
           boost.make_cuts(X, rows, process_group=dist.group.WORLD)))
    dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_cuts_over_gloo_equal_the_cuts_of_the_concatenation(world):
    import multiprocessing as mp
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_cuts_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    X = _frame()
    off = np.concatenate([[0], np.cumsum(_SPLITS[world])])
    rows = np.concatenate([off[r] + np.flatnonzero(np.arange(off[r + 1] - off[r]) % 5 != 0) for r in range(world)])
    want_all, want_rows = boost.make_cuts(X), boost.make_cuts(X, rows)
    # NaNs beside 12 values, a bool, more than 255 distinct values, a constant, integers with repeated quantiles
    assert [len(c) for c in want_all][:4] == [11, 1, 254, 0] and 200 < len(want_all[4]) <= 254
    for _, every, some in got:
        for c, (a, b, wa, wb) in enumerate(zip(every, some, want_all, want_rows)):
            assert a.dtype == np.float32 and a.tobytes() == wa.tobytes(), c
            assert b.tobytes() == wb.tobytes(), c
            np.testing.assert_array_equal(a, br.cuts_of(X.iloc[:, c].to_numpy(), X.iloc[:, c].dtype == bool))


# ----------------------------------------------------------------------------- the C entries
def test_exchange_entries_refuse_bad_arguments_without_a_gpu():
    from socceraction_amd import _native
    lib = _native.load_library()
    assert {'sa_boost_hist_pack', 'sa_boost_hist_unpack'} <= set(_native.EXPORTED_SYMBOLS)
    fake, odd = ctypes.c_void_p(256), ctypes.c_void_p(264)  # never dereferenced on the host
    E = _native.SA_EINVAL

    def pack(hist=fake, tree=fake, pairs=fake, nb=3, nn=5, node0=0, nodes=1, F=4, pay=fake):
        return lib.sa_boost_hist_pack(hist, tree, pairs, nb, nn, node0, nodes, F, pay, None)

    def unpack(pay=fake, pairs=fake, nb=3, nn=5, feat=fake, n_bool=3, node0=0, nodes=1, F=4, hist=fake, tree=fake):
        return lib.sa_boost_hist_unpack(pay, pairs, nb, nn, feat, n_bool, node0, nodes, F, hist, tree, None)

    for call in (pack, unpack):
        assert call(hist=None) == E and b'null' in lib.sa_last_error()
        assert call(tree=None) == E and call(pay=None) == E and call(pairs=None) == E
        assert call(node0=1, nodes=1) == E and b'sizes' in lib.sa_last_error()  # level_ok
        assert call(node0=2, nodes=3) == E and call(node0=63, nodes=64) == E
        assert call(F=0) == E and call(nb=-1) == E and call(nn=-1) == E
        assert call(nb=5, F=4) == E                # more bool pairs than features
        assert call(nb=0, nn=4 * 256 + 1) == E     # more pairs than a node has entries
        assert call(hist=odd) == E and b'aligned' in lib.sa_last_error()
        assert call(pay=odd) == E and call(tree=odd) == E
    assert unpack(n_bool=-1) == E and b'bool feature list' in lib.sa_last_error()
    assert unpack(n_bool=4) == E                   # a longer list than there are bool pairs
    assert unpack(feat=None) == E
    with pytest.raises(ValueError):
        _native.check(unpack(feat=None))
