"""The sharded device learner (``process_group=``): the exchange kernels
``sa_boost_hist_pack`` / ``sa_boost_hist_unpack`` against numpy on one process, whole fits with the
rows split over 2 and 3 ranks that share the test GPU over gloo (tests/boost_shard_rank.py, one
process per rank), and the RCCL path with one rank (tests/boost_shard_rccl1.py).

Expected values come from the numpy restatements on the CONCATENATED table: as in
tests/test_gpu_boost.py a restated tree is built from the device's recorded ``p_t`` (``expf`` against
numpy's ``exp`` is the one float difference the contract allows) -- here the ranks' recorded
columns concatenated in rank order -- and node tables are compared as bytes."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import boost_reference as br
import boost_sample_reference as bsr
import boost_shard_cases as C
import boost_stop_reference as bst

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = br.NODE_DTYPE


@pytest.fixture(scope='module')
def boost():
    from socceraction_amd import _native, boost
    _native.load_library()
    return boost


@pytest.fixture(scope='module')
def whole():
    """The whole table once: host columns, the restated cuts and bins of all rows."""
    X, y = C.table()
    cols = [X[c].to_numpy() for c in X.columns]
    cuts = [br.cuts_of(c, c.dtype == np.bool_) for c in cols]
    B = np.stack([br.bins_of(br.cast32(c), k) for c, k in zip(cols, cuts)])
    return dict(X=X, y=y, cols=cols, cuts=cuts, B=B, is_bool=np.array([c.dtype == np.bool_ for c in cols]))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ----------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize('nodes', [1, 4, 32])
def test_pack_equals_the_numpy_gather(boost, whole, nodes):
    data = boost.bin_host(whole['X'].iloc[:64], cuts=whole['cuts'])
    cut_start = np.concatenate([[0], np.cumsum([len(c) for c in whole['cuts']])])
    lay = boost.exchange_layout(cut_start, whole['is_bool'])
    F = len(whole['cuts'])
    rng = np.random.default_rng(nodes)
    dense = np.zeros(nodes * F * 256 * 2, np.int64)
    at = lay.dense_pairs(nodes)
    dense.reshape(-1, 2)[at] = rng.integers(-2 ** 62, 2 ** 62, (len(at), 2))
    tab = np.zeros(4 * nodes, NODE)
    tab['G'][0], tab['H'][0] = -(2 ** 61) - 5, 2 ** 60 + 9
    tree = _dev(tab.view(np.uint8).reshape(4 * nodes, -1))
    got = boost.hist_pack(data, _dev(dense), tree, nodes).cpu().numpy()
    head = np.array([tab['G'][0], tab['H'][0]]) if nodes == 1 else np.zeros(0, np.int64)
    want = np.concatenate([head, dense.reshape(-1, 2)[at].ravel()])
    assert got.shape == (lay.words(nodes),)
    np.testing.assert_array_equal(got, want)


def _level_inputs(n, nodes, seed):
    rng = np.random.default_rng(seed)
    gq = rng.integers(-2 ** 30, 2 ** 30, n).astype(np.int32)
    hq = rng.integers(0, 2 ** 28, n).astype(np.int32)
    gq[rng.random(n) < 0.05] = 0
    node = rng.integers(0, nodes, n).astype(np.int64)
    node[rng.random(n) < 0.1] = 255  # held-out rows
    return gq, hq, node


@pytest.mark.parametrize('nodes', [1, 4, 32])
def test_unpack_of_summed_parts_is_the_histogram_of_the_whole(boost, whole, nodes):
    """Three parts binned and summed on their own, packed, added in numpy and unpacked: the dense
    histogram of the whole table, bit for bit, every bool feature's bin 0 included -- at level 0
    from the summed root totals, past it from preset global totals."""
    X, cuts, B = whole['X'], whole['cuts'], whole['B']
    gq, hq, node = _level_inputs(C.N, nodes, 100 + nodes)
    want = br.histograms(B, gq, hq, node, nodes)
    live = node != 255
    totals = np.zeros((nodes, 2), np.int64)
    np.add.at(totals[:, 0], node[live], gq[live].astype(np.int64))
    np.add.at(totals[:, 1], node[live], hq[live].astype(np.int64))
    total, parts, a = None, [], 0
    for m in C.PARTS:
        data = boost.bin_host(X.iloc[a:a + m].reset_index(drop=True), cuts=cuts)
        h, tree = boost.level_histogram(data, _dev(gq[a:a + m]), _dev(hq[a:a + m]), _dev(node[a:a + m]), nodes,
                                        None if nodes == 1 else totals)
        pay = boost.hist_pack(data, h, tree, nodes).cpu().numpy()
        total = pay if total is None else total + pay
        parts.append((data, h, tree))
        a += m
    assert a == C.N
    for data, h, tree in parts:  # every rank unpacks the same sum into its own histogram
        if nodes > 1:  # what a rank's own bin 0 was: the global total minus its LOCAL bin 1 -- never summed
            assert not torch.equal(h.cpu(), torch.from_numpy(want))
        boost.hist_unpack(data, _dev(total), h, tree, nodes)
        np.testing.assert_array_equal(h.cpu().numpy(), want)
        tab = tree.cpu().numpy().view(NODE).reshape(-1)[nodes - 1:2 * nodes - 1]
        np.testing.assert_array_equal(np.stack([tab['G'], tab['H']], 1), totals)
    bools = np.flatnonzero(whole['is_bool'])
    np.testing.assert_array_equal(want[:, bools, 0, :] + want[:, bools, 1, :],
                                  np.broadcast_to(totals[:, None, :], (nodes, len(bools), 2)))


def test_unpack_rebuilds_bin_0_of_the_listed_bools_only(boost, whole):
    """Under a column sample the level's bitmap call lists the round's bool features: the others'
    histograms stay zero, bin 0 included."""
    data = boost.bin_host(whole['X'].iloc[:C.PARTS[0]], cuts=whole['cuts'])
    gq, hq, node = _level_inputs(C.PARTS[0], 1, 3)
    h, tree = boost.level_histogram(data, _dev(gq), _dev(hq), _dev(node), 1)
    pay = boost.hist_pack(data, h, tree, 1)
    keep = data.bit_feat[::3]
    for f in np.setdiff1d(data.bit_feat, keep):  # (an unlisted feature travels as zeros)
        pay[2:].view(-1, 2)[list(data.bit_feat).index(f)] = 0
    h2 = torch.zeros_like(h)
    boost.hist_unpack(data, pay, h2, tree, 1, _dev(keep.astype(np.int32)), len(keep))
    got, full = h2.cpu().numpy(), h.cpu().numpy()
    for f in data.bit_feat:
        np.testing.assert_array_equal(got[0, f], full[0, f] if f in keep else 0)
    np.testing.assert_array_equal(got[0, data.num_feat], full[0, data.num_feat])


DEBUG_BUILD = '''
import numpy as np, torch
import boost_shard_cases as C
from socceraction_amd import _native, boost
lib = _native.lib()
assert lib.sa_debug_enabled() == 1
X, y = C.table()
data = boost.bin_host(X)
rng = np.random.default_rng(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
for nodes in (1, 32):
    node = rng.integers(0, nodes, C.N)
    h, tree = boost.level_histogram(data, dev(rng.integers(-9, 9, C.N).astype(np.int32)),
                                    dev(rng.integers(0, 9, C.N).astype(np.int32)), dev(node), nodes)
    want = h.clone()
    pay = boost.hist_pack(data, h, tree, nodes).clone()
    h.zero_()
    boost.hist_unpack(data, pay, h, tree, nodes)
    assert torch.equal(h, want), nodes
_native.check(lib.sa_debug_check())  # no dense offset left its level
print('ok')
'''


def test_exchange_kernels_through_the_debug_build():
    """The debug library's bounds checks on the dense offset stay silent over a whole round trip."""
    path = [ROOT, os.path.join(ROOT, 'tests')] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]
    env = dict(os.environ, SOCCERACTION_AMD_DEBUG='1', PYTHONPATH=os.pathsep.join(path))
    p = subprocess.run([sys.executable, '-c', DEBUG_BUILD], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().endswith('ok')


# ----------------------------------------------------------------------------- ranks over gloo
def _run_world(world, tmp):
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, os.path.join(ROOT, 'tests', 'boost_shard_rank.py')]
    procs = [subprocess.Popen(cmd + [str(r), str(world), str(port), str(tmp)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, cwd=ROOT) for r in range(world)]
    res = []
    try:
        for p in procs:
            _, err = p.communicate(timeout=240)
            assert p.returncode == 0, err[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r in range(world):
        with np.load(os.path.join(str(tmp), f'rank{r}.npz')) as z:
            res.append({k: z[k] for k in z.files})
    return res


@pytest.fixture(scope='module', params=[2, 3])
def ranks(request, tmp_path_factory):
    """Every case of one world, run once: ``(world, [what each rank ended with])``."""
    return request.param, _run_world(request.param, tmp_path_factory.mktemp(f'world{request.param}'))


def _trees(r, name):
    t = r[name + '_trees']
    return t.view(NODE).reshape(t.shape[0], -1)


def _same_on_all_ranks(res, name, whole_cuts):
    for r in res[1:]:
        assert r[name + '_trees'].tobytes() == res[0][name + '_trees'].tobytes(), name
        assert r[name + '_shift'] == res[0][name + '_shift']
    for r in res:
        for f, c in enumerate(whole_cuts):
            assert r[f'{name}_cuts{f}'].tobytes() == c.tobytes(), (name, f)


def _concat(res, key):
    return np.concatenate([r[key] for r in res], axis=-1)


@pytest.mark.parametrize('which', sorted(C.PLAIN))
def test_plain_sharded_fit(ranks, whole, which):
    world, res = ranks
    params, name = C.PLAIN[which], 'plain_' + which
    _same_on_all_ranks(res, name, whole['cuts'])
    trees = _trees(res[0], name)
    assert trees.shape == (params['n_estimators'], 2 ** (params['max_depth'] + 1) - 1)
    P, M = _concat(res, name + '_P'), _concat(res, name + '_M')
    assert P.shape == (params['n_estimators'], C.N)
    y, m = whole['y'], np.full(C.N, br.base_margin(0.5), np.float32)
    for t in range(params['n_estimators']):
        np.testing.assert_allclose(P[t], br.probability(m), rtol=1e-6, atol=0)
        gq, hq = br.quantise(P[t], y)  # the restated tree of the concatenated table from the device's p_t
        tab, node = br.build_tree(whole['B'], gq, hq, whole['cuts'], {**br.DEFAULTS, **params})
        assert tab.tobytes() == trees[t].tobytes(), (t, tab, trees[t])
        m = br.update_margin(m, tab, node)
        assert m.tobytes() == M[t].tobytes(), t
    if which == 'd6':
        assert (trees['exists'][:, 31:63] != 0).sum() > 16  # the 32-node level is exchanged in earnest
    # every rank's p_ are the probabilities of its own rows under the common model
    X32 = np.stack([br.cast32(c) for c in whole['cols']], 1)
    want = br.predict(trees, X32)
    got = _concat(res, name + '_p')
    assert [len(r[name + '_p']) for r in res] == list(C.SHARDS[world])
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    np.testing.assert_allclose(got, br.probability(m), rtol=1e-6, atol=0)
    assert all(bool(r['again_equal']) for r in res)


@pytest.mark.parametrize('name', ['tuned', 'tuned_keys'])
def test_tuned_sharded_fit(ranks, whole, name):
    world, res = ranks
    _same_on_all_ranks(res, name, whole['cuts'])
    params = {**bsr.DEFAULTS, **C.TUNED}
    y, w = whole['y'], C.weights(whole['y'])
    keys = C.row_keys() if name == 'tuned_keys' else np.arange(C.N, dtype=np.int64)  # default: the global index
    we = bsr.effective_weight(w, y, params['scale_pos_weight'])
    e = bsr.shift_of(we.max())
    assert e > bsr.shift_of(we[:-1].max())  # the last row, on the last rank alone, lifts the shift
    assert all(int(r[name + '_shift']) == e for r in res)
    trees = _trees(res[0], name)
    P, M = _concat(res, name + '_P'), _concat(res, name + '_M')
    F, m = len(whole['cuts']), np.full(C.N, br.base_margin(0.5), np.float32)
    sampled = 0
    for t in range(params['n_estimators']):
        np.testing.assert_allclose(P[t], br.probability(m), rtol=1e-6, atol=0)
        rows, cols = bsr.round_inputs(params, t, F, keys)
        sampled += int(rows.sum())
        gq, hq = bsr.quantise(P[t], y, we, e, rows)
        tab, node = bsr.build_tree(whole['B'], gq, hq, whole['cuts'], params, e, cols)
        assert tab.tobytes() == trees[t].tobytes(), (t, tab, trees[t])
        m = br.update_margin(m, tab, node)
        assert m.tobytes() == M[t].tobytes(), t
    assert 0.4 < sampled / (params['n_estimators'] * C.N) < 0.6
    assert (trees['feature'] >= 0).sum() >= params['n_estimators']


def test_tuned_fits_differ_by_their_keys(ranks):
    _, res = ranks
    assert res[0]['tuned_trees'].tobytes() != res[0]['tuned_keys_trees'].tobytes()


def test_early_stopping_on_the_ranks_joint_log_loss(ranks, whole):
    world, res = ranks
    shards, y = C.SHARDS[world], whole['y']
    train, ev = np.zeros(C.N, bool), []
    for (a, _), (tr, e) in zip(C.bounds(shards), C.stop_rows(y, shards)):
        train[a + tr] = True
        ev.append(a + e)
    assert (y[ev[0]] == 0).all() and len(ev[0]) == 150  # rank 0 alone holds one class only
    ev = np.concatenate(ev)
    cuts = [br.cuts_of(c[train], c.dtype == np.bool_) for c in whole['cols']]  # the training rows, rank order
    B = np.stack([br.bins_of(br.cast32(c), k) for c, k in zip(whole['cols'], cuts)])
    _same_on_all_ranks(res, 'stop', cuts)
    for r in res[1:]:
        for k in ('stop_sums', 'stop_scores', 'stop_best'):
            assert r[k].tobytes() == res[0][k].tobytes(), k
    best, run = (int(v) for v in res[0]['stop_best'])
    series = [int(v) for v in res[0]['stop_sums']]
    P, EP = _concat(res, 'stop_P'), _concat(res, 'stop_EP')
    assert P.shape == (run, C.N) and EP.shape == (run, len(ev)) and len(series) == run
    params, tabs = {**br.DEFAULTS, **C.STOP}, []
    for t in range(run):
        gq, hq = br.quantise(P[t], y)
        tabs.append(br.build_tree(B, gq, hq, cuts, params, active=train)[0])
        # the ranks' joint integer against the restatement on all held-out rows: the device's float64
        # log against numpy's, at the 1e-12 relative bar of tests/test_gpu_boost_stop.py
        want = bst.logloss_integer(y[ev], EP[t])
        print(world, t, 'log-loss integer', series[t], 'restated', want)
        assert abs(series[t] - want) <= 1e-12 * want, t
        assert res[0]['stop_scores'][t] == bst.metric_score(series[t], 'logloss', y[ev])
    assert (best, run) == bst.stopping(series, C.STOP_ROUNDS, False)
    assert run < C.STOP['n_estimators'] and run == best + C.STOP_ROUNDS + 1
    kept = _trees(res[0], 'stop')
    assert len(kept) == best + 1
    for t in range(best + 1):
        assert tabs[t].tobytes() == kept[t].tobytes(), t
    # the evaluation rows' probabilities are the kept model's, by the restated walk
    X32 = np.stack([br.cast32(c) for c in whole['cols']], 1)
    np.testing.assert_allclose(EP[best], br.predict(kept, X32[ev]), rtol=1e-6, atol=0)
    # and the restatement alone, with numpy's exp, stops at the same round
    alone = bst.fit(B, y, cuts, train, ev, 'logloss', C.STOP_ROUNDS, **C.STOP)
    assert (alone['best_iteration'], alone['rounds_run']) == (best, run)


def test_one_ranks_refusal_is_every_ranks(ranks):
    world, res = ranks
    for r in res:
        assert 'auc' in str(r['auc_error']) and 'process group' in str(r['auc_error'])
        assert 'finite' in str(r['weight_error'])  # only the last rank held the non-finite weight


@pytest.fixture(scope='module')
def one_gpu_batch_fit():
    """``VAEP.fit_batch`` of all nine games on one device, without a process group."""
    import json

    from socceraction_amd.vaep import VAEP
    games, actions = C.games()
    model = VAEP().fit_batch(games, actions, tree_params=C.BATCH)
    return games, actions, model, [json.dumps(model._VAEP__models[c].to_xgboost_json())
                                   for c in ('scores', 'concedes')]


def test_fit_batch_over_the_ranks_games_is_the_one_gpu_fit(ranks, one_gpu_batch_fit):
    """Every rank passed one range of ``shard.partition_games``: both models are the unsharded
    ones on every rank, each rank rates a game of its own as the unsharded model does, and an
    empty ``actions`` frame on rank 0 is every rank's ``ValueError``."""
    world, res = ranks
    games, actions, model, want = one_gpu_batch_fit
    seen = set()
    for r in res:
        assert [str(m) for m in r['batch_models']] == want
        game = games[games.game_id == int(r['batch_game'])].iloc[0]
        ga = actions[actions.game_id == game.game_id].reset_index(drop=True)
        assert r['batch_values'].tobytes() == model.rate(game, ga)['vaep_value'].to_numpy().tobytes()
        seen.add(int(r['batch_game']))
        assert 'fit_batch' in str(r['batch_error'])
    assert len(seen) == world  # every rank held games of its own
    assert 'actions on every rank' in str(res[0]['batch_error'])


# ----------------------------------------------------------------------------- RCCL, one rank
def test_rccl_world1_sharded_fit_equals_the_unsharded():
    import json
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29531', RANK='0', WORLD_SIZE='1', LOCAL_RANK='0')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'boost_shard_rccl1.py')], env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out['backend'] == 'nccl'
    assert out['fit_binned_trees_equal'] and out['fit_binned_p_equal'] and out['tuned_trees_equal']
    assert out['stop_equal']
    assert out['exchange_launches'] == {'pack': 5 * 3, 'allreduce': 5 * 3, 'unpack': 5 * 3}
    assert out['plain_has_no_exchange']
    assert out['fit_batch_models_equal'] and out['fit_batch_rate_equal']
    assert out['atomic_models_equal']
