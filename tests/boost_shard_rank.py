"""Run by tests/test_gpu_boost_shard.py once per rank, each in its own process: the sharded learner
over gloo with the ranks sharing the test GPU.  ``python boost_shard_rank.py RANK WORLD PORT OUT``:
the rank takes its slice of the shared table (tests/boost_shard_cases.py), runs every case through
``process_group=`` and writes what it ended with to ``OUT/rank{RANK}.npz`` for the test to compare
with the restatements on the whole table.  The process group has a 60 s timeout: a rank left
alone in a collective ends as an error, not as a wait."""
import datetime
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import boost_shard_cases as C  # noqa: E402
from socceraction_amd import boost, shard  # noqa: E402


def _fitted(out, name, clf):
    out[name + '_trees'] = clf.trees_.view(np.uint8)
    out[name + '_p'] = clf.p_.cpu().numpy()
    out[name + '_shift'] = np.int64(clf.quant_shift_)
    out[name + '_P'] = clf.record_['p'].cpu().numpy()
    out[name + '_M'] = clf.record_['margin'].cpu().numpy()
    for f, c in enumerate(clf.cuts_):
        out[f'{name}_cuts{f}'] = c


def _raises(fn):
    try:
        fn()
    except ValueError as e:
        return str(e)
    return ''


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    pg = dist.group.WORLD
    X, y = C.table()
    shards = C.SHARDS[world]
    a, b = C.bounds(shards)[rank]
    Xr, yr = X.iloc[a:b].reset_index(drop=True), y[a:b]
    w, keys = C.weights(y)[a:b], C.row_keys()[a:b]
    out = {}
    # plain fits from the host frames: global cuts, one exchange per level
    for k, params in C.PLAIN.items():
        _fitted(out, 'plain_' + k, boost.DeviceGBTClassifier(record=True, **params).fit(Xr, yr, process_group=pg))
    # tuned fits: weights (the largest on the last rank only), both samples, the L1 penalty
    for k, rk in (('tuned', None), ('tuned_keys', keys)):
        clf = boost.TunedGBTClassifier(record=True, **C.TUNED).fit(Xr, yr, sample_weight=w, row_keys=rk,
                                                                   process_group=pg)
        _fitted(out, k, clf)
    # early stopping by the log loss of held-out rows of every rank with rows
    train, ev = C.stop_rows(y, shards)[rank]
    data = boost.bin_host(Xr, rows=train, process_group=pg)
    yd = torch.zeros(data.ld, dtype=torch.uint8, device=data.device)
    yd[:data.n] = torch.from_numpy(np.ascontiguousarray(yr)).to(data.device)
    clf = boost.DeviceGBTClassifier(record=True, early_stopping_rounds=C.STOP_ROUNDS, eval_metric='logloss', **C.STOP)
    clf.fit_binned(data, yd, rows=torch.from_numpy(train).to(data.device),
                   eval_rows=torch.from_numpy(ev).to(data.device), process_group=pg)
    _fitted(out, 'stop', clf)
    out['stop_EP'] = clf.record_['eval_p'].cpu().numpy()
    out['stop_sums'] = np.array([str(v) for v in clf.eval_sums_])
    out['stop_scores'] = np.array(clf.evals_result_['validation_0']['logloss'])
    out['stop_best'] = np.array([clf.best_iteration, clf.n_rounds_run_])
    # agreement: what one rank refuses, every rank refuses, before any collective of the levels
    auc = boost.DeviceGBTClassifier(n_estimators=2, eval_metric='auc')
    out['auc_error'] = np.array(_raises(lambda: auc.fit_binned(data, yd, eval_rows=torch.from_numpy(ev).to(data.device),
                                                               process_group=pg)))
    bad = w.copy()
    if rank == world - 1:
        bad[0] = np.inf
    out['weight_error'] = np.array(_raises(lambda: boost.DeviceGBTClassifier(n_estimators=2).fit(
        Xr, yr, sample_weight=bad, process_group=pg)))
    # and the group is still usable afterwards
    again = boost.DeviceGBTClassifier(**C.PLAIN['d3']).fit(Xr, yr, process_group=pg)
    out['again_equal'] = np.array(again.trees_.tobytes() == out['plain_d3_trees'].tobytes())
    # the public path: every rank fits its own range of games and rates them with the common models
    from socceraction_amd.vaep import VAEP
    games, actions = C.games()
    g0, g1 = shard.partition_games(C.games_dict()['game_off'], world)[rank]
    mine = games.iloc[g0:g1]
    acts = actions[actions.game_id.isin(mine.game_id)].reset_index(drop=True)
    model = VAEP().fit_batch(mine, acts, tree_params=C.BATCH, process_group=pg)
    out['batch_models'] = np.array([json.dumps(model._VAEP__models[c].to_xgboost_json())
                                    for c in ('scores', 'concedes')])
    game = mine.iloc[0]
    ga = acts[acts.game_id == game.game_id].reset_index(drop=True)
    out['batch_game'] = np.int64(game.game_id)
    out['batch_values'] = model.rate(game, ga)['vaep_value'].to_numpy()
    empty = acts.iloc[:0] if rank == 0 else acts
    out['batch_error'] = np.array(_raises(lambda: VAEP().fit_batch(mine, empty, tree_params=C.BATCH,
                                                                   process_group=pg)))
    np.savez(os.path.join(outdir, f'rank{rank}.npz'), **out)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
