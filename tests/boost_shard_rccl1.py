"""Run by tests/test_gpu_boost_shard.py in its own process: the sharded learner through REAL RCCL
(backend nccl) with one rank on one GPU.  With world size 1 every collective is an identity, but
pack, the device all-reduce and unpack run with the real tensors, stream-ordered, and the level
histogram goes through the exchange layout and back: any entry the layout dropped would change the
trees.  Everything must equal the unsharded path byte for byte."""
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
from socceraction_amd import boost, synthetic  # noqa: E402


def _families(clf):
    out = {}
    for fam, _, _ in clf._events:
        out[fam] = out.get(fam, 0) + 1
    return out


def _models_equal(a, b):
    return all(json.dumps(a._VAEP__models[c].to_xgboost_json()) == json.dumps(b._VAEP__models[c].to_xgboost_json())
               and len(a._VAEP__models[c].trees_) > 0 for c in ('scores', 'concedes'))


def main():
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
    pg = dist.group.WORLD
    out = {'backend': dist.get_backend(pg)}
    X, y = C.table()
    data = boost.bin_host(X)
    yd = torch.zeros(data.ld, dtype=torch.uint8, device=data.device)
    yd[:data.n] = torch.from_numpy(y).to(data.device)
    # 1. fit_binned: plain (with the launch families counted), tuned, early stopping
    params = C.PLAIN['d3']
    one = boost.DeviceGBTClassifier(**params)
    one._events = []
    one.fit_binned(data, yd)
    sharded = boost.DeviceGBTClassifier(**params)
    sharded._events = []
    sharded.fit_binned(data, yd, process_group=pg)
    out['fit_binned_trees_equal'] = sharded.trees_.tobytes() == one.trees_.tobytes()
    out['fit_binned_p_equal'] = bool(torch.equal(sharded.p_, one.p_))
    fam = _families(sharded)
    out['exchange_launches'] = {k: fam.get(k, 0) for k in ('pack', 'allreduce', 'unpack')}
    plain = _families(one)
    out['plain_has_no_exchange'] = not any(k in plain for k in ('pack', 'allreduce', 'unpack')) and \
        {k: v for k, v in fam.items() if k not in ('pack', 'allreduce', 'unpack')} == plain
    w, keys = C.weights(y), C.row_keys()
    a = boost.TunedGBTClassifier(**C.TUNED).fit(X, y, sample_weight=w, row_keys=keys)
    b = boost.TunedGBTClassifier(**C.TUNED).fit(X, y, sample_weight=w, row_keys=keys, process_group=pg)
    out['tuned_trees_equal'] = a.trees_.tobytes() == b.trees_.tobytes() and a.quant_shift_ == b.quant_shift_
    ev =np.arange(C.N)[np.arange(C.N) % 4 == 3]
    train = np.setdiff1d(np.arange(C.N), ev)
    fits = []
    for group in (None, pg):
        clf = boost.DeviceGBTClassifier(early_stopping_rounds=C.STOP_ROUNDS, eval_metric='logloss', **C.STOP)
        fits.append(clf.fit_binned(data, yd, rows=train, eval_rows=ev, process_group=group))
    out['stop_equal'] = fits[0].trees_.tobytes() == fits[1].trees_.tobytes() and \
        fits[0].eval_sums_ == fits[1].eval_sums_ and fits[0].best_iteration == fits[1].best_iteration and \
        fits[0].n_rounds_run_ == fits[1].n_rounds_run_ < C.STOP['n_estimators']
    # 2. the public path: fit_batch on 20 synthetic games, then rate
    from socceraction_amd.atomic.vaep import AtomicVAEP
    from socceraction_amd.vaep import VAEP
    d = synthetic.spadl_games(20, seed=3, mean_actions=300.0)
    games, actions = synthetic.games_frame(d), synthetic.to_frame(d)
    tp = dict(n_estimators=6, max_depth=3)
    m0 = VAEP().fit_batch(games, actions, tree_params=tp)
    m1 = VAEP().fit_batch(games, actions, tree_params=tp, process_group=pg)
    out['fit_batch_models_equal'] = _models_equal(m0, m1)
    game = games.iloc[0]
    ga = actions[actions.game_id == game.game_id].reset_index(drop=True)
    r0, r1 = m0.rate(game, ga), m1.rate(game, ga)
    out['fit_batch_rate_equal'] = all(r0[c].to_numpy().tobytes() == r1[c].to_numpy().tobytes()
                                      for c in ('offensive_value', 'defensive_value', 'vaep_value'))
    da = synthetic.atomic_games(4, seed=5, mean_actions=400.0)
    ag, aa = synthetic.games_frame(da), synthetic.to_frame(da, atomic=True)
    out['atomic_models_equal'] = _models_equal(AtomicVAEP().fit_batch(ag, aa, tree_params=tp),
                                               AtomicVAEP().fit_batch(ag, aa, tree_params=tp, process_group=pg))
    dist.destroy_process_group()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
