"""One device fit of both VAEP learners (socceraction_amd.boost, default parameters: 100 rounds,
depth 3) on the synthetic cfg2-shaped batch of `--games` games, timed per kernel family with HIP
events -- bin, grad, hist_bits, hist_bins, split, advance -- plus the wall clock of the whole
``VAEP.fit_batch`` call, and as a reference point (not a pass mark) scikit-learn's
HistGradientBoostingClassifier with the same shape on the host's CPUs on the same rows copied
out, with the copy-out time.

One warm-up fit (2 rounds) precedes everything timed.  The per-family figures come from one
instrumented fit per learner (an event pair around every launch: the sum over the fit and the
median launch); the wall clock is the median of `--reps` uninstrumented ``fit_batch`` calls.  The
histogram kernels are also held against the bytes a level has to read (bitmaps n_bool / 8, bins
F_num, gradients and node 9 bytes per row).

With ``--val-size`` the reference's random split holds that share of the rows out and the
instrumented fits evaluate them after every round (the families apply, metric and sort: the tree
walk over the held-out rows, ``sa_metric_sums`` / ``sa_auc_keys`` / ``sa_auc_count``, and the sort
of the minority keys); with ``--early-stopping-rounds`` training also stops by the rule, and the
record carries ``n_rounds_run_``, ``best_iteration``, the host's looks at the metric table and the
held-out scores per learner.

``--subsample``, ``--colsample-bytree``, ``--reg-alpha``, ``--scale-pos-weight``, ``--random-state``
and ``--max-weight W`` (a synthetic weight column uniform in [0, W); W > 1 gives a quantisation
shift e > 0) put the learner's tuning parameters into every fit of the run.

``--sampling-record`` instead writes the record of those parameters' cost
(``profiles/boost_fit_sampling.json``): for the default parameters, ``colsample_bytree=0.5``,
``subsample=0.5`` and weights with e > 0 in turn, the median and the spread of `--reps`
``fit_batch`` calls and the per-family event sums of one instrumented fit per learner, each as a
ratio to the default's; ``--parent-json FILE`` (this script's ``--out`` file from the parent
commit, run on the same device in the same session) puts the parent's default figures beside
the first.

``--sharded-record`` writes the record of the sharded fit (``profiles/boost_fit_sharded.json``),
measured with ONE rank through RCCL (backend nccl, world 1 -- nothing about more ranks can be
measured on one device): `--reps` default ``fit_batch`` calls without a process group (with
``--parent-json`` held against the parent commit's own runs: no exchange code may run without a
group; ``--self-json``: this commit's ``--out`` file of the default mode from the same session, the
like-for-like figure), the same calls through ``process_group=``, and from one instrumented sharded fit per learner
the cost of pack + all-reduce + unpack per level and the payload bytes per tree against the dense
level histograms they replace.

    python scripts/boost_time.py [--games 1000] [--reps 3] [--val-size 0.25]
        [--early-stopping-rounds 10] [--eval-metric auc|logloss] [--sklearn] [--out FILE]
        [--subsample S] [--colsample-bytree C] [--reg-alpha A] [--scale-pos-weight P]
        [--random-state R] [--max-weight W] [--sampling-record [--parent-json FILE]]
        [--sharded-record [--parent-json FILE] [--self-json FILE]]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from socceraction_amd import batch as B, boost, ops, synthetic  # noqa: E402
from socceraction_amd.vaep import VAEP  # noqa: E402

HBM_BYTES_PER_S = 8e12
FAMILIES = ('grad', 'hist_bits', 'hist_bins', 'split', 'advance', 'apply', 'metric', 'sort')
EVAL_FAMILIES = ('apply', 'metric', 'sort')
SPLIT_SEED = 0


def sampling_record(args, games, actions, data, lb) -> dict:
    """The four configurations of ``--sampling-record`` on one batch, one after the other."""
    n = data.n
    w = (np.random.default_rng(0).random(n) * args.max_weight).astype(np.float32)
    keys = boost.row_keys(actions['game_id'].to_numpy(), actions['action_id'].to_numpy(), data.device)
    configs = [('default', {}, None), ('colsample_bytree_0.5', dict(colsample_bytree=0.5), None),
               ('subsample_0.5', dict(subsample=0.5), None), (f'weights_below_{args.max_weight:g}', {}, w)]
    out = {}
    for name, tp, weight in configs:
        fams, shift, splits = {}, None, 0
        for col in ('scores', 'concedes'):  # one instrumented fit per learner
            clf = boost.make_classifier(tp)
            clf._events = []
            clf.fit_binned(data, getattr(lb, col), None, None, weight, keys)
            torch.cuda.synchronize()
            for fam, a, b in clf._events:
                fams[fam] = fams.get(fam, 0.0) + a.elapsed_time(b)
            shift, splits = clf.quant_shift_, splits + int(((clf.trees_['feature'] >= 0)
                                                            & (clf.trees_['exists'] != 0)).sum())
        walls, models = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = VAEP().fit_batch(games, actions, tree_params=tp, sample_weight=weight)
            torch.cuda.synchronize()
            walls.append(round((time.perf_counter() - t0) * 1e3, 1))
            models.append(json.dumps(m._VAEP__models['scores'].to_xgboost_json()))
        out[name] = {'tree_params': tp, 'weights': weight is not None, 'quant_shift': shift,
                     'fit_batch_wall_ms': walls, 'fit_batch_wall_ms_median': statistics.median(walls),
                     'fit_batch_wall_ms_spread': round(max(walls) - min(walls), 1),
                     'family_sum_ms_both_learners': {f: round(v, 2) for f, v in fams.items()},
                     'kernel_sum_ms_both_learners': round(sum(fams.values()), 2), 'split_nodes': splits,
                     'run_to_run_equal': len(set(models)) == 1}
        print(name, json.dumps(out[name]), flush=True)
    base = out['default']
    for name, entry in out.items():
        entry['wall_ratio_to_default'] = round(entry['fit_batch_wall_ms_median'] / base['fit_batch_wall_ms_median'], 4)
        entry['kernel_ratio_to_default'] = round(entry['kernel_sum_ms_both_learners']
                                                 / base['kernel_sum_ms_both_learners'], 4)
        entry['hist_ratio_to_default'] = round(
            sum(entry['family_sum_ms_both_learners'][f] for f in ('hist_bits', 'hist_bins'))
            / sum(base['family_sum_ms_both_learners'][f] for f in ('hist_bits', 'hist_bins')), 4)
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        pw = parent['fit_batch_wall_ms']
        out['parent_commit_default'] = {
            'fit_batch_wall_ms': pw, 'fit_batch_wall_ms_median': statistics.median(pw),
            'fit_batch_wall_ms_spread': round(max(pw) - min(pw), 1), 'device': parent.get('device'),
            'rows': parent.get('rows'),
            'family_sum_ms_both_learners': {f: round(parent['scores']['sum_ms'][f] + parent['concedes']['sum_ms'][f], 2)
                                            for f in ('grad', 'hist_bits', 'hist_bins', 'split', 'advance')}}
        out['default_minus_parent_wall_ms'] = round(base['fit_batch_wall_ms_median']
                                                    - out['parent_commit_default']['fit_batch_wall_ms_median'], 1)
    return out


EXCHANGE_FAMILIES = ('pack', 'allreduce', 'unpack')


def sharded_record(args, games, actions, data, lb) -> dict:
    """``--sharded-record``: the default fit with and without a one-rank RCCL process group."""
    import torch.distributed as dist

    def walls_of(group):
        walls = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = VAEP().fit_batch(games, actions, process_group=group)
            torch.cuda.synchronize()
            walls.append(round((time.perf_counter() - t0) * 1e3, 1))
        return {'fit_batch_wall_ms': walls, 'fit_batch_wall_ms_median': statistics.median(walls),
                'fit_batch_wall_ms_spread': round(max(walls) - min(walls), 1)}, \
            {c: json.dumps(m._VAEP__models[c].to_xgboost_json()) for c in ('scores', 'concedes')}

    def families_of(group):
        fams, levels = {}, 0
        for col in ('scores', 'concedes'):  # one instrumented fit per learner
            clf = boost.make_classifier({})
            clf._events = []
            clf.fit_binned(data, getattr(lb, col), process_group=group)
            torch.cuda.synchronize()
            for fam, a, b in clf._events:
                fams[fam] = fams.get(fam, 0.0) + a.elapsed_time(b)
            levels += sum(1 for fam, _, _ in clf._events if fam == 'allreduce')
            clf._events = None
        return fams, levels

    out, models = {}, {}
    # the default call first, in a process that has not yet started RCCL and, as in the default mode, after the
    # instrumented fits: what the parent commit's run measures
    plain_fams, _ = families_of(None)
    out['unsharded'], models['unsharded'] = walls_of(None)
    for k, v in (('MASTER_ADDR', '127.0.0.1'), ('MASTER_PORT', '29541'), ('RANK', '0'), ('WORLD_SIZE', '1')):
        os.environ.setdefault(k, v)
    dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
    pg = dist.group.WORLD
    out.update(backend=dist.get_backend(pg), world=dist.get_world_size(pg),
               note='one rank: every collective is an identity; nothing here says what N > 1 ranks cost')
    VAEP().fit_batch(games, actions, process_group=pg)  # warm-up (RCCL's setup, the payload buffers)
    out['sharded_world1'], models['sharded_world1'] = walls_of(pg)
    out['unsharded_after_rccl_init'], _ = walls_of(None)
    out['models_equal'] = models['unsharded'] == models['sharded_world1']
    fams, levels = families_of(pg)
    exchange = sum(fams.get(f, 0.0) for f in EXCHANGE_FAMILIES)
    lay, D = boost._exchange(data)[0], int(boost.DEFAULTS['max_depth'])
    payload = 8 * sum(lay.words(2 ** level) for level in range(D))
    dense = 16 * 256 * data.n_features * sum(2 ** level for level in range(D))
    out['instrumented'] = {
        'family_sum_ms_both_learners': {f: round(v, 2) for f, v in fams.items()},
        'unsharded_family_sum_ms_both_learners': {f: round(v, 2) for f, v in plain_fams.items()},
        'level_collectives_both_learners': levels,
        'exchange_ms_per_level': {f: round(fams.get(f, 0.0) / levels, 4) for f in EXCHANGE_FAMILIES},
        'exchange_ms_per_level_total': round(exchange / levels, 4),
        'exchange_share_of_kernel_time': round(exchange / sum(fams.values()), 4)}
    out['payload'] = {'pairs_per_node': lay.n_bool + lay.n_num, 'bool_pairs': lay.n_bool, 'numeric_pairs': lay.n_num,
                      'payload_bytes_per_tree': payload, 'dense_bytes_per_tree': dense,
                      'payload_over_dense': round(payload / dense, 4),
                      'payload_bytes_per_level': [8 * lay.words(2 ** level) for level in range(D)]}
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        pw = parent['fit_batch_wall_ms']
        out['parent_commit_unsharded'] = {'fit_batch_wall_ms': pw, 'fit_batch_wall_ms_median': statistics.median(pw),
                                          'fit_batch_wall_ms_spread': round(max(pw) - min(pw), 1),
                                          'device': parent.get('device'), 'rows': parent.get('rows')}
        mine = out['unsharded']
        if args.self_json:  # this commit's own default-mode run: the parent's procedure, call for call
            with open(args.self_json) as f:
                sw = json.load(f)['fit_batch_wall_ms']
            mine = out['this_commit_default_mode'] = {
                'fit_batch_wall_ms': sw, 'fit_batch_wall_ms_median': statistics.median(sw),
                'fit_batch_wall_ms_spread': round(max(sw) - min(sw), 1)}
        med = mine['fit_batch_wall_ms_median']
        out['unsharded_median_within_parent_runs'] = bool(min(pw) <= med <= max(pw))
        out['unsharded_minus_parent_wall_ms'] = round(med - statistics.median(pw), 1)
    dist.destroy_process_group()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--val-size', type=float, default=0.0)
    ap.add_argument('--early-stopping-rounds', type=int, default=None)
    ap.add_argument('--eval-metric', default='auc', choices=boost.EVAL_METRICS)
    ap.add_argument('--sklearn', action='store_true')
    ap.add_argument('--out', default='')
    ap.add_argument('--subsample', type=float, default=1.0)
    ap.add_argument('--colsample-bytree', type=float, default=1.0)
    ap.add_argument('--reg-alpha', type=float, default=0.0)
    ap.add_argument('--scale-pos-weight', type=float, default=1.0)
    ap.add_argument('--random-state', type=int, default=0)
    ap.add_argument('--max-weight', type=float, default=0.0)
    ap.add_argument('--sampling-record', action='store_true')
    ap.add_argument('--parent-json', default='')
    ap.add_argument('--sharded-record', action='store_true')
    ap.add_argument('--self-json', default='')
    args = ap.parse_args()
    tp = {k: v for k, v in dict(subsample=args.subsample, colsample_bytree=args.colsample_bytree,
                                reg_alpha=args.reg_alpha, scale_pos_weight=args.scale_pos_weight,
                                random_state=args.random_state).items() if v != boost.ALL_DEFAULTS[k]}
    if args.sampling_record and not args.max_weight > 0:
        args.max_weight = 5.0
    stop = dict(early_stopping_rounds=args.early_stopping_rounds, eval_metric=args.eval_metric)
    if args.early_stopping_rounds is not None and not args.val_size > 0:
        ap.error('--early-stopping-rounds needs --val-size')
    d = synthetic.spadl_games(args.games, seed=2)
    actions, games = synthetic.to_frame(d), synthetic.games_frame(d)
    model = VAEP()
    known, _ = model._split_xfns()
    home_of = games.set_index('game_id')['home_team_id']
    ab = B.ActionBatch.from_frame(actions, home_team_id=home_of, segments='game')
    n = ab.n
    res = {'device': torch.cuda.get_device_name(0), 'games': args.games, 'rows': n, 'reps': args.reps,
           'params': {**boost.ALL_DEFAULTS, **tp}, 'max_weight': args.max_weight,
           'hbm_bytes_per_s_for_floors': HBM_BYTES_PER_S,
           'val_size': args.val_size, **stop}
    # ---- warm-up, and the model is the same from run to run
    VAEP().fit_batch(games, actions, tree_params=dict(n_estimators=2))
    fb = ops.features(ab, known, 3, bool_bits=True)
    lb = ops.labels(ab)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = val_rows = None
    if args.val_size > 0:  # fit_batch's split, from the same seed
        np.random.seed(SPLIT_SEED)
        idx = np.random.permutation(n)
        cut = math.floor(n * (1 - args.val_size))
        rows = torch.from_numpy(np.sort(idx[:cut])).to(ab.device)
        val_rows = torch.from_numpy(np.sort(idx[cut + 1:])).to(ab.device)
        res['eval_rows'] = int(val_rows.numel())
    t0 = time.perf_counter()
    cuts = boost.make_cuts(fb, rows)
    torch.cuda.synchronize()
    res['make_cuts_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
    e0.record()
    data = boost.bin_blocks(fb, cuts)
    e1.record()
    torch.cuda.synchronize()
    n_bool, f_num = len(data.bit_feat), len(data.num_feat)
    res.update(n_bool=n_bool, f_num=f_num, bin_ms=round(e0.elapsed_time(e1), 3))
    res['bin_GBs'] = round(n * (8 * f_num + f_num) / e0.elapsed_time(e1) * 1e-6, 1)
    bytes_level = {'hist_bits': n * (n_bool / 8 + 9), 'hist_bins': n * (f_num + 9)}
    res['bytes_per_row_per_level'] = {'bitmaps': n_bool / 8, 'bins': f_num, 'gradients_and_node': 9}
    if args.sharded_record:
        res['sharded'] = sharded_record(args, games, actions, data, lb)
    if args.sampling_record:
        res['configurations'] = sampling_record(args, games, actions, data, lb)
    if args.sharded_record or args.sampling_record:
        line = json.dumps(res)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
        print(line)
        return
    weight = None
    if args.max_weight > 0:
        weight = (np.random.default_rng(0).random(n) * args.max_weight).astype(np.float32)
    keys = boost.row_keys(actions['game_id'].to_numpy(), actions['action_id'].to_numpy(), ab.device) \
        if args.subsample != 1.0 else None
    jsons = {}
    for col in ('scores', 'concedes'):
        clf = boost.make_classifier(tp, **stop)
        clf._events = []
        t0 = time.perf_counter()
        clf.fit_binned(data, getattr(lb, col), rows, val_rows, weight, keys)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per = {f: [a.elapsed_time(b) for fam, a, b in clf._events if fam == f] for f in FAMILIES}
        entry = {'instrumented_fit_wall_ms': round(wall, 1),
                 'sum_ms': {f: round(sum(v), 2) for f, v in per.items()},
                 'launches': {f: len(v) for f, v in per.items()},
                 'median_launch_ms': {f: round(statistics.median(v), 4) for f, v in per.items() if v}}
        for f, nbytes in bytes_level.items():
            ms = statistics.median(per[f])
            entry.setdefault('median_GBs', {})[f] = round(nbytes / ms * 1e-6, 1)
            entry.setdefault('fraction_of_hbm_rate', {})[f] = round(nbytes / ms * 1e3 / HBM_BYTES_PER_S, 4)
        # LDS integer atomics a level issues for the numeric bins (two per feature and row), per second
        entry['lds_atomics_per_s'] = {
            'hist_bins': round(2 * f_num * n / (statistics.median(per['hist_bins']) * 1e-3), 0)}
        if val_rows is not None:  # what the evaluation adds to a round, against a round's training
            ran = max(clf.n_rounds_run_, 1)
            entry['rounds_run'] = clf.n_rounds_run_
            entry['best_iteration'] = clf.best_iteration
            entry['best_score'] = clf.best_score
            entry['table_reads_during_fit'] = clf.n_polls_
            entry['eval_ms_per_round'] = round(sum(sum(per[f]) for f in EVAL_FAMILIES) / ran, 4)
            entry['train_ms_per_round'] = round(sum(sum(per[f]) for f in FAMILIES if f not in EVAL_FAMILIES) / ran, 4)
        clf._events = None
        jsons[col] = json.dumps(clf.to_xgboost_json())
        entry['split_nodes'] = int((clf.trees_['feature'] >= 0).sum())
        res[col] = entry
        print(col, json.dumps(entry), flush=True)
    # ---- the call a user makes
    walls = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        np.random.seed(SPLIT_SEED)
        m = VAEP().fit_batch(games, actions, val_size=args.val_size, tree_params=tp, sample_weight=weight, **stop)
        torch.cuda.synchronize()
        walls.append(round((time.perf_counter() - t0) * 1e3, 1))
    res['fit_batch_wall_ms'] = walls
    res['fit_batch_wall_ms_median'] = statistics.median(walls)
    res['run_to_run_equal'] = all(json.dumps(m._VAEP__models[c].to_xgboost_json()) == jsons[c] for c in jsons)
    if args.val_size > 0:
        res['held_out_scores'] = {c: {k: v[k] for k in ('log_loss', 'log_loss_baseline', 'auroc', 'n', 'n_pos')}
                                  for c, v in m.device_eval_.items()}
        res['trees_kept'] = {c: len(m._VAEP__models[c].trees_) for c in jsons}
    res['train_scores'] = {c: {k: v[k] for k in ('log_loss', 'log_loss_baseline', 'auroc')}
                           for c, v in m.score_batch(games, actions).items()}
    line = json.dumps(res)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    if args.sklearn:  # the reference point: the rows copied out, one label, the host's CPUs
        from sklearn.ensemble import HistGradientBoostingClassifier
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X = ops.features(ab, known, 3).to_frame()
        y = lb.scores[:n].cpu().numpy()
        t1 = time.perf_counter()
        sk = HistGradientBoostingClassifier(max_iter=100, max_depth=3, learning_rate=0.3, l2_regularization=1.0,
                                            max_leaf_nodes=None, min_samples_leaf=1, early_stopping=False)
        sk.fit(X, y)
        t2 = time.perf_counter()
        res['sklearn_one_label'] = {'copy_out_ms': round((t1 - t0) * 1e3, 1), 'fit_ms': round((t2 - t1) * 1e3, 1),
                                    'cpus': int(os.environ.get('OMP_NUM_THREADS', 0)) or None}
        line = json.dumps(res)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
    print(line)
    if not res['run_to_run_equal']:
        raise SystemExit(3)


if __name__ == '__main__':
    main()
