"""The expected-goals fit on the synthetic batch of `--games` games (the set of
profiles/boost_fit.json), compact against masked.

Compact (this commit): the shot rows gathered by ``ops.select_rows`` into a table of their own,
binned and fitted with no row mask.  Masked (this commit and its parent alike: the call exists
in both, so ``--package-root`` can point at a checkout of the parent): ``bin_blocks(fb,
rows=shots)`` and ``fit_binned(data, y, rows=shots)`` on the full table, whose histogram kernels
stream every action at every level.  Both fit the notebook's transformers at k = 2 with
XGBClassifier()'s shape (100 trees, depth 6) on every column of the plan, so the two are the same
model; the compact fit on the model's 46 columns is timed as well.

Per figure: `--warmup` untimed calls, then `--reps` timed ones; times are HIP event pairs on the
stream (select_rows) or a host clock around work that ends in a device synchronise (fits);
medians and the spread are recorded, and from one instrumented fit per path (an event pair around
every launch) the sum per kernel family.  select_rows' bytes are held against the algorithmic
bytes: per selected row the row's bytes out and as many in, plus the 8-byte row number.

    python scripts/xg_time.py [--games 1000] [--reps 5] [--warmup 2] [--package-root DIR]
        [--masked-only] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--games', type=int, default=1000)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--warmup', type=int, default=2)
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap.add_argument('--package-root', default=HERE)
ap.add_argument('--masked-only', action='store_true')
ap.add_argument('--out', default='')
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

import torch  # noqa: E402

from socceraction_amd import batch as B, boost, ops, synthetic  # noqa: E402

XFNS = ['actiontype_onehot', 'bodypart_onehot', 'startlocation', 'movement', 'space_delta', 'startpolar', 'team']
K = 2
PARAMS = dict(n_estimators=100, max_depth=6, learning_rate=0.3)
SHOT_TYPES, SUCCESS = (11, 12, 13), 1


def timed(work, events: bool):
    """Median, spread and every value (ms) of `--reps` calls of ``work`` after `--warmup` untimed ones."""
    out, res = [], None
    for rep in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        if events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = work()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
        else:
            t0 = time.perf_counter()
            res = work()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        if rep >= args.warmup:
            out.append(round(ms, 4))
    return {'ms': out, 'median_ms': statistics.median(out), 'spread_ms': round(max(out) - min(out), 4)}, res


def families(data, y, rows) -> dict:
    """One instrumented fit (an event pair around every launch): the sum per kernel family and the launches."""
    c = boost.DeviceGBTClassifier(**PARAMS)
    c._events = []
    c.fit_binned(data, y, rows=rows)
    torch.cuda.synchronize()
    sums, launches = {}, {}
    for fam, a, b in c._events:
        sums[fam] = sums.get(fam, 0.0) + a.elapsed_time(b)
        launches[fam] = launches.get(fam, 0) + 1
    return {'sum_ms': {f: round(v, 3) for f, v in sums.items()}, 'launches': launches,
            'kernel_sum_ms': round(sum(sums.values()), 3)}


def main() -> None:
    assert torch.cuda.is_available(), 'xg_time.py measures on a ROCm GPU'
    d = synthetic.spadl_games(args.games, seed=2)
    actions, games = synthetic.to_frame(d), synthetic.games_frame(d)
    ab = B.ActionBatch.from_frame(actions, home_team_id=games.set_index('game_id')['home_team_id'], segments='game')
    n = ab.n
    fb = ops.features(ab, XFNS, K, bool_bits=True)
    t = ab.cols['type_id'][:n]
    rows = torch.nonzero((t == 11) | (t == 12) | (t == 13)).reshape(-1)
    m = int(rows.numel())
    y_full = (ab.cols['result_id'][:n] == SUCCESS).to(torch.uint8).contiguous()
    y = y_full[rows].contiguous()
    plan = fb.plan
    res = {'device': torch.cuda.get_device_name(0), 'package': 'this checkout' if args.package_root == HERE else
           'another checkout (--package-root)',
           'games': args.games, 'rows': n, 'shots': m, 'shot_share': round(m / n, 5), 'goals': int(y.sum()),
           'reps': args.reps, 'warmup': args.warmup, 'params': PARAMS, 'xfns': XFNS, 'nb_prev_actions': K,
           'n_bool': plan.n_bool, 'n_f64': plan.n_f64, 'n_i64': plan.n_i64}
    clf = lambda: boost.DeviceGBTClassifier(**PARAMS)  # noqa: E731
    # ---- masked: the full table, the shots as a row mask (every column of the plan)
    res['masked_bin'], data = timed(lambda: boost.bin_blocks(fb, rows=rows), events=False)
    res['masked_fit'], masked = timed(lambda: clf().fit_binned(data, y_full, rows=rows), events=False)
    model = json.dumps(masked.to_xgboost_json())
    res['masked_fit']['instrumented'] = families(data, y_full, rows)
    res['masked_fit']['split_nodes'] = int(((masked.trees_['feature'] >= 0) & (masked.trees_['exists'] != 0)).sum())
    if not args.masked_only:
        # ---- compact: select_rows, then the same fit on the gathered table
        res['select_rows'], compact = timed(lambda: ops.select_rows(fb, rows), events=True)
        row_bytes = 8 * (plan.n_f64 + plan.n_i64) + plan.n_bool / 8
        algo = m * (2 * row_bytes + 8)
        res['select_rows'].update(
            row_bytes=row_bytes, algorithmic_bytes=int(algo),
            algorithmic_GBs=round(algo / res['select_rows']['median_ms'] * 1e-6, 2),
            source_table_bytes=int(n * row_bytes))
        res['compact_bin_all_columns'], cdata = timed(lambda: boost.bin_blocks(compact), events=False)
        res['compact_fit_all_columns'], cfit = timed(lambda: clf().fit_binned(cdata, y), events=False)
        res['compact_equals_masked'] = json.dumps(cfit.to_xgboost_json()) == model
        res['compact_fit_all_columns']['instrumented'] = families(cdata, y, None)
        from socceraction_amd import xg
        names = xg.feature_names()
        res['model_columns'] = len(names)
        res['compact_bin_model_columns'], xdata = timed(lambda: boost.bin_blocks(compact, columns=names), events=False)
        res['compact_fit_model_columns'], _ = timed(lambda: clf().fit_binned(xdata, y), events=False)
        res['fit_batch_wall'], _ = timed(lambda: xg.ExpectedGoals().fit_batch(games, actions), events=False)
        res['masked_over_compact_fit'] = round(res['masked_fit']['median_ms']
                                               / res['compact_fit_all_columns']['median_ms'], 3)
    line = json.dumps(res)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
