"""The expected-goals logistic fit on the synthetic batch of `--games` games (the set of
profiles/xg_fit.json), and one moments launch on a large table.

Timed: ``ExpectedGoals.fit_batch(learner='logistic')`` as a whole (host clock around work that
ends in a device synchronise); the fit on the ready compact shot table, from which the time per
Newton iteration; every native ``sa_logit_moments`` call of one instrumented fit (HIP event pairs
through ``linear.LAUNCH_EVENTS``: its two memsets and two kernels, no upload and no allocation);
and sklearn's ``LogisticRegression(solver='newton-cholesky')`` on the same shot frame on the
host as the reference time.  `--warmup` untimed rounds, then `--reps` timed ones; every value,
the median, the min and the max are recorded.

The large launches: `--big-rows` rows (the batch's rows repeated through ``ops.select_rows``) over
VAEP's default columns (its transformers at k = 3: 568 columns) at a fixed-seed coefficient vector,
and over the xG model's 46 columns at the fit's coefficients; timed with HIP events, and their
algorithmic bytes -- per row the bytes of the model's columns, the label byte and the 32-byte row
record written once and read once; the 3 T limb sums are noise -- over the time.

    python scripts/logit_time.py [--games 1000] [--reps 3] [--warmup 1] [--big-rows 16000000] [--out FILE]
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
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--warmup', type=int, default=1)
ap.add_argument('--big-rows', type=int, default=16_000_000)
ap.add_argument('--hbm-GBs', type=float, default=8000.0, help='the peak the large launch is held against')
ap.add_argument('--out', default='')
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from socceraction_amd import linear, ops, synthetic, xg  # noqa: E402


def timed(work, events: bool = False):
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
    return {'ms': out, 'median_ms': statistics.median(out), 'min_ms': min(out), 'max_ms': max(out)}, res


def main() -> None:
    assert torch.cuda.is_available(), 'logit_time.py measures on a ROCm GPU'
    d = synthetic.spadl_games(args.games, seed=2)
    actions, games = synthetic.to_frame(d), synthetic.games_frame(d)
    names = xg.feature_names()
    res = {'device': torch.cuda.get_device_name(0), 'games': args.games, 'rows': len(actions), 'reps': args.reps,
           'warmup': args.warmup, 'model_columns': len(names), 'items': linear.n_items(len(names)),
           'item_splits': linear.item_splits(len(names))}
    res['fit_batch_wall'], model = timed(lambda: xg.ExpectedGoals().fit_batch(games, actions, learner='logistic'))
    clf = model.model_
    res['n_iter'] = int(clf.n_iter_[0])
    # the fit on the ready compact table
    ab = xg._game_batch(games, actions)
    rows, compact = xg._shot_blocks(ab, xg._known_xfns(xg.XFNS), xg.NB_PREV_ACTIONS)
    y = xg.shot_labels(ab, rows)
    res['shots'], res['goals'] = int(rows.numel()), int(y.sum())
    res['fit_blocks'], again = timed(lambda: linear.DeviceLogisticRegression().fit_blocks(compact, y, columns=names))
    res['same_coefficients'] = again.coef_.tobytes() == clf.coef_.tobytes()
    linear.LAUNCH_EVENTS = []
    linear.DeviceLogisticRegression().fit_blocks(compact, y, columns=names)
    torch.cuda.synchronize()
    launches = [a.elapsed_time(b) for a, b in linear.LAUNCH_EVENTS]
    linear.LAUNCH_EVENTS = None
    res['moments_calls'] = {'count': len(launches), 'ms': [round(v, 4) for v in launches],
                            'median_ms': statistics.median(launches), 'min_ms': min(launches),
                            'max_ms': max(launches), 'sum_ms': round(sum(launches), 4),
                            'what': 'the native sa_logit_moments call: two memsets, the row kernel, the pair kernel'}
    res['ms_per_iteration'] = round(res['fit_blocks']['median_ms'] / len(launches), 4)
    # sklearn on the same shot frame (host)
    from sklearn.linear_model import LogisticRegression
    frame = compact.to_frame()[names]
    yh = y.cpu().numpy()
    res['sklearn_newton_cholesky'], ref = timed(lambda: LogisticRegression(solver='newton-cholesky', tol=1e-12,
                                                                            max_iter=1000).fit(frame, yh))
    res['sklearn_newton_cholesky']['n_iter'] = int(ref.n_iter_[0])
    res['max_abs_p_minus_sklearn'] = float(np.abs(clf.predict_proba(frame)[:, 1] - ref.predict_proba(frame)[:, 1]).max())
    # one launch on a large table: VAEP's default columns, then the xG model's
    if args.big_rows > 0:
        from socceraction_amd.vaep.base import xfns_default
        pick = torch.arange(args.big_rows, device=ab.device) % ab.n
        yb = (ab.cols['result_id'][:ab.n][pick] == xg.SUCCESS).to(torch.uint8).contiguous()
        for key, known, k, cols in (('big_launch_vaep_columns', xg._known_xfns(xfns_default), 3, None),
                                    ('big_launch_xg_columns', xg._known_xfns(xg.XFNS), xg.NB_PREV_ACTIONS, names)):
            big = ops.select_rows(ops.features(ab, known, k, bool_bits=True), pick)
            _, kc = linear.model_slots(big, cols)
            col_exp = linear.column_exps(big, kc)
            if cols is None:
                rng = np.random.default_rng(0)
                beta = rng.normal(size=len(kc) + 1) * 0.05 / np.append(2.0 ** np.array(col_exp[:-1]), 1.0)
            else:
                beta = np.append(clf.coef_[0], clf.intercept_[0])
            le = linear.loss_exponent(beta, col_exp)
            res[key], out = timed(lambda: linear.moments_limbs(big, kc, beta, yb, None, col_exp, le), events=True)
            assert int(out[1].item()) == 0
            row_bytes = sum(0.125 if kd == 'b' else 8 for kd, _ in kc) + 1 + 64
            algo = args.big_rows * row_bytes
            gbs = algo / res[key]['median_ms'] * 1e-6
            res[key].update(rows=args.big_rows, columns=len(kc), bool_columns=sum(kd == 'b' for kd, _ in kc),
                            row_bytes=row_bytes, algorithmic_bytes=int(algo), algorithmic_GBs=round(gbs, 2),
                            hbm_peak_GBs=args.hbm_GBs, fraction_of_hbm_peak=round(gbs / args.hbm_GBs, 5),
                            items=linear.n_items(len(kc)), item_grid=list(linear.item_grid(len(kc))),
                            candidate_terms_per_s=round(args.big_rows * linear.n_items(len(kc))
                                                        / res[key]['median_ms'] * 1e3, 0))
            del big, out
    line = json.dumps(res)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
