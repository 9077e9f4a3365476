"""The binary scores of one label column of the cfg2 batch (15,992,198 rows): Brier score, log
loss and exact AUROC on the device (metrics.binary_scores: sa_metric_sums, sa_auc_keys,
torch.sort of the minority keys, sa_auc_count) for float32 and float64 probabilities at positive
rates 0.2 % (`concedes`), 1.2 % (`scores`) and 50 % (the worst case of the minority sort), against
two alternatives on the same tensors: torch.sort of every row plus a cumulative sum (the usual
on-device AUROC), and scikit-learn on the host after a copy back (what VAEP.score does).

Per form: each kernel alone (one HIP event pair per launch through the bare C ABI, warmed up,
the best of `reps`), the whole binary_scores call as a user makes it (host clock; the call ends in
its own copy back), the sort-everything alternative (event pair), and scikit-learn (host clock,
copy back included, one run).  Each streaming pass is also held against its byte floor:
sizeof(p) + 1 bytes per row.  Results are compared before anything is timed.

    python scripts/score_time.py [--rows 15992198] [--reps 10] [--out FILE] [--no-sklearn]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from socceraction_amd import _native, batch as B, metrics, ops  # noqa: E402

HBM_BYTES_PER_S = 8e12


def event_ms(fn, reps: int, before=None):
    """Per-launch HIP event timings of fn(), `before()` outside the pair."""
    fn()
    out = []
    for _ in range(reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(round(e0.elapsed_time(e1), 4))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=15992198)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default='')
    ap.add_argument('--no-sklearn', action='store_true')
    args = ap.parse_args()
    dev = B.device()
    n = args.rows
    lib = _native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    res = {'rows': n, 'reps': args.reps, 'hbm_bytes_per_s_for_floors': HBM_BYTES_PER_S, 'forms': {}}
    for rate in (0.002, 0.012, 0.5):
        rng = np.random.default_rng([11, int(rate * 1000)])
        y_host = (rng.random(n) < rate).astype(np.uint8)
        p64 = np.clip(0.15 * y_host + rng.beta(0.6, 12.0, n), 0.0, 1.0)
        for f32 in (True, False):
            name = f"{'f32' if f32 else 'f64'}_rate_{rate}"
            p_host = p64.astype(np.float32) if f32 else p64
            y, p = torch.from_numpy(y_host).to(dev), torch.from_numpy(p_host).to(dev)
            width = 4 if f32 else 8
            floor_ms = (width + 1) * n / HBM_BYTES_PER_S * 1e3
            # ---- the results, before any timing
            first = metrics.binary_scores(y, p)
            again = metrics.binary_scores(y, p)
            n_pos = first['n_pos']
            minority = int(n_pos <= n - n_pos)
            m = n_pos if minority else n - n_pos
            entry = {'n_pos': n_pos, 'minority_rows': m, 'scores': first,
                     'run_to_run_equal': first == again,
                     'byte_floor_ms_sums_pass': round(floor_ms, 4), 'byte_floor_ms_count_pass': round(floor_ms, 4),
                     'bytes_per_row_streaming_pass': width + 1}
            # ---- each kernel alone
            acc = ops.BinaryMetrics(torch.zeros(10, dtype=torch.int64, device=dev))
            keys = torch.empty(m, dtype=torch.int32 if f32 else torch.int64, device=dev)
            cursor = torch.zeros(1, dtype=torch.int64, device=dev)

            def sums():
                _native.check(lib.sa_metric_sums(y.data_ptr(), p.data_ptr(), int(f32), n, acc.count.data_ptr(),
                                                 acc.limbs.data_ptr(), acc.err.data_ptr(), stream))

            def compact():
                _native.check(lib.sa_auc_keys(y.data_ptr(), p.data_ptr(), int(f32), n, minority, keys.data_ptr(), m,
                                              cursor.data_ptr(), stream))

            kernel = {'sa_metric_sums': event_ms(sums, args.reps, before=lambda: acc.buf.zero_()),
                      'sa_auc_keys': event_ms(compact, args.reps, before=lambda: cursor.zero_())}
            assert int(cursor.item()) == m
            sorted_keys = torch.sort(keys).values
            kernel['torch_sort_minority_keys'] = event_ms(lambda: torch.sort(keys), args.reps)

            def count():
                _native.check(lib.sa_auc_count(y.data_ptr(), p.data_ptr(), int(f32), n, sorted_keys.data_ptr(), m,
                                               minority, acc.u2.data_ptr(), stream))

            kernel['sa_auc_count'] = event_ms(count, args.reps, before=lambda: acc.buf.zero_())
            entry['kernel_ms'] = kernel
            best = {k: min(v) for k, v in kernel.items()}
            entry['best_kernel_ms'] = best
            entry['fraction_of_byte_floor'] = {k: round(floor_ms / best[k], 4)
                                               for k in ('sa_metric_sums', 'sa_auc_keys', 'sa_auc_count')}
            entry['GBs_streamed'] = {k: round((width + 1) * n / best[k] * 1e-6, 1)
                                     for k in ('sa_metric_sums', 'sa_auc_keys', 'sa_auc_count')}
            # ---- the whole call
            whole = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                metrics.binary_scores(y, p)
                whole.append(round((time.perf_counter() - t0) * 1e3, 4))
            entry['binary_scores_ms'] = whole
            entry['best_binary_scores_ms'] = min(whole)

            # ---- sort every row + cumulative sum (ties broken arbitrarily: a timing alternative)
            def sort_all():
                order = torch.argsort(p)
                ys = y[order].to(torch.int64)
                below = torch.cumsum(1 - ys, 0)  # negatives at or before each row
                return (ys * below).sum()

            u = int(sort_all().item())
            entry['sort_all_auroc'] = u / (n_pos * (n - n_pos))
            entry['sort_all_ms'] = event_ms(sort_all, max(3, args.reps // 2))
            entry['best_sort_all_ms'] = min(entry['sort_all_ms'])
            # ---- scikit-learn on the host after a copy back
            if not args.no_sklearn:
                from sklearn.metrics import brier_score_loss, log_loss, roc_auc_score
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                yh, ph = y.cpu().numpy(), p.cpu().numpy()
                t1 = time.perf_counter()
                sk = {'brier': float(brier_score_loss(yh, ph)), 'log_loss': float(log_loss(yh, ph)),
                      'auroc': float(roc_auc_score(yh, ph))}
                t2 = time.perf_counter()
                entry['sklearn_ms'] = {'copy_back': round((t1 - t0) * 1e3, 2), 'metrics': round((t2 - t1) * 1e3, 2)}
                entry['sklearn_scores'] = sk
                entry['abs_diff_vs_sklearn'] = {k: abs(first[k] - sk[k]) for k in sk}
            res['forms'][name] = entry
            print(name, json.dumps({k: entry[k] for k in ('best_kernel_ms', 'best_binary_scores_ms',
                                                          'best_sort_all_ms', 'fraction_of_byte_floor')}),
                  flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    if not all(e['run_to_run_equal'] for e in res['forms'].values()):
        raise SystemExit(3)


if __name__ == '__main__':
    main()
