"""The ten most valuable actions of a selection (the last cell of the reference's notebook 4) at
`--games` synthetic games (1000: ~1.6M actions, 10000: ~16M): VAEP.top_actions(k=10), which
keeps the [3, n] values in HBM and selects with ops.top_rows, against the path the package had
before it: rate_batch (every value copied back) and a pandas sort_values(...).head(10).  Both in
one process, alternating, host clock around calls that end in their own copy back; results are
compared before anything is timed.

Below the model: ops.top_rows on the vaep row of the same [3, ld] tensor with the same mask, as a
whole call and launch by launch through the bare C ABI (one HIP event pair per launch, the best
and the median of `reps`), every row pass held against its bytes: sizeof(value) + 1 mask byte
per row at HBM_BYTES_PER_S.  With `--hist-lib TAG=FILE` (repeatable; a build with another
-DSA_TOP_AGG_ROUNDS: the number of wave-aggregated adds per row slot before the per-lane LDS
atomics) the same launches are timed with that library's sa_top_hist.

    python -m socceraction_amd.build -DSA_TOP_AGG_ROUNDS=8 --variant=top_agg8
    python scripts/top_rows_time.py [--games 10000] [--reps 10] [--rounds 3] [--out FILE]
                                    [--hist-lib agg8=socceraction_amd/_lib/libsocceraction_amd_top_agg8.so]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from socceraction_amd import _native, batch as B, ops, ratings, synthetic  # noqa: E402
import socceraction_amd.vaep as vaep  # noqa: E402
from socceraction_amd.spadl.config import actiontypes  # noqa: E402

HBM_BYTES_PER_S = 8e12
K = 10


def fitted_model(seed: int = 21):
    """VAEP with two small HistGradientBoosting models (float64 probabilities: the [3, n] float64
    values of the notebook), fitted on six synthetic games."""
    from sklearn.ensemble import HistGradientBoostingClassifier
    d = synthetic.spadl_games(6, seed=seed)
    actions, games = synthetic.to_frame(d), synthetic.games_frame(d)
    model = vaep.VAEP()
    X = model.compute_features_batch(games, actions)
    Y = model.compute_labels_batch(games, actions)
    model._VAEP__models = {c: HistGradientBoostingClassifier(max_iter=20, max_depth=3, random_state=0).fit(X, Y[c])
                           for c in ('scores', 'concedes')}
    assert model._device_models() is not None
    return model


def launches(lib, v, keep, k, largest, hist_lib=None):
    """One selection through the C ABI, every launch between its own event pair: [(name, ms)]
    and the rows.  hist_lib: the library whose sa_top_hist is used (the same device buffers)."""
    n, f32 = int(v.numel()), int(v.dtype == torch.float32)
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(_native.SA_TOP_STATE_WORDS + (1 << _native.SA_TOP_DIGIT_BITS) // 2, dtype=torch.int64,
                      device=v.device)
    state, hist = buf[:_native.SA_TOP_STATE_WORDS], buf[_native.SA_TOP_STATE_WORDS:]
    n_chunks = (n + _native.SA_TOP_CHUNK_ROWS - 1) // _native.SA_TOP_CHUNK_ROWS
    ties = torch.empty(n_chunks, dtype=torch.int32, device=v.device)
    rows = torch.empty(k, dtype=torch.int64, device=v.device)
    kp = keep.data_ptr() if keep is not None else None
    pairs = []

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        pairs.append((name, e0, e1))
        return out

    hl = hist_lib or lib
    for p in range(lib.sa_top_passes(f32)):
        timed(f'sa_top_hist[{p}]', lambda: _native.check(hl.sa_top_hist(
            v.data_ptr(), f32, kp, n, int(largest), p, state.data_ptr(), hist.data_ptr(), st)))
        timed(f'sa_top_pick[{p}]', lambda: _native.check(lib.sa_top_pick(f32, k, p, state.data_ptr(), hist.data_ptr(),
                                                                         st)))
    timed('sa_top_tie_count', lambda: _native.check(lib.sa_top_tie_count(
        v.data_ptr(), f32, kp, n, int(largest), state.data_ptr(), ties.data_ptr(), st)))
    base = timed('torch_cumsum_chunk_ties', lambda: torch.cumsum(ties, 0, dtype=torch.int64) - ties)
    timed('sa_top_collect', lambda: _native.check(lib.sa_top_collect(
        v.data_ptr(), f32, kp, n, int(largest), k, state.data_ptr(), base.data_ptr(), rows.data_ptr(), st)))
    torch.cuda.synchronize()
    m = int(state[6].item())
    return [(name, e0.elapsed_time(e1)) for name, e0, e1 in pairs], torch.sort(rows[:m]).values


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--hist-lib', action='append', default=[], metavar='TAG=FILE')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = B.device()
    lib = _native.lib()
    model = fitted_model()
    d = synthetic.spadl_games(args.games)
    actions, games = synthetic.to_frame(d), synthetic.games_frame(d)
    n = len(actions)
    names = pd.Series(np.asarray(actiontypes)[actions.type_id.to_numpy()], index=actions.index)
    where = (actions.team_id % 2 == 0) & ~names.str.contains('shot')  # half of the teams, no shot types
    res = {'games': args.games, 'actions': n, 'k': K, 'selected_fraction': round(float(where.mean()), 4),
           'reps': args.reps, 'rounds': args.rounds, 'hbm_bytes_per_s_for_fractions': HBM_BYTES_PER_S}

    # ---- the model methods: results first, then alternating timed runs
    def parent_path():
        A = pd.concat([actions, model.rate_batch(games, actions)], axis=1)
        A = A.sort_values('vaep_value', ascending=False, kind='stable')
        return A[where.loc[A.index]].dropna(subset=['vaep_value']).head(K)  # the notebook: sort, then filter

    def device_path():
        return model.top_actions(games, actions, k=K, where=where)

    want, got = parent_path(), device_path()
    pd.testing.assert_frame_equal(got, want)
    res['frames_equal'] = True
    t = {'rate_batch_then_sort_values': [], 'VAEP.top_actions': []}
    for _ in range(args.rounds):
        for name, fn in (('rate_batch_then_sort_values', parent_path), ('VAEP.top_actions', device_path)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[name].append(round((time.perf_counter() - t0) * 1e3, 2))
    res['model_ms'] = t
    res['model_ms_median'] = {k: statistics.median(v) for k, v in t.items()}
    # what follows the shared part (the encode of the frame and the feature / tree / formula
    # launches, the same in both): the copy back of [3, n] and the host sort, against the select
    v3 = model._values_batch(games, actions)
    torch.cuda.synchronize()
    tail = {'copy_back_then_sort_values': [], 'mask_upload_top_rows_gather': []}
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = v3.cpu().numpy()[:, :n]
        A = pd.concat([actions, pd.DataFrame({'offensive_value': h[0], 'defensive_value': h[1],
                                              'vaep_value': h[2]})], axis=1)
        A = A.sort_values('vaep_value', ascending=False, kind='stable')
        A[where.loc[A.index]].dropna(subset=['vaep_value']).head(K)
        tail['copy_back_then_sort_values'].append(round((time.perf_counter() - t0) * 1e3, 2))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = ratings.mask_tensor(where, n, dev, actions.index)
        rows, _ = ops.top_rows(v3[2, :n], K, keep)
        sel = v3[:, rows].cpu().numpy()
        out = actions.iloc[rows.cpu().numpy()].copy()
        out['vaep_value'] = sel[2]
        tail['mask_upload_top_rows_gather'].append(round((time.perf_counter() - t0) * 1e3, 2))
    res['after_the_values_ms'] = tail
    res['after_the_values_ms_median'] = {k: statistics.median(v) for k, v in tail.items()}

    # ---- ops.top_rows on the same column: the whole call, then launch by launch
    hist_libs = [('', None)] + [('_' + a.split('=', 1)[0], _native.load_library(os.path.abspath(a.split('=', 1)[1])))
                                for a in args.hist_lib]
    res['top_rows'] = {}
    keep = ratings.mask_tensor(where, n, dev, actions.index)
    for dt in (torch.float64, torch.float32):
        for masked in (True, False):
            v = v3[2, :n].to(dt).contiguous()
            kp = keep if masked else None
            width = v.element_size()
            row_bytes = (width + (1 if masked else 0)) * n
            whole = []
            first = ops.top_rows(v, K, kp)
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = ops.top_rows(v, K, kp)
                torch.cuda.synchronize()
                whole.append(round((time.perf_counter() - t0) * 1e3, 4))
            assert torch.equal(r[0], first[0])
            entry = {'whole_call_ms': whole, 'whole_call_ms_median': statistics.median(whole),
                     'row_pass_bytes': row_bytes,
                     'row_pass_floor_ms': round(row_bytes / HBM_BYTES_PER_S * 1e3, 4)}
            for tag, hl in hist_libs:
                per = {}
                for _ in range(args.reps + 1):  # the first run warms up
                    times, rows = launches(lib, v, kp, K, True, hist_lib=hl)
                    assert torch.equal(rows, torch.sort(first[0]).values)
                    for name, ms in times:
                        per.setdefault(name, []).append(round(ms, 4))
                per = {k: v_[1:] for k, v_ in per.items()}
                entry['launch_ms_best' + tag] = {k: min(v_) for k, v_ in per.items()}
                entry['launch_ms_median' + tag] = {k: statistics.median(v_) for k, v_ in per.items()}
                entry['fraction_of_hbm_rate' + tag] = {
                    k: round(row_bytes / (min(v_) * 1e-3) / HBM_BYTES_PER_S, 4) for k, v_ in per.items()
                    if k.startswith('sa_top_hist') or k in ('sa_top_tie_count', 'sa_top_collect')}
                entry['launches_sum_ms_best' + tag] = round(sum(min(v_) for v_ in per.values()), 4)
            name = f"{'f64' if dt == torch.float64 else 'f32'}_{'masked' if masked else 'all_rows'}"
            res['top_rows'][name] = entry
            print(name, json.dumps({k: entry[k] for k in entry if k.startswith('launch_ms_best') or
                                    k == 'whole_call_ms_median'}), flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
