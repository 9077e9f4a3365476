"""The rating table of the cfg2 batch (10k synthetic games, ~16M actions, V = 3 value columns,
synthetic player ids): the order-independent grouped sums (sa_group_sums + sa_group_finalize,
zeroing the table included) against torch.index_add_ on float64 over the same tensors, the
non-reproducible alternative.  Also three key patterns that price the LDS same-address adds of
the kernel: 256 keys dealt round-robin (no two lanes of a wave share a slot), 22 random keys (a
game's players) and one key (every lane on one slot).

HIP events around `reps` calls, warmed up, rounds interleaved; tables compared before timing.
Two figures per form: `ms`, the whole call as a user makes it (table zeroing + sums + finalise
through the Python layer; `host_enqueue_ms` is the host's time to enqueue one such call, and a
call cannot be faster than that), and `kernel_ms`, group_sums_kernel alone: `kreps` back-to-back
sa_group_sums launches through the bare C ABI into an already zeroed table, the queue kept full.

    python scripts/group_sums_time.py [--games 10000] [--reps 10] [--out FILE]
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

from socceraction_amd import _native, batch as B, ops, synthetic  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--kreps', type=int, default=20, help='launches per kernel-only window (kreps * actions < 2**30)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = B.device()
    d = synthetic.spadl_games(args.games)
    n = int(d['game_off'][-1])
    player = (d['team_id'] * 100 + d['pos'] % 11).astype(np.int64)  # synthetic.to_frame's ids
    uniq, codes = np.unique(player, return_inverse=True)
    G = len(uniq)
    p, q = synthetic.probabilities(n, seed=3), synthetic.probabilities(n, seed=4)
    off, de = p['scores'] - q['scores'], q['concedes'] - p['concedes']
    host = np.stack([off, de, off + de])
    vals = torch.from_numpy(host).to(dev)
    cols = list(vals)
    E = (2, 2, 2)
    rng = np.random.default_rng(1)
    keysets = {'players': (codes.astype(np.int32), G),
               'spread256': ((np.arange(n) % 256).astype(np.int32), 256),
               'random22': (rng.integers(0, 22, n).astype(np.int32), 22),
               'same1': (np.zeros(n, np.int32), 1)}
    dk = {k: (torch.from_numpy(v).to(dev), g) for k, (v, g) in keysets.items()}
    accs = {k: ops.group_sums_zero(g, 3, E, dev) for k, (_, g) in dk.items()}

    def fixed(name):
        k, g = dk[name]
        acc = accs[name].zero_()
        ops.group_sums(k, cols, g, scale_exp=E, acc=acc)
        return acc.finalize()

    k64 = dk['players'][0].to(torch.int64)
    ia_out = torch.empty((3, G), dtype=torch.float64, device=dev)

    def index_add():
        ia_out.zero_()
        for c in range(3):
            ia_out[c].index_add_(0, k64, cols[c])
        return ia_out

    forms = {'group_sums_' + k: (lambda k=k: fixed(k)) for k in dk}
    forms['index_add_f64'] = index_add
    # the tables before any timing: run to run, and against a float64 bincount on the host
    a = fixed('players').clone()
    b = fixed('players').clone()
    accs['players'].check_errors()
    i0 = index_add().clone()
    i1 = index_add().clone()
    ref = np.stack([np.bincount(codes, weights=host[c], minlength=G) for c in range(3)])
    checks = {'group_sums_run_to_run_equal': bool(torch.equal(a, b)),
              'index_add_run_to_run_equal': bool(torch.equal(i0, i1)),
              'group_sums_max_abs_diff_vs_bincount': float(np.abs(a.cpu().numpy() - ref).max()),
              'index_add_max_abs_diff_vs_bincount': float(np.abs(i0.cpu().numpy() - ref).max())}
    # the kernel alone: the bare C-ABI call, arguments built once
    import ctypes
    lib = _native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = (ctypes.c_void_p * 3)(*[c.data_ptr() for c in cols])
    exps = (ctypes.c_int32 * 3)(*E)
    if args.kreps * n >= ops.GROUP_MAX_ROWS:
        raise SystemExit('kreps * actions must stay below 2**30 rows per table')

    def launch(name):
        k, g = dk[name]
        acc = accs[name]
        _native.check(lib.sa_group_sums(k.data_ptr(), ptrs, 3, 0, n, g, exps, acc.limbs.data_ptr(),
                                        acc.count.data_ptr(), acc.err.data_ptr(), stream))

    ms = {k: [] for k in forms}
    enq = {k: [] for k in forms}
    kms = {k: [] for k in dk}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(round(e0.elapsed_time(e1) / args.reps, 4))
            enq[k].append(round((t1 - t0) * 1e3 / args.reps, 4))
        for k in dk:
            accs[k].zero_()
            launch(k)
            accs[k].zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.kreps):
                launch(k)
            e1.record()
            torch.cuda.synchronize()
            kms[k].append(round(e0.elapsed_time(e1) / args.kreps, 4))
    best = {k: min(v) for k, v in ms.items()}
    kbest = {k: min(v) for k, v in kms.items()}
    floor_us = 28 * n / 8e12 * 1e6  # 4 B key + 3 x 8 B values per action at 8 TB/s
    res = {'actions': n, 'groups': G, 'value_columns': 3, 'scale_exp': list(E), 'checks': checks, 'ms': ms,
           'best_ms': best, 'host_enqueue_ms': {k: min(v) for k, v in enq.items()},
           'kernel_ms': kms, 'best_kernel_ms': kbest,
           'kernel_fraction_of_floor': {k: round(floor_us * 1e-3 / v, 4) for k, v in kbest.items()},
           'kernel_GBs_28B': {k: round(28 * n / v * 1e-6, 1) for k, v in kbest.items()},
           'bytes_per_action': 28, 'floor_us_at_8TBs': round(floor_us, 1),
           'fraction_of_floor': {k: round(floor_us * 1e-3 / v, 4) for k, v in best.items()},
           'GBs_28B': {k: round(28 * n / v * 1e-6, 1) for k, v in best.items()},
           'lds_slots': _native.SA_GROUP_LDS_SLOTS}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    if not checks['group_sums_run_to_run_equal']:
        raise SystemExit(3)


if __name__ == '__main__':
    main()
