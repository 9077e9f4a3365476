"""SHA-256 of what the xT fit and rate return on a fixed synthetic season, one JSON line per
fit: small grids (register, one-workgroup and compact solves), 105 x 68 in the default,
exact_order and fused fit + rate forms, and 120 x 80 (dense solve, interpolated rate from
global memory).  Two builds that print the same lines compute the same bits.

    python scripts/xt_fit_hashes.py [--games 200]
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from socceraction_amd import batch as B  # noqa: E402
from socceraction_amd import ops, synthetic, xthreat  # noqa: E402


def _sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', type=int, default=200)
    args = ap.parse_args()
    d = synthetic.spadl_games(args.games, seed=17)
    df = synthetic.to_frame(d)
    fits = [(16, 12, False), (30, 20, False), (40, 30, False), (105, 68, False), (105, 68, True),
            (120, 80, False)]
    for l, w, exact in fits:
        m = xthreat.ExpectedThreat(l, w)
        with contextlib.redirect_stdout(io.StringIO()):  # fit prints the iteration count
            m.fit(df, exact_order=exact)
        print(json.dumps({'fit': f'{l}x{w}' + ('/exact_order' if exact else ''), 'path': m.solve_path,
                          'n_iter': len(m.heatmaps) - 1, 'surface': _sha(m.xT),
                          'heatmaps': _sha(np.stack(m.heatmaps)), 'rate': _sha(m.rate(df)),
                          'rate_interp': _sha(m.rate(df, use_interpolation=True))}), flush=True)
    ab = B.ActionBatch.from_columns(d)
    ic = [ops.xt_interp_codes_buffer(ab.n, ab.device)]
    acc = ops.xt_count_many([ab], 105, 68, interp_codes=ic, dense=False)
    sol, rates, err = ops.xt_fit_rate_interp_codes(acc, ic, [ab.n])
    assert int(err.item()) == 0
    print(json.dumps({'fit': '105x68/fused', 'path': sol.path, 'n_iter': sol.n_iter,
                      'surface': _sha(sol.mats[3].cpu().numpy()), 'heatmaps': _sha(sol.heatmaps.cpu().numpy()),
                      'rate_interp': _sha(rates[0][:ab.n].cpu().numpy())}), flush=True)


if __name__ == '__main__':
    main()
