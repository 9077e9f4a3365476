"""Golden vectors at the float64 thresholds behind discrete outputs, produced by running the
*reference* on the inputs of tests/threshold_cases.py (build container only; the reference never
travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_thresholds.py

* ``dribbles_thresholds.npz``: ``socceraction.spadl.base._add_dribbles`` on a ~500-row frame in
  which every consecutive pair sits on a distance or duration threshold (the layout of
  make_golden_dribbles.py: whole DataFrames, dtypes included);
* ``xt_edges.npz``: ``xthreat._get_cell_indexes``, ``_count`` and ``move_transition_matrix`` on
  coordinates at the cell edges +-2 ulp, outside the pitch and past the int64 range, for the
  16 x 12 and 105 x 68 grids (keys ``g<l>x<w>_...``; the transition matrix as its non-zero
  entries).  The reference raises on a non-finite move coordinate, so there is no inf or NaN;
* ``formula_samephase.npz``: ``vaep.formula.value`` (float64 and float32 probabilities) on a
  ~600-row batch whose consecutive time differences sit on the same-phase rule's 10 s, one
  segment at a time (the reference's functions see one game).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import make_golden as mg  # noqa: E402  (reference import + shims)
from make_golden_dribbles import _store  # noqa: E402

from socceraction.spadl.base import _add_dribbles  # noqa: E402

import threshold_cases as tc  # noqa: E402

SPADL_IN = mg.SPADL_IN


def dribbles() -> None:
    f = tc.dribble_frame(per_threshold=230)
    df = pd.DataFrame({c: f[c] for c in tc.DRIBBLE_COLS})
    res = _add_dribbles(df.copy())
    out = {}
    _store(out, 'in_', df)
    _store(out, 'out_', res)
    np.savez_compressed(os.path.join(HERE, 'dribbles_thresholds.npz'), **out)
    print('dribbles thresholds', len(df), '->', len(res), 'rows')


def xt_edges() -> None:
    out = {}
    for l, w in tc.GOLDEN_GRIDS:
        d = tc.binning_batch(l, w)
        df = pd.DataFrame({c: d[c] for c in SPADL_IN})
        tag = f'g{l}x{w}_'
        for c in SPADL_IN:
            out[tag + 'in_' + c] = d[c]
        for c in ('game_off', 'home_team_id'):
            out[tag + c] = d[c]
        for side in ('start', 'end'):
            xi, yj = mg.ref_xt._get_cell_indexes(df[side + '_x'], df[side + '_y'], l, w)
            out[tag + side + '_xi'] = xi.to_numpy()
            out[tag + side + '_yj'] = yj.to_numpy()
        shots = df[df.type_id == 11]
        goals = shots[shots.result_id == 1]
        moves = mg.ref_xt.get_move_actions(df)
        for name, a in (('shot', shots), ('goal', goals), ('move', moves)):
            out[tag + name] = mg.ref_xt._count(a.start_x, a.start_y, l, w).astype(np.int64)
        T = mg.ref_xt.move_transition_matrix(df, l, w)
        nz = np.flatnonzero(T)
        out[tag + 'trans_idx'] = nz.astype(np.int64)
        out[tag + 'trans_val'] = T.reshape(-1)[nz]
        print('xt edges', l, w, len(df), 'rows,', len(nz), 'transitions')
    # the inputs of the first grid in the layout every xt_* golden has (no fitted grid beside them)
    l, w = tc.GOLDEN_GRIDS[0]
    for c in SPADL_IN:
        out['in_' + c] = out[f'g{l}x{w}_in_{c}']
    np.savez_compressed(os.path.join(HERE, 'xt_edges.npz'), **out)


def formula() -> None:
    d = tc.samephase_batch(600)
    off = d['game_off']
    out = {'in_' + c: d[c] for c in SPADL_IN}
    out.update(game_off=off, home_team_id=d['home_team_id'], ps=d['ps'], pc=d['pc'])
    df = pd.DataFrame({c: d[c] for c in SPADL_IN})
    for tag, dt in (('64', np.float64), ('32', np.float32)):
        parts = []
        for s, e in zip(off[:-1], off[1:]):
            seg = mg.ref_spadl.add_names(df.iloc[s:e].reset_index(drop=True))
            parts.append(mg.ref_formula.value(seg, pd.Series(d['ps'][s:e].astype(dt)),
                                              pd.Series(d['pc'][s:e].astype(dt))))
        V = pd.concat(parts, ignore_index=True)
        for c in ('offensive_value', 'defensive_value', 'vaep_value'):
            assert V[c].dtype == dt, (c, V[c].dtype)
            out[f'{c}_{tag}'] = V[c].to_numpy()
    np.savez_compressed(os.path.join(HERE, 'formula_samephase.npz'), **out)
    print('formula same-phase', len(df), 'rows,', len(off) - 1, 'segments')


if __name__ == '__main__':
    dribbles()
    xt_edges()
    formula()
