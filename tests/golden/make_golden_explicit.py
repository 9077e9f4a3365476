"""Golden fixtures for explicit game-state lists whose frames are NOT shifts of one another: the
*reference's* module-level transformers (``xfns_default`` of ``socceraction.vaep.base`` and of
``socceraction.atomic.vaep.base``) run on a list of k = 4 frames of 70 rows, frame 0 a synthetic
game and frame i the same rows under its own random permutation
(``tests/window_cases.permuted_frames``), once as built (``plain``) and once after the
reference's own ``play_left_to_right`` (``ltr``), through the same shims as ``make_golden.py``.
The frames each run saw are stored beside its output.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_explicit.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (imports the reference with the shims)

import socceraction.atomic.vaep.base as ref_abase  # noqa: E402
import socceraction.vaep.base as ref_base  # noqa: E402

import window_cases as wc  # noqa: E402

N, K, HOME = 70, 4, 100


def case(atomic: bool) -> None:
    cols = wc.ATOMIC_COLS if atomic else wc.SPADL_COLS
    xfns = ref_abase.xfns_default if atomic else ref_base.xfns_default
    add_names = mg.ref_aspadl.add_names if atomic else mg.ref_spadl.add_names
    ltr = mg.ref_afs.play_left_to_right if atomic else mg.ref_fs.play_left_to_right
    out = dict(k=np.array([K], np.int64), home_team_id=np.array([HOME], np.int64))
    for tag in ('plain', 'ltr'):
        frames = wc.permuted_frames(N, K, atomic)
        for f in frames:
            mg._check_spadl(f, atomic)
            assert f.index.equals(pd.RangeIndex(N))
        states = [add_names(f) for f in frames]
        if tag == 'ltr':
            states = ltr(states, HOME)
        X = pd.concat([fn(states) for fn in xfns], axis=1)
        assert len(X) == N
        for i, s in enumerate(states):
            for c in cols:
                out[f'{tag}_f{i}_{c}'] = s[c].to_numpy()
        for key, v in mg._split_features(X).items():
            out[f'{tag}_{key}'] = v
    name = 'explicit_atomic' if atomic else 'explicit_spadl'
    np.savez_compressed(os.path.join(HERE, f'{name}.npz'), **out)
    print(name, N, 'rows', K, 'frames', X.shape[1], 'columns')


if __name__ == '__main__':
    case(False)
    case(True)
