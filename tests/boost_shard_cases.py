"""The table, shards and parameter sets the sharded-learner tests share (tests/test_boost_shard_host.py,
tests/test_gpu_boost_shard.py and the per-rank helper tests/boost_shard_rank.py): built the same in
every process from a fixed seed, so a rank takes its slice and the test the whole."""
import numpy as np
import pandas as pd

N = 3000
PARTS = (1027, 64, 1909)  # none a multiple of 2048, 1027 no multiple of 64: every part masks its bitmap tail
SHARDS = {2: (1027, 1973), 3: (1500, 0, 1500)}
N_BOOL = 70
NUM_AT = {10: 'nan', 40: 'wide', 72: 'const'}  # model positions of the numeric features among the bools

PLAIN = {'d3': dict(n_estimators=5, max_depth=3), 'd6': dict(n_estimators=2, max_depth=6)}
TUNED = dict(n_estimators=4, max_depth=3, scale_pos_weight=3.0, subsample=0.5, colsample_bytree=0.5, reg_alpha=0.1,
             random_state=11)
STOP = dict(n_estimators=30, max_depth=3, learning_rate=1.0)
STOP_ROUNDS = 2


BATCH = dict(n_estimators=4, max_depth=3)


def games_dict():
    from socceraction_amd import synthetic
    return synthetic.spadl_games(9, seed=4, mean_actions=200.0)


def games():
    """``(games, actions)``: nine small synthetic games for the public path (``VAEP.fit_batch``)."""
    from socceraction_amd import synthetic
    d = games_dict()
    return synthetic.games_frame(d), synthetic.to_frame(d)


def table(n=N, seed=7):
    """``(X, y)``: 70 bool columns of mixed density and three numeric ones interleaved in model
    order -- a float column of ten values with NaNs, a float column of distinct values (254 cuts)
    and a constant integer column (0 cuts)."""
    rng = np.random.default_rng(seed)
    cols, z, b = {}, np.zeros(n), 0
    for f in range(N_BOOL + len(NUM_AT)):
        kind = NUM_AT.get(f)
        if kind == 'nan':
            v = rng.integers(0, 10, n).astype(np.float64)
            z += 0.3 * (v - 4.5)
            v[rng.random(n) < 0.1] = np.nan
            cols['x_nan'] = v
        elif kind == 'wide':
            v = rng.standard_normal(n)
            z += 1.5 * v
            cols['x_wide'] = v
        elif kind == 'const':
            cols['x_const'] = np.full(n, 3, np.int64)
        else:
            v = rng.random(n) < (0.02 + 0.9 * (b % 7) / 7)
            z += (0.8 if b % 3 == 0 else -0.2) * v
            cols[f'b{b}'] = v
            b += 1
    y = (rng.random(n) < 1 / (1 + np.exp(-(z - z.mean())))).astype(np.uint8)
    return pd.DataFrame(cols), y


def weights(y, n=N, seed=8):
    """Float32 weights in [0.25, 2) and one of 20.0 on the last row (it lies on the last rank only):
    the effective maximum, and with it the quantisation shift, is known to one rank alone."""
    w = (0.25 + 1.75 * np.random.default_rng(seed).random(n)).astype(np.float32)
    w[-1] = np.float32(20.0)
    return w


def row_keys(n=N, seed=9):
    return np.random.default_rng(seed).permutation(n).astype(np.int64) * 7919 + 13


def bounds(shards):
    off = np.concatenate([[0], np.cumsum(shards)])
    return [(int(off[r]), int(off[r + 1])) for r in range(len(shards))]


def stop_rows(y, shards):
    """Per rank ``(train, held-out)`` local row indices: rank 0 holds out 150 negatives only, every
    other rank with rows its every fourth row -- only the ranks' rows together hold both classes."""
    out = []
    for r, (a, b) in enumerate(bounds(shards)):
        loc = np.arange(b - a)
        ev = np.flatnonzero(y[a:b] == 0)[:150] if r == 0 else loc[loc % 4 == 3]
        out.append((np.setdiff1d(loc, ev), ev))
    return out
