"""Numpy restatement of contract items 13-17 of the boosted-tree trainer (DESIGN.md §3 "Boosted-tree
training"): effective weights and the power-of-two quantisation shift, weighted gradients, the L1
penalty, and the counter-hash row and column samples; TEST INFRASTRUCTURE ONLY.  Written from the
contract, not from the kernels or ``socceraction_amd.boost``.  Items 1-12 come from
``boost_reference`` (imported, not edited); with every new input neutral :func:`fit` is
``boost_reference.fit`` byte for byte.
"""
from __future__ import annotations

import numpy as np

import boost_reference as br

NODE_DTYPE = br.NODE_DTYPE
SALT_ROWS, SALT_COLS = 0x726F77, 0x636F6C
MAX_SHIFT = 20
DEFAULTS = dict(br.DEFAULTS, subsample=1.0, colsample_bytree=1.0, reg_alpha=0.0, scale_pos_weight=1.0,
                random_state=0)
U = np.uint64


# --------------------------------------------------------------------------- the hash (item 16)
def fm(z):
    """splitmix64's finaliser on uint64 (scalar or array), wrapping."""
    z = np.array(z, dtype=U, copy=True)
    with np.errstate(over='ignore'):
        z ^= z >> U(30)
        z *= U(0xBF58476D1CE4E5B9)
        z ^= z >> U(27)
        z *= U(0x94D049BB133111EB)
        z ^= z >> U(31)
    return z


def draw(salt, seed, t, keys):
    """``fm(fm(fm(seed ^ salt) + t) + key)`` for an array of keys (any integer dtype; int64 keys
    are taken as their uint64 bit patterns)."""
    keys = np.asarray(keys)
    keys = keys.astype(np.int64).view(U) if keys.dtype.kind == 'i' else keys.astype(U)
    with np.errstate(over='ignore'):
        base = fm(fm(U(int(seed) ^ int(salt))) + U(int(t)))
        return fm(base + keys)


def threshold(subsample):
    return int(np.floor(np.float64(subsample) * np.float64(2.0 ** 32)))


def row_sample(seed, t, keys, thr):
    """Which rows are in round t's sample: ``(draw >> 32) < thr`` as 64-bit integers."""
    return (draw(SALT_ROWS, seed, t, keys) >> U(32)) < U(int(thr))


def column_sample(seed, t, F, colsample_bytree):
    """Round t's ``k = max(1, floor(colsample_bytree F))`` features, ascending."""
    k = max(1, int(np.floor(np.float64(colsample_bytree) * F)))
    d = draw(SALT_COLS, seed, t, np.arange(F, dtype=np.int64))
    order = sorted(range(F), key=lambda f: (int(d[f]), f))
    return np.array(sorted(order[:k]), np.int64)


# --------------------------------------------------------------------------- weights (items 13, 14)
def effective_weight(w, y, s=1.0):
    """``we = w * (y ? (float)s : 1.0f)``, one float32 multiplication (``w = 1`` when absent)."""
    y = np.asarray(y).astype(bool)
    w = np.ones(len(y), np.float32) if w is None else np.asarray(w, np.float32)
    return (w * np.where(y, np.float32(s), np.float32(1.0)).astype(np.float32)).astype(np.float32)


def shift_of(mx):
    """The smallest integer ``e >= 0`` with ``mx <= 2^e``; the range rule of item 13."""
    mx = float(mx)
    if not (np.isfinite(mx) and 0 < mx <= 2.0 ** MAX_SHIFT):
        raise ValueError('the largest effective weight must be in (0, 2^20]')
    e = 0
    while mx > 2.0 ** e:
        e += 1
    return e


def quantise(p, y, we, e, sampled=None):
    """Item 14 from a float32 probability column: every product a float32 operation of its own."""
    p = np.asarray(p, np.float32)
    y32 = np.asarray(y).astype(bool).astype(np.float32)
    we = np.asarray(we, np.float32)
    scale = np.float32(2.0 ** (30 - e))
    g = ((p - y32).astype(np.float32) * we).astype(np.float32)
    h = ((p * (np.float32(1.0) - p).astype(np.float32)).astype(np.float32) * we).astype(np.float32)
    gq = np.rint((g * scale).astype(np.float32)).astype(np.int32)
    hq = np.rint((h * scale).astype(np.float32)).astype(np.int32)
    if sampled is not None:
        gq[~sampled] = 0
        hq[~sampled] = 0
    return gq, hq


# --------------------------------------------------------------------------- splits (items 14, 15, 17)
def shrink(G, a):
    """``T(G) = G > a ? G - a : (G < -a ? G + a : 0.0)`` in float64."""
    G = np.asarray(G, np.float64)
    return np.where(G > a, G - a, np.where(G < -a, G + a, 0.0))


def best_split(hist, G, H, cuts, reg_lambda=1.0, min_child_weight=1.0, gamma=0.0, reg_alpha=0.0, e=0,
               features=None):
    """One node's ``(feature, cut, gain, GL, HL)`` or None; ``features``: the round's column
    sample (None: all)."""
    F = hist.shape[0]
    inv = 2.0 ** (e - 30)
    m = np.array([len(c) for c in cuts])
    gl = np.cumsum(hist[:, :, 0], axis=1)[:, :255]
    hl = np.cumsum(hist[:, :, 1], axis=1)[:, :255]
    Gf, Hf = float(G) * inv, float(H) * inv
    GL, HL = gl.astype(np.float64) * inv, hl.astype(np.float64) * inv
    GR, HR = (G - gl).astype(np.float64) * inv, (H - hl).astype(np.float64) * inv
    TL, TR, TG = shrink(GL, reg_alpha), shrink(GR, reg_alpha), float(shrink(Gf, reg_alpha))
    with np.errstate(all='ignore'):
        gain = ((TL * TL) / (HL + reg_lambda) + (TR * TR) / (HR + reg_lambda)) - (TG * TG) / (Hf + reg_lambda)
    valid = (HL >= min_child_weight) & (HR >= min_child_weight) & ~np.isnan(gain)
    valid &= np.arange(255)[None, :] < m[:, None]
    if features is not None:
        keep = np.zeros(F, bool)
        keep[np.asarray(features, np.int64)] = True
        valid &= keep[:, None]
    if not valid.any():
        return None
    gain = np.where(valid, gain, -np.inf)
    f, i = divmod(int(np.argmax(gain)), 255)  # the first maximum: lowest feature, then lowest cut
    if not gain[f, i] > gamma:
        return None
    return f, i, float(gain[f, i]), int(gl[f, i]), int(hl[f, i])


def leaf_value(G, H, learning_rate=0.3, reg_lambda=1.0, reg_alpha=0.0, e=0):
    inv = 2.0 ** (e - 30)
    with np.errstate(all='ignore'):
        return np.float32(learning_rate * (-(float(shrink(float(G) * inv, reg_alpha)) / (float(H) * inv + reg_lambda))))


def build_tree(B, gq, hq, cuts, params, e=0, features=None, active=None):
    """One round (``boost_reference.build_tree`` with items 14, 15 and 17): a row outside the
    round's row sample comes with ``gq = hq = 0`` and walks the tree like any other."""
    p = {**DEFAULTS, **params}
    D, a = int(p['max_depth']), float(p['reg_alpha'])
    n = B.shape[1]
    tab = np.zeros(2 ** (D + 1) - 1, NODE_DTYPE)
    node = np.zeros(n, np.int64)
    if active is not None:
        node[~np.asarray(active, bool)] = 255
    g64, h64 = np.asarray(gq, np.int64), np.asarray(hq, np.int64)
    tab['exists'][0] = 1
    tab['G'][0] = g64[node == 0].sum()
    tab['H'][0] = h64[node == 0].sum()
    for level in range(D + 1):
        for k in range(2 ** level - 1, 2 ** (level + 1) - 1):
            if not tab['exists'][k]:
                continue
            G, H = int(tab['G'][k]), int(tab['H'][k])
            tab['value'][k] = leaf_value(G, H, p['learning_rate'], p['reg_lambda'], a, e)
            tab['feature'][k] = tab['cut'][k] = -1
            if level == D:
                continue
            rows = np.flatnonzero(node == k)
            best = best_split(br._fast_hist(B, g64, h64, rows), G, H, cuts, p['reg_lambda'], p['min_child_weight'],
                              p['gamma'], a, e, features)
            if best is None:
                continue
            f, i, gain, gl, hl = best
            tab['feature'][k], tab['cut'][k], tab['gain'][k], tab['thr'][k] = f, i, gain, cuts[f][i]
            for c, (cg, ch) in ((2 * k + 1, (gl, hl)), (2 * k + 2, (G - gl, H - hl))):
                tab['exists'][c], tab['G'][c], tab['H'][c], tab['feature'][c] = 1, cg, ch, -1
            left = B[f, rows] <= i
            node[rows[left]] = 2 * k + 1
            node[rows[~left]] = 2 * k + 2
    return tab, node


def round_inputs(params, t, F, keys):
    """``(row sample or None, column sample or None)`` of round t."""
    p = {**DEFAULTS, **params}
    thr = threshold(p['subsample'])
    rows = None if thr >= 2 ** 32 else row_sample(p['random_state'], t, keys, thr)
    cols = None if float(p['colsample_bytree']) == 1.0 else column_sample(p['random_state'], t, F,
                                                                           p['colsample_bytree'])
    return rows, cols


def fit(B, y, cuts, sample_weight=None, row_keys=None, **params):
    """The whole trainer: ``(tables [T, M], final margin, [p_t], e)`` with numpy's own exp."""
    p = {**DEFAULTS, **params}
    F, n = B.shape
    we = effective_weight(sample_weight, y, p['scale_pos_weight'])
    if not (np.isfinite(we).all() and (we >= 0).all()):
        raise ValueError('weights must be finite and not negative')
    e = shift_of(we.max())
    keys = np.arange(n, dtype=np.int64) if row_keys is None else np.asarray(row_keys)
    m = np.full(n, br.base_margin(p['base_score']), np.float32)
    tabs, ps = [], []
    for t in range(int(p['n_estimators'])):
        pt = br.probability(m)
        rows, cols = round_inputs(p, t, F, keys)
        gq, hq = quantise(pt, y, we, e, rows)
        tab, node = build_tree(B, gq, hq, cuts, p, e, cols)
        m = br.update_margin(m, tab, node)
        tabs.append(tab)
        ps.append(pt)
    return (np.stack(tabs) if tabs else np.zeros((0, 2 ** (int(p['max_depth']) + 1) - 1), NODE_DTYPE)), m, ps, e
