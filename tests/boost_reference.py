"""Numpy restatement of the boosted-tree trainer's arithmetic contract (DESIGN.md §3
"Boosted-tree training"); TEST INFRASTRUCTURE ONLY.  Written from the contract, not from the
kernels or ``socceraction_amd.boost``: cuts, bins, quantised gradients, integer histograms, the
float64 gain with its tie rule, leaf values, the float32 margin update.

Everything works on a host bin matrix ``B [F, n]`` uint8 (a bool feature's bin is its bit).
"""
from __future__ import annotations

import numpy as np

NODE_DTYPE = np.dtype([('G', '<i8'), ('H', '<i8'), ('gain', '<f8'), ('feature', '<i4'), ('cut', '<i4'),
                       ('thr', '<f4'), ('value', '<f4'), ('exists', '<i4'), ('pad', '<i4')])
SCALE = np.float32(2.0 ** 30)
INV = 2.0 ** -30
DEFAULTS = dict(n_estimators=100, max_depth=3, learning_rate=0.3, reg_lambda=1.0, min_child_weight=1.0,
                gamma=0.0, base_score=0.5)


# --------------------------------------------------------------------------- cuts and bins
def cast32(col):
    col = np.asarray(col)
    if col.dtype.kind in 'iu':
        return col.astype(np.int64).astype(np.float64).astype(np.float32)
    with np.errstate(over='ignore'):  # a double beyond float32's range becomes +-inf
        return col.astype(np.float32)


def sample_rows(n):
    S = min(n, 65536)
    return np.array([(i * n) // S for i in range(S)], np.int64)


def cuts_of(col, is_bool=False):
    """Contract item 1 on a whole column (its deterministic sample is taken here)."""
    if is_bool:
        return np.array([0.5], np.float32)
    col = np.asarray(col)
    s = cast32(col[sample_rows(len(col))])
    s = np.sort(s[~np.isnan(s)])
    distinct = sorted(set(s.tolist()))
    if len(distinct) <= 255:
        return np.array(distinct[1:], np.float32)
    L = len(s)
    picked = sorted({float(s[(i * L) // 255]) for i in range(1, 255)})
    return np.array([c for c in picked if c != float(s[0])], np.float32)


def bins_of(x32, cuts):
    """Contract item 2: #{i : c_i <= x32}, NaN -> 255."""
    x32 = np.asarray(x32, np.float32)
    cuts = np.asarray(cuts, np.float32)
    with np.errstate(invalid='ignore'):
        b = (cuts[None, :] <= x32[:, None]).sum(1).astype(np.uint8)
    b[np.isnan(x32)] = 255
    return b


# --------------------------------------------------------------------------- gradients
def probability(m):
    m = np.asarray(m, np.float32)
    with np.errstate(over='ignore'):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-m).astype(np.float32))).astype(np.float32)


def quantise(p, y):
    """Contract item 3 from a float32 probability column: (gq, hq) int32."""
    p = np.asarray(p, np.float32)
    y32 = np.asarray(y).astype(bool).astype(np.float32)
    g = (p - y32).astype(np.float32)
    h = (p * (np.float32(1.0) - p).astype(np.float32)).astype(np.float32)
    return (np.rint((g * SCALE).astype(np.float32)).astype(np.int32),
            np.rint((h * SCALE).astype(np.float32)).astype(np.int32))


# --------------------------------------------------------------------------- histograms
def histograms(B, gq, hq, node, n_nodes):
    """Contract item 4 with np.add.at: [n_nodes, F, 256, 2] int64; node 255 = not taking part."""
    F, n = B.shape
    hist = np.zeros((n_nodes, F, 256, 2), np.int64)
    node = np.asarray(node).astype(np.int64)
    live = np.flatnonzero(node != 255)
    g, h = np.asarray(gq, np.int64)[live], np.asarray(hq, np.int64)[live]
    for f in range(F):
        np.add.at(hist[:, f, :, 0], (node[live], B[f, live]), g)
        np.add.at(hist[:, f, :, 1], (node[live], B[f, live]), h)
    return hist


def _fast_hist(B, g, h, rows):
    """[F, 256, 2] int64 of the rows of one node.  bincount sums float64 weights; every partial
    sum is an integer below 2^53 for fewer than 2^22 rows, so the result is the exact integer."""
    F = B.shape[0]
    assert B.shape[1] < 2 ** 22
    key = (np.arange(F, dtype=np.int64)[:, None] * 256 + B[:, rows]).ravel()
    out = np.empty((F, 256, 2), np.int64)
    for c, v in enumerate((g, h)):
        w = np.broadcast_to(v[rows].astype(np.float64), (F, len(rows))).ravel()
        out[:, :, c] = np.bincount(key, weights=w, minlength=F * 256).reshape(F, 256).astype(np.int64)
    return out


# --------------------------------------------------------------------------- splits
def best_split(hist, G, H, cuts, reg_lambda=1.0, min_child_weight=1.0, gamma=0.0):
    """Contract item 5 for one node: ``(feature, cut, gain, GL, HL)`` or None.  hist [F, 256, 2]
    int64, G / H the node's integer totals."""
    F = hist.shape[0]
    m = np.array([len(c) for c in cuts])
    gl = np.cumsum(hist[:, :, 0], axis=1)[:, :255]
    hl = np.cumsum(hist[:, :, 1], axis=1)[:, :255]
    Gf, Hf = float(G) * INV, float(H) * INV
    GL, HL = gl.astype(np.float64) * INV, hl.astype(np.float64) * INV
    GR, HR = (G - gl).astype(np.float64) * INV, (H - hl).astype(np.float64) * INV
    with np.errstate(all='ignore'):
        gain = ((GL * GL) / (HL + reg_lambda) + (GR * GR) / (HR + reg_lambda)) - (Gf * Gf) / (Hf + reg_lambda)
    valid = (HL >= min_child_weight) & (HR >= min_child_weight) & ~np.isnan(gain)
    valid &= np.arange(255)[None, :] < m[:, None]
    if not valid.any():
        return None
    gain = np.where(valid, gain, -np.inf)
    flat = int(np.argmax(gain))  # the first maximum: lowest feature, then lowest cut
    f, i = divmod(flat, 255)
    if not gain[f, i] > gamma:
        return None
    return f, i, float(gain[f, i]), int(gl[f, i]), int(hl[f, i])


def leaf_value(G, H, learning_rate=0.3, reg_lambda=1.0):
    """Contract item 6."""
    with np.errstate(all='ignore'):
        return np.float32(learning_rate * (-((float(G) * INV) / (float(H) * INV + reg_lambda))))


def build_tree(B, gq, hq, cuts, params, active=None):
    """One round: the heap node table and every row's final node (255 = not taking part)."""
    p = {**DEFAULTS, **params}
    D = int(p['max_depth'])
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
            tab['value'][k] = leaf_value(G, H, p['learning_rate'], p['reg_lambda'])
            tab['feature'][k] = tab['cut'][k] = -1
            if level == D:
                continue
            rows = np.flatnonzero(node == k)
            best = best_split(_fast_hist(B, g64, h64, rows), G, H, cuts, p['reg_lambda'],
                              p['min_child_weight'], p['gamma'])
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


def base_margin(base_score=0.5):
    p = np.float32(float(base_score))
    return np.float32(-np.log(np.float32(1.0) / p - np.float32(1.0)))


def update_margin(m, tab, node):
    """Contract item 7: m + leaf in float32 for the rows taking part."""
    m = np.asarray(m, np.float32).copy()
    live = node != 255
    m[live] = (m[live] + tab['value'][node[live]]).astype(np.float32)
    return m


def fit(B, y, cuts, **params):
    """The whole trainer: ``(tables [T, M], final margin, [p_t])`` with numpy's own exp."""
    p = {**DEFAULTS, **params}
    n = B.shape[1]
    m = np.full(n, base_margin(p['base_score']), np.float32)
    tabs, ps = [], []
    for _ in range(int(p['n_estimators'])):
        pt = probability(m)
        gq, hq = quantise(pt, y)
        tab, node = build_tree(B, gq, hq, cuts, p)
        m = update_margin(m, tab, node)
        tabs.append(tab)
        ps.append(pt)
    return np.stack(tabs) if tabs else np.zeros((0, 2 ** (int(p['max_depth']) + 1) - 1), NODE_DTYPE), m, ps


def predict(tabs, X32, base_score=0.5):
    """P(class 1) float32 of node tables on float32 values [n, F] (x < thr left, NaN right)."""
    n = X32.shape[0]
    m = np.full(n, base_margin(base_score), np.float32)
    for tab in tabs:
        node = np.zeros(n, np.int64)
        for _ in range(8):
            f = tab['feature'][node]
            live = np.flatnonzero(f >= 0)
            if not len(live):
                break
            with np.errstate(invalid='ignore'):
                left = X32[live, f[live]] < tab['thr'][node[live]]
            node[live] = np.where(left, 2 * node[live] + 1, 2 * node[live] + 2)
        m = (m + tab['value'][node]).astype(np.float32)
    return probability(m)
