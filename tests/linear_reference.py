"""Host oracle of the device logistic regression (socceraction_amd.linear, csrc/sa_linear.hip):
numpy and Python integers only.

The design matrix of ``d`` columns has ``D = d + 1`` columns, the last one the constant 1 of the
intercept; ``beta`` holds ``D`` values, the intercept last.  Item order of the sums: the upper
triangle of ``(w x_j) x_k`` row-major, then the ``D`` terms ``r x_k``, then the loss.
"""
from fractions import Fraction

import numpy as np

FRAC_BITS = 95


# ----------------------------------------------------------------------------- the data
def shot_like(n, rng):
    """Shot-like rows: 27 one-hot columns with an all-zero one, coordinates up to 105, a distance,
    an angle, a movement, a 0/1 column and a duplicated column; labels drawn from a logistic
    model.  Hessian condition number 1e7 - 1e8."""
    t = rng.integers(0, 23, n)
    b = rng.integers(0, 4, n)
    oh = np.zeros((n, 27))
    oh[np.arange(n), t] = 1
    oh[np.arange(n), 23 + b] = 1
    oh[:, 5] = 0
    x = rng.uniform(60, 105, n)
    y = rng.uniform(0, 68, n)
    dx, dy = 105 - x, 34 - y
    dist, ang = np.hypot(dx, dy), np.arctan2(np.abs(dy), dx)
    mov = rng.uniform(0, 40, n)
    team = rng.integers(0, 2, n).astype(float)
    X = np.column_stack([oh, x, y, dist, ang, mov, team, x + 0.0])
    z = -1.0 - 0.08 * dist + 1.2 * (ang < 0.5) + 0.5 * oh[:, 3]
    yy = (rng.uniform(size=n) < 1 / (1 + np.exp(-z))).astype(np.uint8)
    return X, yy


def shot_like_sets():
    """The 300-row and the 5,000-row set, drawn one after the other from ``default_rng(0)``."""
    rng = np.random.default_rng(0)
    return {300: shot_like(300, rng), 5000: shot_like(5000, rng)}


# ----------------------------------------------------------------------------- per-row values
def design(X):
    X = np.asarray(X)
    return np.column_stack([X.astype(np.float64), np.ones(len(X))])


def linear_predictor(A, beta):
    """z = b + sum_j beta_j x_j in column order, every product and add rounded on its own."""
    z = np.full(len(A), float(beta[-1]))
    for j in range(A.shape[1] - 1):
        z = z + float(beta[j]) * A[:, j]
    return z


def row_values(A, y, beta):
    """``(w, r, loss)`` of every row."""
    z = linear_predictor(A, beta)
    yy = (np.asarray(y) != 0).astype(np.float64)
    with np.errstate(over='ignore'):
        p = 1.0 / (1.0 + np.exp(-z))
    loss = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))) - yy * z
    return p * (1.0 - p), p - yy, loss


def sigmoid_of(X, beta):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-linear_predictor(design(X), beta)))


def _rows(mask, n):
    return np.arange(n) if mask is None else np.flatnonzero(np.asarray(mask)[:n])


def _term_blocks(A, w, r, loss):
    """The terms of every item as ``[rows, items of the block]`` arrays, in item order."""
    D = A.shape[1]
    for j in range(D):
        yield (w * A[:, j])[:, None] * A[:, j:]
    yield r[:, None] * A
    yield loss[:, None]


# ----------------------------------------------------------------------------- float64 moments
def moments(X, y, beta, mask=None, with_abs=False):
    """``(gradient [D], Hessian [D, D], loss)`` in float64, each entry the extended-precision sum
    of its rows' float64 terms.  ``with_abs``: also the sums of the terms' magnitudes."""
    A = design(X)
    rows = _rows(mask, len(A))
    A, y = A[rows], np.asarray(y)[rows]
    w, r, loss = row_values(A, y, beta)
    D = A.shape[1]
    sums, mags = [], []
    for blk in _term_blocks(A, w, r, loss):
        ext = blk.astype(np.longdouble)
        sums.append(ext.sum(axis=0))
        mags.append(np.abs(ext).sum(axis=0))
    flat, flat_abs = np.concatenate(sums).astype(np.float64), np.concatenate(mags).astype(np.float64)

    def shape(v):
        H = np.zeros((D, D))
        iu = np.triu_indices(D)
        H[iu] = v[:len(iu[0])]
        H = H + np.triu(H, 1).T
        return v[len(iu[0]):len(iu[0]) + D].copy(), H, float(v[-1])

    return shape(flat) + shape(flat_abs) if with_abs else shape(flat)


def objective_gradient(X, y, beta, C, fit_intercept=True):
    """The gradient of ``sum(loss) + ||w||^2 / (2 C)`` at ``beta`` (``D`` values; without an
    intercept the last one must be 0 and its entry is dropped)."""
    g, _, _ = moments(X, y, beta)
    d = len(beta) - 1
    g[:d] += np.asarray(beta[:d], np.float64) / C
    return g if fit_intercept else g[:d]


# ----------------------------------------------------------------------------- exact limb sums
def item_exps(col_exp, loss_exp):
    D = len(col_exp)
    return [col_exp[j] + col_exp[k] - 2 for j in range(D) for k in range(j, D)] + list(col_exp) + [loss_exp]


def quantize(v, E):
    """Q = trunc(v 2^(95 - E)) toward zero as a Python integer, from the exact value of ``v``."""
    q = Fraction(float(v)) * Fraction(2) ** (FRAC_BITS - E)
    return int(q)  # int() of a Fraction truncates toward zero


def limbs_of(q):
    """The three 32-bit limbs of Q, each carrying its sign."""
    s, m = (-1 if q < 0 else 1), abs(q)
    assert m < 1 << 96
    return [s * (m & 0xFFFFFFFF), s * ((m >> 32) & 0xFFFFFFFF), s * (m >> 64)]


def quantize_columns(v, E):
    """The signed limbs of every element of ``v [rows, items]`` at the per-item exponents ``E``:
    int64 ``[3, rows, items]``.  |v| < 2^E is the caller's."""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(np.abs(v))                        # |v| = m 2^e, m in [0.5, 1)
    M = np.ldexp(m, 53).astype(np.uint64)             # exact: 53-bit integers
    sh = e.astype(np.int64) - 53 + FRAC_BITS - np.asarray(E, np.int64)[None, :]
    assert (sh[v != 0] <= 42).all(), 'a value reaches its scale exponent'
    up = np.clip(sh, 0, 63).astype(np.uint64)
    down = np.clip(-sh, 0, 63).astype(np.uint64)
    lo = np.where(sh >= 0, M << up, np.where(sh > -64, M >> down, np.uint64(0)))
    hi = np.where(sh > 0, M >> (np.uint64(64) - np.clip(sh, 1, 63).astype(np.uint64)), np.uint64(0))
    sign = np.where(np.signbit(v), -1, 1).astype(np.int64)
    mask32 = np.uint64(0xFFFFFFFF)
    return np.stack([sign * (lo & mask32).astype(np.int64), sign * (lo >> np.uint64(32)).astype(np.int64),
                     sign * hi.astype(np.int64)])


def moments_limbs(X, y, beta, mask, exps):
    """The limb sums ``[items][3]`` (Python integers) of the float64 terms at ``beta``; ``exps``:
    the scale exponent of every item (:func:`item_exps`)."""
    A = design(X)
    rows = _rows(mask, len(A))
    A, y = A[rows], np.asarray(y)[rows]
    w, r, loss = row_values(A, y, beta)
    out, at = [], 0
    for blk in _term_blocks(A, w, r, loss):
        E = exps[at:at + blk.shape[1]]
        at += blk.shape[1]
        out += [[int(x) for x in col] for col in quantize_columns(blk, E).sum(axis=1).T]
    assert at == len(exps)
    return out


def moments_limbs_at_zero(X, y, mask, exps):
    """At beta = 0: p = 1/2, w = 1/4 and r = +-1/2 exactly, so every term is an exactly rounded
    float64 product and the limb sums are THE sums, whoever computes them."""
    return moments_limbs(X, y, np.zeros(np.asarray(X).shape[1] + 1), mask, exps)


# ----------------------------------------------------------------------------- the solve
def newton(X, y, C=1.0, tol=1e-10, max_iter=100, fit_intercept=True):
    """Newton's method with step halving from beta = 0 on ``sum(loss) + ||w||^2 / (2 C)``:
    ``(beta [D], iterations)``; stops at ``max|g| <= tol max(1, max|g(0)|)``."""
    d = np.asarray(X).shape[1]
    D = d + 1 if fit_intercept else d
    lam = np.full(D, 1.0 / C)
    if fit_intercept:
        lam[-1] = 0.0

    def full(b):
        g, H, f = moments(X, y, b if fit_intercept else np.append(b, 0.0))
        g, H = g[:D], H[:D, :D]
        return g + lam * b, H + np.diag(lam), f + 0.5 * float(np.sum(lam * b * b))

    beta = np.zeros(D)
    g, H, f = full(beta)
    g0 = np.abs(g).max()
    for it in range(max_iter):
        if np.abs(g).max() <= tol * max(1.0, g0):
            break
        step = np.linalg.solve(H, g)
        dec, t = float(g @ step), 1.0
        while True:
            cand = beta - t * step
            g2, H2, f2 = full(cand)
            if f2 <= f - 1e-4 * t * dec:
                break
            if abs(f2 - f) <= 16 * np.finfo(float).eps * abs(f) and np.abs(g2).max() < np.abs(g).max():
                break
            t *= 0.5
            assert t >= 2.0 ** -30, 'the step halving found no decrease'
        beta, g, H, f = cand, g2, H2, f2
    else:
        it = max_iter
    return (beta if fit_intercept else np.append(beta, 0.0)), it


# ----------------------------------------------------------------------------- sklearn
# max |probability difference| between :func:`newton` (tol 1e-10) and sklearn 1.7's
# LogisticRegression(solver='newton-cholesky', tol=1e-12, max_iter=1000) on :func:`shot_like_sets`,
# as measured on the host; key (rows, C, fit_intercept).  Two float64 solves of a 1e7-conditioned
# system differ in their last digits and each stops somewhere inside its own tolerance, so
# tests/test_linear_host.py and tests/test_gpu_linear.py (whose device fit runs the same iteration)
# both allow 10 x these figures.  A measured figure below one float64 ulp of a probability near 1
# (2.3e-16) is recorded as that ulp.
MEASURED_VS_SKLEARN = {
    (300, 1.0, True): 3.7e-12, (300, 0.01, True): 3.4e-16, (300, 1.0, False): 2.1e-12,
    (5000, 1.0, True): 6.7e-16, (5000, 0.01, True): 6.2e-16, (5000, 1.0, False): 3.7e-10,
}


def sklearn_fit(X, y, C, fit_intercept):
    from sklearn.linear_model import LogisticRegression
    return LogisticRegression(C=C, fit_intercept=fit_intercept, solver='newton-cholesky', tol=1e-12,
                              max_iter=1000).fit(X, y)
