"""The device logistic regression (socceraction_amd.linear, csrc/sa_linear.hip) against the host
oracle tests/linear_reference.py: the raw limb sums integer for integer at beta = 0, the
finalised moments at a beta that meets both tails of the sigmoid, order and grid independence
byte for byte, the fit against the optimality condition and sklearn's Newton solver, the
predictor, the kernel's error flags and the expected-goals model's logistic learner."""
import warnings

import numpy as np
import pandas as pd
import pytest

import linear_reference as lr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

N_BOOL, N_F64, N_I64 = 587, 43, 10  # 640 columns: the widest model the kernels take
N_VAEP = 568  # VAEP's default feature set (k = 3)
N_MAX = 2 * 2048 + 777  # two numeric tiles of 2048 rows and a remainder


@pytest.fixture(scope='module')
def sa():
    from socceraction_amd import _native, batch, catalog, linear, metrics, ops, synthetic, xg
    _native.load_library()
    return dict(native=_native, batch=batch, catalog=catalog, linear=linear, metrics=metrics, ops=ops,
                synthetic=synthetic, xg=xg)


# ----------------------------------------------------------------------------- the case batch
def _host_batch():
    """N_MAX rows of 587 bool, 43 float64 and 10 int64 columns and a label column, built once."""
    rng = np.random.default_rng(20240607)
    n = N_MAX
    cols = {}
    for c in range(N_BOOL):
        cols[f'b{c}'] = rng.uniform(size=n) < (0.0 if c == 7 else 0.03 + 0.9 * rng.uniform())
    scales = [105.0, 68.0, 1.0, np.pi, 1e-3, 40.0, 3e4, 0.5]
    for c in range(N_F64):
        v = rng.uniform(-1.0, 1.0, n) * scales[c % len(scales)]
        if c % 3 == 0:
            v = np.abs(v)
        if c == 5:
            v[rng.uniform(size=n) < 0.5] = 0.0
        cols[f'f{c}'] = v
    cols['f9'] = cols['f1'].copy()  # a duplicated column
    for c in range(N_I64):
        cols[f'i{c}'] = rng.integers(-3, 4, n) if c % 2 else rng.integers(0, 1000 if c == 4 else 12, n)
    y = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    y[:2] = (1, 0)
    return cols, y


COLS, Y = _host_batch()
ORDER = [(name, name[0], int(name[1:])) for name in COLS]


def _wide_width():
    """The narrowest model whose item table spans more than one block of SA_LOGIT_BLOCK_K columns
    (and several blocks of SA_LOGIT_BLOCK_J rows)."""
    from socceraction_amd import linear
    d = 1
    while linear.item_grid(d)[1] < 2:
        d += 1
    assert linear.item_grid(d)[0] > 2
    return d


def _column_sets():
    rng = np.random.default_rng(11)
    names = list(COLS)
    bools, fs, ints = names[:N_BOOL], names[N_BOOL:N_BOOL + N_F64], names[N_BOOL + N_F64:]
    xg46 = [str(c) for c in rng.permutation(bools[:30] + fs[:11] + ints[:5])]
    mixed = [str(c) for c in rng.permutation(bools[:40] + fs[:16] + ints)]
    wide = mixed[:_wide_width()]
    vaep = [str(c) for c in rng.permutation(bools[:N_VAEP - 53] + fs + ints)]  # 515 bool + 53 numeric, as VAEP's
    widest = [str(c) for c in rng.permutation(names)]
    assert len(vaep) == N_VAEP and len(widest) == 640
    return {'bool_only': bools[3:8], 'num_only': ['f0', 'i4', 'f4', 'i1', 'f6'], 'one': ['f3'], 'xg46': xg46,
            'wide': wide, 'vaep568': vaep, 'max640': widest}


SETS = _column_sets()
# both sides of the kernel's 64-row tile and of a second tile, one row, and two numeric tiles + remainder
ROW_COUNTS = [1, 63, 64, 65, 129, N_MAX]
# the two widest sets run at the small row counts: their oracle has 162,735 and 206,403 items per row
ZERO_CASES = [(n, c) for n in ROW_COUNTS for c in SETS if n <= 129 or c not in ('vaep568', 'max640')]
ZERO_CASES = [(n, c) for n, c in ZERO_CASES if c != 'max640' or n in (1, 65)]


def _matrix(names, rows=None, f32=False):
    """The oracle's X: the named host columns as float64 (through float32 for ``num32`` blocks)."""
    out = []
    for name in names:
        v = COLS[name] if rows is None else COLS[name][rows]
        v = v.astype(np.float64)
        out.append(v.astype(np.float32).astype(np.float64) if f32 and name[0] != 'b' else v)
    return np.column_stack(out)


_BLOCKS = {}


def _blocks(sa, n, num32=False):
    """Rows 0 .. n - 1 of the batch as bitmap-form feature blocks whose numeric tile is smaller
    than n (16 rows up to 129, 2048 beyond); the tiles' padding holds NaN / a huge integer and the
    bitmaps' tail bits are set: nothing may read them."""
    key = (n, num32)
    if key not in _BLOCKS:
        R = 16 if n <= 129 else 2048
        tiles = -(-n // R)
        fdt, idt = (np.float32, np.float32) if num32 else (np.float64, np.int64)
        hf = np.full((tiles, N_F64, R), np.nan, fdt)
        hi = np.full((tiles, N_I64, R), 3e9 if num32 else 1 << 40, idt)
        for t in range(tiles):
            a, b = t * R, min(n, (t + 1) * R)
            for c in range(N_F64):
                hf[t, c, :b - a] = COLS[f'f{c}'][a:b]
            for c in range(N_I64):
                hi[t, c, :b - a] = COLS[f'i{c}'][a:b]
        words = (n + 63) // 64
        hb = np.zeros((N_BOOL, words * 64), bool)
        hb[:, n:] = True
        for c in range(N_BOOL):
            hb[c, :n] = COLS[f'b{c}'][:n]
        bits = np.packbits(hb, axis=1, bitorder='little').view(np.int64)
        plan = sa['catalog'].FeaturePlan((), 1, False, N_BOOL, N_F64, N_I64, list(ORDER), None)
        _BLOCKS[key] = sa['ops'].FeatureBlocks(plan, n, 1024, R, None, torch.from_numpy(hf).cuda(),
                                               torch.from_numpy(hi).cuda(), torch.from_numpy(bits).cuda())
    return _BLOCKS[key]


def _mask(n):
    """A row mask whose last set row sits in the middle of a 64-row bitmap word."""
    m = (np.random.default_rng(n).uniform(size=n) < 0.7).astype(np.uint8)
    last = n // 64 * 64 + 20
    if last >= n:
        last = max(0, last - 64) if n > 64 else min(n - 1, 20)
    m[last] = 1
    m[last + 1:] = 0
    assert last == n - 1 or last % 64 not in (0, 63)
    return m


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(sa, blocks, names, beta, y, mask, grid_x=0):
    """``(limbs as nested Python integers, col_exp, loss_exp)`` of one launch; no error bit."""
    lin = sa['linear']
    _, kc = lin.model_slots(blocks, names)
    dmask = None if mask is None else _dev(mask)
    col_exp = lin.column_exps(blocks, kc, dmask)
    loss_exp = lin.loss_exponent(np.asarray(beta, np.float64), col_exp)
    limbs, err = lin.moments_limbs(blocks, kc, beta, _dev(y), dmask, col_exp, loss_exp, grid_x)
    assert int(err.item()) == 0
    return limbs.cpu().numpy(), col_exp, loss_exp


def _check_exps(X, mask, col_exp):
    """|x_j| < 2^E_j over the rows that take part, and no exponent larger than needed."""
    rows = slice(None) if mask is None else np.flatnonzero(mask)
    mx = np.abs(X[rows]).max(axis=0) if X.shape[1] else np.zeros(0)
    for m, e in zip(mx, col_exp[:-1]):
        assert m < 2.0 ** e and (m == 0 or m >= 2.0 ** (e - 1) or X.dtype == bool)
    assert col_exp[-1] == 1


# ----------------------------------------------------------------------------- 1. exact at beta = 0
@pytest.mark.parametrize('variant', ['plain', 'mask', 'num32', 'compact'])
@pytest.mark.parametrize('n, cols', ZERO_CASES)
def test_limb_sums_at_zero_are_exact(sa, n, cols, variant):
    """Gradient, Hessian and loss limbs equal the oracle's integer for integer."""
    names = SETS[cols]
    blocks = _blocks(sa, n, num32=variant == 'num32')
    mask, rows, y = None, None, Y[:n]
    if variant == 'mask':
        mask = _mask(n)
    if variant == 'compact':  # repeated and unordered rows out of select_rows
        rows = np.random.default_rng(n + 1).integers(0, n, n + 7)
        blocks = sa['ops'].select_rows(blocks, _dev(rows))
        y = y[rows]
    X = _matrix(names, slice(0, n) if rows is None else rows, f32=variant == 'num32')
    beta = np.zeros(len(names) + 1)
    got, col_exp, loss_exp = _raw(sa, blocks, names, beta, y, mask)
    _check_exps(X, mask, col_exp)
    assert loss_exp == 1
    want = lr.moments_limbs_at_zero(X, y, mask, lr.item_exps(col_exp, loss_exp))
    assert got.shape == (sa['linear'].n_items(len(names)), 3)
    assert got.tolist() == want


def test_a_model_wider_than_the_limit_is_refused(sa):
    lin = sa['linear']
    X = np.zeros((8, sa['native'].SA_LOGIT_MAX_COLS + 1))
    X[::2, 0] = 1.0
    blocks = lin.host_blocks(X)
    y = _dev(np.array([0, 1] * 4, np.uint8))
    with pytest.raises(ValueError, match='at most 640 columns: got 641'):
        lin.DeviceLogisticRegression().fit_blocks(blocks, y)
    fitted = lin.DeviceLogisticRegression().fit_blocks(blocks, y, columns=[f'f{j}' for j in range(640)])
    assert fitted.coef_.shape == (1, 640) and fitted.coef_[0, 0] < 0 and not fitted.coef_[0, 1:].any()


# ----------------------------------------------------------------------------- 2. a non-zero beta
def _tail_beta(X, seed=3):
    """A fixed-seed beta whose z reaches about +-30 on X: both tails of the sigmoid."""
    rng = np.random.default_rng(seed)
    beta = rng.normal(size=X.shape[1] + 1) / np.append(np.maximum(np.abs(X).max(axis=0), 1e-3), 1.0)
    z = lr.linear_predictor(lr.design(X), beta)
    return beta * (30.0 / max(np.abs(z).max(), 1e-30))


@pytest.mark.parametrize('n, cols', [(n, c) for n in (65, N_MAX) for c in ('num_only', 'xg46', 'wide')]
                         + [(129, 'vaep568')])
def test_moments_at_a_nonzero_beta(sa, n, cols):
    """Entry by entry within 1e-12 of the entry's sum of |terms|: each term differs from the
    oracle's by a few ulp of exp (a few times 1e-16 relative) and the limb truncation is 2^-95 of
    the scale, so 1e-12 leaves three orders of margin and still catches a dropped or doubled row."""
    lin, names = sa['linear'], SETS[cols]
    X, y, mask = _matrix(names, slice(0, n)), Y[:n], _mask(n)
    beta = _tail_beta(X)
    z = lr.linear_predictor(lr.design(X), beta)[np.flatnonzero(mask)]
    if n == N_MAX:
        assert z.max() > 10 and z.min() < -10
    got, col_exp, loss_exp = _raw(sa, _blocks(sa, n), names, beta, y, mask)
    g, H, f = lin.finalize(got, col_exp, loss_exp)
    rg, rH, rf, ag, aH, af = lr.moments(X, y, beta, mask, with_abs=True)
    eg, eH, ef = np.abs(g - rg) / np.maximum(ag, 1e-300), np.abs(H - rH) / np.maximum(aH, 1e-300), abs(f - rf) / af
    print(f'n={n} {cols}: max relative-to-|terms| error: gradient {eg.max():.2e}, Hessian {eH.max():.2e}, '
          f'loss {ef:.2e}')
    assert (np.abs(g - rg) <= 1e-12 * ag).all()
    assert (np.abs(H - rH) <= 1e-12 * aH).all()
    assert abs(f - rf) <= 1e-12 * af
    assert f > 0 and (np.diag(H) >= 0).all() and np.array_equal(H, H.T)


# ----------------------------------------------------------------------------- 3. order independence
def _permuted_blocks(sa, names, perm):
    X = pd.DataFrame({c: COLS[c][perm] for c in names})
    return sa['linear'].host_blocks(X)


@pytest.mark.parametrize('cols', ['xg46', 'wide'])
def test_limbs_do_not_depend_on_row_order_or_grid(sa, cols):
    n, names = N_MAX, SETS[cols]
    X, y, mask = _matrix(names, slice(0, n)), Y[:n], _mask(n)
    beta = _tail_beta(X)
    base, col_exp, loss_exp = _raw(sa, _blocks(sa, n), names, beta, y, mask)
    assert np.abs(base).sum() > 0
    for grid_x in (1, 2, 7, 33, 100000):  # one workgroup takes every tile ... one tile per workgroup
        again, _, _ = _raw(sa, _blocks(sa, n), names, beta, y, mask, grid_x)
        assert again.tobytes() == base.tobytes(), grid_x
    perm = np.random.default_rng(8).permutation(n)
    moved, ce, le = _raw(sa, _permuted_blocks(sa, names, perm), names, beta, y[perm], mask[perm])
    assert (ce, le) == (col_exp, loss_exp)
    assert moved.tobytes() == base.tobytes()
    # the same rows padded out by masked rows: another n, another grid
    keep = np.flatnonzero(mask)
    small, ce, le = _raw(sa, _permuted_blocks(sa, names, keep), names, beta, y[keep], None)
    assert (ce, le) == (col_exp, loss_exp) and small.tobytes() == base.tobytes()


def test_fits_are_reproducible_byte_for_byte(sa):
    """Two fits in one process, a fit on permuted rows and a fit through a row list of the tiled
    table end in the same bytes."""
    lin, names = sa['linear'], SETS['xg46']
    rng = np.random.default_rng(2)
    rows = np.sort(rng.permutation(N_MAX)[:1000])
    X = _matrix(names, rows)
    z = lr.linear_predictor(lr.design(X), _tail_beta(X) / 10)
    y = (rng.uniform(size=len(rows)) < 1 / (1 + np.exp(-z))).astype(np.uint8)
    first = lin.DeviceLogisticRegression().fit_blocks(_permuted_blocks(sa, names, rows), _dev(y))
    again = lin.DeviceLogisticRegression().fit_blocks(_permuted_blocks(sa, names, rows), _dev(y))
    perm = rng.permutation(len(rows))
    moved = lin.DeviceLogisticRegression().fit_blocks(_permuted_blocks(sa, names, rows[perm]), _dev(y[perm]))
    y_full = np.ones(N_MAX, np.uint8)
    y_full[rows] = y
    listed = lin.DeviceLogisticRegression().fit_blocks(_blocks(sa, N_MAX), _dev(y_full), rows=_dev(rows[perm]),
                                                       columns=names)
    for other in (again, moved, listed):
        assert first.coef_.tobytes() == other.coef_.tobytes()
        assert first.intercept_.tobytes() == other.intercept_.tobytes()
        assert int(first.n_iter_[0]) == int(other.n_iter_[0])
    assert first.coef_.shape == (1, 46) and list(first.feature_names_in_) == names and np.abs(first.coef_).max() > 0
    beta = np.append(first.coef_[0], first.intercept_[0])
    g0 = np.abs(lr.objective_gradient(X, y, np.zeros(len(beta)), 1.0)).max()
    assert np.abs(lr.objective_gradient(X, y, beta, 1.0)).max() <= 2e-10 * max(1.0, g0)


# ----------------------------------------------------------------------------- 4. the optimum
@pytest.fixture(scope='module')
def shot_sets():
    return lr.shot_like_sets()


@pytest.mark.parametrize('n, C, fit_intercept', sorted(lr.MEASURED_VS_SKLEARN, key=str))
def test_the_fit_is_the_optimum(sa, shot_sets, n, C, fit_intercept):
    """The optimality condition in numpy, sklearn's newton-cholesky fit and the oracle's iteration
    count.  The probability bound is the host test's: 10 x ``linear_reference.MEASURED_VS_SKLEARN``.
    The device fit's own max |p - sklearn|, measured on an MI355X (rows, C, intercept): (300, 1, yes)
    3.66e-12, (300, 0.01, yes) 3.89e-16, (300, 1, no) 2.08e-12, (5000, 1, yes) 7.77e-16, (5000, 0.01,
    yes) 6.11e-16, (5000, 1, no) 3.68e-10 -- the host oracle's figures to within an ulp, as both run
    the same iteration."""
    X, y = shot_sets[n]
    tol = 1e-10
    from sklearn.exceptions import ConvergenceWarning
    with warnings.catch_warnings():
        warnings.simplefilter('error', ConvergenceWarning)
        model = sa['linear'].DeviceLogisticRegression(C=C, fit_intercept=fit_intercept, tol=tol).fit(X, y)
    beta = np.append(model.coef_[0], model.intercept_[0])
    assert model.coef_.shape == (1, X.shape[1]) and model.intercept_.shape == (1,)
    assert fit_intercept or model.intercept_[0] == 0.0
    g0 = np.abs(lr.objective_gradient(X, y, np.zeros(len(beta)), C, fit_intercept)).max()
    g = np.abs(lr.objective_gradient(X, y, beta, C, fit_intercept)).max()
    ref = lr.sklearn_fit(X, y, C, fit_intercept)
    proba = model.predict_proba(X)
    diff = np.abs(proba[:, 1] - ref.predict_proba(X)[:, 1]).max()
    _, it = lr.newton(X, y, C=C, tol=tol, fit_intercept=fit_intercept)
    print(f'n={n} C={C} intercept={fit_intercept}: |g| {g:.3g} (bound {2 * tol * max(1.0, g0):.3g}), '
          f'max |p - sklearn| {diff:.3g}, iterations {int(model.n_iter_[0])} (oracle {it})')
    assert g <= 2 * tol * max(1.0, g0)
    assert diff <= 10 * lr.MEASURED_VS_SKLEARN[(n, C, fit_intercept)]
    assert int(model.n_iter_[0]) <= it + 1
    assert proba.shape == (n, 2) and np.array_equal(proba[:, 0], 1.0 - proba[:, 1])
    assert list(model.classes_) == [0, 1]
    assert np.array_equal(model.predict(X), (proba[:, 1] > 0.5).astype(y.dtype))
    assert (model.predict(X) == ref.predict(X)).mean() > 0.999


def test_max_iter_raises_sklearns_warning(sa, shot_sets):
    from sklearn.exceptions import ConvergenceWarning
    X, y = shot_sets[300]
    with pytest.warns(ConvergenceWarning):
        model = sa['linear'].DeviceLogisticRegression(max_iter=2).fit(X, y)
    assert int(model.n_iter_[0]) == 2


# ----------------------------------------------------------------------------- 5. the predictor
def _ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize('table', ['tiled', 'num32', 'compact'])
def test_predict_blocks(sa, table):
    lin, names, n = sa['linear'], SETS['xg46'], N_MAX
    blocks = _blocks(sa, n, num32=table == 'num32')
    rows = slice(0, n)
    if table == 'compact':
        rows = np.random.default_rng(4).integers(0, n, 1500)
        blocks = sa['ops'].select_rows(blocks, _dev(rows))
    X = _matrix(names, rows, f32=table == 'num32')
    model = lin.DeviceLogisticRegression()
    model.feature_names_in_ = np.array(names, dtype=object)
    for beta in (_tail_beta(X), np.zeros(len(names) + 1)):
        model.coef_, model.intercept_ = beta[:-1].reshape(1, -1), beta[-1:]
        want = lr.sigmoid_of(X, beta)
        p64 = model.predict_blocks(blocks).cpu().numpy()
        p32 = model.predict_blocks(blocks, dtype=torch.float32).cpu().numpy()
        assert p64.dtype == np.float64 and p32.dtype == np.float32 and len(p64) == len(p32) == len(X)
        if not beta.any():
            assert (p64 == 0.5).all() and (p32 == 0.5).all()
            continue
        assert want.min() < 1e-6 and want.max() > 1 - 1e-6
        assert _ulps(p64, want).max() <= 4
        assert _ulps(p32, want.astype(np.float32)).max() <= 4


# ----------------------------------------------------------------------------- 6. the kernel's flags
def test_nonfinite_features_raise_from_the_kernels_flag(sa):
    lin, ops, names, n = sa['linear'], sa['ops'], SETS['num_only'], 129
    base = _blocks(sa, n)
    y = _dev(Y[:n])
    rows = np.array([r for r in range(n) if r not in (70, 100)])
    good = lin.DeviceLogisticRegression().fit_blocks(base, y, rows=_dev(rows), columns=names)
    for value in (float('nan'), float('inf'), float('-inf')):
        for row in (70, 100):  # tile 4 of 16 rows, offset 6; tile 6, offset 4
            f = base.f64_block.clone()
            f[row // 16, 4, row % 16] = value  # f4 is one of the model's columns
            blocks = ops.FeatureBlocks(base.plan, n, 1024, base.Rn, None, f, base.i64_block, base.bool_bits)
            with pytest.raises(ValueError, match='NaN or infinity'):
                lin.DeviceLogisticRegression().fit_blocks(blocks, y, columns=names)
            with pytest.raises(ValueError, match='NaN or infinity'):
                lin.DeviceLogisticRegression().fit_blocks(blocks, y, rows=_dev(np.append(rows, row)), columns=names)
            # the same value in a row outside the mask is never looked at
            masked = lin.DeviceLogisticRegression().fit_blocks(blocks, y, rows=_dev(rows), columns=names)
            assert masked.coef_.tobytes() == good.coef_.tobytes()
            # a column the model does not read may hold anything
            lin.DeviceLogisticRegression().fit_blocks(blocks, y, columns=['f0', 'i1'])
    with pytest.raises(ValueError, match='only one class'):
        lin.DeviceLogisticRegression().fit_blocks(base, torch.ones(n, dtype=torch.uint8, device='cuda'), columns=names)
    with pytest.raises(ValueError, match='only one class'):
        lin.DeviceLogisticRegression().fit_blocks(base, y, rows=_dev(np.flatnonzero(Y[:n] == 0)), columns=names)


# ----------------------------------------------------------------------------- 7. expected goals
@pytest.fixture(scope='module')
def games(sa):
    """The six synthetic games of tests/test_gpu_xg.py."""
    syn = sa['synthetic']
    d = syn.spadl_games(6, seed=3)
    return syn.games_frame(d), syn.to_frame(d)


def test_expected_goals_logistic_learner(sa, games):
    xg, lin, metrics = sa['xg'], sa['linear'], sa['metrics']
    games_df, actions = games
    model = xg.ExpectedGoals().fit_batch(games_df, actions, learner='logistic')
    shots = xg.get_shots(games_df, actions, xfns=xg.XFNS, nb_prev_actions=xg.NB_PREV_ACTIONS)
    names = xg.feature_names()
    assert len(names) == 46 and model.feature_names_in_ == names
    frame = shots[names]
    labels = (actions['result_id'].to_numpy() == xg.SUCCESS)[shots.index.to_numpy()].astype(np.uint8)
    assert 0 < labels.sum() < len(labels)
    host = lin.DeviceLogisticRegression().fit(frame, labels)
    assert isinstance(model.model_, lin.DeviceLogisticRegression)
    assert model.model_.coef_.tobytes() == host.coef_.tobytes()
    assert model.model_.intercept_.tobytes() == host.intercept_.tobytes()
    assert list(host.feature_names_in_) == names and np.abs(host.coef_).max() > 0
    # the fit is the optimum of the shots' objective
    X = frame.to_numpy(dtype=np.float64)
    beta = np.append(host.coef_[0], host.intercept_[0])
    g0 = np.abs(lr.objective_gradient(X, labels, np.zeros(len(beta)), 1.0)).max()
    assert np.abs(lr.objective_gradient(X, labels, beta, 1.0)).max() <= 2e-10 * max(1.0, g0)
    # rate, score
    proba = host.predict_proba(frame)[:, 1]
    rated = model.rate_batch(games_df, actions)
    assert rated['xg'].dtype == np.float32 and list(rated.index) == list(actions.index[shots.index.to_numpy()])
    assert _ulps(rated['xg'].to_numpy(), proba.astype(np.float32)).max() <= 4
    g = games_df.iloc[0]
    one = model.rate(g, actions[actions.game_id == g.game_id])
    assert one['xg'].to_numpy().tobytes() == rated['xg'].to_numpy()[:len(one)].tobytes()
    scores = model.score_batch(games_df, actions)
    want = metrics.binary_scores(_dev(labels), _dev(rated['xg'].to_numpy()))
    assert scores == want and scores['n'] == len(labels) and 0.5 < scores['auroc'] <= 1.0
    with pytest.raises(ValueError, match='no xgboost form'):
        model.to_xgboost_json()
    # held-out shots
    np.random.seed(5)
    held = xg.ExpectedGoals().fit_batch(games_df, actions, learner='logistic', val_size=0.25,
                                        linear_params=dict(C=0.5))
    assert held.device_eval_ is not None and 0 < held.device_eval_['n'] < len(labels)
    assert held.model_.C == 0.5 and held.model_.coef_.tobytes() != host.coef_.tobytes()
    with pytest.raises(ValueError, match='early_stopping_rounds'):
        xg.ExpectedGoals().fit_batch(games_df, actions, learner='logistic', val_size=0.25, early_stopping_rounds=3)
