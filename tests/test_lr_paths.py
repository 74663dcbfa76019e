"""Every kernel route of the STRUCTURED quasi-Newton update (B = lam0 I + W^T diag(mu - lam0) W, r explicit rows) against a
dense replay in the oracle: `lr_fused_step` of csrc/lrstep.hip (the one-call step, `sella_opt_step`) and
`lr_lowrank_update` of csrc/eigh.hip (`sella_update_h_lr`), at shapes chosen to land on each side of the thresholds where
they switch kernels — rows nr = r + 2 against LR_SMALL (128), the 128 x 128 GEMM tiles of W+ = Q^T E (nr >= 192), the
general `lr_pre` (nr > 256), the hand-back to the general route (nr > LR_DEV_MAX = 512); n against the 64 chunks of the
fused chain (n > 4096: unchained); the options lr_chain, gemm_mfma, lr_overlap; the view job of pinned coordinates.

The starting state is built directly — W from the QR of a random matrix, mu a chosen spectrum (negative values, a
cluster within 1e-10, values within 1e-9 of lam0, a spread of 1e-4 .. 1e3), B materialised from them on the device —
and ONE update is driven through the route under test.  The reference is the oracle's TS-BFGS (`secant.update_H`) on
that B.  Compared: the spectrum, the matrix rebuilt from (W, mu) (W itself is not unique for clustered mu), W W^T = I,
the order of mu, the rank bound of include/sella_hip.h, and for the one-call step the trust radius, ratio and proposed
step against the oracle's restricted step on the updated matrix."""
import contextlib

import numpy as np
import pytest

import oracle.sella_oracle as orc
from oracle.sella_oracle.secant import update_H as oracle_update_H
from oracle.sella_oracle.stepsolve import get_restricted_step as oracle_restricted_step

LAM0 = 0.7
# one update on O(1e3)-scaled matrices: the update itself costs a few ulps of the scale; the spectrum and the rebuilt
# matrix are compared at 1e-12 x scale
TOL = 1e-12


@pytest.fixture(autouse=True)
def structured_everywhere():
    """Structured form from 96 degrees of freedom and up to 0.95 n explicit rows (emulation sizes reach high ranks)."""
    from sella_amd import linalg
    old = linalg.LR_MIN_DIM, linalg.LR_MAX_FRACTION
    linalg.LR_MIN_DIM, linalg.LR_MAX_FRACTION = 96, 0.95
    yield
    linalg.LR_MIN_DIM, linalg.LR_MAX_FRACTION = old


@pytest.fixture
def options(ctx):
    """`options(key, value)` sets an option for the rest of one test; what the context had comes back afterwards."""
    with contextlib.ExitStack() as stack:
        yield lambda key, value: stack.enter_context(ctx.options(**{key: value}))


# ---- the starting state -------------------------------------------------------------------------------------------
def _spectrum(r, rng):
    """r ascending eigenvalues: two negative ones, a cluster of three within 1e-10, three within 1e-9 of lam0, the rest
    log-uniform over 1e-4 .. 1e3."""
    special = [-2.5, -0.3, 1.3, 1.3 + 4e-11, 1.3 + 8e-11, LAM0 - 6e-10, LAM0 + 5e-10, LAM0 + 9e-10, 1e-4, 1e3]
    rest = np.exp(rng.uniform(np.log(1e-4), np.log(1e3), max(r - len(special), 0)))
    return np.sort(np.concatenate((special, rest))[:r])


def _structured(ctx, n, r, seed, capacity=None):
    """(H, W, mu, B0): an ApproximateHessian in structured form — r explicit rows W (QR of a random n x r matrix), mu from
    `_spectrum`, lam0 = LAM0, the dense B materialised from them by `sella_lr_materialize` — and B0 = that matrix."""
    from sella_amd.linalg import ApproximateHessian
    rng = np.random.RandomState(seed)
    W = np.linalg.qr(rng.normal(size=(n, r)))[0].T.copy()
    mu = _spectrum(r, rng)
    cap = capacity or r + 8
    Wpad = np.zeros((cap, n))
    Wpad[:r] = W
    mus = np.zeros(cap)
    mus[:r] = mu
    lr = dict(Wt=ctx.upload(Wpad), r=r, mu=mus, lam0=LAM0)
    B = ctx.zeros(n, n)
    ctx.lr_materialize(B, lr['Wt'], r, mus, LAM0)
    H = ApproximateHessian(n, n, B)
    H._lr = lr
    return H, W, mu, B.numpy()


def _secant(B0, n, seed, kind='generic', W=None):
    """(dx, dg): a secant pair for one update."""
    rng = np.random.RandomState(seed + 1000)
    dx = rng.normal(size=n)
    dx *= 0.3 / np.linalg.norm(dx)
    if kind == 'in_span':                      # dx inside span(W): the residual row of s is zero
        dx = W.T @ rng.normal(size=W.shape[0])
        dx *= 0.3 / np.linalg.norm(dx)
    elif kind.startswith('tiny'):
        dx *= {'tiny_above': 1.02e-8, 'tiny_below': 0.98e-8}[kind] / np.linalg.norm(dx)
    Bdx = B0 @ dx
    if kind == 'lam0':                         # dg = lam0 dx
        return dx, LAM0 * dx
    noise = rng.normal(size=n)
    return dx, Bdx + 0.05 * np.linalg.norm(Bdx) / np.linalg.norm(noise) * noise


# ---- the reference ------------------------------------------------------------------------------------------------
def _reference(B0, W, mu, S, Y):
    """TS-BFGS of the oracle on B0, with B0's eigendecomposition given in closed form (lam0 on the complement of span(W);
    an n x n eigh would dominate the run time at n = 6000 and add nothing).  Returns (B_ref, invariant basis): B_ref maps
    span(W^T, S, Y) into itself and acts as lam0 on its complement."""
    n, r = B0.shape[0], W.shape[0]
    vecs = np.linalg.qr(W.T, mode='complete')[0]
    vecs[:, :r] = W.T
    lams = np.concatenate((mu, np.full(n - r, LAM0)))
    B_ref = oracle_update_H(B0, S, Y, method='TS-BFGS', symm=2, lams=lams, vecs=vecs)
    return 0.5 * (B_ref + B_ref.T), np.linalg.qr(np.hstack((W.T, S.reshape(n, -1), Y.reshape(n, -1))))[0]


def _spectrum_of(B, basis, lam0):
    """All n eigenvalues of B from its invariant subspace `basis` and lam0 on the complement (ascending)."""
    w = np.linalg.eigvalsh(basis.T @ (B @ basis))
    return np.sort(np.concatenate((w, np.full(B.shape[0] - basis.shape[1], lam0))))


def _check_structured(lr, r_before, k, B_ref, basis, tol=TOL):
    """The structured form (lr) after the update against the dense reference B_ref."""
    n = B_ref.shape[0]
    r = lr['r']
    assert 0 <= r <= min(n, r_before + 4 * k), (r, r_before, k)          # include/sella_hip.h: r grows by <= 4k per call
    W = lr['Wt'].numpy()[:r]
    mu, lam0 = lr['mu'][:r], lr['lam0']
    assert np.all(np.diff(mu) >= 0)
    np.testing.assert_allclose(W @ W.T, np.eye(r), atol=tol * max(1.0, np.sqrt(r)))
    scale = np.abs(B_ref).max()
    Brec = (W.T * (mu - lam0)) @ W
    Brec[np.diag_indices(n)] += lam0
    np.testing.assert_allclose(Brec, B_ref, rtol=0, atol=tol * scale)
    got = np.sort(np.concatenate((mu, np.full(n - r, lam0))))
    # Hoffman-Wielandt: the sorted spectra of two symmetric matrices differ (2-norm over all n) by at most the Frobenius
    # norm of their difference — the bound the entrywise check above allows, without a factor of n on every eigenvalue
    dev = np.linalg.norm(got - _spectrum_of(B_ref, basis, lam0))
    assert dev <= np.linalg.norm(Brec - B_ref) + tol * scale, (dev, np.linalg.norm(Brec - B_ref))
    return W, mu


class _PES:
    """What the oracle's restricted step reads: no constraint displacement, the free space `U` (orthonormal columns)."""
    int = None
    n_cell_dof = 0

    def __init__(self, B, g, U):
        self.B, self.g, self.U = B, g, U

    def get_g(self):
        return self.g.copy()

    def get_scons(self):
        return np.zeros(len(self.g))

    def get_H(self):
        return self.B

    def get_Unred(self):
        return np.eye(len(self.g))

    def get_Ufree(self):
        return self.U

    def get_HL_projected(self, U):
        return orc.QuasiNewtonHessian(U.shape[1], 0, U.T @ (self.B @ U))


def _oracle_step(B, g, U, order, delta, rs, method):
    """The oracle's restricted step on B with free space U.  U may be any orthonormal basis of a B-invariant subspace that
    holds the (projected) gradient plus `order` + 1 directions of the lam0 cluster: the step families then see the same
    modes with a gradient component, and the same ordering of the lowest ones, as on the whole space."""
    return oracle_restricted_step(rs)(_PES(B, g, U), order, delta, method).get_s()


def _free_basis(invariant, g, extra, seed):
    """Orthonormal basis of span(invariant, g) + `extra` random directions orthogonal to it (all invariant under B)."""
    n = invariant.shape[0]
    R = np.random.RandomState(seed).normal(size=(n, extra))
    return np.linalg.qr(np.hstack((invariant, g[:, None], R)))[0]


# ---- the one-call step --------------------------------------------------------------------------------------------
STEP = dict(delta_min=1e-4, sigma_inc=1.15, sigma_dec=0.65, rho_inc=1.035, rho_dec=5.0)
FAMILY = {'prfo': (2, 1, 1e-15), 'rfo': (1, 0, 1e-15), 'qn': (0, 0, 1e-10)}       # kind, order, tolerance


def _radius(delta, smag, ratio):
    """optimize.py:413-434."""
    if not (1.0 / STEP['rho_dec'] <= ratio <= STEP['rho_dec']):
        return max(smag * STEP['sigma_dec'], STEP['delta_min'])
    if 1.0 / STEP['rho_inc'] < ratio < STEP['rho_inc']:
        return max(STEP['sigma_inc'] * smag, delta)
    return delta


def _block(n, H, dx, g_old, g_new, f_new, method, rs, view=None):
    from sella_amd.device import CONSTRAINT_KINDS, OptStep
    blk = OptStep(n)
    blk.set_hessian(H._B_gpu, H._lr, 'TS-BFGS', 2, view)
    c = blk.c
    c.flags = blk.LEARN | blk.PROPOSE
    blk.point('dx', np.ascontiguousarray(dx))
    blk.point('g_old', np.ascontiguousarray(g_old))
    blk.point('g_new', np.ascontiguousarray(g_new))
    c.f_old, c.f_new = 0.0, float(f_new)
    c.smag = c.delta = 0.3                                  # the step taken ended on the trust boundary
    c.rho = 1.0
    for key, value in STEP.items():
        setattr(c, key, value)
    c.stepper_kind, c.order, c.tol = FAMILY[method]
    c.cons, c.maxiter = CONSTRAINT_KINDS[rs], 1000
    return blk


def _view_form(ctx, W, mu, B0, idx, capacity, restrict=False):
    """(Bsub DeviceMatrix, lr_sub): the principal submatrix B0[idx][idx] with a structured form of its own — from
    `sella_lr_restrict`, or built here from the QR of W[:, idx]^T and the eigenpairs of the r x r core."""
    m = len(idx)
    Bsub = ctx.upload(np.ascontiguousarray(B0[np.ix_(idx, idx)]))
    if restrict:
        lr = dict(Wt=ctx.upload(np.vstack((W, np.zeros((4, W.shape[1]))))), r=W.shape[0],
                  mu=np.concatenate((mu, np.zeros(4))), lam0=LAM0)
        return Bsub, ctx.lr_restrict(lr, idx, capacity)
    Q, R = np.linalg.qr(W[:, idx].T)
    w, V = np.linalg.eigh((R * (mu - LAM0)) @ R.T)
    rs = len(w)
    Wpad = np.zeros((capacity, m))
    Wpad[:rs] = (Q @ V).T
    mus = np.zeros(capacity)
    mus[:rs] = LAM0 + w
    return Bsub, dict(Wt=ctx.upload(Wpad), r=rs, mu=mus, lam0=LAM0)


def _device_case(ctx, n, r, seed, method='prfo', rs='tr', kind='generic', m=None, restrict=False):
    """One `sella_opt_step` (LEARN | PROPOSE) from a chosen structured state; returns everything a check needs."""
    H, W, mu, B0 = _structured(ctx, n, r, seed)
    dx, dg = _secant(B0, n, seed, kind, W)
    rng = np.random.RandomState(seed + 7)
    g_old = rng.normal(size=n)
    g_new = g_old + dg
    dg = g_new - g_old                                       # the pair the library forms (y = g_new - g_old, rounded)
    predicted = g_old @ dx + 0.5 * dx @ (B0 @ dx)
    f_new = 1.01 * predicted
    view, idx, r_sub0 = None, None, None
    if m is not None:
        idx = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int32)
        Bsub, lrs = _view_form(ctx, W, mu, B0, idx, min(m, r + 8), restrict)
        view = (Bsub, idx, lrs)
        r_sub0 = lrs['r']
    blk = _block(n, H, dx, g_old, g_new, f_new, method, rs, view)
    ctx.opt_step(blk)
    ctx.sync()
    out = dict(blk=blk, H=H, W=W, mu=mu, B0=B0, dx=dx, dg=dg, g_new=g_new, predicted=predicted, f_new=f_new,
               view=view, idx=idx, r0=r, r_sub0=r_sub0)
    out['s'], out['Wt'] = blk.s.copy(), H._lr['Wt'].numpy()
    out['mu_new'] = H._lr['mu'].copy()
    if view is not None:
        out['Wt_sub'], out['mu_sub'] = view[2]['Wt'].numpy(), view[2]['mu'].copy()
    return out


def _check_device(ctx, case, method, rs, route):
    """The update, the trust radius and the proposed step of one `_device_case` against the oracle.  `route`: 'coord' (the
    coordinate kernels of lrstep.hip ran: the dense mirror is left stale) or 'general' (sella_update_h_lr)."""
    blk, H = case['blk'], case['H']
    c = blk.c
    assert c.updated == 1
    assert c.B_stale == (1 if route == 'coord' else 0), (c.B_stale, route)
    n = case['B0'].shape[0]
    B_ref, basis = _reference(case['B0'], case['W'], case['mu'], case['dx'], case['dg'])
    H._lr['r'] = blk.r
    _check_structured(H._lr, case['r0'], 1, B_ref, basis)
    # the model prediction, the ratio and the radius (optimize.py:413-434)
    assert c.df_pred == pytest.approx(case['predicted'], rel=1e-12)
    assert c.ratio_valid == 1 and c.ratio == pytest.approx(1.01, rel=1e-12)
    delta = _radius(0.3, 0.3, case['f_new'] / case['predicted'])
    assert c.delta == pytest.approx(delta, rel=1e-14) and c.rho == pytest.approx(1.01, rel=1e-12)
    # the proposed step at the new point
    order = FAMILY[method][1]
    if case['view'] is None:
        U = _free_basis(basis, case['g_new'], order + 1, 5)
    else:
        idx = case['idx']
        Bsub, _, lrs = case['view']
        lrs['r'] = blk.r_sub
        sub_ref = B_ref[np.ix_(idx, idx)]
        sub_basis = np.linalg.qr(np.hstack((case['W'][:, idx].T, case['dx'][idx, None], case['dg'][idx, None])))[0]
        _check_structured(lrs, case['r_sub0'], 1, sub_ref, sub_basis)
        if c.Bsub_stale == 0:                               # (general route: the view's dense matrix is updated too)
            np.testing.assert_allclose(Bsub.numpy(), sub_ref, rtol=0, atol=TOL * np.abs(sub_ref).max())
        Usub = _free_basis(sub_basis, case['g_new'][idx], order + 1, 5)
        Wsub = np.zeros((n, Usub.shape[1]))
        Wsub[idx] = Usub
        U = Wsub
    s_ref, smag_ref = _oracle_step(B_ref, case['g_new'], U, order, delta, rs, method)
    # the root of |s(alpha)| = delta is found to the family's tolerance (1e-10 for qn, 1e-15 otherwise) by two different
    # schedules (batched trial alphas on the device, Newton / bisection in the oracle)
    tol = 1e-9 if method == 'qn' else 1e-11
    np.testing.assert_allclose(case['s'], s_ref, rtol=0, atol=tol * max(1.0, np.abs(s_ref).max()))
    assert c.smag_out == pytest.approx(smag_ref, rel=tol)


def _same_bits(a, b):
    np.testing.assert_array_equal(a['s'], b['s'])
    np.testing.assert_array_equal(a['Wt'], b['Wt'])
    np.testing.assert_array_equal(a['mu_new'], b['mu_new'])
    assert a['blk'].r == b['blk'].r and a['blk'].c.delta == b['blk'].c.delta
    if a['view'] is not None:
        np.testing.assert_array_equal(a['Wt_sub'], b['Wt_sub'])
        np.testing.assert_array_equal(a['mu_sub'], b['mu_sub'])


def _run_device(ctx, n, r, seed, method='prfo', rs='tr', kind='generic', m=None, restrict=False, route=None):
    """Run a device case, check it against the oracle, and (on the device) run it again: the same bits."""
    if route is None:
        route = 'coord' if r + 2 <= 512 and (m is None or min(r, m) + 2 <= 512) else 'general'
    a = _device_case(ctx, n, r, seed, method, rs, kind, m, restrict)
    _check_device(ctx, a, method, rs, route)
    if ctx.backend == 'hip':
        _same_bits(a, _device_case(ctx, n, r, seed, method, rs, kind, m, restrict))
    return a


def _heavy(*cases):
    return [pytest.param(*c, marks=pytest.mark.emu_heavy) for c in cases]


# rows nr = r + 2: merged coordinate kernels up to LR_SMALL = 128; the W+ GEMM on 128 x 128 tiles from nr = 192; the
# general lr_pre above 256; the coordinate route up to LR_DEV_MAX = 512, then the general route (sella_update_h_lr)
@pytest.mark.parametrize('n,nr', [(300, 127), (300, 128), (300, 129)] + _heavy(
    (300, 191), (300, 192), (300, 193), (300, 255), (300, 256), (300, 257), (1000, 512), (1000, 513), (1000, 514)))
@pytest.mark.parametrize('chain', [1, 0])
def test_device_route_rows(ctx, options, n, nr, chain):
    options('lr_chain', chain)
    _run_device(ctx, n, nr - 2, 11 + nr, 'prfo', 'tr')


# n: the fused chain covers up to 64 chunks of 64 (n <= 4096); from 4104 on the update is unchained
@pytest.mark.parametrize('n,nr,method,rs', _heavy(
    (1000, 200, 'prfo', 'tr'), (3072, 130, 'rfo', 'ras'), (4096, 127, 'prfo', 'tr'), (4096, 300, 'prfo', 'tr'),
    (4104, 127, 'prfo', 'ras'), (4104, 300, 'qn', 'tr'), (6003, 200, 'prfo', 'ras'), (6003, 514, 'prfo', 'tr')))
def test_device_route_sizes(ctx, n, nr, method, rs):
    _run_device(ctx, n, nr - 2, 3 + n + nr, method, rs)


@pytest.mark.parametrize('mfma,tile', [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize('nr', [129, pytest.param(200, marks=pytest.mark.emu_heavy)])
def test_device_route_gemm_options(ctx, options, mfma, tile, nr):
    """W+ = Q^T E on the 128 x 128 MFMA tiles, the 64 x 64 MFMA tiles and the VALU tiles: the same update."""
    options('gemm_mfma', mfma)
    options('gemm_tile128', tile)
    _run_device(ctx, 300, nr - 2, 5 + nr, 'prfo', 'tr')


@pytest.mark.parametrize('method,rs', [('prfo', 'tr'), ('rfo', 'ras'), ('qn', 'tr'), ('qn', 'ras')])
def test_device_route_families(ctx, method, rs):
    _run_device(ctx, 300, 60, 17, method, rs)


@pytest.mark.parametrize('kind', ['in_span', 'lam0', 'tiny_above'])
@pytest.mark.parametrize('chain', [1, 0])
def test_device_route_edge_pairs(ctx, options, kind, chain):
    """dx inside span(W) (zero residual row), dg = lam0 dx (no curvature information outside the cluster), |dx| just
    above the 1e-8 below which the update is skipped."""
    options('lr_chain', chain)
    _run_device(ctx, 300, 40, 23, 'prfo', 'tr', kind)


def test_device_route_skips_a_tiny_step(ctx):
    """|dx| just below 1e-8: B, W and mu are left alone (hessian_update.py:48-49); the step is still proposed."""
    case = _device_case(ctx, 300, 40, 29, 'prfo', 'tr', 'tiny_below')
    c = case['blk'].c
    assert c.updated == 0 and c.B_stale == 0 and case['blk'].r == 40
    np.testing.assert_array_equal(case['mu_new'][:40], case['mu'])
    np.testing.assert_array_equal(case['Wt'][:40], case['W'])
    B0 = case['B0']
    U = _free_basis(np.linalg.qr(case['W'].T)[0], case['g_new'], 2, 5)
    s_ref, _ = _oracle_step(B0, case['g_new'], U, 1, c.delta, 'tr', 'prfo')
    np.testing.assert_allclose(case['s'], s_ref, rtol=0, atol=1e-11 * max(1.0, np.abs(s_ref).max()))


def test_device_route_repeated_pair_deflates(ctx, options):
    """The same pair twice: after the first update B dx = dg holds, so the second one changes nothing but roundoff and
    every new direction deflates."""
    H, W, mu, B0 = _structured(ctx, 300, 50, 31)
    dx, dg = _secant(B0, 300, 31)
    g = np.random.RandomState(3).normal(size=300)
    B_ref, basis = _reference(B0, W, mu, dx, dg)
    for _ in range(2):
        blk = _block(300, H, dx, g, g + dg, 0.5, 'prfo', 'tr')
        ctx.opt_step(blk)
        assert blk.c.updated == 1 and blk.c.B_stale == 1
        H._lr['r'] = blk.r
    _check_structured(H._lr, 50, 2, B_ref, basis)
    assert blk.r <= 52


def test_device_route_new_eigenvalue_on_an_old_one(ctx):
    """A pair that places a new eigenvalue exactly on an existing mu: dx along a new direction, dg = mu_j dx."""
    H, W, mu, B0 = _structured(ctx, 300, 50, 37)
    rng = np.random.RandomState(37)
    dx = rng.normal(size=300)
    dx -= W.T @ (W @ dx)
    dx *= 0.3 / np.linalg.norm(dx)
    dg = mu[20] * dx
    g = rng.normal(size=300)
    blk = _block(300, H, dx, g, g + dg, 0.5, 'prfo', 'tr')
    ctx.opt_step(blk)
    assert blk.c.updated == 1 and blk.c.B_stale == 1
    H._lr['r'] = blk.r
    B_ref, basis = _reference(B0, W, mu, dx, dg)
    _, mu_new = _check_structured(H._lr, 50, 1, B_ref, basis)
    assert np.sum(np.abs(mu_new - mu[20]) <= 1e-12 * 1e3) >= 2


# ---- the view job (pinned coordinates) ----------------------------------------------------------------------------
@pytest.mark.parametrize('m,nr', [(200, 60), (240, 129)] + _heavy((600, 192), (600, 257), (700, 512), (700, 514)))
@pytest.mark.parametrize('chain', [1, 0])
def test_device_route_views(ctx, options, m, nr, chain):
    """The view B[idx][idx] with a structured form of its own: `vfused` (lr_chain = 1) and the gather route (0)."""
    options('lr_chain', chain)
    n = 300 if m <= 300 else 1000
    _run_device(ctx, n, nr - 2, 41 + m + nr, 'prfo', 'ras' if n % 3 == 0 else 'tr', m=m)


@pytest.mark.parametrize('r', [100, pytest.param(300, marks=pytest.mark.emu_heavy)])
def test_device_route_view_from_restrict(ctx, r):
    """The view's structured form from `sella_lr_restrict` (what `register_view` does up to r = 256) and, above that
    rank, from the eigenpairs of the restricted core (register_view leaves the view dense there)."""
    n = 300 if r <= 120 else 1000
    _run_device(ctx, n, r, 43 + r, 'prfo', 'tr', m=n - 60, restrict=r <= 256)


def test_register_view_restricts_up_to_256(ctx):
    from sella_amd.linalg import ApproximateHessian
    from sella_amd.utilities.math import register_selection
    n = 300
    free = np.arange(20, n)
    U = register_selection(np.ascontiguousarray(np.eye(n)[:, free]), free)
    H, W, mu, B0 = _structured(ctx, n, 120, 47)
    sub = ApproximateHessian(len(free), 0, ctx.upload(B0[np.ix_(free, free)]))
    H.register_view(U, sub)
    lrs = sub.device_eig_lr()
    assert lrs is not None and lrs['r'] == 120
    Ws = lrs['Wt'].numpy()[:120]
    Bs = (Ws.T * (lrs['mu'][:120] - LAM0)) @ Ws + LAM0 * np.eye(len(free))
    np.testing.assert_allclose(Bs, B0[np.ix_(free, free)], rtol=0, atol=TOL * 1e3)


@pytest.mark.parametrize('nr', [130, pytest.param(200, marks=pytest.mark.emu_heavy)])
def test_overlap_is_bit_identical_to_serial(ctx, options, nr):
    """lr_overlap = 1 (the view job on a second stream) against 0: the same bits — at nr >= 192 the W+ product takes
    the 128 x 128 tiles, a plain launch that must follow the coordinate kernels of its own job."""
    out = {}
    for flag in (0, 1):
        options('lr_overlap', flag)
        out[flag] = _device_case(ctx, 600 if nr > 130 else 300, nr - 2, 53, 'prfo', 'tr', m=240 if nr <= 130 else 500)
        assert out[flag]['blk'].c.B_stale == 1
    _same_bits(out[0], out[1])
    _check_device(ctx, out[1], 'prfo', 'tr', 'coord')


# ---- the host-planned route (sella_update_h_lr) -------------------------------------------------------------------
def _host_case(ctx, n, r, k, seed, deficient=False):
    H, W, mu, B0 = _structured(ctx, n, r, seed, capacity=r + 4 * k + 8)
    rng = np.random.RandomState(seed)
    if deficient:
        # the secant pairs of a Krylov run: S an orthonormal basis of span(x, A x, ..., A^(k-1) x) and Y = A S, so the 2k
        # update vectors (combinations of S and Y) span only k + 1 dimensions
        Z = np.linalg.qr(rng.normal(size=(n, n)))[0]
        A = (Z * np.exp(rng.uniform(np.log(0.5), np.log(7.0), n))) @ Z.T
        S = np.empty((n, k))
        S[:, 0] = rng.normal(size=n)
        for j in range(1, k):
            S[:, j] = A @ S[:, j - 1]
        S = 0.3 * np.linalg.qr(S)[0]
        Y = A @ S
    else:
        S = 0.3 * rng.normal(size=(n, k)) / np.sqrt(n)
        Y = B0 @ S + 0.05 * rng.normal(size=(n, k)) * np.linalg.norm(B0 @ S, axis=0) / np.sqrt(n)
    return H, W, mu, B0, S, Y


@pytest.mark.parametrize('k', [1, 3, 4, pytest.param(32, marks=pytest.mark.emu_heavy)])
def test_host_route_blocks(ctx, k):
    """k = 1 (pair terms), k = 3 (vector Gram-Schmidt), k >= 4 (2k >= 8: the Cholesky-QR block), k = 32 (the largest
    block)."""
    n, r = 300, 100
    H, W, mu, B0, S, Y = _host_case(ctx, n, r, k, 59 + k)
    ctx.update_h_lr(H._B_gpu, S, Y, H._lr)
    B_ref, basis = _reference(B0, W, mu, S, Y)
    _check_structured(H._lr, r, k, B_ref, basis)
    np.testing.assert_allclose(H._B_gpu.numpy(), B_ref, rtol=0, atol=TOL * np.abs(B_ref).max())


def test_host_route_rank_deficient_block(ctx):
    n, r, k = 300, 60, 6
    H, W, mu, B0, S, Y = _host_case(ctx, n, r, k, 61, deficient=True)
    ctx.update_h_lr(H._B_gpu, S, Y, H._lr)
    B_ref, basis = _reference(B0, W, mu, S, Y)
    _check_structured(H._lr, r, k, B_ref, basis)


@pytest.mark.emu_heavy
def test_host_route_33_pairs_in_two_blocks(ctx):
    """lr_lowrank_update takes at most 32 pairs per call (it refuses more); the update splits 33 into 32 + 1."""
    n, r = 300, 20
    H, W, mu, B0, S, Y = _host_case(ctx, n, r, 33, 67)
    ctx.update_h_lr(H._B_gpu, S, Y, H._lr)
    B_ref, basis = _reference(B0, W, mu, S, Y)
    _check_structured(H._lr, r, 33, B_ref, basis)


def test_host_route_capacity_growth(ctx):
    """`ApproximateHessian.update` grows the panel when the rank passes its capacity: the same update."""
    n, r = 300, 100
    H, W, mu, B0 = _structured(ctx, n, r, 71, capacity=r + 2)
    rng = np.random.RandomState(71)
    S = 0.1 * rng.normal(size=(n, 4)) / np.sqrt(n)
    Y = B0 @ S + 0.01 * rng.normal(size=(n, 4))
    H.update(S, Y)
    assert H._lr is not None and H._lr['Wt'].shape[0] >= H._lr['r'] > r + 2
    B_ref, basis = _reference(B0, W, mu, S, Y)
    _check_structured(H._lr, r, 4, B_ref, basis)


# ---- the dense mirror and the step families on a structured form --------------------------------------------------
@pytest.mark.parametrize('r', [130, pytest.param(300, marks=pytest.mark.emu_heavy),
                               pytest.param(510, marks=pytest.mark.emu_heavy)])
def test_materialize_and_stepper_against_dense(ctx, r):
    from oracle.sella_oracle.stepsolve import get_stepper as oracle_stepper
    from sella_amd.optimize.stepper import get_stepper
    n = 300 if r < 300 else 1000
    H, W, mu, B0 = _structured(ctx, n, r, 73 + r)
    Bd = (W.T * (mu - LAM0)) @ W
    Bd[np.diag_indices(n)] += LAM0
    np.testing.assert_allclose(B0, Bd, rtol=0, atol=TOL * 1e3)
    np.testing.assert_array_equal(B0, B0.T)
    g = np.random.RandomState(r).normal(size=n)
    dense = orc.QuasiNewtonHessian(n, 0, Bd)
    for kind, order in (('qn', 1), ('rfo', 0), ('prfo', 1)):
        st_lr = get_stepper(kind)(g, H, order)
        st_de = oracle_stepper(kind)(g, dense, order)
        # (the tolerances of test_lr_eig.py: eigenvalues of 1e-4 beside a scale of 1e3 leave LAPACK's eigenvectors
        # good to ~1e-10 relative, and ds/dalpha ~ g / lambda^2 magnifies that)
        for alpha in ((0.0 if kind == 'qn' else 1e-3), 0.3, 1.0):
            s1, d1 = st_lr.get_s(alpha)
            s0, d0 = st_de.get_s(alpha)
            np.testing.assert_allclose(s1, s0, rtol=0, atol=1e-9 * max(1.0, np.abs(s0).max()), err_msg=f'{kind} {alpha}')
            np.testing.assert_allclose(d1, d0, rtol=0, atol=1e-8 * max(1.0, np.abs(d0).max()), err_msg=f'{kind} {alpha}')
