"""The secular root finders behind every optimizer step (`bordered_root_core`, csrc/bordered.h) against a 60-digit
reference (tests/secular_reference.py) on the spectra real runs start from or pass through: coincident poles (the scaled
identity every run starts with), clusters at the edge of a P-RFO block, weights that vanish or underflow, gradients at
convergence, alpha deep in a root search, the true hard case.

  host path      `DeviceStepper.get_s` (rfo_block / eval_hat, csrc/stepper.hip), both backends
  batched path   `rs_batch_kernel` through `restricted_step(rs_batch=1)` in its three size regimes; the final step is
                 re-evaluated on the host, so the kernel shows through the SEQUENCE of trial alphas it steers

`dsda` is NOT the derivative of `s`: the reference implementation's formula (stepper.py:142-156) divides by
L_j - L_o where perturbation theory has L_o - L_j, and the library reproduces the reference (g7 golden parity).  It is
therefore only checked for finiteness and, where no pole and no eigenvalue is within 1e-9 of the selected root, against
the oracle's own `get_s`; closer than that both sides are the reference's 1e-12 clamps.
"""
import numpy as np
import pytest

import oracle.sella_oracle.stepsolve as orc_step
import secular_reference as sr

M = 40
ALPHAS = (1e-13, 1e-6, 1e-2, 1.0)
# (kind, order); the last one follows an INTERIOR root and takes the distinct-pole cases only
FAMILIES = [('qn', 1), ('rfo', 0), ('prfo', 1), ('prfo', 3), ('rfo', 1)]
FAMILY_IDS = ['qn1', 'rfo0', 'prfo1', 'prfo3', 'rfo1_interior']

# V = I: componentwise.  Worst measured, the same on both backends (it is host code): 2.6e-15 in the true hard case
# (lam = -0.8 with a weight of 1e-9 at alpha = 0.01, where the step is a quotient of two rounded tiny numbers), 1.2e-15
# elsewhere.
TOL_IDENTITY = 4e-15
# V = I - 2 u u^T (dense), normwise against max |s_ref|: ten times the worst error measured against the reference at
# m = 40, because the two products with V add m eps.  Measured: 1.40e-15 on both backends (interior root, g x 1e6,
# alpha = 1; 9.5e-16 on the exterior roots).  The batched searches at m = 42 / 1101 / 2100 end within 7.1e-16 /
# 2.5e-15 / 3.4e-15 of the reference on the device: inside the same bound.
REFLECTOR_MEASURED = 1.40e-15
TOL_REFLECTOR = 10 * REFLECTOR_MEASURED
# structured families, n = 96: measured 1.34e-15 on the device, 1.15e-15 on the emulator (r = 5, RFO, alpha = 1)
LR_MEASURED = 1.34e-15
TOL_LR = 10 * LR_MEASURED


def _spectrum(m, order, rng):
    """Ascending eigenvalues: log-uniform over 0.05 .. 50, the `order` lowest negative."""
    lam = np.sort(np.exp(rng.uniform(np.log(0.05), np.log(50.0), m)))
    lam[:order] = -np.linspace(1.5, 1.0, order)
    return lam


def hard_cases(kind, order, m=M):
    """[(name, lam, ghat)] in the eigenbasis.  `o` is the lower edge of the min block (P-RFO) / the selected root's
    upper neighbour (RFO)."""
    rng = np.random.RandomState(5)
    lam = _spectrum(m, order, rng)
    gh = 0.3 * rng.normal(size=m)
    small = 1e-3 * rng.normal(size=m)
    o = order
    interior = kind == 'rfo' and order > 0
    out = [('generic', lam, gh)]

    def add(name, lam_=None, gh_=None, **at):
        l2, g2 = (lam if lam_ is None else lam_).copy(), (gh if gh_ is None else gh_).copy()
        for key, (idx, val) in at.items():
            (l2 if key == 'lam' else g2)[idx] = val
        out.append((name, l2, g2))

    if not interior:
        add('scaled_identity', lam_=np.full(m, 70.0))
        add('four_equal_edge', lam=(slice(o, o + 4), lam[o]))
        add('edge_weight_0', gh=(o, 0.0))                       # lam[o] > 0: the root lies outside the pole
    add('edge_pair_1ulp', lam=(o + 1, np.nextafter(lam[o], np.inf)))
    add('edge_weight_1e-17', gh=(o, 1e-17))
    if order > 0 and not interior:
        add('max_block_1e-9', gh=(slice(0, o), 1e-9))
        add('max_block_1e-170', gh=(slice(0, o), 1e-170))       # b^2 underflows
    add('g_1e-12', gh_=gh * 1e-12)
    add('g_1e6', gh_=gh * 1e6)
    add('lam_1e-8', lam_=lam * 1e-8)
    add('lam_1e8', lam_=lam * 1e8)
    if not interior:
        # the true hard case with a tiny weight: the step is 1e5 ... 1e13, the clamp applies at 1e-14 and alpha = 1
        add('hard_1e-9', gh_=small, lam=(o, -0.8), gh=(o, 1e-9))
        add('hard_1e-14', gh_=small, lam=(o, -0.8), gh=(o, 1e-14))
    return out


# the cases whose step does not hinge on a gradient component below the rounding of V^T g
REFLECTOR_CASES = ('generic', 'scaled_identity', 'four_equal_edge', 'edge_pair_1ulp', 'g_1e-12', 'g_1e6', 'lam_1e-8',
                   'lam_1e8')


def reflector(m, seed=3):
    u = np.random.RandomState(seed).normal(size=m)
    u /= np.linalg.norm(u)
    return np.eye(m) - 2.0 * np.outer(u, u)


@pytest.fixture(scope='module')
def identity(ctx):
    I = np.eye(M)
    return ctx.upload(I), ctx.upload(I)


@pytest.fixture(scope='module')
def mirror(ctx):
    Q = reflector(M)
    return Q, ctx.upload(Q), ctx.upload(Q.T.copy())


_ref_cache = {}


def _shat_ref(kind, order, name, lam, gh, alpha):
    key = (kind, order, name, alpha)
    if key not in _ref_cache:
        _ref_cache[key] = sr.shat_ref(kind, lam, gh, order, alpha)
    return _ref_cache[key]


@pytest.mark.parametrize('kind,order', FAMILIES, ids=FAMILY_IDS)
def test_host_path_identity_basis(ctx, identity, kind, order):
    """V = I: every component of the step to 4e-15 of the 60-digit value, `dsda` finite."""
    from sella_amd.device import DeviceStepper
    V, Vt = identity
    worst = (0.0, None)
    for name, lam, gh in hard_cases(kind, order):
        st = DeviceStepper(ctx, kind, V, Vt, lam, gh, order)
        for alpha in ALPHAS:
            s, dsda = st.get_s(alpha)
            ref = _shat_ref(kind, order, name, lam, gh, alpha)
            assert np.isfinite(s).all() and np.isfinite(dsda).all(), (name, alpha)
            err = np.abs(s - ref)
            nz = ref != 0.0
            rel = (err[nz] / np.abs(ref[nz])).max()
            worst = max(worst, (rel, (name, alpha)))
            assert (err <= TOL_IDENTITY * np.abs(ref)).all(), (name, alpha, rel)
    print(f'MEASURED identity {kind} order {order}: worst componentwise {worst[0]:.2e} at {worst[1]}')


def test_host_path_irc_family(ctx, identity):
    """The IRC quasi-Newton family (closed form, stepper.py:99-111) on the same inputs."""
    from sella_amd.device import DeviceStepper
    V, Vt = identity
    d1hat = 0.1 * np.random.RandomState(6).normal(size=M)
    for name, lam, gh in hard_cases('qn', 1):
        st = DeviceStepper(ctx, 'qn_irc', V, Vt, lam, gh, 0)
        st.set_d1hat(d1hat)
        for alpha in ALPHAS:
            s, dsda = st.get_s(alpha)
            ref = sr.shat_ref('qn_irc', lam, gh, 0, alpha, d1hat)
            assert np.isfinite(dsda).all(), (name, alpha)
            # (the numerator ghat + alpha d1hat may cancel: the bound is relative to its terms, two roundings each)
            size = (np.abs(gh) + alpha * np.abs(d1hat)) / (np.abs(lam) + alpha)
            assert (np.abs(s - ref) <= TOL_IDENTITY * size).all(), (name, alpha)


@pytest.mark.parametrize('kind,order', FAMILIES, ids=FAMILY_IDS)
def test_host_path_reflector_basis(ctx, mirror, kind, order):
    """V = I - 2 u u^T: the step through both products with a dense V, normwise against max |s_ref|.
    Measured worst (m = 40, both backends) REFLECTOR_MEASURED; the bound is ten times that."""
    from sella_amd.device import DeviceStepper
    Q, V, Vt = mirror
    worst = (0.0, None)
    for name, lam, gh in hard_cases(kind, order):
        if name not in REFLECTOR_CASES:
            continue
        g = Q @ gh
        st = DeviceStepper(ctx, kind, V, Vt, lam, g, order)
        for alpha in ALPHAS:
            s, dsda = st.get_s(alpha)
            ref = sr.step_ref(kind, Q, lam, g, order, alpha)
            assert np.isfinite(dsda).all(), (name, alpha)
            rel = np.abs(s - ref).max() / np.abs(ref).max()
            worst = max(worst, (rel, (name, alpha)))
            assert rel <= TOL_REFLECTOR, (name, alpha, rel)
    print(f'MEASURED reflector {kind} order {order}: worst normwise {worst[0]:.2e} at {worst[1]}')


class _EigH:
    """What the oracle's step families read from a Hessian, for H = diag(lam)."""

    def __init__(self, A):
        self.A = A
        self.evals, self.evecs = np.diag(A).copy(), np.eye(len(A))

    def asarray(self):
        return self.A

    def project(self, U):
        P = _EigH.__new__(_EigH)
        P.A, P.evals, P.evecs = U.T @ self.A @ U, None, None
        return P


def _separated(lam, gh, j, alpha):
    """No pole and no other eigenvalue of the scaled augmented matrix within 1e-9 of its eigenvalue j."""
    if len(lam) == 0:
        return True
    A = np.diag(np.append(alpha * alpha * lam, 0.0))
    A[-1, :-1] = A[:-1, -1] = alpha * gh
    L = np.linalg.eigvalsh(A)
    return min(np.abs(alpha * alpha * lam - L[j]).min(), np.abs(np.delete(L, j) - L[j]).min()) >= 1e-9


def _dsda_formula(kind, lam, gh, order, alpha):
    """The reference's dsda formula at 60 digits, or None where it does not apply (coincident poles, zero weights)."""
    try:
        if kind == 'rfo':
            return sr.dsda_formula_ref(lam, gh, order, alpha)
        if kind == 'prfo':
            return np.concatenate((sr.dsda_formula_ref(lam[:order], gh[:order], order, alpha),
                                   sr.dsda_formula_ref(lam[order:], gh[order:], 0, alpha)))
    except ValueError:
        pass
    return None


@pytest.mark.parametrize('kind,order', FAMILIES, ids=FAMILY_IDS)
def test_dsda_matches_the_oracle_where_separated(ctx, identity, kind, order):
    from sella_amd.device import DeviceStepper
    V, Vt = identity
    cls = {'qn': orc_step.QuasiNewtonStep, 'rfo': orc_step.RFOStep, 'prfo': orc_step.PRFOStep}[kind]
    compared, lost = 0, []
    for name, lam, gh in hard_cases(kind, order):
        if not np.isfinite(lam * lam).all() or np.abs(lam).max() > 1e6:
            continue                                # (the oracle's dense eigh of lam x 1e8 has no 1e-9 to offer)
        st = DeviceStepper(ctx, kind, V, Vt, lam, gh, order)
        ref = cls(gh.copy(), _EigH(np.diag(lam)), order)
        for alpha in ALPHAS:
            if kind == 'rfo' and not _separated(lam, gh, order, alpha):
                continue
            if kind == 'prfo' and not (_separated(lam[:order], gh[:order], order, alpha) and
                                       _separated(lam[order:], gh[order:], 0, alpha)):
                continue
            s, dsda = st.get_s(alpha)
            so, do = ref.get_s(alpha)
            tol = 1e-9 * np.abs(do).max()
            d60 = _dsda_formula(kind, lam, gh, order, alpha)
            # The oracle's dense float64 eigh has an ABSOLUTE eigenvector error and an arbitrary basis inside a cluster:
            # against the 60-digit evaluation of its own formula it is off by 2e-7 ... 2e-6 of max |dsda| with a
            # gradient of 1e-12 or 1e6 next to the curvatures, and by 4e-5 in one component with three coincident
            # poles in the max block.  Where it cannot deliver the tolerance, the 60-digit evaluation alone stands;
            # everywhere else both do.
            if d60 is None or np.abs(do - d60).max() <= tol:
                np.testing.assert_allclose(dsda, do, rtol=0, atol=tol, err_msg=f'{name} {alpha}')
                compared += 1
            else:
                lost.append((name, alpha))
            if d60 is not None:
                np.testing.assert_allclose(dsda, d60, rtol=0, atol=tol, err_msg=f'{name} {alpha} (60 digits)')
    print(f'MEASURED dsda {kind} order {order}: {compared} comparisons with the oracle; oracle short of 1e-9 at {lost}')
    assert compared >= 4 and len(lost) <= compared // 2


@pytest.mark.parametrize('kind,order', [('rfo', 0), ('prfo', 1), ('prfo', 3)], ids=['rfo0', 'prfo1', 'prfo3'])
@pytest.mark.parametrize('ncoincident', [1, 2])
def test_clamp_semantics_of_the_weightless_hard_case(ctx, identity, kind, order, ncoincident):
    """ghat = 0 on the softest mode(s) of the minimised block, below the root of the rest: that pole is the selected
    eigenvalue, its eigenvector a unit vector with last component 0, and the reference's clamp (stepper.py:134-137)
    makes the step alpha / 1e-12 along it — the FIRST of coincident poles.  Host path."""
    from sella_amd.device import DeviceStepper
    V, Vt = identity
    rng = np.random.RandomState(9)
    lam = _spectrum(M, order, rng)
    gh = 1e-3 * rng.normal(size=M)
    o = order
    lam[o:o + ncoincident] = -0.8
    gh[o:o + ncoincident] = 0.0
    st = DeviceStepper(ctx, kind, V, Vt, lam, gh, order)
    clamped = []
    for alpha in ALPHAS:
        s, dsda = st.get_s(alpha)
        try:
            ref = sr.shat_ref(kind, lam, gh, order, alpha)
        except sr.WeightlessPole:
            clamped.append(alpha)
            assert s[o] == alpha / 1e-12 and dsda[o] == 1.0 / 1e-12, (alpha, s[o], dsda[o])
            assert not s[o + 1:].any() and not dsda[o + 1:].any(), alpha
            if order:                                 # the max block is an ordinary problem
                np.testing.assert_allclose(s[:o], sr.rfo_block_ref(lam[:o], gh[:o], o, alpha), rtol=TOL_IDENTITY, atol=0)
        else:                                         # small alpha: the root of the rest lies below the pole
            assert (np.abs(s - ref) <= TOL_IDENTITY * np.abs(ref)).all() and np.isfinite(dsda).all(), alpha
    assert clamped == [1e-2, 1.0]
    if kind != 'rfo':
        return
    # the |shat|^2-only evaluation of the eigenbasis search (orthonormal trust region, bisection phase) agrees with
    # get_s: the search replayed on |get_s(alpha)| visits the same alphas and ends on the same step
    delta = 0.02
    s, val, alphas = st.restricted_step(cons='tr', delta=delta, alpha0=1.0, alphamin=0.0, alphamax=1.0, slope=1.0,
                                        newton_safe=False, tol=0.0, orthonormal=True)

    def measure(alpha):
        sa, da = st.get_s(alpha)
        v = np.linalg.norm(sa)
        return v, da @ sa / max(v, 1e-12)

    replay = _replay_search(measure, delta, 1.0, 0.0, 1.0, 1.0, False, 0.0)
    # (the measure jumps from alpha / 1e-12 to the ordinary step where the pole stops being the lowest eigenvalue:
    #  the search closes in on that alpha, every decision far from the radius)
    assert len(alphas) > 20 and abs(len(alphas) - len(replay)) <= 1
    k = min(len(alphas), len(replay)) - 2
    np.testing.assert_allclose(alphas[:k], replay[:k], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(s, st.get_s(alphas[-1])[0])
    assert val == delta


def _replay_search(measure, delta, alpha0, alphamin, alphamax, slope, newton_safe, tol, maxiter=1000):
    """The trial alphas of restricted_step.py:78-120 for a measure given as alpha -> (val, dval)."""
    alpha = alpha0
    trace = [alpha]
    val, dval = measure(alpha)
    if val < delta:
        return trace
    err, lower, upper = val - delta, alphamin, alphamax
    for niter in range(maxiter):
        if abs(err) <= tol or np.nextafter(lower, upper) >= upper:
            break
        if err * slope > 0:
            upper = alpha
        else:
            lower = alpha
        a1 = alpha - err / dval
        if np.isnan(a1) or a1 <= lower or a1 >= upper or (niter > 4 and not newton_safe):
            alpha = (lower + upper) / 2.0
        else:
            alpha = a1
        trace.append(alpha)
        val, dval = measure(alpha)
        err = val - delta
    return trace


# ---- structured families (`lr=` / sella_stepper_create_lr) -------------------------------------------------------------
LR_N = 96


def _lr_problem(ctx, r, gkind):
    from test_lr_paths import LAM0, _spectrum as lr_spectrum
    rng = np.random.RandomState(100 + r)
    mu = lr_spectrum(r, rng)
    if gkind == 'generic':
        W = np.linalg.qr(rng.normal(size=(LR_N, max(r, 1))))[0].T.copy()[:r]
        g = rng.normal(size=LR_N)
    else:
        # "inside span(W)" and "orthogonal to W" EXACTLY: rows of a 64 x 64 Hadamard matrix / 8 with signs flipped, on 64
        # of the n coordinates, and a gradient of multiples of 2^-10 — every product and partial sum is exact in
        # float64, in any order, so the weights that should vanish are zeros on both sides and not two different
        # roundings (which 1 / mu = 1e4 would turn into a difference of 1e-12)
        H = np.ones((1, 1))
        while len(H) < 64:
            H = np.block([[H, H], [H, -H]])
        W = np.zeros((r, LR_N))
        W[:, np.sort(rng.permutation(LR_N)[:64])] = H[rng.permutation(64)[:r]] * rng.choice([-1.0, 1.0], size=64) / 8.0
        raw = rng.randint(-2048, 2049, size=LR_N) / 1024.0
        inside = W.T @ (W @ raw)
        g = inside if gkind == 'in_span' else raw - inside
        assert not (W @ W.T - np.eye(r)).any()
        assert not (g - W.T @ (W @ g)).any() if gkind == 'in_span' else not (W @ g).any()
    cap = r + 8
    Wpad, mus = np.zeros((cap, LR_N)), np.zeros(cap)
    Wpad[:r], mus[:r] = W, mu
    lr = dict(Wt=ctx.upload(Wpad), r=r, mu=mus, lam0=LAM0)
    # the equivalent dense problem: the explicit modes, ONE weighted mode of the cluster (the normalised component of g
    # outside span(W)) first within the cluster, and its other n - r - 1 modes without weight (columns of zeros: they
    # carry no step)
    gp = g - W.T @ (W @ g)
    gp = gp - W.T @ (W @ gp)
    col = gp / np.linalg.norm(gp) if np.linalg.norm(gp) > 1e-13 * np.linalg.norm(g) else np.zeros(LR_N)
    nlow = int((mu < LAM0).sum())
    lam_d = np.concatenate((mu[:nlow], np.full(LR_N - r, LAM0), mu[nlow:]))
    V_d = np.zeros((LR_N, LR_N))
    V_d[:, :nlow] = W[:nlow].T
    V_d[:, nlow] = col
    V_d[:, nlow + LR_N - r:] = W[nlow:].T
    return lr, g, lam_d, V_d, nlow


@pytest.mark.parametrize('r', [0, 5, 40])
def test_structured_families_match_the_dense_problem(ctx, r):
    """`sella_stepper_create_lr` compresses the cluster of lam0 into one weighted mode plus weightless copies; the step
    must be that of the dense problem with all n modes, also where `order` exceeds the number of explicit modes below
    lam0 and the copies enter the max block.  Normwise against max |s_ref|; measured worst LR_MEASURED, bound ten times.
    (g inside span(W) and g orthogonal to W stay with order <= 1: with the order beyond the negative modes a mode
    WITHOUT weight would be maximised along, which is the clamp of the weightless hard case, not a step to compare.)"""
    from sella_amd.device import DeviceStepper
    worst = (0.0, None)
    compared = 0
    for gkind in (('generic',) if r == 0 else ('generic', 'in_span', 'orthogonal')):
        lr, g, lam_d, V_d, nlow = _lr_problem(ctx, r, gkind)
        orders = (0, 1, 3) if gkind == 'generic' else (0, 1)
        if gkind == 'generic':
            assert max(orders) > nlow or r == 40
        for order in orders:
            for kind in (('qn', 'rfo') if order == 0 else ('qn', 'prfo')):
                st = DeviceStepper(ctx, kind, None, None, None, g, order, lr=lr)
                for alpha in ALPHAS:
                    s, dsda = st.get_s(alpha)
                    ref = sr.step_ref(kind, V_d, lam_d, g, order, alpha)
                    assert np.isfinite(dsda).all()
                    rel = np.abs(s - ref).max() / np.abs(ref).max()
                    worst = max(worst, (rel, (gkind, kind, order, alpha)))
                    assert rel <= TOL_LR, (gkind, kind, order, alpha, rel)
                    compared += 1
    print(f'MEASURED structured r = {r}: worst normwise {worst[0]:.2e} at {worst[1]} ({compared} steps)')


# ---- the batched trial-alpha kernel in its three size regimes ---------------------------------------------------------
# rs_batch_vb (csrc/stepper.hip): m <= 1024 one wavefront; 1024 < m <= RS_LDS_MAX = 2048 the whole workgroup with the
# spectrum in LDS; m > RS_LDS_MAX the whole workgroup reading global memory.  A change to either threshold moves these
# sizes (all multiples of 3: the per-atom measure).
BATCH_SIZES = [pytest.param(42, id='wave42'),
               pytest.param(1101, id='lds1101', marks=pytest.mark.emu_heavy),
               pytest.param(2100, id='global2100', marks=pytest.mark.emu_heavy)]
BATCH_FAMILIES = [('prfo', 1), ('prfo', 2), ('rfo', 0)]
BATCH_SPECTRA = ('generic', 'scaled_identity', 'edge_pair_1e-17')
_batch_basis = {}


def _batch_problem(m, order, spectrum):
    rng = np.random.RandomState(m + 7 * order)
    lam = _spectrum(m, order, rng)
    gh = 0.3 * rng.normal(size=m)
    if spectrum == 'scaled_identity':
        # With all poles equal the step is a multiple of g at every alpha and the measure a smooth, concave, saturating
        # function of alpha: Newton would finish such a search before the bisection phase (and the batch kernel) is
        # reached unless it starts on the plateau.  So: small forces everywhere (|g| << 70, alpha = 1 is on the plateau)
        # and one atom with a force of 4.5, whose plateau step 4.5 / 70 is outside both radii.
        g = 0.02 * rng.normal(size=m)
        g[:3] = (3.0, -2.5, 2.2)
        lam, gh = np.full(m, 70.0), reflector(m) @ g
    elif spectrum == 'edge_pair_1e-17':
        gh[order:order + 2] = 1e-17
    return lam, gh


def _basis(ctx, m):
    key = (id(ctx), m)
    if key not in _batch_basis:
        _batch_basis.clear()                        # one basis on the device at a time
        Q = reflector(m)
        _batch_basis[key] = (Q, ctx.upload(Q), ctx.upload(Q.T.copy()))
    return _batch_basis[key]


def _per_atom(s):
    return np.linalg.norm(s.reshape(-1, 3), axis=1).max()


def _batched_against_sequential(ctx, m, kind, order, lam, gh, delta, measure, **kw):
    from sella_amd.device import DeviceStepper
    Q, V, Vt = _basis(ctx, m)
    g = Q @ gh
    out = {}
    for flag in (0, 1):
        with ctx.options(rs_batch=flag):
            st = DeviceStepper(ctx, kind, V, Vt, lam, g, order)
            out[flag] = st.restricted_step(delta=delta, alpha0=1.0, alphamin=0.0, alphamax=1.0, slope=1.0,
                                           newton_safe=False, tol=1e-15, **kw)
    (s0, v0, a0), (s1, v1, a1) = out[0], out[1]
    tag = (m, kind, order, delta)
    assert len(a0) > 20, tag                                          # the schedule did reach its bisection phase
    assert abs(len(a0) - len(a1)) <= 1, tag
    k = min(len(a0), len(a1)) - 2                                     # the last levels sit in the rounding noise of val
    np.testing.assert_allclose(a1[:k], a0[:k], rtol=1e-12, atol=0, err_msg=str(tag))
    np.testing.assert_allclose(s1, s0, atol=1e-12 * max(1.0, np.abs(s0).max()), err_msg=str(tag))
    worst = 0.0
    for s, v, a in out.values():
        ref = sr.step_ref(kind, Q, lam, g, order, a[-1])
        rel = np.abs(s - ref).max() / np.abs(ref).max()
        worst = max(worst, rel)
        assert rel <= TOL_REFLECTOR, (tag, rel)
        got = measure(s)
        if v < delta:
            assert abs(got - v) <= 1e-15 * v, (tag, got, v)           # inside the radius: the reported value
        else:
            assert v == delta and abs(got - delta) <= 2e-15 + 1e-12 * delta, (tag, got)
    return worst


@pytest.mark.parametrize('spectrum', BATCH_SPECTRA)
@pytest.mark.parametrize('kind,order', BATCH_FAMILIES, ids=['prfo1', 'prfo2', 'rfo0'])
@pytest.mark.parametrize('m', BATCH_SIZES)
def test_batched_kernel_size_regimes(ctx, m, kind, order, spectrum):
    """Per-atom measure, dense V: the batched search visits the sequential search's alphas, and the step it returns is
    the 60-digit step at the final alpha (the reflector bound of the host-path test) and sits on the radius."""
    lam, gh = _batch_problem(m, order, spectrum)
    worst = max(_batched_against_sequential(ctx, m, kind, order, lam, gh, delta, _per_atom, cons='ras')
                for delta in (0.02, 1e-4))
    print(f'MEASURED batched m = {m} {kind} order {order} {spectrum}: worst normwise {worst:.2e}')


@pytest.mark.parametrize('m', BATCH_SIZES)
def test_batched_kernel_weighted_component_measure(ctx, m):
    """'mis' with random weights, so that rs_measure_kernel reduces nout > 2048 components as well."""
    lam, gh = _batch_problem(m, 1, 'generic')
    w = np.random.RandomState(m).uniform(0.5, 2.0, size=m)
    worst = _batched_against_sequential(ctx, m, 'prfo', 1, lam, gh, 0.02, lambda s: np.abs(s * w).max(), cons='mis', w=w)
    print(f'MEASURED batched mis m = {m}: worst normwise {worst:.2e}')
