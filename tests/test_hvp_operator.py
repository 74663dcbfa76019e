"""The device-resident Hessian-vector operator (`sella_hvp_*`, `sella_davidson_hvp`; csrc/calc.hip, emt_hessian.hip,
davidson.hip), `DeviceHvpOperator` / `AnalyticHessian` on top of it, and the opt-in `hessian_vector_product=` of `PES` and
`Sella`.

The yardstick of a product is the dense analytic Hessian `calc.get_hessian(at)`, which test_emt_hessian.py pins to the
oracle's Richardson extrapolant; the tolerance is that file's for product against dense (`test_product_matches_dense_hessian`):
both sides are, per component, sums of at most n products h_ab v_b, so 2 n eps max_a sum_b |h_ab| max|v|."""
import ctypes
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

from conftest import hessian_like, make_context
from test_emt_hessian import EPS, cu_cluster, make_case, overflowing_args, slab


@pytest.fixture(scope='module')
def hip_ctx(request):
    """Hardware only, for the sizes of the device."""
    yield from make_context(request, 'hip')


def product_bound(H, v, n=None):
    n = H.shape[0] if n is None else n
    return 2 * n * EPS * np.abs(H).sum(axis=1).max() * np.abs(v).max()


def every_seventh_pinned(n):
    return np.array([i for i in range(n) if i % 7 != 6], dtype=np.int32)


def resident(at):
    at.get_potential_energy()
    return at.calc.device_calculator()


# ---- the model: f = x.A x / 2 + c / 3 sum_j (u_j . x)^3 with A = hessian_like(96): lowest eigenvalue -1, next >= 0.05 ----------
def model_atoms(ctx, n=96, seed=41, nu=8, c=0.05):
    from sella_amd.atoms import Atoms, QuadraticCubicModel
    A = hessian_like(n, seed, nneg=1)[0]
    dA = ctx.upload(A)
    rng = np.random.RandomState(seed + 1)
    U = rng.normal(size=(nu, n))
    U /= np.linalg.norm(U, axis=1)[:, None]
    at = Atoms(['X'] * (n // 3), 0.05 * rng.normal(size=(n // 3, 3)), pbc=True)
    at.calc = QuadraticCubicModel(lambda x: ctx.symm_mm(dA, x), U, c=c, device_matrix=dA)
    at.model = (A, U, c)
    return at


def model_hessian(at):
    A, U, c = at.model
    return A + 2 * c * np.einsum('j,ja,jb->ab', U @ at.positions.ravel(), U, U)


# ---- 1. a product against the dense Hessian ---------------------------------------------------------------------------------
@pytest.mark.parametrize('pinned', [False, True], ids=['all', 'pinned'])
@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow'])
def test_product_matches_dense_hessian(ctx, name, pinned):
    from sella_amd.device import DeviceCalculator, DeviceHvpOperator
    at = make_case(name)
    n = at.positions.size
    H = at.calc.get_hessian(at)
    dc = resident(at)
    x0 = at.positions.ravel()
    free = every_seventh_pinned(n) if pinned else None
    sel = np.arange(n) if free is None else free
    op = DeviceHvpOperator(dc, x0, free)
    assert op.shape == (len(sel), len(sel))
    with ctx.options(emt_hcap=1):
        op1 = DeviceHvpOperator(dc, x0, free)                          # lists of one slot: the sweep wherever they overflow
    rng = np.random.RandomState(11)
    Hs = H[sel][:, sel]
    for scale in (1.0, 1e-3):
        v = scale * rng.normal(size=len(sel))
        got = op.apply(v)
        err, tol = float(np.abs(got - Hs @ v).max()), product_bound(H, v)
        print(f'{name} pinned={pinned} scale={scale}: max|op v - H v| {err:.2e}  bound {tol:.2e}')
        assert err <= tol
        assert np.array_equal(op1.apply(v), got)
    zero = op.apply(np.zeros(len(sel)))
    assert zero.shape == (len(sel),) and not zero.any()
    # the opened cutoff, where every workgroup's lists overflow with one slot and none does with eight: both operators
    # against the dense Hessian of that cutoff, and against each other bit for bit
    pos, par, shifts, rc, acut, cutoff, beta = overflowing_args(at)
    wide = DeviceCalculator.emt(ctx, len(pos), par, shifts, rc, acut, cutoff, beta)
    Hw = ctx.emt_hessian(pos, par, shifts, rc, acut, cutoff, beta).numpy()
    opw = DeviceHvpOperator(wide, x0, free)
    with ctx.options(emt_hcap=1):
        opw1 = DeviceHvpOperator(wide, x0, free)
    v = rng.normal(size=len(sel))
    got = opw.apply(v)
    assert np.abs(got - Hw[sel][:, sel] @ v).max() <= product_bound(Hw, v)
    assert np.array_equal(opw1.apply(v), got)
    assert wide.ncalls == 0


# ---- 2. the record ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pinned', [False, True], ids=['all', 'pinned'])
def test_record_of_pairs(ctx, pinned):
    from sella_amd.device import DeviceHvpOperator
    at = make_case('Cu')
    n = at.positions.size
    H = at.calc.get_hessian(at)
    dc = resident(at)
    before, before_dc = at.calc.ncalls, dc.ncalls
    free = every_seventh_pinned(n) if pinned else None
    sel = np.arange(n) if free is None else free
    op = DeviceHvpOperator(dc, at.positions.ravel(), free)
    assert op.calls == 0 and op.Vs.shape == (n, 0) and op.AVs.shape == (n, 0)
    rng = np.random.RandomState(12)
    vs = [rng.normal(size=len(sel)), np.zeros(len(sel)), 1e-3 * rng.normal(size=len(sel)), rng.normal(size=len(sel))]
    for v in vs:
        op.apply(v)
    assert op.calls == 4
    Vs, AVs = op.Vs, op.AVs
    assert Vs.shape == (n, 3) and AVs.shape == (n, 3)
    want = np.zeros((n, 3))
    want[sel] = np.array([vs[0], vs[2], vs[3]]).T
    assert np.array_equal(Vs, want)                                    # zeros on the pinned rows
    for q in range(3):                                                 # all n rows of the product, pinned ones included
        assert np.abs(AVs[:, q] - H @ Vs[:, q]).max() <= product_bound(H, Vs[:, q])
    # more products than one chunk of the record holds
    for q in range(20):
        op.apply(rng.normal(size=len(sel)))
    assert op.calls == 24 and op.Vs.shape == (n, 23)
    V2, AV2 = op.Vs, op.AVs
    assert np.array_equal(V2[:, :3], Vs) and np.array_equal(AV2[:, :3], AVs)
    assert np.abs(AV2 - H @ V2).max() <= product_bound(H, V2)
    assert at.calc.ncalls == before and dc.ncalls == before_dc


# ---- 3. the model kind --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pinned', [False, True], ids=['all', 'pinned'])
def test_model_kind(ctx, pinned):
    """n = 30, nu = 3, c = 0.05 and the tolerance of test_emt_hessian.test_model_calculator_hessian_and_product: per
    component an n-term dot product with A, nu products p_j t_j u_ja of two n-term dot products: (2 n + nu + 4) eps against
    the sum of the absolute values of the terms."""
    from sella_amd.device import DeviceCalculator, DeviceHvpOperator
    rng = np.random.RandomState(4)
    n, nu, c = 30, 3, 0.05
    A = rng.normal(size=(n, n))
    A = A + A.T
    U = rng.normal(size=(nu, n))
    x = rng.normal(size=n)
    want = A + 2 * c * np.einsum('j,ja,jb->ab', U @ x, U, U)
    terms = np.abs(A) + 2 * abs(c) * np.einsum('j,ja,jb->ab', np.abs(U) @ np.abs(x), np.abs(U), np.abs(U))
    dA = ctx.upload(A)
    calc = DeviceCalculator.model(ctx, dA, U, c)
    free = every_seventh_pinned(n) if pinned else None
    sel = np.arange(n) if free is None else free
    op = DeviceHvpOperator(calc, x, free)
    V = rng.normal(size=(5, len(sel)))
    Vfull = np.zeros((5, n))
    Vfull[:, sel] = V
    tol = (2 * n + nu + 4) * EPS * (np.abs(Vfull) @ terms.T).max()
    for v, vf in zip(V, Vfull):
        assert np.abs(op.apply(v) - (want @ vf)[sel]).max() <= tol
    assert not op.apply(np.zeros(len(sel))).any()
    assert op.calls == 6 and calc.ncalls == 0
    Vs, AVs = op.Vs, op.AVs
    assert np.array_equal(Vs, Vfull.T)
    assert np.abs(AVs - want @ Vs).max() <= tol


# ---- 4. the device branch of the eigensolver -------------------------------------------------------------------------------------
def davidson_through_callback(ctx, op, n, v0, gamma, method, maxiter, Pvecs=None, PvecsT=None, pevals=None):
    """The unchanged `sella_davidson` with `sella_hvp_matvec` as its host callback; what `Context.davidson` returns."""
    from sella_amd import _lib
    from sella_amd._lib import ptr
    from sella_amd.device import DAVIDSON_METHODS, SELLA_NO_MAT, check
    v0 = np.ascontiguousarray(np.asarray(v0, dtype=np.float64).reshape(n, -1))
    kmax = min(n, max(maxiter, v0.shape[1]))
    lams, V, AV = np.zeros(kmax + 1), np.empty(n * (kmax + 1)), np.empty(n * (kmax + 1))
    k, nmv = c_int(0), c_int(0)
    pe = None if pevals is None else np.ascontiguousarray(pevals, dtype=np.float64)
    check(_lib.lib().sella_davidson(ctx._h, SELLA_NO_MAT, op.callback(), op._h,
                                    SELLA_NO_MAT if Pvecs is None else Pvecs.handle,
                                    SELLA_NO_MAT if PvecsT is None else PvecsT.handle, ptr(pe), 1.0, n, ptr(v0), v0.shape[1],
                                    float(gamma), DAVIDSON_METHODS[method], int(maxiter), None, 0.99, ptr(lams), ptr(V), ptr(AV),
                                    byref(k), byref(nmv)))
    kk = k.value
    return lams[:kk].copy(), V[:n * kk].reshape(n, kk).copy(), AV[:n * kk].reshape(n, kk).copy(), nmv.value


def assert_same_run(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert x.shape == y.shape and np.array_equal(x, y)
    assert a[3] == b[3]


@pytest.mark.parametrize('pinned', [False, True], ids=['all', 'pinned'])
def test_davidson_on_the_model(ctx, pinned):
    from sella_amd.device import DeviceHvpOperator
    at = model_atoms(ctx)
    n = at.positions.size
    H = model_hessian(at)
    dc = at.calc.device_calculator()
    free = every_seventh_pinned(n) if pinned else None
    sel = np.arange(n) if free is None else free
    m = len(sel)
    Hs = H[sel][:, sel]
    P = hessian_like(n, 41, nneg=1)[1][sel][:, sel]
    dP = ctx.upload(np.ascontiguousarray(P))
    w, Q, Qt = ctx.eigh(dP)
    pre = dict(Pvecs=Q, PvecsT=Qt, pevals=w)
    v0 = Qt.numpy()[:1].T
    gamma, maxiter = 0.1, 40
    op, op2 = DeviceHvpOperator(dc, at.positions.ravel(), free), DeviceHvpOperator(dc, at.positions.ravel(), free)
    run = ctx.davidson(op, m, v0, gamma, method='jd0', maxiter=maxiter, **pre)
    ref = davidson_through_callback(ctx, op2, m, v0, gamma, 'jd0', maxiter, **pre)
    assert_same_run(run, ref)
    lams, V, AV, nmatvec = run
    assert nmatvec == op.calls == op2.calls and dc.ncalls == 0
    assert np.array_equal(op.Vs, op2.Vs) and np.array_equal(op.AVs, op2.AVs)
    k = len(lams)
    r = np.linalg.norm(AV[:, 0] - lams[0] * V[:, 0])
    print(f'model pinned={pinned}: k {k}  lam0 {lams[0]:.6f}  |r| {r:.2e}')
    if k < maxiter:
        assert r <= gamma * abs(lams[0])
    assert abs(lams[0] - np.linalg.eigvalsh(Hs)[0]) <= r               # an eigenvalue lies within |r| of a Ritz value
    assert np.abs(AV - Hs @ V).max() <= product_bound(H, V)


def test_davidson_on_emt(ctx):
    from sella_amd.device import DeviceHvpOperator
    at = make_case('Cu')
    n = at.positions.size
    H = at.calc.get_hessian(at)
    dc = resident(at)
    free = every_seventh_pinned(n)
    m = len(free)
    v0 = np.random.RandomState(13).normal(size=(m, 1))
    before = dc.ncalls
    op, op2 = DeviceHvpOperator(dc, at.positions.ravel(), free), DeviceHvpOperator(dc, at.positions.ravel(), free)
    run = ctx.davidson(op, m, v0, 0.1, method='jd0', maxiter=6)
    ref = davidson_through_callback(ctx, op2, m, v0, 0.1, 'jd0', 6)
    assert_same_run(run, ref)
    lams, V, AV, nmatvec = run
    assert nmatvec == op.calls and dc.ncalls == before
    assert np.abs(AV - H[free][:, free] @ V).max() <= product_bound(H, V)
    assert np.abs(op.AVs - H @ op.Vs).max() <= product_bound(H, op.Vs)


# ---- 5. PES.diag ----------------------------------------------------------------------------------------------------------------
class Spy:
    """Counts the constructions of the two operators and keeps what `ApproximateHessian.update` receives."""

    def __init__(self, monkeypatch):
        from sella_amd import device, peswrapper
        from sella_amd.linalg import ApproximateHessian
        from sella_amd.peswrapper import PES
        self.made, self.pairs = [], []
        monkeypatch.setattr(peswrapper, 'NumericalHessian', lambda *a, **k: pytest.fail('NumericalHessian constructed'))
        monkeypatch.setattr(PES, '_library_fd_operator', lambda *a, **k: pytest.fail('finite-difference operator asked for'))
        real_dev, real_host, real_update = device.DeviceHvpOperator, peswrapper.AnalyticHessian, ApproximateHessian.update

        made = self.made

        class dev(real_dev):
            def __init__(self, *a, **k):
                made.append('device')
                real_dev.__init__(self, *a, **k)

        class host(real_host):
            def __init__(self, *a, **k):
                made.append('host')
                real_host.__init__(self, *a, **k)

        def update(hess, dx, dg):
            self.pairs.append((np.array(dx), np.array(dg)))
            return real_update(hess, dx, dg)
        monkeypatch.setattr(device, 'DeviceHvpOperator', dev)
        monkeypatch.setattr(peswrapper, 'AnalyticHessian', host)
        monkeypatch.setattr(ApproximateHessian, 'update', update)


def check_diag(pes, at, H, spy, route):
    before = at.calc.ncalls
    pes.diag(maxiter=4)
    grown = at.calc.ncalls - before
    assert pes.nhvp > 0 and not pes.first_diag
    assert grown <= 1 and pes.neval == grown                           # the evaluation of the point itself, no more
    assert spy.made == [route]
    (S, Y), = spy.pairs
    S, Y = S.reshape(H.shape[0], -1), Y.reshape(H.shape[0], -1)
    npairs = S.shape[1]
    assert 0 < npairs <= pes.nhvp
    err, tol = float(np.abs(Y - H @ S).max()), npairs * product_bound(H, S)
    print(f'{route}: {npairs} pairs  max|Y - H S| {err:.2e}  bound {tol:.2e}')
    assert err <= tol


class Listener:
    """A trajectory as the PES sees one."""
    written = 0

    def write(self):
        self.written += 1

    def close(self):
        pass


@pytest.mark.parametrize('case', ['model', 'model-free', 'model-pinned', 'narrow', 'narrow-pinned', 'callable', 'trajectory'])
def test_pes_diag(ctx, monkeypatch, case):
    from sella_amd.internal import Constraints
    from sella_amd.peswrapper import PES
    if case.startswith('narrow'):
        at = make_case('narrow')
        H = at.calc.get_hessian(at)
    else:
        at = model_atoms(ctx)
        H = model_hessian(at)
    kw, route = dict(hessian_vector_product=True), 'device'
    if case in ('model', 'narrow'):
        # the default constraint fixes the centre of the system: no selection of coordinates
        route = 'host'
    elif case == 'model-free':
        kw.update(constraints=Constraints(at), proj_trans=False)
    elif case.endswith('pinned'):
        cons = Constraints(at)
        cons.fix_translation(0)
        kw.update(constraints=cons)
    elif case == 'callable':
        kw.update(hessian_vector_product=lambda atoms, V: V @ H, constraints=Constraints(at), proj_trans=False)
        route = 'host'
    elif case == 'trajectory':
        kw.update(trajectory=Listener(), constraints=Constraints(at), proj_trans=False)
        route = 'host'
    spy = Spy(monkeypatch)
    pes = PES(at, **kw)
    check_diag(pes, at, H, spy, route)


# ---- 6. a saddle search ---------------------------------------------------------------------------------------------------------
def test_saddle_search_on_the_model(ctx, monkeypatch):
    from sella_amd import Sella, peswrapper
    monkeypatch.setattr(peswrapper, 'NumericalHessian', lambda *a, **k: pytest.fail('NumericalHessian constructed'))
    at = model_atoms(ctx)
    # (the model has no translational symmetry: no constraint on the centre, so that convergence is about the forces)
    opt = Sella(at, order=1, hessian_vector_product=True, logfile=None, proj_trans=False)
    assert opt._lib_kw is None                                         # the general driver, like hessian_function runs
    fmax = 1e-3
    opt.run(fmax=fmax, steps=200)
    assert opt.converged()
    assert np.abs(at.get_forces()).max() < fmax
    assert opt.pes.nhvp > 0
    w = np.linalg.eigvalsh(model_hessian(at))
    print(f'steps {opt.nsteps}  products {opt.pes.nhvp}  force calls {opt.pes.neval}  lowest eigenvalues {w[:3]}')
    assert w[0] < 0 < w[1]


@pytest.mark.emu_heavy
def test_minimum_of_the_cluster(ctx, monkeypatch):
    from sella_amd import Sella, peswrapper
    monkeypatch.setattr(peswrapper, 'NumericalHessian', lambda *a, **k: pytest.fail('NumericalHessian constructed'))
    at = cu_cluster()
    opt = Sella(at, order=0, eig=True, hessian_vector_product=True, logfile=None)
    opt.run(fmax=1e-3, steps=100)
    assert opt.converged() and opt.pes.nhvp > 0
    assert np.abs(at.get_forces()).max() < 1e-3


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from sella_amd import Sella
    from sella_amd.atoms import EMT, MorseCluster
    from sella_amd.peswrapper import PES, CellCartesianPES, InternalPES
    at = make_case('narrow')
    with pytest.raises(ValueError, match='two sources of curvature'):
        Sella(at, order=0, hessian_function=at.calc.get_hessian, hessian_vector_product=True, logfile=None)
    with pytest.raises(NotImplementedError):
        Sella(at, order=0, internal=True, hessian_vector_product=True, logfile=None)
    with pytest.raises(NotImplementedError):
        Sella(at, order=0, optimize_cell=True, hessian_vector_product=True, logfile=None)
    with pytest.raises(NotImplementedError):
        CellCartesianPES(at, hessian_vector_product=True)
    with pytest.raises(NotImplementedError):
        InternalPES(cu_cluster(), None, hessian_vector_product=True)
    morse = make_case('narrow')
    morse.calc = MorseCluster()
    with pytest.raises(NotImplementedError, match='MorseCluster'):
        Sella(morse, order=1, hessian_vector_product=True, logfile=None)
    with pytest.raises(NotImplementedError, match='MorseCluster'):
        PES(morse, hessian_vector_product=True)
    plain = make_case('narrow')
    plain.calc = EMT()
    assert PES(plain).nhvp == 0 and PES(plain)._hvp is None              # without the keyword nothing is resolved


def test_invalid_arguments(ctx):
    from sella_amd import _lib
    from sella_amd._lib import ptr
    L = _lib.lib()
    INVALID = -1                                                       # SELLA_E_INVALID
    at = make_case('narrow')
    dc = resident(at)
    x = np.ascontiguousarray(at.positions).ravel()
    n = x.size
    idx = np.arange(n - 2, dtype=np.int32)
    pidx = idx.ctypes.data_as(c_void_p)
    h = c_void_p()
    assert L.sella_hvp_create(None, n, ptr(x), None, 0, byref(h)) == INVALID
    assert L.sella_hvp_create(dc._h, n, None, None, 0, byref(h)) == INVALID
    assert L.sella_hvp_create(dc._h, n, ptr(x), None, 0, None) == INVALID
    assert L.sella_hvp_create(dc._h, n - 3, ptr(x), None, 0, byref(h)) == INVALID
    assert L.sella_hvp_create(dc._h, n, ptr(x), pidx, 0, byref(h)) == INVALID
    assert L.sella_hvp_create(dc._h, n, ptr(x), pidx, n + 1, byref(h)) == INVALID
    assert L.sella_hvp_create(dc._h, n, ptr(x), pidx, len(idx), byref(h)) == 0
    m = len(idx)
    v, out = np.ones(m), np.empty(m)
    assert L.sella_hvp_matvec(None, ptr(v), ptr(out), m) == INVALID
    assert L.sella_hvp_matvec(h, None, ptr(out), m) == INVALID
    assert L.sella_hvp_matvec(h, ptr(v), None, m) == INVALID
    assert L.sella_hvp_matvec(h, ptr(v), ptr(out), m - 1) == INVALID
    assert L.sella_hvp_pairs(h, None, None) == INVALID
    assert L.sella_hvp_calls(h) == 0 and L.sella_hvp_npairs(h) == 0
    lams, V, AV = np.zeros(8), np.zeros(8 * m), np.zeros(8 * m)
    k, nmv = c_int(0), c_int(0)
    tail = (-1, -1, None, ctypes.c_double(1.0))
    rest = (ptr(v), 1, ctypes.c_double(0.1), 2, 3, None, ctypes.c_double(0.99), ptr(lams), ptr(V), ptr(AV), byref(k), byref(nmv))
    assert L.sella_davidson_hvp(ctx._h, None, *tail, m, *rest) == INVALID
    assert L.sella_davidson_hvp(None, h, *tail, m, *rest) == INVALID
    assert L.sella_davidson_hvp(ctx._h, h, *tail, n, *rest) == INVALID
    assert L.sella_hvp_calls(h) == 0
    # a valid call afterwards still works
    assert L.sella_davidson_hvp(ctx._h, h, *tail, m, *rest) == 0
    assert k.value >= 1 and nmv.value == L.sella_hvp_calls(h) > 0
    assert L.sella_hvp_matvec(h, ptr(v), ptr(out), m) == 0
    H = at.calc.get_hessian(at)
    assert np.abs(out - H[idx][:, idx] @ v).max() <= product_bound(H, v)
    assert L.sella_hvp_destroy(h) == 0


# ---- 8. the sizes of the device ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('size', [(8, 8, 16), (10, 10, 11)], ids=['N1024', 'N1100'])
def test_large_sizes(hip_ctx, monkeypatch, size):
    """N = 1024: the largest size with the positions staged in LDS by the density pass; N = 1100: unstaged, and not a
    multiple of the 256 threads.  Against `calc.hessian_vector_product`, which test_emt_hessian.test_large_sizes pins to
    the device gradient's extrapolant, under the bound of the dense Hessian."""
    from sella_amd import device
    from sella_amd.device import DeviceHvpOperator
    monkeypatch.setattr(device, '_default', hip_ctx)
    at = slab(size, seed=len(size) + size[2])
    n = at.positions.size
    H = at.calc.get_hessian(at)
    dc = resident(at)
    before = dc.ncalls
    rng = np.random.RandomState(5)
    v = rng.normal(size=n)
    v /= np.linalg.norm(v)
    tol = product_bound(H, v)
    want = at.calc.hessian_vector_product(at, v)
    op = DeviceHvpOperator(dc, at.positions.ravel())
    got = op.apply(v)
    err = float(np.abs(got - want).max())
    print(f'N={n // 3}: max|op v - HV| {err:.2e}  bound {tol:.2e}')
    assert err <= tol
    free = every_seventh_pinned(n)
    vf = np.zeros(n)
    vf[free] = v[free]
    opf = DeviceHvpOperator(dc, at.positions.ravel(), free)
    gotf = opf.apply(v[free])
    wantf = at.calc.hessian_vector_product(at, vf)
    assert np.abs(gotf - wantf[free]).max() <= tol
    assert np.abs(opf.AVs[:, 0] - wantf).max() <= tol and np.array_equal(opf.Vs[:, 0], vf)
    assert dc.ncalls == before
