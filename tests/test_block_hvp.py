"""The block form of the device-resident Hessian-vector operator (`hvp_device_apply_block`, `sella_hvp_apply_block`,
`sella_hvp_diag`; csrc/calc.hip, emt_hessian.hip), the matrix-free block Davidson on top of it (`sella_davidson_block_hvp`,
csrc/davidson_block.hip; `Context.davidson_block` with a `DeviceHvpOperator`) and `sella_amd.lowest_modes`.

Yardstick: the dense analytic Hessian `calc.get_hessian(at)` (pinned to the oracle's Richardson extrapolant by
test_emt_hessian.py) and numpy's `eigvalsh` of its free block.  A product — and an entry of the diagonal, a sum of at most
as many terms — is held to test_hvp_operator's bound for product against dense, `product_bound`: 2 n eps max_a sum_b |h_ab|
max|v|.  An eigenvalue is held to tol |lambda| (the solver's stopping rule |r| <= tol |theta|: an eigenvalue lies within |r|
of a converged Ritz value) plus twice that bound for unit vectors (the Rayleigh quotient of the operator against that of
the dense matrix, and eigvalsh's own backward error, each a product's worth)."""
from ctypes import byref, c_double, c_int

import numpy as np
import pytest

from conftest import make_context
from test_emt_hessian import EPS, cu_cluster, make_case, overflowing_args, slab  # noqa: F401 (EPS, cu_cluster: the shared set)
from test_hvp_operator import every_seventh_pinned, model_atoms, model_hessian, product_bound, resident

TOL = 1e-8


@pytest.fixture(scope='module')
def hip_ctx(request):
    """Hardware only, for the sizes of the device."""
    yield from make_context(request, 'hip')


_CASES = {}


def case(ctx, name):
    """(atoms, dense Hessian, library calculator) of a case, made once per backend and left unchanged."""
    key = (ctx.backend, id(ctx), name)
    if key not in _CASES:
        if name in ('model', 'banded'):
            at = model_atoms(ctx, n=96) if name == 'model' else banded_model_atoms(ctx)
            _CASES[key] = (at, model_hessian(at), at.calc.device_calculator())
        else:
            at = make_case(name)
            _CASES[key] = (at, at.calc.get_hessian(at), resident(at))
    return _CASES[key]


def banded_model_atoms(ctx, n=96, seed=43, nu=8, c=0.05):
    """The model PES of test_hvp_operator.model_atoms with a matrix whose diagonal means something: A = diag(0.5 .. 30) plus
    a symmetric Gaussian perturbation.  Its lowest pairs are well separated (gaps of 0.3 - 0.8 under a spectrum of width 40),
    so every leg of the eigenpair test converges in tens of iterations, and a product is two panel products on a 96 x 96
    matrix: the case that keeps the restart legs, with blocks of 4 and of 16, on the emulator."""
    from sella_amd.atoms import Atoms, QuadraticCubicModel
    rng = np.random.RandomState(seed)
    N = rng.normal(size=(n, n))
    A = np.diag(np.linspace(0.5, 30.0, n)) + 0.5 * (N + N.T)
    dA = ctx.upload(A)
    U = rng.normal(size=(nu, n))
    U /= np.linalg.norm(U, axis=1)[:, None]
    at = Atoms(['X'] * (n // 3), 0.05 * rng.normal(size=(n // 3, 3)), pbc=True)
    at.calc = QuadraticCubicModel(lambda x: ctx.symm_mm(dA, x), U, c=c, device_matrix=dA)
    at.model = (A, U, c)
    return at


def selection(n, pinned):
    free = every_seventh_pinned(n) if pinned else None
    return free, (np.arange(n) if free is None else free)


def check_block(op, H, sel, V, label):
    """Every row against the bound of ITS vector (the rows of a panel may differ in scale)."""
    got = op.apply_block(V)
    assert got.shape == V.shape
    err = np.abs(got - V @ H[sel][:, sel]).max(axis=1)
    tol = np.array([product_bound(H, v) for v in V])
    print(f'{label}: k {len(V)}  largest max|apply_block(V) - H V| / bound over the rows {(err / tol).max():.2e}')
    assert (err <= tol).all()
    return got


# ---- 1. the block product against the dense Hessian -----------------------------------------------------------------------
HEAVY = pytest.mark.emu_heavy              # tens of seconds fibre by fibre: on the device only; the narrow cell and the pinned
#                                            Cu and CuAu cells keep every path of the same code on the emulator


@pytest.mark.parametrize('name,pinned', [pytest.param('Cu', False, marks=HEAVY), ('Cu', True),
                                         pytest.param('CuAu', False, marks=HEAVY), ('CuAu', True),
                                         ('narrow', False), ('narrow', True)])
def test_block_product_matches_dense_hessian(ctx, name, pinned):
    from sella_amd.device import DeviceCalculator, DeviceHvpOperator
    at, H, dc = case(ctx, name)
    n = at.positions.size
    x0 = at.positions.ravel()
    free, sel = selection(n, pinned)
    if pinned:
        assert len(sel) % 8 != 0
    op = DeviceHvpOperator(dc, x0, free)
    with ctx.options(emt_hcap=1):
        op1 = DeviceHvpOperator(dc, x0, free)                          # lists of one slot: the sweep wherever they overflow
    rng = np.random.RandomState(21)
    calls = 0
    # both scales in every panel, row by row in turn (k = 1: one panel each)
    for k, first in ((1, 1.0), (1, 1e-3), (7, 1.0), (8, 1e-3), (9, 1.0), (16, 1e-3), (17, 1.0)):
        scales = np.where(np.arange(k) % 2 == 0, first, 1e-3 if first == 1.0 else 1.0)
        V = scales[:, None] * rng.normal(size=(k, len(sel)))
        got = check_block(op, H, sel, V, f'{name} pinned={pinned}')
        assert np.array_equal(op1.apply_block(V), got)
        calls += k
    assert op.calls == calls and op.Vs.shape == (n, 0)                 # k calls each, nothing recorded
    # the opened cutoff: every workgroup's lists overflow with one slot and none does with eight
    pos, par, shifts, rc, acut, cutoff, beta = overflowing_args(at)
    wide = DeviceCalculator.emt(ctx, len(pos), par, shifts, rc, acut, cutoff, beta)
    Hw = ctx.emt_hessian(pos, par, shifts, rc, acut, cutoff, beta).numpy()
    opw = DeviceHvpOperator(wide, x0, free)
    with ctx.options(emt_hcap=1):
        opw1 = DeviceHvpOperator(wide, x0, free)
    V = rng.normal(size=(17, len(sel)))
    got = check_block(opw, Hw, sel, V, f'{name} pinned={pinned} opened cutoff')
    assert np.array_equal(opw1.apply_block(V), got)
    assert wide.ncalls == 0


# ---- 2. rows do not see each other ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('pinned', [False, True], ids=['all', 'pinned'])
def test_rows_are_independent(ctx, pinned):
    from sella_amd.device import DeviceHvpOperator
    at, H, dc = case(ctx, 'narrow')                                    # (125 images: every neighbour through several of them)
    n = at.positions.size
    free, sel = selection(n, pinned)
    m = len(sel)
    op = DeviceHvpOperator(dc, at.positions.ravel(), free)
    rng = np.random.RandomState(22)
    v = rng.normal(size=m)
    alone = op.apply_block(v[None, :])[0]
    P = rng.normal(size=(16, m))
    P[11] = v
    P[3] = 0.0
    out16 = op.apply_block(P)
    assert np.array_equal(out16[11], alone)
    assert not out16[3].any()                                          # a zero row gives an exactly zero row
    Q = 1e3 * rng.normal(size=(17, m))
    Q[16] = v
    assert np.array_equal(op.apply_block(Q)[16], alone)                # the second chunk, one row long
    Q[16], Q[5] = Q[5].copy(), v
    assert np.array_equal(op.apply_block(Q)[5], alone)


# ---- 3. the model kind ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pinned', [False, True], ids=['all', 'pinned'])
def test_model_kind(ctx, pinned):
    from sella_amd.device import DeviceHvpOperator
    at, H, dc = case(ctx, 'model')
    n = at.positions.size
    free, sel = selection(n, pinned)
    op = DeviceHvpOperator(dc, at.positions.ravel(), free)
    rng = np.random.RandomState(23)
    for k in (1, 9, 16, 17):
        check_block(op, H, sel, rng.normal(size=(k, len(sel))), f'model pinned={pinned}')
    Z = rng.normal(size=(3, len(sel)))
    Z[1] = 0.0
    assert not op.apply_block(Z)[1].any()
    assert op.calls == 1 + 9 + 16 + 17 + 3 and dc.ncalls == 0 and op.Vs.shape == (n, 0)


# ---- 4. the diagonal ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pinned', [False, True], ids=['all', 'pinned'])
@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow', 'model'])
def test_diagonal(ctx, name, pinned):
    from sella_amd.device import DeviceHvpOperator
    at, H, dc = case(ctx, name)
    n = at.positions.size
    free, sel = selection(n, pinned)
    op = DeviceHvpOperator(dc, at.positions.ravel(), free)
    before, before_dc = at.calc.ncalls, dc.ncalls
    d = op.diagonal()
    assert d.shape == (len(sel),)
    err, tol = float(np.abs(d - np.diag(H)[sel]).max()), product_bound(H, np.ones(n))
    print(f'{name} pinned={pinned}: max|diagonal - diag(H)| {err:.2e}  bound {tol:.2e}')
    assert err <= tol
    assert op.calls == 0 and at.calc.ncalls == before and dc.ncalls == before_dc
    if name != 'model':
        with ctx.options(emt_hcap=1):
            assert np.array_equal(DeviceHvpOperator(dc, at.positions.ravel(), free).diagonal(), d)


# ---- 5. eigenpairs --------------------------------------------------------------------------------------------------------
def eig_selection(name, n):
    """Cu and the models as everywhere in this file.  The narrow cell is one conventional cell of four atoms: pinning every
    seventh coordinate pins ONE coordinate there and leaves two rigid translations, exact zero modes, on which the relative
    stopping rule cannot converge — so its first atom is pinned whole (9 free coordinates), which removes them."""
    if name == 'narrow':
        return np.arange(3, n, dtype=np.int32)
    if name in ('model', 'banded'):
        return None
    return every_seventh_pinned(n)


def eig_tolerance(H, lam):
    return TOL * abs(lam) + 2 * product_bound(H, np.ones(1))


def check_pairs(out, H, Hs, w, nev, label):
    lams, V = out['lams'], out['V']
    print(f'{label}: niter {out["niter"]}  nmatvec {out["nmatvec"]}  nconv {out["nconv"]}  '
          f'max|lams - w| {np.abs(lams - w[:nev]).max():.2e}  res {out["res"].max():.2e}')
    assert out['nconv'] == nev
    assert V.shape == (Hs.shape[0], nev)
    for h in range(nev):
        assert abs(lams[h] - w[h]) <= eig_tolerance(H, lams[h])
        r = np.linalg.norm(Hs @ V[:, h] - lams[h] * V[:, h])
        assert r <= TOL * abs(lams[h]) + product_bound(H, V[:, h])
    assert np.abs(V.T @ V - np.eye(nev)).max() <= 1e-10


# nev per case: one of {3, 4, 5} for which the input condition below holds.  Every case runs every leg — blocks of 4 and of
# 16, the default basis and one of nev + 2 block vectors, the operator's diagonal and no preconditioner, and the existing
# dense route — with the iteration limit the case needs:
#   Cu      83 free of 96; tens to a hundred iterations.  32 atoms: seconds per product fibre by fibre, device only.
#   narrow  9 free (eig_selection): nev + 2 block >= 11 exceeds them, the basis limit is clamped to 9 and spans everything, so
#           NO run on this cell can restart, whatever is pinned (12 coordinates, three of them translations): its restart
#           legs run and must converge, the restart assertion needs maxvec < m.
#   model   test_hvp_operator's: the wanted pairs sit in a cluster (0.0600, 0.0603, 0.0639, 0.0703 under a spectrum that
#           reaches 49) with random eigenvectors, so its diagonal tells a correction nothing and the iteration is a restarted
#           Lanczos: 350 - 750 iterations with block 16, 1500 - 12000 with block 4 — on the existing dense route just the same
#           (measured side by side on the device; each leg under a second there).  Hence maxiter 20000, and device only.
#   banded  banded_model_atoms: the same code paths in tens of iterations — the restart legs of the emulator.
@pytest.mark.parametrize('block', [4, 16])
@pytest.mark.parametrize('name,nev', [pytest.param('Cu', 3, marks=pytest.mark.emu_heavy), ('narrow', 3),
                                      pytest.param('model', 4, marks=pytest.mark.emu_heavy), ('banded', 4)])
def test_eigenpairs(ctx, name, nev, block):
    from sella_amd.device import DeviceHvpOperator
    at, H, dc = case(ctx, name)
    n = at.positions.size
    free = eig_selection(name, n)
    sel = np.arange(n) if free is None else free
    m = len(sel)
    Hs = np.ascontiguousarray(H[sel][:, sel])
    w = np.linalg.eigvalsh(Hs)
    # the input: the wanted pairs are separated from the rest by far more than the tolerance (a missed eigenvalue cannot
    # hide behind it) and none of them is a zero mode (the stopping rule is relative)
    print(f'{name}: m {m}  lowest eigenvalues {w[:nev + 1]}  largest |w| {np.abs(w).max():.3f}')
    assert w[nev] - w[nev - 1] > 100 * eig_tolerance(H, w[nev - 1])
    assert np.abs(w[:nev]).min() >= 1e-3 * np.abs(w).max()
    x0 = at.positions.ravel()
    kw = dict(nev=nev, block=block, tol=TOL, maxiter=20000 if name == 'model' else 500)
    before, before_dc = at.calc.ncalls, dc.ncalls
    op = DeviceHvpOperator(dc, x0, free)
    diag = op.diagonal()
    out = ctx.davidson_block(op, **kw, diag=diag)
    check_pairs(out, H, Hs, w, nev, f'{name} block {block} default maxvec')
    assert out['nmatvec'] == op.calls
    # a basis of nev + 2 block vectors: thick restarts.  The start block has min(block, m) rows and every iteration that
    # does not end the run adds at least one, so without a restart the basis would hold min(block, m) + niter - 1 rows
    maxvec = nev + 2 * block
    op2 = DeviceHvpOperator(dc, x0, free)
    out2 = ctx.davidson_block(op2, m, **kw, maxvec=maxvec, diag=diag)
    check_pairs(out2, H, Hs, w, nev, f'{name} block {block} maxvec {maxvec}')
    assert out2['nmatvec'] == op2.calls
    assert (maxvec < m) == (name != 'narrow')
    if maxvec < m:
        assert min(block, m) + out2['niter'] - 1 > maxvec                # more rows than the basis holds: it was restarted
    # no preconditioner, default basis and the small one
    for mv in (0, maxvec):
        op3 = DeviceHvpOperator(dc, x0, free)
        check_pairs(ctx.davidson_block(op3, **kw, maxvec=mv), H, Hs, w, nev, f'{name} block {block} maxvec {mv} no preconditioner')
    # the existing route on the dense free block: the same eigenvalues within the same tolerance
    dA = ctx.upload(Hs)
    dense = ctx.davidson_block(dA, m, **kw, diag=np.ascontiguousarray(np.diag(Hs)))
    dA.free()
    assert dense['nconv'] == nev
    for h in range(nev):
        assert abs(dense['lams'][h] - out['lams'][h]) <= eig_tolerance(H, out['lams'][h])
    assert at.calc.ncalls == before and dc.ncalls == before_dc


# ---- 6. counters ----------------------------------------------------------------------------------------------------------
def test_counters_and_the_pair_record(ctx):
    from sella_amd import _lib
    from sella_amd.device import DeviceHvpOperator
    at, H, dc = case(ctx, 'narrow')
    n = at.positions.size
    free = eig_selection('narrow', n)
    m = len(free)
    op = DeviceHvpOperator(dc, at.positions.ravel(), free)
    v = np.random.RandomState(26).normal(size=m)
    first = DeviceHvpOperator(dc, at.positions.ravel(), free).apply(v)
    before, before_dc = at.calc.ncalls, dc.ncalls
    out = ctx.davidson_block(op, nev=3, block=4, tol=TOL, diag=op.diagonal())
    assert out['nconv'] == 3 and out['nmatvec'] > 0
    assert op.calls == out['nmatvec']
    assert _lib.lib().sella_hvp_npairs(op._h) == 0 and op.Vs.shape == (n, 0)
    assert at.calc.ncalls == before and dc.ncalls == before_dc
    again = op.apply(v)
    assert np.array_equal(again, first)
    assert op.calls == out['nmatvec'] + 1
    Vs, AVs = op.Vs, op.AVs                                            # ... recorded as pair 0
    assert Vs.shape == (n, 1) and np.array_equal(Vs[free, 0], v) and np.array_equal(AVs[free, 0], first)
    op.apply_block(np.ones((2, m)))
    op.apply(2 * v)
    assert op.calls == out['nmatvec'] + 4 and op.Vs.shape == (n, 2) and np.array_equal(op.Vs[free, 1], 2 * v)


# ---- 7. lowest_modes ------------------------------------------------------------------------------------------------------
def small_slab():
    """fcc111 Cu (2, 2, 3), 12 atoms, and the indices of its bottom layer."""
    at = slab((2, 2, 3), seed=5)
    return at, np.sort(np.argsort(at.positions[:, 2])[:4])


@pytest.mark.parametrize('how', ['constraints', pytest.param('free', marks=pytest.mark.emu_heavy)])
def test_lowest_modes(ctx, how):
    import sella_amd
    from sella_amd.internal import Constraints
    at, bottom = small_slab()
    n, nev = at.positions.size, 4
    H = at.calc.get_hessian(at)
    sel = np.array([3 * i + c for i in range(len(at)) if i not in bottom for c in range(3)], dtype=np.int32)
    w = np.linalg.eigvalsh(H[sel][:, sel])
    assert w[nev] - w[nev - 1] > 100 * eig_tolerance(H, w[nev - 1]) and np.abs(w[:nev]).min() >= 1e-3 * np.abs(w).max()
    if how == 'constraints':
        cons = Constraints(at)
        for i in bottom:                                               # atom by atom: single-coordinate pins
            cons.fix_translation(int(i))
        out = sella_amd.lowest_modes(at, nev=nev, constraints=cons, tol=TOL)
    else:
        out = sella_amd.lowest_modes(at, nev=nev, free=sel, tol=TOL)
    lams, modes = out['lams'], out['modes']
    print(f'{how}: lams {lams}  niter {out["niter"]}  nmatvec {out["nmatvec"]}')
    assert out['nconv'] == nev and lams.shape == (nev,) and modes.shape == (nev, len(at), 3)
    assert not modes[:, bottom].any()
    M = modes.reshape(nev, n)
    assert np.abs(M @ M.T - np.eye(nev)).max() <= 1e-10
    for h in range(nev):
        assert abs(lams[h] - w[h]) <= eig_tolerance(H, lams[h])
        assert np.linalg.norm((H @ M[h])[sel] - lams[h] * M[h][sel]) <= TOL * abs(lams[h]) + product_bound(H, M[h])
    assert set(out) == {'lams', 'modes', 'res', 'niter', 'nmatvec', 'nconv'}


def test_lowest_modes_refusals(ctx):
    from sella_amd import lowest_modes
    from sella_amd.atoms import MorseCluster
    from sella_amd.internal import Constraints
    at, bottom = small_slab()
    n = at.positions.size
    sel = np.array([3 * i + c for i in range(len(at)) if i not in bottom for c in range(3)], dtype=np.int32)
    morse, _ = small_slab()
    morse.calc = MorseCluster()
    with pytest.raises(NotImplementedError, match='MorseCluster'):
        lowest_modes(morse, nev=2, free=sel)
    bond = Constraints(at)
    bond.fix_bond((0, 1))
    with pytest.raises(NotImplementedError):
        lowest_modes(at, nev=2, constraints=bond)
    cons = Constraints(at)
    for i in bottom:
        cons.fix_translation(int(i))
    with pytest.raises(ValueError, match='not both'):
        lowest_modes(at, nev=2, constraints=cons, free=sel)
    with pytest.raises(ValueError):
        lowest_modes(at, nev=len(sel) + 1, free=sel)
    with pytest.raises(ValueError):
        lowest_modes(at, nev=2, free=sel[::-1])
    with pytest.raises(RuntimeError, match='nconv'):
        lowest_modes(at, nev=4, free=sel, maxiter=1)
    out = lowest_modes(at, nev=4, free=sel, maxiter=1, allow_unconverged=True)
    assert out['nconv'] < 4 and out['modes'].shape == (4, n // 3, 3)


# ---- 8. the ABI -----------------------------------------------------------------------------------------------------------
def test_invalid_arguments(ctx):
    from sella_amd import _lib
    from sella_amd._lib import ptr
    from sella_amd.device import DeviceHvpOperator
    L = _lib.lib()
    INVALID = -1                                                       # SELLA_E_INVALID
    at, H, dc = case(ctx, 'narrow')
    n = at.positions.size
    free = np.arange(3, n, dtype=np.int32)
    m = len(free)
    op = DeviceHvpOperator(dc, at.positions.ravel(), free)
    nev = 3
    lams, V, res = np.zeros(16), np.zeros(16 * m), np.zeros(16)
    niter, nmv, nconv = c_int(0), c_int(0), c_int(0)
    V0 = np.random.RandomState(28).normal(size=(m, 17))

    def run(h=op._h, pv=-1, pvt=-1, pe=None, v0=None, nv0=0, nev=nev, block=4):
        return L.sella_davidson_block_hvp(ctx._h, h, pv, pvt, ptr(pe), None, ptr(v0), nv0, nev, block, 0, c_double(TOL), 50,
                                          ptr(lams), ptr(V), ptr(res), byref(niter), byref(nmv), byref(nconv))
    assert run(h=None) == INVALID
    assert run(nev=0) == INVALID
    assert run(nev=m + 1) == INVALID
    assert run(block=0) == INVALID
    assert run(block=17) == INVALID
    assert run(v0=V0, nv0=17) == INVALID
    big, bigt = ctx.zeros(m + 1, m + 1), ctx.zeros(m + 1, m + 1)
    assert run(pv=big.handle, pvt=bigt.handle, pe=np.ones(m + 1)) == INVALID
    assert op.calls == 0
    out = np.empty((1, m))
    assert L.sella_hvp_apply_block(None, ptr(out), 1, ptr(out)) == INVALID
    assert L.sella_hvp_apply_block(op._h, ptr(out), 0, ptr(out)) == INVALID
    assert L.sella_hvp_diag(op._h, None) == INVALID and L.sella_hvp_diag(None, ptr(out)) == INVALID
    # a valid call afterwards still works
    assert run() == 0
    assert nconv.value == nev and nmv.value == op.calls > 0
    w = np.linalg.eigvalsh(H[free][:, free])
    assert np.abs(lams[:nev] - w[:nev]).max() <= eig_tolerance(H, w[nev - 1])
    with pytest.raises(ValueError):
        ctx.davidson_block(op, nev=nev, row0=1)
    with pytest.raises(ValueError):
        ctx.davidson_block(op, nev=nev, world=2)
    with pytest.raises(ValueError):
        ctx.davidson_block(op, nev=nev, allgather=lambda *a: None)
    with pytest.raises(ValueError):
        ctx.davidson_block(op, m + 1, nev)
    with pytest.raises(ValueError):
        op.apply_block(np.zeros((2, m + 1)))


# ---- 9. the sizes of the device -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('size', [(8, 8, 16), (10, 10, 11)], ids=['N1024', 'N1100'])
def test_large_sizes(hip_ctx, monkeypatch, size):
    """N = 1024: the largest size with the positions staged in LDS by the density pass; N = 1100: unstaged, and not a
    multiple of the 256 threads.  The lower half of the slab pinned atom by atom."""
    import sella_amd
    from sella_amd import device
    from sella_amd.device import DeviceHvpOperator
    monkeypatch.setattr(device, '_default', hip_ctx)
    at = slab(size, seed=len(size) + size[2])
    n = at.positions.size
    H = at.calc.get_hessian(at)
    dc = resident(at)
    before = dc.ncalls
    upper = np.sort(np.argsort(at.positions[:, 2])[len(at) // 2:])
    free = (3 * upper[:, None] + np.arange(3)).ravel().astype(np.int32)
    m = len(free)
    rng = np.random.RandomState(9)
    V = rng.normal(size=(16, m))
    V /= np.linalg.norm(V, axis=1)[:, None]
    Vfull = np.zeros((16, n))
    Vfull[:, free] = V
    want = at.calc.hessian_vector_product(at, Vfull)[:, free]
    tol = product_bound(H, V)
    op = DeviceHvpOperator(dc, at.positions.ravel(), free)
    err = float(np.abs(op.apply_block(V) - want).max())
    print(f'N={n // 3}: max|apply_block(V) - HV| {err:.2e}  bound {tol:.2e}')
    assert err <= tol
    nev = 4
    w = np.linalg.eigvalsh(H[free][:, free])
    out = sella_amd.lowest_modes(at, nev=nev, free=free, tol=TOL)
    print(f'N={n // 3}: lams {out["lams"]}  eigvalsh {w[:nev + 1]}  niter {out["niter"]}  nmatvec {out["nmatvec"]}')
    assert out['nconv'] == nev
    for h in range(nev):
        assert abs(out['lams'][h] - w[h]) <= eig_tolerance(H, out['lams'][h])
    assert dc.ncalls == before
