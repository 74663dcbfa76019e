"""The device-resident Hessian-vector operator of positions and cell (`sella_hvp_create_cell`; csrc/calc.hip,
emt_hessian.hip), `DeviceHvpOperator.for_cell` on top of it, the route `CellCartesianPES.diag` takes through it, and
`lowest_modes(cell=True)`.

Coordinates: those of `CellCartesianPES`, [x (3N Cartesian); p (the masked log-deformation parameters)]; the eigensolver
sees the free position coordinates followed by p.

Yardstick: `Hp = pes._convert_cell_hessian(calc.get_cell_hessian(at))`, the dense Hessian carried into the same coordinates
(both functions have tests of their own), restricted to the free set.  A product is held to the project's bound for this
operator (test_emt_cell_hvp.test_operator_in_pes_coordinates): a dim-term dot product plus the two nine-term contractions
with J on either side, 2 (dim + 18) eps max_row sum|Hp| max|v|.  Eigenvalues and residuals are held to test_block_hvp's
rules with test_hvp_operator's (slightly narrower) `product_bound` of Hp.

Cases: the 4-atom cell of `jittered_cell(1)`, strained by 2-3 % AFTER the PES was made (125 images, every atom its own
neighbour, U != 0 and dE/dC != 0, so the second derivative of the exponential map counts) with the upper-triangular mask and a
pressure, and with the full mask and none; and the 32-atom alloy (two species, lists that overflow with one slot) with the
full mask and a pressure.

Rows per workgroup of the block kernels: four, and sixteen rows per panel, so k = 1 is a remainder alone, 4 one group, 5 a
group and a remainder, 16 a full panel, 17 a second chunk one row long."""
from ctypes import byref, c_void_p
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import make_context
from test_block_hvp import TOL, eig_tolerance
from test_emt_cell_hvp import STRAIN, UPPER
from test_emt_hessian import EPS, jittered_cell, make_case, slab
from test_hvp_operator import Listener, Spy, assert_same_run, every_seventh_pinned, product_bound

INVALID = -1                                            # SELLA_E_INVALID
MASKS = {'upper': (UPPER, 0.01), 'full': (None, 0.0), 'CuAu': (None, 0.01)}
HEAVY = pytest.mark.emu_heavy


@pytest.fixture(scope='module')
def hip_ctx(request):
    """Hardware only, for the sizes of the device."""
    yield from make_context(request, 'hip')


def bound(Hp, v):
    return 2 * (Hp.shape[0] + 18) * EPS * np.abs(Hp).sum(axis=1).max() * np.abs(v).max()


def strain(at):
    at.set_cell(np.array(at.cell) @ (np.eye(3) + STRAIN), scale_atoms=True)


def describe(at, pes):
    """What the tests need of a geometry: the yardstick, the library calculator and the arguments of `for_cell`."""
    Hp = pes._convert_cell_hessian(at.calc.get_cell_hessian(at))
    J, G0, P = pes._cell_param_maps()
    at.get_potential_energy()
    return SimpleNamespace(at=at, pes=pes, Hp=Hp, dc=at.calc.device_calculator(), x0=at.positions.ravel().copy(),
                           cell=np.array(at.cell, dtype=float), J=J, G=0.5 * (G0 + G0.T), P=P, n=at.positions.size,
                           mc=pes.n_cell_dof, dim=pes.dim)


_CASES = {}


def case(ctx, name):
    """A case, made once per backend and left unchanged."""
    from sella_amd.peswrapper import CellCartesianPES
    key = (ctx.backend, id(ctx), name)
    if key not in _CASES:
        mask, pressure = MASKS[name]
        at = make_case('CuAu') if name == 'CuAu' else jittered_cell(1)
        pes = CellCartesianPES(at, cell_mask=mask, scalar_pressure=pressure, cell_hessian_vector_product=True)
        if name != 'CuAu':
            strain(at)
            assert np.abs(pes.get_x()[pes.ncart:]).max() > 0.01 * pes.exp_cell_factor         # U != 0
        assert np.abs(pes.get_g()[pes.ncart:]).max() > 1e-3                                   # dE/dC != 0
        _CASES[key] = describe(at, pes)
    return _CASES[key]


def free_set(c, how):
    """(free position coordinates or None, the same as indices into [x; p])."""
    free = {'all': None, 'atom0': np.arange(3, c.n, dtype=np.int32), 'seventh': every_seventh_pinned(c.n)}[how]
    sel = np.arange(c.n) if free is None else free
    return free, np.concatenate([sel, c.n + np.arange(c.mc)])


def make_op(c, free, **kw):
    from sella_amd.device import DeviceHvpOperator
    return DeviceHvpOperator.for_cell(c.dc, c.x0, c.cell, c.J, c.G, c.P, free=free, **kw)


def mixed_scales(rng, k, m, first):
    scales = np.where(np.arange(k) % 2 == 0, first, 1e-3 if first == 1.0 else 1.0)
    return scales[:, None] * rng.normal(size=(k, m))


def check_rows(got, V, Hs, Hp, label):
    assert got.shape == V.shape
    err = np.abs(got - V @ Hs).max(axis=1)
    tol = np.array([bound(Hp, v) for v in V])
    print(f'{label}: k {len(V)}  largest max|op V - Hp V| / bound over the rows {(err / tol).max():.3f}')
    assert (err <= tol).all()


# ---- 1. products against the converted dense Hessian ------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['all', 'atom0', 'seventh'])
@pytest.mark.parametrize('name', ['upper', 'full', pytest.param('CuAu', marks=HEAVY)])
def test_products_match_converted_hessian(ctx, name, how):
    c = case(ctx, name)
    free, full = free_set(c, how)
    m = len(full)
    Hs = c.Hp[full][:, full]
    ncalls, nhess, ncell = c.at.calc.ncalls, c.at.calc.nhessians, c.at.calc.ncellhvps
    before_dc = c.dc.ncalls
    op = make_op(c, free)
    assert op.shape == (m, m) and op.ntrue == c.n + c.mc
    with ctx.options(emt_hcap=1):
        op1 = make_op(c, free)                                          # lists of one slot: the sweep wherever they overflow
    rng = np.random.RandomState(31)
    calls = 0
    for scale in (1.0, 1e-3):
        v = scale * rng.normal(size=m)
        got = op.apply(v)
        check_rows(got[None], v[None], Hs, c.Hp, f'{name} {how} apply scale {scale}')
        assert np.array_equal(op1.apply(v), got)
        calls += 1
    for k, first in ((1, 1.0), (4, 1e-3), (5, 1.0), (16, 1e-3), (17, 1.0)):
        V = mixed_scales(rng, k, m, first)
        got = op.apply_block(V)
        check_rows(got, V, Hs, c.Hp, f'{name} {how} apply_block')
        assert np.array_equal(op1.apply_block(V), got)
        assert np.array_equal(op.apply_block(V), got)                   # the same bits from call to call
        calls += 2 * k
    assert op.calls == calls
    # neither force calls nor Hessians, and nothing the calculator counts
    assert (c.at.calc.ncalls, c.at.calc.nhessians, c.at.calc.ncellhvps, c.dc.ncalls) == (ncalls, nhess, ncell, before_dc)


# ---- 2. rows do not see each other ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['all', 'atom0'])
@pytest.mark.parametrize('name', ['upper', 'full'])
def test_rows_are_independent(ctx, name, how):
    c = case(ctx, name)
    free, full = free_set(c, how)
    m = len(full)
    op = make_op(c, free)
    rng = np.random.RandomState(32)
    v = rng.normal(size=m)
    alone = op.apply_block(v[None, :])[0]
    P = rng.normal(size=(16, m))
    P[11] = v
    P[3] = 0.0
    out16 = op.apply_block(P)
    assert np.array_equal(out16[11], alone)
    assert out16[3].shape == (m,) and not out16[3].any()               # a zero row gives an exactly zero row, cell entries too
    Q = 1e3 * rng.normal(size=(17, m))
    Q[16] = v
    assert np.array_equal(op.apply_block(Q)[16], alone)                # the second chunk, one row long
    Q[16], Q[5] = Q[5].copy(), v
    assert np.array_equal(op.apply_block(Q)[5], alone)
    for nh in (2, 3, 6, 7):                                            # every position within a group of four, and a shorter panel
        R = rng.normal(size=(nh, m))
        R[nh - 1] = v
        assert np.array_equal(op.apply_block(R)[nh - 1], alone)


# ---- 3. the record and the counters -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['all', 'seventh'])
def test_record_and_counters(ctx, how):
    c = case(ctx, 'upper')
    free, full = free_set(c, how)
    m, dim = len(full), c.n + c.mc
    mx = m - c.mc
    op = make_op(c, free)
    assert op.calls == 0 and op.Vs.shape == (dim, 0) and op.AVs.shape == (dim, 0)
    rng = np.random.RandomState(33)
    only_cell = np.zeros(m)
    only_cell[mx:] = rng.normal(size=c.mc)                             # no position entry: the rule is about the WHOLE vector
    tiny_cell = np.zeros(m)
    tiny_cell[m - 1] = 1e-13                                           # |v| < 1e-12 through a cell entry alone
    vs = [rng.normal(size=m), np.zeros(m), 1e-3 * rng.normal(size=m), only_cell, tiny_cell, rng.normal(size=m)]
    outs = [op.apply(v) for v in vs]
    assert not outs[1].any() and not outs[4].any()                     # a vanishing vector: a zero product ...
    assert op.calls == 6                                               # ... counted ...
    Vs, AVs = op.Vs, op.AVs
    assert Vs.shape == (dim, 4) and AVs.shape == (dim, 4)              # ... and not recorded
    kept = [vs[0], vs[2], vs[3], vs[5]]
    want = np.zeros((dim, 4))
    want[full] = np.array(kept).T
    assert np.array_equal(Vs, want)                                    # zeros on the pinned rows
    assert np.array_equal(AVs[full], np.array([outs[0], outs[2], outs[3], outs[5]]).T)
    for q in range(4):                                                 # all rows of the product, pinned ones included
        err, tol = float(np.abs(AVs[:, q] - c.Hp @ Vs[:, q]).max()), bound(c.Hp, Vs[:, q])
        print(f'{how} pair {q}: max|AVs - Hp Vs| {err:.2e}  bound {tol:.2e}')
        assert err <= tol
    op.apply_block(rng.normal(size=(5, m)))                            # block rows: counted, not recorded
    assert op.calls == 11 and op.Vs.shape == (dim, 4)
    for q in range(14):                                                # more products than one chunk of the record holds
        op.apply(rng.normal(size=m))
    assert op.calls == 25 and op.Vs.shape == (dim, 18)
    V2, AV2 = op.Vs, op.AVs
    assert np.array_equal(V2[:, :4], Vs) and np.array_equal(AV2[:, :4], AVs)
    assert np.abs(AV2 - c.Hp @ V2).max() <= bound(c.Hp, V2)


# ---- 4. the diagonal ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['all', 'seventh'])
@pytest.mark.parametrize('name', ['upper', 'full', pytest.param('CuAu', marks=HEAVY)])
def test_diagonal(ctx, name, how):
    c = case(ctx, name)
    free, full = free_set(c, how)
    m = len(full)
    mx = m - c.mc
    op = make_op(c, free)
    op.apply(np.ones(m))
    d = op.diagonal()
    assert d.shape == (m,)
    want = np.diag(c.Hp)[full]
    Hxx = c.Hp[:c.n, :c.n]
    err_x, tol_x = float(np.abs(d[:mx] - want[:mx]).max()), product_bound(Hxx, np.ones(c.n))
    err_p, tol_p = float(np.abs(d[mx:] - want[mx:]).max()), bound(c.Hp, np.ones(1))
    print(f'{name} {how}: positions {err_x:.2e} (bound {tol_x:.2e})  cell {err_p:.2e} (bound {tol_p:.2e})')
    assert err_x <= tol_x and err_p <= tol_p
    assert op.calls == 1 and op.Vs.shape == (c.n + c.mc, 1)            # neither a product nor recorded
    with ctx.options(emt_hcap=1):
        assert np.array_equal(make_op(c, free).diagonal(), d)


# ---- 5. Davidson --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['all', 'seventh'])
def test_davidson_device_and_host_vectors_agree(ctx, how):
    c = case(ctx, 'upper')
    free, full = free_set(c, how)
    m = len(full)
    v0 = np.random.RandomState(34).normal(size=(m, 1))
    before = c.dc.ncalls
    op, op2 = make_op(c, free), make_op(c, free, through_host=True)
    run = ctx.davidson(op, m, v0, 0.1, method='jd0', maxiter=6)
    ref = ctx.davidson(op2, m, v0, 0.1, method='jd0', maxiter=6)
    assert_same_run(run, ref)
    lams, V, AV, nmatvec = run
    assert nmatvec == op.calls == op2.calls > 0 and c.dc.ncalls == before
    assert np.array_equal(op.Vs, op2.Vs) and np.array_equal(op.AVs, op2.AVs)
    assert np.abs(AV - c.Hp[full][:, full] @ V).max() <= bound(c.Hp, V)
    assert op.Vs.shape[0] == c.n + c.mc
    assert np.abs(op.AVs - c.Hp @ op.Vs).max() <= bound(c.Hp, op.Vs)


def check_pairs(lams, V, w, Hp, Hs, nev):
    for h in range(nev):
        assert abs(lams[h] - w[h]) <= eig_tolerance(Hp, lams[h])
        r = np.linalg.norm(Hs @ V[:, h] - lams[h] * V[:, h])
        assert r <= TOL * abs(lams[h]) + product_bound(Hp, V[:, h])
    assert np.abs(V.T @ V - np.eye(nev)).max() <= 1e-10


def gap_condition(w, Hp, nev):
    """The input of an eigenpair test: the wanted pairs are separated from the rest by far more than the tolerance and none of
    them is a zero mode (the stopping rule is relative)."""
    assert w[nev] - w[nev - 1] > 100 * eig_tolerance(Hp, w[nev - 1])
    assert np.abs(w[:nev]).min() >= 1e-3 * np.abs(w).max()


@pytest.mark.parametrize('block', [4, 16])
def test_block_davidson(ctx, block):
    """Atom 0 pinned: no translations.  The upper-triangular mask leaves the cell no rotation."""
    c = case(ctx, 'upper')
    free, full = free_set(c, 'atom0')
    nev = 3
    Hs = np.ascontiguousarray(c.Hp[full][:, full])
    w = np.linalg.eigvalsh(Hs)
    print(f'm {len(full)}  lowest eigenvalues {w[:nev + 1]}  largest |w| {np.abs(w).max():.3f}')
    gap_condition(w, c.Hp, nev)
    assert w[0] > 0
    before = c.dc.ncalls
    op = make_op(c, free)
    out = ctx.davidson_block(op, nev=nev, block=block, tol=TOL, diag=op.diagonal())
    print(f'block {block}: niter {out["niter"]}  nmatvec {out["nmatvec"]}  lams {out["lams"]}  res {out["res"].max():.2e}')
    assert out['nconv'] == nev and out['V'].shape == (len(full), nev)
    check_pairs(out['lams'], out['V'], w, c.Hp, Hs, nev)
    assert out['nmatvec'] == op.calls and op.Vs.shape == (c.n + c.mc, 0) and c.dc.ncalls == before


# ---- 6. PES.diag takes the route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['device', 'device-pinned', 'centre', 'callable', 'trajectory', 'no-library'])
def test_pes_diag(ctx, monkeypatch, which):
    from sella_amd.internal import Constraints
    from sella_amd.peswrapper import CellCartesianPES
    at = jittered_cell(1)
    dense = lambda atoms, V: V @ atoms.calc.get_cell_hessian(atoms)   # noqa: E731
    kw = dict(cell_mask=UPPER, scalar_pressure=0.01, cell_hessian_vector_product=True, constraints=Constraints(at),
              proj_trans=False)
    route = 'device'
    if which == 'device-pinned':
        kw['constraints'].fix_translation(0)
        kw.pop('proj_trans')
    elif which == 'centre':
        kw.pop('constraints')                                          # the default fixes the centre: no selection of coordinates
        kw.pop('proj_trans')
        route = 'host'
    elif which == 'callable':
        kw.update(cell_hessian_vector_product=dense)
        route = 'host'
    elif which == 'trajectory':
        kw.update(trajectory=Listener())
        route = 'host'
    spy = Spy(monkeypatch)
    pes = CellCartesianPES(at, **kw)
    if which == 'no-library':
        pes.use_library_calculator = False
        route = 'host'
    strain(at)
    derivatives, real = [], pes._expm_derivatives
    pes._expm_derivatives = lambda U: derivatives.append(1) or real(U)
    calc = at.calc
    pes.get_g()                                                        # the evaluation of the point itself
    ncalls, neval, nhess, ncell = calc.ncalls, pes.neval, calc.nhessians, calc.ncellhvps
    pes.diag(maxiter=4)
    assert spy.made == [route]
    assert pes.nhvp > 0 and not pes.first_diag
    assert calc.ncalls == ncalls and pes.neval == neval                # products are not force calls
    if which == 'callable':
        assert calc.ncellhvps == ncell and calc.nhessians == nhess + 1  # (the callable asked for ONE dense Hessian, cached)
    else:
        assert calc.nhessians == nhess
        grown = calc.ncellhvps - ncell
        assert grown == pes.nhvp if route == 'device' else 0 < grown <= pes.nhvp
    assert len(derivatives) == 1                                       # J, G and the p V term: once per geometry
    Hp = pes._convert_cell_hessian(calc.get_cell_hessian(at))
    assert len(derivatives) == 1
    (S, Y), = spy.pairs                                                # the (dim, k) record reaches H.update
    S, Y = S.reshape(pes.dim, -1), Y.reshape(pes.dim, -1)
    npairs = S.shape[1]
    assert 0 < npairs <= pes.nhvp
    # S = Vs X and Y = AVs X with X orthogonal, so Y - Hp S = (AVs - Hp Vs) X: an entry is a row of the recorded products'
    # errors times a unit column of X, at most sqrt(npairs) times the bound of one product.  The recorded vectors are the
    # eigensolver's orthonormal iterates (and S with them, asserted here), so max|v| <= 1 in that bound.
    off = float(np.abs(S.T @ S - np.eye(npairs)).max())
    err, tol = float(np.abs(Y - Hp @ S).max()), np.sqrt(npairs) * bound(Hp, np.ones(1))
    print(f'{which}: {npairs} pairs  max|S^T S - I| {off:.2e}  max|Y - Hp S| {err:.2e}  bound {tol:.2e}')
    assert off <= 1e-10
    assert err <= tol
    if which == 'device-pinned':
        assert not S[:3].any()                                         # zero on the pinned atom


def test_cell_pes_keeps_off_the_finite_difference_route(ctx):
    from sella_amd.internal import Constraints
    from sella_amd.peswrapper import CellCartesianPES
    at = jittered_cell(1)
    pes = CellCartesianPES(at, cell_hessian_vector_product=True, constraints=Constraints(at), proj_trans=False)
    pes.get_g()
    assert pes._library_fd_operator(pes.get_Ufree(), False) is None
    assert pes._library_hvp_operator(pes.get_Ufree()) is not None
    plain = CellCartesianPES(jittered_cell(1), constraints=Constraints(at), proj_trans=False)
    plain.get_g()
    assert plain._library_hvp_operator(plain.get_Ufree()) is None      # without the keyword there are no exact products


@pytest.mark.parametrize('exact', [False, True])
def test_the_route_leaves_the_basis_cache_alone(ctx, exact):
    """The route is found from the constraints, not from notes kept beside the bases: at every one of a series of geometries
    the basis is computed once and then served from the cache under the geometry's own key, with or without the feature."""
    from sella_amd.internal import Constraints
    from sella_amd.peswrapper import CellCartesianPES
    at = jittered_cell(1)
    cons = Constraints(at)
    cons.fix_translation(0)
    pes = CellCartesianPES(at, cell_hessian_vector_product=True if exact else None, constraints=cons)
    rng = np.random.RandomState(3)
    for _ in range(6):
        at.positions[1:] += 1e-3 * rng.normal(size=(len(at) - 1, 3))
        first = pes._calc_basis()
        assert pes._calc_basis() is first and pes._basis_cache.get(pes._state_hash()) is first
        assert all(isinstance(e[0], bytes) for e in pes._basis_cache._entries if e is not None)
    if exact:
        pes.get_g()
        op = pes._library_hvp_operator(pes.get_Ufree())              # free: everything but the three pinned coordinates
        assert op is not None and op.shape[0] == pes.dim - 3


# ---- 7. a run -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rep', [1, pytest.param(2, marks=HEAVY)], ids=['4atoms', '32atoms'])
def test_cell_minimum_on_the_device_route(ctx, monkeypatch, rep):
    """The criterion of test_emt_cell_hvp.test_cell_minimum_with_exact_products: both runs stop with every force below fmax
    and every cell gradient below smax, so each lies within (N fmax^2 + n_cell smax^2) / (2 lambda_min) of the minimum, and
    the two differ by at most twice that; lambda_min is taken at the minimum (the host run continued to 1e-6), off the zero
    modes.  Atom 0 is pinned in both runs: that removes the translations, and the basis is then a selection of coordinates,
    which the device route needs (the default constraint, a fixed centre, is none)."""
    from sella_amd import Sella, peswrapper
    from sella_amd.internal import Constraints
    fmax = smax = 1e-3
    spy = Spy(monkeypatch)                                             # (NumericalHessian fails when constructed)
    assert peswrapper.NumericalHessian is not None

    def search(on_device):
        at = jittered_cell(rep)
        cons = Constraints(at)
        cons.fix_translation(0)
        opt = Sella(at, order=0, eig=True, optimize_cell=True, cell_hessian_vector_product=True, constraints=cons, logfile=None)
        if not on_device:
            opt.pes.use_library_calculator = False
        del spy.made[:]
        opt.run(fmax, 200)
        assert opt.converged()
        done, worst_force, _, worst_cell = opt.pes.converged(fmax, smax=smax)
        assert done and worst_force < fmax and worst_cell < smax
        assert spy.made and set(spy.made) == {'device' if on_device else 'host'}
        pes = opt.pes
        assert pes.nhvp > 0 and at.calc.nhessians == 0 and pes.neval <= opt.nsteps + 1
        assert at.calc.ncellhvps == pes.nhvp if on_device else 0 < at.calc.ncellhvps <= pes.nhvp
        return at, opt

    at, opt = search(True)
    host, opt0 = search(False)
    diff = abs(at.get_potential_energy() - host.get_potential_energy())
    steps0 = opt0.nsteps
    opt0.run(1e-6, 200)
    assert opt0.converged()
    w = np.linalg.eigvalsh(opt0.pes._convert_cell_hessian(host.calc.get_cell_hessian(host))[3:, 3:])
    zero = np.abs(w) < 1e-6 * w[-1]
    lam_min = w[~zero].min()
    assert zero.sum() <= 3 and lam_min > 0, w[:8]                      # (the full mask: rotations of cell and atoms together)
    tol = 2 * (len(at) * fmax ** 2 + opt.pes.n_cell_dof * smax ** 2) / (2 * lam_min)
    print(f'steps {opt.nsteps} / {steps0}  products {opt.pes.nhvp} / {opt0.pes.nhvp}  lambda_min {lam_min:.3e}  '
          f'|dE| {diff:.2e}  bound {tol:.2e}')
    assert diff <= tol


# ---- 8. lowest_modes(cell=True) ---------------------------------------------------------------------------------------------------
def strained_atoms():
    at = jittered_cell(1)
    strain(at)
    return at


@pytest.mark.parametrize('how', ['constraints', 'free'])
def test_lowest_cell_modes(ctx, how):
    """The geometry of test_block_davidson; `lowest_modes` takes the log-deformation about the CURRENT cell, so the yardstick
    is the conversion by a PES made at the strained cell."""
    import sella_amd
    from sella_amd.internal import Constraints
    from sella_amd.peswrapper import CellCartesianPES
    at = strained_atoms()
    n, nev, mc = at.positions.size, 3, 6
    pes = CellCartesianPES(at, cell_mask=UPPER, scalar_pressure=0.01)
    Hp = pes._convert_cell_hessian(at.calc.get_cell_hessian(at))
    Hs = np.ascontiguousarray(Hp[3:, 3:])
    w = np.linalg.eigvalsh(Hs)
    print(f'lowest eigenvalues {w[:nev + 1]}  largest |w| {np.abs(w).max():.3f}')
    gap_condition(w, Hp, nev)
    kw = dict(nev=nev, tol=TOL, cell=True, cell_mask=UPPER, scalar_pressure=0.01)
    if how == 'constraints':
        cons = Constraints(at)
        cons.fix_translation(0)
        out = sella_amd.lowest_modes(at, constraints=cons, **kw)
    else:
        out = sella_amd.lowest_modes(at, free=np.arange(3, n), **kw)
    assert set(out) == {'lams', 'modes', 'cell_modes', 'res', 'niter', 'nmatvec', 'nconv'}
    lams, modes, cell_modes = out['lams'], out['modes'], out['cell_modes']
    print(f'{how}: lams {lams}  niter {out["niter"]}  nmatvec {out["nmatvec"]}')
    assert out['nconv'] == nev and lams.shape == (nev,)
    assert modes.shape == (nev, len(at), 3) and cell_modes.shape == (nev, 3, 3)
    assert not modes[:, 0].any() and not cell_modes[:, ~UPPER].any()
    V = np.hstack([modes.reshape(nev, n)[:, 3:], cell_modes[:, UPPER]]).T                 # (m, nev) over the free set
    assert V.shape == (n - 3 + mc, nev)
    check_pairs(lams, V, w, Hp, Hs, nev)


def test_lowest_modes_cell_refusals(ctx):
    from sella_amd import lowest_modes
    from sella_amd.atoms import MorseCluster
    at = strained_atoms()
    n = at.positions.size
    free = np.arange(3, n)
    morse = strained_atoms()
    morse.calc = MorseCluster()
    with pytest.raises(NotImplementedError, match='MorseCluster'):
        lowest_modes(morse, nev=2, free=free, cell=True)
    surface = slab((2, 2, 3), seed=5)
    assert not np.all(surface.pbc)
    with pytest.raises(NotImplementedError, match='periodic'):
        lowest_modes(surface, nev=2, cell=True)
    with pytest.raises(ValueError, match='cell_mask'):
        lowest_modes(at, nev=2, free=free, cell=True, cell_mask=np.zeros((3, 3), dtype=bool))
    with pytest.raises(ValueError):
        lowest_modes(at, nev=n - 3 + 9 + 1, free=free, cell=True)
    out = lowest_modes(at, nev=2, free=free, tol=TOL)                  # without cell=True: exactly the keys it had
    assert set(out) == {'lams', 'modes', 'res', 'niter', 'nmatvec', 'nconv'}


# ---- 9. the ABI -----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(ctx):
    from sella_amd import _lib
    from sella_amd._lib import ptr
    from sella_amd.device import DeviceCalculator
    L = _lib.lib()
    c = case(ctx, 'upper')
    n, mc = c.n, c.mc
    idx = np.arange(3, n, dtype=np.int32)
    P = np.ascontiguousarray(c.P)
    handles = []

    def create(calc=c.dc._h, n=n, x0=c.x0, cell=c.cell, idx=None, mx=0, mc=mc, J=c.J, G=c.G, P=P, out=True):
        h = c_void_p()
        J = None if J is None else np.ascontiguousarray(J)
        status = L.sella_hvp_create_cell(calc, n, ptr(x0), ptr(cell), None if idx is None else idx.ctypes.data_as(c_void_p), mx, mc,
                                         ptr(J), ptr(G), ptr(P), byref(h) if out else None)
        if status == 0:
            handles.append(h)
        return status, L.sella_last_error().decode()
    for kwargs in (dict(calc=None), dict(x0=None), dict(cell=None), dict(J=None), dict(G=None), dict(out=False),   # null pointers
                   dict(n=n - 3), dict(n=n + 3),                                               # n != sella_calc_dim
                   dict(mc=0), dict(mc=10), dict(mc=-1),
                   dict(idx=idx[::-1].copy(), mx=len(idx)),                                    # not ascending
                   dict(idx=np.array([0, 0, 1], dtype=np.int32), mx=3),                        # repeated
                   dict(idx=np.array([0, n], dtype=np.int32), mx=2),                           # out of range
                   dict(idx=np.array([-1, 2], dtype=np.int32), mx=2),
                   dict(idx=idx, mx=n + 1), dict(idx=idx, mx=-1)):
        status, message = create(**kwargs)
        assert status == INVALID and message, kwargs
    rng = np.random.RandomState(35)
    A = rng.normal(size=(n, n))
    model = DeviceCalculator.model(ctx, ctx.upload(A + A.T), rng.normal(size=(2, n)), 0.05)
    status, message = create(calc=model._h)                            # not the EMT kind
    assert status == INVALID and 'EMT' in message
    flat = c.cell.copy()
    flat[2] = flat[0] + flat[1]
    status, message = create(cell=flat)
    assert status == INVALID and 'singular' in message
    status, message = create(cell=np.ascontiguousarray(c.cell * 1.01))  # the calculator's shifts are another cell's translations
    assert status == INVALID and 'no lattice translation' in message
    # valid calls afterwards: with and without a pressure term and a selection
    for kwargs in (dict(), dict(P=None), dict(idx=idx, mx=len(idx))):
        assert create(**kwargs)[0] == 0
    h = handles[0]
    v = rng.normal(size=n + mc)
    y = np.empty_like(v)
    assert L.sella_hvp_matvec(h, ptr(v), ptr(y), n + mc - 1) == INVALID
    assert L.sella_hvp_matvec(h, ptr(v), ptr(y), n + mc) == 0
    assert np.abs(y - c.Hp @ v).max() <= bound(c.Hp, v)
    assert np.array_equal(y, make_op(c, None).apply(v))
    for h in handles:
        assert L.sella_hvp_destroy(h) == 0
    with pytest.raises(ValueError):
        make_op(c, None).apply_block(np.zeros((2, n + mc + 1)))
    with pytest.raises(ValueError):
        from sella_amd.device import DeviceHvpOperator
        DeviceHvpOperator.for_cell(c.dc, c.x0, c.cell, c.J[:8], c.G, c.P)


# ---- 10. the sizes of the device --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('size,how', [((8, 8, 16), 'all'), ((10, 10, 11), 'seventh')], ids=['N1024', 'N1100'])
def test_large_sizes(hip_ctx, monkeypatch, size, how):
    """N = 1024: the largest size with the positions staged in LDS by the density pass; N = 1100: unstaged, and not a
    multiple of the 256 threads.  One single product, a block of five and the diagonal against the converted dense
    Hessian."""
    from sella_amd import device
    from sella_amd.peswrapper import CellCartesianPES
    monkeypatch.setattr(device, '_default', hip_ctx)
    at = slab(size, seed=len(size) + size[2])
    pes = CellCartesianPES(at, cell_mask=UPPER, scalar_pressure=0.01, cell_hessian_vector_product=True)
    c = describe(at, pes)
    assert c.n == 3 * size[0] * size[1] * size[2]
    free, full = free_set(c, how)
    m = len(full)
    mx = m - c.mc
    Hs = c.Hp[full][:, full]
    before = c.dc.ncalls
    op = make_op(c, free)
    rng = np.random.RandomState(36)
    v = rng.normal(size=m)
    check_rows(op.apply(v)[None], v[None], Hs, c.Hp, f'N={c.n // 3} apply')
    V = mixed_scales(rng, 5, m, 1.0)
    check_rows(op.apply_block(V), V, Hs, c.Hp, f'N={c.n // 3} apply_block')
    d = op.diagonal()
    want = np.diag(c.Hp)[full]
    err_x, tol_x = float(np.abs(d[:mx] - want[:mx]).max()), product_bound(c.Hp[:c.n, :c.n], np.ones(c.n))
    err_p, tol_p = float(np.abs(d[mx:] - want[mx:]).max()), bound(c.Hp, np.ones(1))
    print(f'N={c.n // 3}: diagonal positions {err_x:.2e} (bound {tol_x:.2e})  cell {err_p:.2e} (bound {tol_p:.2e})')
    assert err_x <= tol_x and err_p <= tol_p
    assert op.calls == 6 and c.dc.ncalls == before
    Vs, AVs = op.Vs, op.AVs
    assert Vs.shape == (c.n + c.mc, 1)
    assert np.abs(AVs - c.Hp @ Vs).max() <= bound(c.Hp, Vs)
