"""Products with the analytic EMT Hessian of positions and cell without forming it (`sella_emt_cell_hvp`;
csrc/emt_hessian.hip), `Calculator.cell_hessian_vector_product` on top of it, the operator of `CellCartesianPES` in its own
coordinates, and `Sella(..., optimize_cell=True, cell_hessian_vector_product=True)`.

Coordinates of the device product: rows [v (3N); W.ravel() (9)] in [x; C.ravel()] as for `sella_emt_cell_hessian` (lattice
vectors in the rows of C, positions fixed while C varies).

Yardsticks: the dense Hessian of the same geometry (`get_cell_hessian`, which has tests of its own) with the bound of a
(3N + 9)-term dot product on either side, 2 (3N + 9) eps max_row sum|h| max|V| (the bound of the product at fixed cell in
test_emt_hessian.py with the dimension replaced), and the Richardson extrapolant of central differences of the device's
full gradient along mixed directions, with the error estimate of test_emt_cell_hessian.py's yardstick.

Vectors per workgroup: four (CHVP_KQ), so k = 1 is a remainder alone, 4 one full group, 5 a full group and a remainder,
11 two full groups and a remainder."""
import numpy as np
import pytest

from test_emt_cell_hessian import cell_args, cell_cutoff_gap, full_gradient, image_indices, yardstick
from test_emt_hessian import EPS, H_STEP, emt_args, hip_ctx, jittered_cell, make_case, overflowing_args, slab  # noqa: F401

INVALID = -1                                            # SELLA_E_INVALID


def bound(H, V):
    """2 dim eps max_row sum|h| max|V|: a dim-term dot product per component, once for either side."""
    return 2 * H.shape[0] * EPS * np.abs(H).sum(axis=1).max() * np.abs(V).max()


_DENSE = {}


def dense(name):
    """The dense Hessian of positions and cell of a case, once per backend in use (read only)."""
    from sella_amd.device import get_context
    key = (name, get_context().backend)
    if key not in _DENSE:
        at = make_case(name)
        _DENSE[key] = at.calc.get_cell_hessian(at)
    return _DENSE[key]


# ---- 1. against the dense Hessian ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow'])
@pytest.mark.parametrize('k', [1, 4, 5, 11])
def test_product_matches_dense_cell_hessian(ctx, name, k):
    at = make_case(name)
    dim = at.positions.size + 9
    H = dense(name)
    V = np.random.RandomState(k).normal(size=(k, dim))
    calls, hessians = at.calc.ncalls, at.calc.nhessians
    HV = at.calc.cell_hessian_vector_product(at, V)
    assert HV.shape == (k, dim)
    assert at.calc.ncalls == calls and at.calc.nhessians == hessians   # neither a force call nor a Hessian
    assert at.calc.ncellhvps == 1
    tol = bound(H, V)
    err = float(np.abs(HV - V @ H).max())
    print(f'{name} k={k}: max|HV - H V| {err:.2e}  bound {tol:.2e}  ratio {err / tol:.3f}')
    assert err <= tol
    one = at.calc.cell_hessian_vector_product(at, V[0])                # a single vector keeps its shape
    assert one.shape == (dim,) and np.array_equal(one, HV[0])
    assert at.calc.ncalls == calls and at.calc.nhessians == hessians and at.calc.ncellhvps == 2


# ---- 2. lists against sweep ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow'])
def test_lists_against_sweep(ctx, name):
    at = make_case(name)
    dim = at.positions.size + 9
    V = np.random.RandomState(5).normal(size=(5, dim))
    args = cell_args(at, emt_args(at))
    HV = ctx.emt_cell_hvp(*args, V)
    with ctx.options(emt_hcap=1):                                      # (the alloy's lists overflow in every workgroup)
        assert np.array_equal(ctx.emt_cell_hvp(*args, V), HV)
    wide = cell_args(at, overflowing_args(at))                         # sweep against lists in every workgroup
    HVw = ctx.emt_cell_hvp(*wide, V)
    with ctx.options(emt_hcap=1):
        assert np.array_equal(ctx.emt_cell_hvp(*wide, V), HVw)
    Hw = ctx.emt_cell_hessian(*wide).numpy()
    err, tol = float(np.abs(HVw - V @ Hw).max()), bound(Hw, V)
    print(f'{name}: opened cutoff  max|HV - H V| {err:.2e}  bound {tol:.2e}  ratio {err / tol:.3f}')
    assert err <= tol


# ---- 3. against the Richardson directional derivative -------------------------------------------------------------------
def reach(atoms, v, W):
    """max over the visits (pairs inside the cutoff, an atom's own images included) of |v_j - v_i + n_s W|: how far a unit
    step along [v; W] moves a pair, with the device calculator's own images and cutoff."""
    nimg = image_indices(atoms)
    S = atoms.calc._setup[1]
    pos, v = atoms.positions, v.reshape(-1, 3)
    out = 0.0
    for sft, n in zip(S['shifts'], nimg):
        r = np.linalg.norm(pos[None, :, :] + sft - pos[:, None, :], axis=2)
        inside = (r < S['cutoff']) & (r > 1e-8)
        dd = v[None, :, :] - v[:, None, :] + n @ W
        if inside.any():
            out = max(out, float(np.linalg.norm(dd, axis=2)[inside].max()))
    return out


def central_direction(atoms, v, W, h):
    x0, C0 = atoms.positions.copy(), np.array(atoms.cell, dtype=float)
    out = []
    try:
        for sign in (1.0, -1.0):
            atoms.positions = x0 + sign * h * v.reshape(-1, 3)
            atoms.set_cell(C0 + sign * h * W, scale_atoms=False)
            out.append(full_gradient(atoms))
    finally:
        atoms.positions = x0
        atoms.set_cell(C0, scale_atoms=False)
    return (out[0] - out[1]) / (2 * h)


@pytest.mark.parametrize('name', ['Cu', 'narrow'])
def test_product_matches_richardson_directional_derivative(ctx, name):
    """Directions of reach 1 displace a pair by at most h max(1, |n_s|) under a step h, as far as the coordinate steps of
    the yardstick do, so the directional extrapolant carries the error estimated there."""
    _, est = yardstick(name)
    at = make_case(name)
    n = at.positions.size
    assert cell_cutoff_gap(at) > 1.5 * H_STEP
    V = np.random.RandomState(2).normal(size=(3, n + 9))
    for row in V:
        row /= reach(at, row[:n], row[n:].reshape(3, 3))
        assert abs(reach(at, row[:n], row[n:].reshape(3, 3)) - 1.0) < 1e-12
    D = np.array([(4 * central_direction(at, row[:n], row[n:].reshape(3, 3), H_STEP / 2)
                   - central_direction(at, row[:n], row[n:].reshape(3, 3), H_STEP)) / 3 for row in V])
    HV = at.calc.cell_hessian_vector_product(at, V)
    err = float(np.abs(HV - D).max())
    print(f'{name}: max|HV - D| {err:.2e}  estimate {est:.2e}  ratio {err / est:.2f}  max|D| {np.abs(D).max():.3f}')
    assert err <= 10 * est


# ---- 4. structure -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow'])
def test_product_structure(ctx, name):
    at = make_case(name)
    n = at.positions.size
    H = dense(name)
    rng = np.random.RandomState(4)
    V = rng.normal(size=(4, n + 9))
    V[2, n:] = 0.0                                                     # W = 0: the product at fixed cell in the first 3N
    V[3, :n] = np.tile(rng.normal(size=3), n // 3)                     # a rigid translation, W = 0
    V[3, n:] = 0.0
    HV = at.calc.cell_hessian_vector_product(at, V)
    tol = bound(H, V)
    sym = abs(float(V[0] @ HV[1] - V[1] @ HV[0]))
    print(f'{name}: |u.Hv - v.Hu| {sym:.2e}  bound {2 * tol:.2e}  translation {np.abs(HV[3]).max():.2e}')
    assert sym <= 2 * tol                                              # u . (H v) = v . (H u)
    assert np.abs(HV[3]).max() <= 1e-10 * np.abs(H).max()              # the cap of the acoustic sums elsewhere
    fixed = at.calc.hessian_vector_product(at, V[2, :n])
    assert np.abs(HV[2, :n] - fixed).max() <= tol
    if ctx.backend == 'emu':
        # the position rows are the arithmetic of the product at fixed cell (one gather body, csrc/emt_hessian.hip): bit for
        # bit where nothing is contracted; on the device the 8- and the 4-vector instantiation may fuse differently
        assert np.array_equal(HV[2, :n], fixed)
    assert np.array_equal(at.calc.cell_hessian_vector_product(at, V), HV)


# ---- 5. the operator in the coordinates of CellCartesianPES -----------------------------------------------------------------
UPPER = np.triu(np.ones((3, 3), dtype=bool))
STRAIN = np.array([[0.020, 0.025, -0.015], [-0.010, -0.022, 0.018], [0.012, -0.020, 0.026]])     # 2-3 %, not symmetric


@pytest.mark.parametrize('mask,pressure,source', [(UPPER, 0.01, 'calculator'), (None, 0.0, 'calculator'), (UPPER, 0.01, 'callable')],
                         ids=['upper-pressure', 'full', 'callable'])
def test_operator_in_pes_coordinates(ctx, mask, pressure, source):
    """After the strain U != 0 and dE/dC != 0, so the second derivative of the exponential map counts.  The operator must
    agree with the converted dense Hessian within the bound of a dim-term dot product plus the two nine-term contractions
    with J on either side."""
    from sella_amd.peswrapper import CellCartesianPES
    at = jittered_cell(1)
    seen = []

    def product(atoms, V):
        seen.append(V.shape)
        return V @ atoms.calc.get_cell_hessian(atoms)

    pes = CellCartesianPES(at, cell_mask=mask, scalar_pressure=pressure,
                           cell_hessian_vector_product=True if source == 'calculator' else product)
    at.set_cell(np.array(at.cell) @ (np.eye(3) + STRAIN), scale_atoms=True)
    dim, nc = pes.dim, pes.ncart
    assert dim == nc + (6 if mask is not None else 9)
    assert np.abs(pes.get_x()[nc:]).max() > 0.01 * pes.exp_cell_factor
    assert np.abs(pes.get_g()[nc:]).max() > 1e-3                       # dE/dC != 0
    Hp = pes._convert_cell_hessian(at.calc.get_cell_hessian(at))
    assert Hp.shape == (dim, dim)
    v = np.random.RandomState(3).normal(size=(3, dim))
    calls, neval = at.calc.ncalls, pes.neval
    y = pes._hvp(v)
    assert y.shape == (3, dim) and at.calc.ncalls == calls and pes.neval == neval
    tol = 2 * (dim + 18) * EPS * np.abs(Hp).sum(axis=1).max() * np.abs(v).max()
    err = float(np.abs(y - v @ Hp).max())
    print(f'{source} m={dim - nc} p={pressure}: max|y - Hp v| {err:.2e}  bound {tol:.2e}  ratio {err / tol:.3f}')
    assert err <= tol
    if source == 'callable':
        assert seen == [(3, nc + 9)]
    else:
        assert at.calc.ncellhvps == 1
    # J, G and the pV term are computed once per geometry, not per product
    pes._expm_derivatives = lambda U: pytest.fail('the derivatives of the exponential map were computed again')
    assert np.array_equal(pes._hvp(v), y)


# ---- 6. runs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rep', [1, pytest.param(2, marks=pytest.mark.emu_heavy)], ids=['4atoms', '32atoms'])
def test_cell_minimum_with_exact_products(ctx, monkeypatch, rep):
    """The criterion of test_emt_cell_hessian.py's run: both runs stop with every force below fmax and every cell gradient
    below smax; around the minimum E - E_min <= |g|^2 / (2 lambda_min) with |g|^2 <= N fmax^2 + n_cell smax^2 and lambda_min
    the smallest eigenvalue of the Hessian off its (at most six) zero modes; two runs, each within that of the minimum,
    differ by at most twice it.
    lambda_min is taken where the bound needs it, at the minimum: the run with the dense Hessian is continued to 1e-6 for
    it.  At its 1e-3 end point the rotations of cell and atoms together, zero modes of the minimum, still have curvatures of
    the order of the residual gradient (-4.6e-5, -3.7e-5 from this start, both runs alike), above the 1e-6 lambda_max line
    that separates zero modes there."""
    from sella_amd import Sella, peswrapper
    fmax = smax = 1e-3
    monkeypatch.setattr(peswrapper, 'NumericalHessian',
                        lambda *a, **kw: pytest.fail('finite differences of the gradient ran with exact products'))
    at = jittered_cell(rep)
    opt = Sella(at, order=0, eig=True, optimize_cell=True, cell_hessian_vector_product=True, logfile=None)
    opt.run(1e-3, 200)
    assert opt.converged()
    pes = opt.pes
    done, worst_force, _, worst_cell = pes.converged(fmax, smax=smax)
    assert done and worst_force < fmax and worst_cell < smax
    assert pes.nhvp > 0 and 0 < at.calc.ncellhvps <= pes.nhvp and at.calc.nhessians == 0
    # one force call per step and one at the start (this driver rejects no step): none came from a product
    assert pes.neval <= opt.nsteps + 1
    monkeypatch.undo()
    dense_run = jittered_cell(rep)
    opt0 = Sella(dense_run, order=0, eig=True, optimize_cell=True, hessian_function=dense_run.calc.get_device_cell_hessian,
                 logfile=None)
    opt0.run(1e-3, 200)
    assert opt0.converged()
    diff, steps0 = abs(at.get_potential_energy() - dense_run.get_potential_energy()), opt0.nsteps
    opt0.run(1e-6, 200)
    assert opt0.converged()
    w = np.linalg.eigvalsh(opt0.pes._convert_cell_hessian(dense_run.calc.get_cell_hessian(dense_run)))
    zero = np.abs(w) < 1e-6 * w[-1]
    lam_min = w[~zero].min()
    assert zero.sum() <= 6 and lam_min > 0, w[:8]
    tol = 2 * (len(at) * fmax ** 2 + pes.n_cell_dof * smax ** 2) / (2 * lam_min)
    print(f'spectrum {w[:8]}  lambda_max {w[-1]:.3f}')
    print(f'steps {opt.nsteps} / {steps0}  products {pes.nhvp}  force calls {pes.neval}  lambda_min {lam_min:.3e}  '
          f'|dE| {diff:.2e}  bound {tol:.2e}')
    assert diff <= tol


# ---- 7. refusals and invalid arguments --------------------------------------------------------------------------------------
def test_wrong_arguments_are_invalid(ctx):
    from ctypes import c_double
    from sella_amd import _lib
    from sella_amd._lib import ptr
    L = _lib.lib()
    at = make_case('narrow')
    pos, par, shifts, rc, acut, cutoff, beta = emt_args(at)
    cell = np.array(at.cell, dtype=float)
    n, ns = len(pos), len(shifts)
    tail = (c_double(rc), c_double(acut), c_double(cutoff), c_double(beta))
    V = np.random.RandomState(0).normal(size=(2, 3 * n + 9))
    HV = np.zeros_like(V)

    def call(cell=cell, V=V, k=2, HV=HV, n=n, ns=ns):
        status = L.sella_emt_cell_hvp(ctx._h, n, ptr(pos), ptr(par), ns, ptr(shifts), ptr(cell), *tail, ptr(V), k, ptr(HV))
        return status, L.sella_last_error().decode()
    for kwargs in (dict(k=0), dict(V=None), dict(HV=None), dict(cell=None), dict(n=0), dict(ns=0), dict(ns=128)):
        status, message = call(**kwargs)
        assert status == INVALID and message, kwargs
    flat = cell.copy()
    flat[2] = flat[0] + flat[1]
    status, message = call(cell=flat)                                  # a singular cell
    assert status == INVALID and 'singular' in message
    status, message = call(cell=np.ascontiguousarray(cell * 1.01))     # the shifts are another cell's translations
    assert status == INVALID and 'no lattice translation' in message
    assert call()[0] == 0
    assert np.array_equal(HV, at.calc.cell_hessian_vector_product(at, V))
    with pytest.raises(ValueError):
        ctx.emt_cell_hvp(pos, par, shifts, cell, rc, acut, cutoff, beta, np.zeros((2, 3 * n + 8)))
    with pytest.raises(ValueError, match=str(3 * n + 9)):
        at.calc.cell_hessian_vector_product(at, np.zeros(3 * n))


def test_refusals(ctx):
    from sella_amd import Sella
    from sella_amd.atoms import EMT, Calculator, MorseCluster, supports_cell_hvp
    from sella_amd.peswrapper import CellCartesianPES
    at = make_case('narrow')
    with pytest.raises(ValueError, match='optimize_cell'):
        Sella(at, order=0, cell_hessian_vector_product=True, logfile=None)
    with pytest.raises(ValueError, match='two sources of curvature'):
        Sella(at, order=0, optimize_cell=True, hessian_function=at.calc.get_device_cell_hessian,
              cell_hessian_vector_product=True, logfile=None)
    with pytest.raises(TypeError):
        CellCartesianPES(at, cell_hessian_vector_product=3)
    morse = make_case('narrow')
    morse.calc = MorseCluster()
    with pytest.raises(NotImplementedError, match='MorseCluster'):
        CellCartesianPES(morse, cell_hessian_vector_product=True)
    with pytest.raises(NotImplementedError, match='MorseCluster'):
        MorseCluster().cell_hessian_vector_product(at, np.zeros(21))
    with pytest.raises(NotImplementedError):
        Calculator().cell_hessian_vector_product(at, np.zeros(21))
    assert supports_cell_hvp(EMT())
    assert not supports_cell_hvp(MorseCluster()) and not supports_cell_hvp(None)
    plain = CellCartesianPES(at)
    assert plain._hvp is None and plain.nhvp == 0                      # without the keyword nothing is resolved


# ---- 8. sizes of the device ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('size', [(8, 8, 16), (10, 10, 11)], ids=['N1024', 'N1100'])
def test_large_sizes(hip_ctx, size):
    """N = 1024: the largest size with the positions staged in LDS; N = 1100: unstaged, and not a multiple of the 256
    threads.  Sixteen vectors (four groups) against the dense Hessian of the same geometry."""
    at = slab(size, seed=len(size) + size[2])
    n = at.positions.size
    assert n == 3 * size[0] * size[1] * size[2]
    H = at.calc.get_cell_hessian(at)
    V = np.random.RandomState(16).normal(size=(16, n + 9))
    HV = at.calc.cell_hessian_vector_product(at, V)
    err, tol = float(np.abs(HV - V @ H).max()), bound(H, V)
    print(f'N={n // 3}: max|HV - H V| {err:.2e}  bound {tol:.2e}  ratio {err / tol:.3f}')
    assert err <= tol
