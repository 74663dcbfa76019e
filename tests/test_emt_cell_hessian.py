"""The analytic EMT Hessian of positions and cell (`sella_emt_cell_hessian`; csrc/emt_hessian.hip), the `Calculator`
methods on top of it, its transformation into the coordinates of `CellCartesianPES`, and
`Sella(..., optimize_cell=True, hessian_function=calc.get_device_cell_hessian)`.

Coordinates of the device result: [x (3N Cartesian positions); C.ravel() (nine cell entries, row-major, lattice vectors in
the rows)], the positions held fixed while C varies (`set_cell(scale_atoms=False)`).

Yardstick, by the convention of test_emt_hessian.py: the Richardson extrapolant (4 D_{h/2} - D_h) / 3 of central
differences of a gradient that has tests of its own — the device's [-forces; dEdC], dEdC = solve(C^T, V sigma + pos^T f)
from `get_stress` / `get_forces` (pinned in test_cell_optimization.py).  Its error is estimated from itself (the asymmetry
of its 9 x 9 block; the difference between the cell columns, from displaced cell entries, and the transposed block, from
displaced positions and differenced dEdC), and the analytic result must lie within 10 x the estimate.

A step h of a cell entry moves a pair distance by at most h max_k |n_sk| (n_s the image index of the visit), so no pair
may come within that of the cutoff: `cell_cutoff_gap`, asserted per case."""
import numpy as np
import pytest

from test_cell_optimization import fcc_cubic
from test_emt_hessian import H_STEP, emt_args, hip_ctx, jittered_cell, list_counts, make_case, overflowing_args, slab  # noqa: F401

INVALID = -1                                            # SELLA_E_INVALID


# ---- the yardstick -----------------------------------------------------------------------------------------------------
def image_indices(atoms):
    atoms.calc._prepare(atoms)
    n = atoms.calc._setup[1]['shifts'] @ np.linalg.inv(np.asarray(atoms.cell, dtype=float))
    assert np.abs(n - np.rint(n)).max() < 1e-9
    return np.rint(n)


def cell_cutoff_gap(atoms):
    """Smallest |r - cutoff| / max(1, |n_s|_inf) over all visits, with the device calculator's own images and cutoff."""
    nimg = image_indices(atoms)
    S = atoms.calc._setup[1]
    pos = atoms.positions
    gap = np.inf
    for sft, n in zip(S['shifts'], nimg):
        r = np.linalg.norm(pos[None, :, :] + sft - pos[:, None, :], axis=2)
        gap = min(gap, float(np.abs(r - S['cutoff']).min()) / max(1.0, float(np.abs(n).max())))
    return gap


def full_gradient(atoms):
    """[dE/dx; dE/dC] (3N + 9) at fixed Cartesian positions, from the device's forces and stress."""
    from sella_amd.atoms import voigt_to_matrix
    sigma = voigt_to_matrix(atoms.get_stress())
    f = atoms.get_forces()
    C = np.array(atoms.cell, dtype=float)
    dEdC = np.linalg.solve(C.T, abs(np.linalg.det(C)) * sigma + atoms.positions.T @ f)
    return np.concatenate([-f.ravel(), dEdC.ravel()])


def central(atoms, k, h):
    """(G(q + h e_k) - G(q - h e_k)) / 2h of the full gradient along coordinate k of [x; C.ravel()]; the geometry is put
    back."""
    n = atoms.positions.size
    x0, C0 = atoms.positions.copy(), np.array(atoms.cell, dtype=float)
    out = []
    try:
        for sign in (1.0, -1.0):
            if k < n:
                x = x0.ravel().copy()
                x[k] += sign * h
                atoms.positions = x.reshape(-1, 3)
            else:
                C = C0.ravel().copy()
                C[k - n] += sign * h
                atoms.set_cell(C.reshape(3, 3), scale_atoms=False)
            out.append(full_gradient(atoms))
    finally:
        atoms.positions = x0
        atoms.set_cell(C0, scale_atoms=False)
    return (out[0] - out[1]) / (2 * h)


def richardson(atoms, k, h=H_STEP):
    return (4 * central(atoms, k, h / 2) - central(atoms, k, h)) / 3


_YARDSTICKS = {}


def yardstick(name):
    """(R (3N + 9, 9): the cell columns, estimate of its error) of a case, computed once per session (from the device
    gradient of whichever backend asks first: the two agree far below the estimate)."""
    if name not in _YARDSTICKS:
        at = make_case(name)
        n = at.positions.size
        assert cell_cutoff_gap(at) > 1.5 * H_STEP
        R = np.array([richardson(at, n + q) for q in range(9)]).T
        # ... and rows of the transposed block, from displaced positions and differenced dEdC: all twelve of the narrow
        # cell, every eighth coordinate (x, y and z four times each) of the 32-atom cells
        rows = list(range(0, n, max(1, n // 12)))
        T = np.array([richardson(at, k)[n:] for k in rows])
        est = max(float(np.abs(R[n:] - R[n:].T).max()), float(np.abs(R[rows] - T).max()))
        _YARDSTICKS[name] = (R, est)
    return _YARDSTICKS[name]


# ---- 1. against the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow'])
def test_cell_columns_match_richardson_yardstick(ctx, name):
    R, est = yardstick(name)
    at = make_case(name)
    n = at.positions.size
    before = at.calc.ncalls
    H = at.calc.get_cell_hessian(at)
    assert H.shape == (n + 9, n + 9)
    assert at.calc.ncalls == before and at.calc.nhessians == 1         # not a force call
    e_cols, e_cell = float(np.abs(H[:n, n:] - R[:n]).max()), float(np.abs(H[n:, n:] - R[n:]).max())
    print(f'{name}: max|R| {np.abs(R).max():.3f}  estimate {est:.2e}  max|A - R| {e_cols:.2e}  max|B - R| {e_cell:.2e}  '
          f'ratio {max(e_cols, e_cell) / est:.2f}')
    assert est < 1e-6 * np.abs(R).max()                                # the yardstick itself is sound
    assert e_cols <= 10 * est and e_cell <= 10 * est
    if name == 'narrow':
        assert len(at.calc._setup[1]['shifts']) == 125                 # really the many-image case: own images, |n| = 2
        assert np.abs(image_indices(at)).max() == 2


# ---- 2. structure ------------------------------------------------------------------------------------------------------------
def cell_args(atoms, args):
    pos, par, shifts, *tail = args
    return (pos, par, shifts, np.array(atoms.cell, dtype=float), *tail)


@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow'])
def test_cell_hessian_structure(ctx, name):
    at = make_case(name)
    n = at.positions.size
    args = cell_args(at, emt_args(at))
    H = ctx.emt_cell_hessian(*args).numpy()
    assert np.array_equal(H, H.T)
    assert np.array_equal(H[:n, :n], at.calc.get_hessian(at))          # the passes of sella_emt_hessian, bit for bit
    assert np.array_equal(at.calc.get_cell_hessian(at), H)
    # a rigid translation changes neither a force nor dE/dC: the cap of the acoustic sums of test_emt_hessian.py
    sums = np.abs(H[:n, n:].reshape(n // 3, 3, 9).sum(axis=0)).max()
    assert sums <= 1e-10 * np.abs(H).max()
    with ctx.options(emt_hcap=1):                                      # (the alloy's lists overflow in every workgroup)
        assert np.array_equal(ctx.emt_cell_hessian(*args).numpy(), H)
    wide = cell_args(at, overflowing_args(at))                         # sweep against lists in every workgroup
    Hw = ctx.emt_cell_hessian(*wide).numpy()
    with ctx.options(emt_hcap=1):
        assert np.array_equal(ctx.emt_cell_hessian(*wide).numpy(), Hw)
    assert np.array_equal(Hw, Hw.T)
    assert np.abs(Hw[:n, n:].reshape(n // 3, 3, 9).sum(axis=0)).max() <= 1e-10 * np.abs(Hw).max()
    assert np.array_equal(Hw[:n, :n], ctx.emt_hessian(*overflowing_args(at)).numpy())


def test_cell_hessian_is_cached_per_geometry(ctx):
    at = make_case('Cu')
    H = at.calc.get_cell_hessian(at)
    dH = at.calc.get_device_cell_hessian(at)
    assert at.calc.nhessians == 1 and np.array_equal(dH.numpy(), H)
    dH.free()                                                          # the caller's own copy: the cache is untouched
    assert np.array_equal(at.calc.get_cell_hessian(at), H) and at.calc.nhessians == 1
    at.positions[0, 0] += 0.01
    assert not np.array_equal(at.calc.get_cell_hessian(at), H) and at.calc.nhessians == 2
    at.set_cell(at.cell * 1.001)                                       # the cell alone: a new geometry too
    at.calc.get_cell_hessian(at)
    assert at.calc.nhessians == 3 and at.calc.ncalls == 0


# ---- 3. the transformation into the coordinates of CellCartesianPES --------------------------------------------------------------
MASKS = dict(full=np.ones((3, 3), dtype=bool), upper=np.triu(np.ones((3, 3), dtype=bool)), diagonal=np.eye(3, dtype=bool))
# the first seeds of the test point whose pair distances keep 1.5 H_STEP away from the cutoff (5.7e-3, 3.7e-3, 2.3e-3)
SEEDS = dict(full=1, upper=10, diagonal=1)


def pes_richardson(pes, x0, k, h):
    def quotient(step):
        g = []
        for sign in (1.0, -1.0):
            x = x0.copy()
            x[k] += sign * step
            pes.set_x(x)
            g.append(pes.eval()[1])
        pes.set_x(x0)
        return (g[0] - g[1]) / (2 * step)
    return (4 * quotient(h / 2) - quotient(h)) / 3


@pytest.mark.parametrize('mask,pressure', [('full', 0.0), ('upper', 0.0), ('diagonal', 0.0), ('full', 0.01)],
                         ids=['full', 'upper', 'diagonal', 'pressure'])
def test_transformation_to_pes_coordinates(ctx, mask, pressure):
    """`pes.H` after `calculate_hessian()` against the Richardson extrapolant of central differences of the PES's own
    gradient, at a point with U != 0: all cell parameters (steps H_STEP exp_cell_factor, so the cell moves by H_STEP)
    and a handful of positions.  The estimate of the yardstick's error: the asymmetry of its parameter block, and its
    parameter columns against the parameter rows of its position columns.

    The cutoff precondition asserted is that of the position steps.  A parameter step strains the cell by H_STEP, which
    moves a pair through image n_s by up to H_STEP |n_s C|, about 1e-2 A for the far images; the 32-atom cell has pairs
    that close to the cutoff at every test point tried (400 seeds), so some cross it inside the parameter steps.  The
    cutoff function is 1.4e-6 there, and by the size of the pair terms one crossing changes a difference quotient of the
    parameter gradient by several 1e-8: the yardstick's parameter columns are good to about 1e-7 only, which its own
    estimate shows (1.2e-7 to 1.4e-7, against 1e-10 for the columns of test 1), while the position columns agree with
    the analytic ones to 3e-10.  Measured max |H_p - R|: 1.5e-7 (full, with and without pressure), 2.9e-7 (upper),
    8.9e-7 (diagonal: 7.7 estimates), the same on both backends."""
    from sella_amd.peswrapper import CellCartesianPES
    at = make_case('Cu')
    pes = CellCartesianPES(at, cell_mask=MASKS[mask], scalar_pressure=pressure, hessian_function=at.calc.get_cell_hessian)
    dev = CellCartesianPES(at, cell_mask=MASKS[mask], scalar_pressure=pressure,      # (the same reference cell)
                           hessian_function=at.calc.get_device_cell_hessian)
    nc, m, fac = pes.ncart, pes.n_cell_dof, pes.exp_cell_factor
    rng = np.random.RandomState(SEEDS[mask])
    x0 = pes.get_x()
    x0[:nc] += 0.02 * rng.normal(size=nc)
    x0[nc:] += 0.02 * fac * rng.uniform(0.5, 1.0, size=m) * rng.choice([-1.0, 1.0], size=m)
    pes.set_x(x0)
    x0 = pes.get_x()
    assert np.abs(x0[nc:]).min() > 0.005 * fac
    assert cell_cutoff_gap(at) > 1.5 * H_STEP
    pes.get_g()
    before = at.calc.ncalls
    pes.calculate_hessian()
    assert at.calc.ncalls == before                                    # dEdC of this geometry: a cache hit
    B = pes.H.B.copy()
    assert B.shape == (nc + m, nc + m) and np.array_equal(B, B.T)
    assert np.array_equal(B[:nc, :nc], at.calc.get_hessian(at))
    dev.get_g()
    dev.calculate_hessian()
    assert np.array_equal(dev.H.B, B)                                  # array and DeviceMatrix: the same B bit for bit
    some = [0, 31, 47, 62, 95]
    Rp = np.array([pes_richardson(pes, x0, nc + q, H_STEP * fac) for q in range(m)]).T          # (dim, m)
    Rx = np.array([pes_richardson(pes, x0, k, H_STEP) for k in some]).T                         # (dim, 5)
    est = max(float(np.abs(Rp[nc:] - Rp[nc:].T).max()), float(np.abs(Rp[some] - Rx[nc:].T).max()))
    scale = max(np.abs(Rp).max(), np.abs(Rx).max())
    e_p, e_x = float(np.abs(B[:, nc:] - Rp).max()), float(np.abs(B[:, some] - Rx).max())
    print(f'{mask} p={pressure}: max|R| {scale:.3f}  estimate {est:.2e}  max|H_p - R| {e_p:.2e}  max|H_x - R| {e_x:.2e}')
    assert est < 1e-6 * scale
    assert e_p <= 10 * est and e_x <= 10 * est


# ---- 4. the driver -----------------------------------------------------------------------------------------------------------------
def sheared_cell():
    at = jittered_cell(1)
    shear = np.eye(3) + 0.03 * np.random.RandomState(2).normal(size=(3, 3))
    at.set_cell(at.cell @ shear, scale_atoms=True)
    return at


def test_cell_minimum_with_the_calculators_own_hessian(ctx, monkeypatch):
    """Both runs stop with every force below fmax and every cell gradient below smax.  Around the minimum
    E - E_min <= |g|^2 / (2 lambda_min) with |g|^2 <= N fmax^2 + n_cell smax^2 and lambda_min the smallest eigenvalue of the
    Hessian off its zero modes (translations, and rotations of cell and atoms together: the gradient has no component
    along them); two runs, each within that of the minimum, differ by at most twice it."""
    from sella_amd import Sella
    from sella_amd.peswrapper import PES, CellCartesianPES
    fmax = smax = 1e-3
    monkeypatch.setattr(PES, 'diag', lambda self, **kw: pytest.fail('Davidson ran with a hessian_function'))
    monkeypatch.setattr(CellCartesianPES, '_cell_hessian_columns',
                        lambda self, delta: pytest.fail('finite differences ran with a hessian_function'))
    at = sheared_cell()
    opt = Sella(at, order=0, eig=True, optimize_cell=True, smax=smax, hessian_function=at.calc.get_device_cell_hessian,
                refine_initial_hessian=True, logfile=None)
    opt.run(fmax=fmax, steps=200)
    assert opt.converged() and at.calc.nhessians >= 1
    monkeypatch.undo()
    plain = sheared_cell()
    opt0 = Sella(plain, order=0, optimize_cell=True, smax=smax, logfile=None)
    opt0.run(fmax=fmax, steps=400)
    assert opt0.converged()
    w = np.linalg.eigvalsh(opt.pes._convert_cell_hessian(at.calc.get_cell_hessian(at)))
    zero = np.abs(w) < 1e-6 * w[-1]
    lam_min = w[~zero].min()
    print(f'steps {opt.nsteps} / {opt0.nsteps}  zero modes {zero.sum()}  spectrum {w[:8]}  lambda_max {w[-1]:.3f}')
    assert zero.sum() <= 6 and lam_min > 0, w[:8]
    tol = 2 * (len(at) * fmax ** 2 + opt.pes.n_cell_dof * smax ** 2) / (2 * lam_min)
    diff = abs(at.get_potential_energy() - plain.get_potential_energy())
    print(f'lambda_min {lam_min:.3e}  |dE| {diff:.2e}  bound {tol:.2e}')
    assert diff <= tol


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_fixed_cell_hessian_in_a_cell_run_is_refused(ctx):
    from sella_amd.peswrapper import CellCartesianPES
    at = make_case('narrow')
    for fn in (at.calc.get_hessian, at.calc.get_device_hessian):
        pes = CellCartesianPES(at, hessian_function=fn)
        pes.get_g()
        with pytest.raises(ValueError, match=r'21 x 21.*12 x 12.*12 x 12 is the Hessian at fixed cell.*get_device_cell_hessian'):
            pes.calculate_hessian()


def test_calculator_without_cell_hessian(ctx):
    from sella_amd.atoms import EMT, Calculator, MorseCluster, supports_cell_hessian
    at = fcc_cubic('Cu', 3.6, 1)
    assert supports_cell_hessian(EMT())
    assert not supports_cell_hessian(MorseCluster()) and not supports_cell_hessian(None)
    for call in (lambda: MorseCluster().get_cell_hessian(at), lambda: MorseCluster().get_device_cell_hessian(at),
                 lambda: Calculator().get_cell_hessian(at)):
        with pytest.raises(NotImplementedError):
            call()


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
    fixed, right = ctx.zeros(3 * n, 3 * n), ctx.zeros(3 * n + 9, 3 * n + 9)

    def call(cell, out, n=n, ns=ns):
        return L.sella_emt_cell_hessian(ctx._h, n, ptr(pos), ptr(par), ns, ptr(shifts), ptr(cell), *tail, out)
    assert call(cell, fixed.handle) == INVALID
    assert call(cell, -1) == INVALID
    assert call(cell, right.handle, n=0) == INVALID
    assert call(None, right.handle) == INVALID
    flat = cell.copy()
    flat[2] = flat[0] + flat[1]
    assert call(flat, right.handle) == INVALID                         # a singular cell
    assert call(np.zeros((3, 3)), right.handle) == INVALID
    assert call(np.ascontiguousarray(cell * 1.01), right.handle) == INVALID    # the shifts are not its lattice translations
    assert call(cell, right.handle) == 0
    assert np.array_equal(right.numpy(), at.calc.get_cell_hessian(at))
    with pytest.raises(ValueError):
        ctx.emt_cell_hessian(pos, par, shifts, np.zeros(6), rc, acut, cutoff, beta)


# ---- 6. a large size (device only) -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_large_slab(hip_ctx):
    """N = 1100: positions not staged in LDS, N no multiple of the 256 threads, periodic in two directions — the third
    lattice vector is in no image translation.  Yardstick: Richardson directional derivatives of the device gradient along
    the six entries of the periodic lattice vectors, their error estimated as the difference of two successive
    extrapolants (steps h, h/2 and h/2, h/4)."""
    at = slab((10, 10, 11), seed=14)
    n = at.positions.size
    assert n == 3300 and list(at.pbc) == [True, True, False]
    assert cell_cutoff_gap(at) > 1.5 * H_STEP
    H = at.calc.get_cell_hessian(at)
    assert np.array_equal(H, H.T)
    assert np.array_equal(H[:n, :n], at.calc.get_hessian(at))
    assert np.abs(H[:n, n:].reshape(n // 3, 3, 9).sum(axis=0)).max() <= 1e-10 * np.abs(H).max()
    assert not H[n + 6:].any() and not H[:, n + 6:].any()              # the non-periodic lattice vector
    D1 = np.array([richardson(at, n + q, H_STEP) for q in range(6)]).T
    D2 = np.array([richardson(at, n + q, H_STEP / 2) for q in range(6)]).T
    est = float(np.abs(D1 - D2).max())
    err = float(np.abs(H[:, n:n + 6] - D1).max())
    print(f'N={n // 3}: estimate {est:.2e}  max|H - D| {err:.2e}  max|D| {np.abs(D1).max():.3f}')
    assert est < 1e-6 * np.abs(D1).max()
    assert err <= 10 * est
