"""The analytic EMT Hessian and Hessian-vector product (`sella_emt_hessian`, `sella_emt_hvp`, `sella_calc_hessian`,
`sella_calc_hvp`; csrc/emt_hessian.hip), the `Calculator` methods on top of them, and the two PES classes that take them
as `hessian_function`.

Yardstick of the second derivatives: the Richardson extrapolant R = (4 H_{h/2} - H_h) / 3 of central differences of a
GRADIENT that has tests of its own — `EMTOracle`'s (NumPy) where the oracle covers the cell, the device gradient
(`sella_emt_eval`) where it does not (cells narrower than the cutoff, sizes the oracle is too slow for).  The yardstick's
own error is estimated from the yardstick alone (its asymmetry; for directional derivatives, the difference of two
successive extrapolants) and the analytic result must lie within 10 x that estimate: the extrapolant and the analytic
Hessian see the gradient's summation order differently, which the factor covers.

The EMT energy jumps by ~1e-4 of a pair term where a pair crosses the cutoff, so a difference quotient is only a
derivative if no pair distance comes within the displacement of the cutoff: asserted per case (`cutoff_gap`), with the
yardstick's own data."""
import numpy as np
import pytest

from oracle.sella_oracle.emt import EMTOracle           # checker only

from conftest import make_context
from test_cell_optimization import distorted, fcc_cubic

H_STEP = 1e-3                                           # displacement of the difference quotients (and H_STEP / 2), Angstrom
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope='module')
def hip_ctx(request):
    """Hardware only, for the sizes of the device (no host emulation of them, on either machine)."""
    yield from make_context(request, 'hip')


# ---- the cases and their yardsticks -----------------------------------------------------------------------------------
def make_case(name):
    from sella_amd.atoms import EMT
    if name == 'Cu':
        at = distorted(np.random.RandomState(7))
    elif name == 'CuAu':
        # seed 6: the first whose pair distances keep 2 H_STEP away from the cutoff (3.5e-3; seeds 0-5 come within 8e-4)
        symbols = [('Au' if k % 3 == 0 else 'Cu') for k in range(32)]
        at = distorted(np.random.RandomState(6), a=3.7, symbols=symbols)
    elif name == 'narrow':
        # one conventional cell, 3.6 A wide: 5^3 images, every atom its own neighbour, every neighbour seen several times
        at = fcc_cubic('Cu', 3.6, 1)
        at.positions += 0.05 * np.random.RandomState(3).normal(size=at.positions.shape)
    else:
        raise KeyError(name)
    at.calc = EMT()
    return at


def pair_distances(pos, shifts):
    return np.concatenate([np.linalg.norm(pos[None, :, :] + sft - pos[:, None, :], axis=2).ravel() for sft in shifts])


def cutoff_gap(atoms, source):
    """Smallest distance of a pair distance from the cutoff, with the images and the cutoff of `source`: 'oracle' or the
    device calculator's own set-up."""
    if source == 'oracle':
        orc = EMTOracle()
        orc.get_potential_energy(atoms)
        S = orc._setup[1]
    else:
        atoms.calc._prepare(atoms)
        S = atoms.calc._setup[1]
    return float(np.abs(pair_distances(atoms.positions, S['shifts']) - S['cutoff']).min())


def oracle_gradient():
    orc = EMTOracle()
    return lambda atoms: -orc.get_forces(atoms).ravel()


def device_gradient(atoms):
    return -atoms.get_forces().ravel()


def central(atoms, gradient, v, h):
    """(g(x + h v) - g(x - h v)) / 2 h; the positions are put back."""
    x0 = atoms.positions.copy()
    try:
        atoms.positions = x0 + h * v.reshape(-1, 3)
        gp = gradient(atoms)
        atoms.positions = x0 - h * v.reshape(-1, 3)
        gm = gradient(atoms)
    finally:
        atoms.positions = x0
    return (gp - gm) / (2 * h)


def richardson_direction(atoms, gradient, v, h=H_STEP):
    return (4 * central(atoms, gradient, v, h / 2) - central(atoms, gradient, v, h)) / 3


def richardson_hessian(atoms, gradient, h=H_STEP):
    n = atoms.positions.size
    return np.array([richardson_direction(atoms, gradient, e, h) for e in np.eye(n)]).T


_YARDSTICKS = {}


def yardstick(name):
    """(R, max |R - R^T|) of a case, computed once per session (the oracle does not depend on the backend; the narrow
    cell's comes from the device gradient of whichever backend asks first — the two agree far below the estimate)."""
    if name not in _YARDSTICKS:
        at = make_case(name)
        source = 'device' if name == 'narrow' else 'oracle'
        assert cutoff_gap(at, source) > 2 * H_STEP
        R = richardson_hessian(at, device_gradient if name == 'narrow' else oracle_gradient())
        _YARDSTICKS[name] = (R, float(np.abs(R - R.T).max()))
    return _YARDSTICKS[name]


def acoustic_residual(H):
    """max_a |sum_b H[a, 3 b + c]|: a rigid translation changes no force."""
    n = H.shape[0]
    return float(np.abs(H.reshape(n, n // 3, 3).sum(axis=1)).max())


def emt_args(atoms):
    from sella_amd.atoms import EMT
    atoms.calc._prepare(atoms)
    S = atoms.calc._setup[1]
    return atoms.positions, S['par'], S['shifts'], S['rc'], S['acut'], S['cutoff'], EMT._BETA


def list_counts(pos, shifts, cutoff):
    """(n, 256) neighbours each thread of atom i's workgroup notes in the density pass: candidate (image s, atom j) belongs
    to thread (s n + j) mod 256 and is noted if its squared distance passes the widened cutoff (emt_pairs_impl).  A thread
    that finds more than `emt_hcap` marks the lists of its atom incomplete, and every later pass sweeps for that atom."""
    n = len(pos)
    cut2 = cutoff * cutoff * (1.0 + 1e-12)
    counts = np.zeros((n, 256), dtype=int)
    for s, sft in enumerate(shifts):
        d = pos[None, :, :] + sft - pos[:, None, :]
        i, j = np.nonzero((d * d).sum(axis=2) <= cut2)
        np.add.at(counts, (i, (s * n + j) % 256), 1)
    return counts


def overflowing_args(atoms):
    """The arguments of `emt_args` with the cutoff opened to rc + 2.5 A, where one slot per thread (emt_hcap = 1) is too
    few in EVERY workgroup of every case here while the eight of the default hold everything: asserted, so the
    comparison of the two really is sweep against lists.  (At EMT's own cutoff only the alloy cell overflows.)"""
    pos, par, shifts, rc, acut, _, beta = emt_args(atoms)
    cutoff = rc + 2.5
    counts = list_counts(pos, shifts, cutoff)
    assert counts.max() <= 8 and (counts.max(axis=1) >= 2).all()
    return pos, par, shifts, rc, acut, cutoff, beta


# ---- 1. against the oracle, 2. the narrow cell ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow'])
def test_hessian_matches_richardson_yardstick(ctx, name):
    R, est = yardstick(name)
    at = make_case(name)
    before = at.calc.ncalls
    H = at.calc.get_hessian(at)
    assert at.calc.ncalls == before and at.calc.nhessians == 1         # not a force call
    err = float(np.abs(H - R).max())
    print(f'{name}: max|H| {np.abs(H).max():.3f}  yardstick asymmetry {est:.2e}  max|H - R| {err:.2e}  ratio {err / est:.2f}')
    assert est < 1e-6 * np.abs(R).max()                                # the yardstick itself is sound
    assert err <= 10 * est
    if name == 'narrow':
        assert len(at.calc._setup[1]['shifts']) == 125                 # really the many-image case


def test_hessian_is_cached_per_geometry(ctx):
    at = make_case('Cu')
    H = at.calc.get_hessian(at)
    dH = at.calc.get_device_hessian(at)
    assert at.calc.nhessians == 1 and np.array_equal(dH.numpy(), H)
    dH.free()                                                          # the caller's own copy: the cache is untouched
    assert np.array_equal(at.calc.get_hessian(at), H) and at.calc.nhessians == 1
    at.positions[0, 0] += 0.01
    assert not np.array_equal(at.calc.get_hessian(at), H) and at.calc.nhessians == 2
    at.set_cell(at.cell * 1.001)                                       # the cell alone: a new geometry too
    at.calc.get_hessian(at)
    assert at.calc.nhessians == 3 and at.calc.ncalls == 0


# ---- 3. structure ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow'])
def test_hessian_structure(ctx, name):
    at = make_case(name)
    args = emt_args(at)
    H = ctx.emt_hessian(*args).numpy()
    assert np.array_equal(H, H.T)
    # a cap against a dropped term (~1e-2), far above the rounding of the row sums (~1e-14)
    assert acoustic_residual(H) <= 1e-10 * np.abs(H).max()
    with ctx.options(emt_hcap=1):                                      # the alloy's lists overflow in every workgroup here,
        assert np.array_equal(ctx.emt_hessian(*args).numpy(), H)       # the other two cells' in none:
    if name == 'CuAu':
        assert (list_counts(args[0], args[2], args[5]).max(axis=1) >= 2).all()
    wide = overflowing_args(at)                                        # ... so once more where all of them do
    Hw = ctx.emt_hessian(*wide).numpy()
    with ctx.options(emt_hcap=1):
        assert np.array_equal(ctx.emt_hessian(*wide).numpy(), Hw)
    assert np.array_equal(Hw, Hw.T) and acoustic_residual(Hw) <= 1e-10 * np.abs(Hw).max()
    at.get_potential_energy()
    resident = at.calc.device_calculator()
    calls = resident.ncalls
    assert np.array_equal(resident.hessian(at.positions).numpy(), H)
    assert resident.ncalls == calls
    assert np.array_equal(at.calc.get_hessian(at), H)


# ---- 4. the product ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['Cu', 'CuAu', 'narrow'])
@pytest.mark.parametrize('k', [1, 5, 11])
def test_product_matches_dense_hessian(ctx, name, k):
    """k = 11: a second group of vectors (eight per workgroup).  Both sides are, per component, sums of at most 3N products h_ab v_b whose factors carry a few roundings each: the
    bound of a 3N-term dot product, 3N eps sum_b |h_ab| |v_b| (Higham, Accuracy and Stability, 3.1), taken against the
    largest row of |H| and the largest component of V, once for either side."""
    at = make_case(name)
    n = at.positions.size
    H = at.calc.get_hessian(at)
    V = np.random.RandomState(k).normal(size=(k, n))
    before = at.calc.ncalls
    HV = at.calc.hessian_vector_product(at, V)
    assert HV.shape == (k, n) and at.calc.ncalls == before
    tol = 2 * n * EPS * np.abs(H).sum(axis=1).max() * np.abs(V).max()
    err = float(np.abs(HV - V @ H).max())
    print(f'{name} k={k}: max|HV - H V| {err:.2e}  bound {tol:.2e}')
    assert err <= tol
    one = at.calc.hessian_vector_product(at, V[0])                     # a single vector keeps its shape
    assert one.shape == (n,) and np.array_equal(one, HV[0])
    with ctx.options(emt_hcap=1):
        assert np.array_equal(ctx.emt_hvp(*emt_args(at), V), HV)
    # the sweep of both product kernels against their list path, where every workgroup's lists overflow, and both
    # against the dense Hessian of the same (opened) cutoff
    wide = overflowing_args(at)
    HVw = ctx.emt_hvp(*wide, V)
    with ctx.options(emt_hcap=1):
        assert np.array_equal(ctx.emt_hvp(*wide, V), HVw)
    Hw = ctx.emt_hessian(*wide).numpy()
    assert np.abs(HVw - V @ Hw).max() <= 2 * n * EPS * np.abs(Hw).sum(axis=1).max() * np.abs(V).max()
    at.get_potential_energy()
    assert np.array_equal(at.calc.device_calculator().hvp(at.positions, V), HV)


@pytest.mark.parametrize('name', ['Cu', 'narrow'])
def test_product_matches_richardson_directional_derivative(ctx, name):
    """Unit directions displace the geometry as far as the coordinate steps of the yardstick do, so the directional
    extrapolant carries the error estimated there."""
    _, est = yardstick(name)
    at = make_case(name)
    n = at.positions.size
    V = np.random.RandomState(2).normal(size=(3, n))
    V /= np.linalg.norm(V, axis=1)[:, None]
    gradient = device_gradient if name == 'narrow' else oracle_gradient()
    D = np.array([richardson_direction(at, gradient, v) for v in V])
    HV = at.calc.hessian_vector_product(at, V)
    err = float(np.abs(HV - D).max())
    print(f'{name}: max|HV - D| {err:.2e}  estimate {est:.2e}')
    assert err <= 10 * est


# ---- 5. large sizes (device only) ------------------------------------------------------------------------------------------------
def slab(size, seed):
    from sella_amd.atoms import EMT, fcc111
    at = fcc111('Cu', size, vacuum=7.5)
    # 0.02 A: the fourth and fifth neighbour shells (5.11, 5.71 A) stay clear of the cutoff (5.27 A)
    at.positions += 0.02 * np.random.RandomState(seed).normal(size=at.positions.shape)
    at.calc = EMT()
    return at


@pytest.mark.gpu
@pytest.mark.parametrize('size', [(8, 8, 16), (10, 10, 11)], ids=['N1024', 'N1100'])
def test_large_sizes(hip_ctx, size):
    """N = 1024: the largest size with the positions staged in LDS; N = 1100: unstaged, and not a multiple of the 256
    threads.  The yardstick is the device gradient; its error is estimated as the difference of two successive Richardson
    extrapolants (steps h, h/2 and h/2, h/4), the usual estimate of the coarser one."""
    at = slab(size, seed=len(size) + size[2])
    n = at.positions.size
    assert n == 3 * size[0] * size[1] * size[2]
    assert cutoff_gap(at, 'device') > 2 * H_STEP
    H = at.calc.get_hessian(at)
    assert np.array_equal(H, H.T)
    assert acoustic_residual(H) <= 1e-10 * np.abs(H).max()
    V = np.random.RandomState(5).normal(size=(8, n))
    V /= np.linalg.norm(V, axis=1)[:, None]
    D1 = np.array([richardson_direction(at, device_gradient, v, H_STEP) for v in V])
    D2 = np.array([richardson_direction(at, device_gradient, v, H_STEP / 2) for v in V])
    est = float(np.abs(D1 - D2).max())
    HV = at.calc.hessian_vector_product(at, V)
    e_dense, e_prod = float(np.abs(V @ H - D1).max()), float(np.abs(HV - D1).max())
    print(f'N={n // 3}: estimate {est:.2e}  max|H v - D| {e_dense:.2e}  max|HV - D| {e_prod:.2e}  max|D| {np.abs(D1).max():.3f}')
    assert est < 1e-6 * np.abs(D1).max()
    assert e_dense <= 10 * est and e_prod <= 10 * est


# ---- 6. the model calculator -------------------------------------------------------------------------------------------------------
def test_model_calculator_hessian_and_product(ctx):
    """f = x.A x / 2 + c / 3 sum_j (u_j . x)^3 has the Hessian A + 2 c sum_j (u_j . x) u_j u_j^T.  Tolerances: the terms
    of an entry are A_ab and nu products p_j u_ja u_jb, p_j an n-term dot product: (n + nu + 4) eps against the sum of
    the absolute values of the terms; the product adds an n-term dot product per component."""
    from sella_amd.atoms import Atoms, QuadraticCubicModel, supports_hessian
    from sella_amd.device import DeviceCalculator
    rng = np.random.RandomState(4)
    n, nu, c = 30, 3, 0.05
    A = rng.normal(size=(n, n))
    A = A + A.T
    U = rng.normal(size=(nu, n))
    x = rng.normal(size=n)
    p = U @ x
    want = A + 2 * c * np.einsum('j,ja,jb->ab', p, U, U)
    terms = np.abs(A) + 2 * abs(c) * np.einsum('j,ja,jb->ab', np.abs(U) @ np.abs(x), np.abs(U), np.abs(U))
    dA = ctx.upload(A)
    calc = DeviceCalculator.model(ctx, dA, U, c)
    H = calc.hessian(x).numpy()
    assert np.abs(H - want).max() <= (n + nu + 4) * EPS * terms.max()
    V = rng.normal(size=(5, n))
    HV = calc.hvp(x, V)
    assert np.abs(HV - V @ want.T).max() <= (2 * n + nu + 4) * EPS * (np.abs(V) @ terms.T).max()
    assert calc.ncalls == 0
    # the same through the host calculator that owns the device matrix
    at = Atoms(['X'] * (n // 3), x.reshape(-1, 3))
    at.calc = QuadraticCubicModel(lambda v: A @ v, U, c, device_matrix=dA)
    assert supports_hessian(at.calc)
    assert np.array_equal(at.calc.get_hessian(at), H)
    assert np.array_equal(at.calc.get_device_hessian(at).numpy(), H)
    assert np.array_equal(at.calc.hessian_vector_product(at, V), HV)
    plain = QuadraticCubicModel(A, U, c)                               # no device matrix: no library form, no Hessian
    assert not supports_hessian(plain)
    with pytest.raises(NotImplementedError):
        plain.get_hessian(at)


# ---- 7. the driver -----------------------------------------------------------------------------------------------------------------
def jittered_cell(rep):
    from sella_amd.atoms import EMT
    at = fcc_cubic('Cu', 3.6, rep)
    at.positions += 0.05 * np.random.RandomState(1).normal(size=at.positions.shape)
    at.calc = EMT()
    return at


# 32 atoms: whole searches of that size take minutes fibre by fibre, so the emulation runs the 4-atom cell (12 degrees of
# freedom, 125 images) and the device both
@pytest.mark.parametrize('rep', [1, pytest.param(2, marks=pytest.mark.emu_heavy)], ids=['4atoms', '32atoms'])
@pytest.mark.parametrize('form', ['array', 'device'])
def test_minimum_with_the_calculators_own_hessian(ctx, monkeypatch, form, rep):
    """Both runs stop with every force below fmax.  Around the minimum E - E_min <= g.H^-1 g / 2 <= |g|^2 / (2 lambda_min)
    with |g|^2 <= N fmax^2 and lambda_min the smallest eigenvalue of the Hessian off the three translations (the
    gradient has no component along them); two runs, each within that of the minimum, differ by at most twice it.
    lambda_min is taken from the analytic Hessian at the end point."""
    from sella_amd import Sella
    from sella_amd.device import DeviceMatrix
    from sella_amd.linalg import ApproximateHessian
    from sella_amd.peswrapper import PES
    fmax = 1e-3
    fed, inside = [], []
    real_set_B, real_calculate = ApproximateHessian.set_B, PES.calculate_hessian

    def recording(self, target):
        if inside:                                                     # what calculate_hessian hands to pes.H
            fed.append(type(target))
        return real_set_B(self, target)

    def calculate(self):
        inside.append(1)
        try:
            return real_calculate(self)
        finally:
            inside.pop()
    monkeypatch.setattr(ApproximateHessian, 'set_B', recording)
    monkeypatch.setattr(PES, 'calculate_hessian', calculate)
    monkeypatch.setattr(PES, 'diag', lambda self, **kw: pytest.fail('Davidson ran with a hessian_function'))
    at = jittered_cell(rep)
    fn = at.calc.get_hessian if form == 'array' else at.calc.get_device_hessian
    opt = Sella(at, order=0, eig=True, hessian_function=fn, logfile=None)
    opt.run(fmax=fmax, steps=100)
    assert opt.converged() and at.calc.nhessians >= 1
    assert fed and set(fed) == {DeviceMatrix if form == 'device' else np.ndarray}
    monkeypatch.undo()
    plain = jittered_cell(rep)
    opt0 = Sella(plain, order=0, logfile=None)
    opt0.run(fmax=fmax, steps=200)
    assert opt0.converged()
    w = np.linalg.eigvalsh(at.calc.get_hessian(at))
    assert np.abs(w[:3]).max() < 1e-8 and w[3] > 1e-2, w[:5]          # a minimum: three translations, then curvature
    tol = len(at) * fmax ** 2 / w[3]
    diff = abs(at.get_potential_energy() - plain.get_potential_energy())
    print(f'{form}: steps {opt.nsteps} / {opt0.nsteps}  lambda_min {w[3]:.3f}  |dE| {diff:.2e}  bound {tol:.2e}')
    assert diff <= tol


def cu_cluster():
    from sella_amd.atoms import EMT, Atoms
    d = 2.5
    pos = d * np.array([[0, 0, 0], [1, 0, 0], [0.5, np.sqrt(3) / 2, 0], [0.5, np.sqrt(3) / 6, np.sqrt(2.0 / 3)],
                        [1.5, np.sqrt(3) / 2, 0]])
    at = Atoms(['Cu'] * len(pos), pos + 0.05 * np.random.RandomState(0).normal(size=pos.shape), pbc=False)
    at.calc = EMT()
    return at


def test_internal_conversion_takes_the_device_matrix(ctx):
    from sella_amd.internal import InternalCoordinates
    from sella_amd.peswrapper import InternalPES
    at = cu_cluster()
    pes = InternalPES(at, InternalCoordinates.from_atoms(at))
    H = at.calc.get_hessian(at)
    dH = at.calc.get_device_hessian(at)
    from_array = pes._convert_cartesian_hessian_to_internal(H).numpy()
    from_device = pes._convert_cartesian_hessian_to_internal(dH).numpy()
    assert np.array_equal(from_array, from_device)
    assert np.array_equal(dH.numpy(), H)                               # the caller's matrix is not written to
    with pytest.raises(ValueError, match='15 x 15'):
        pes._convert_cartesian_hessian_to_internal(dH.ctx.zeros(3, 3))


@pytest.mark.emu_heavy
def test_internal_search_with_the_calculators_own_hessian(ctx):
    from sella_amd import Sella
    at = cu_cluster()
    opt = Sella(at, internal=True, order=0, eig=True, hessian_function=at.calc.get_device_hessian, logfile=None)
    opt.run(fmax=1e-3, steps=100)
    assert opt.converged() and at.calc.nhessians >= 1
    assert np.abs(at.get_forces()).max() < 1e-3


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_calculator_without_hessian(ctx):
    from sella_amd.atoms import Calculator, MorseCluster, supports_hessian
    at = fcc_cubic('Cu', 3.6, 1)
    assert not supports_hessian(MorseCluster()) and not supports_hessian(None)
    for call in (lambda: MorseCluster().get_hessian(at), lambda: MorseCluster().get_device_hessian(at),
                 lambda: MorseCluster().hessian_vector_product(at, np.zeros(12)), lambda: Calculator().get_hessian(at)):
        with pytest.raises(NotImplementedError):
            call()
    from sella_amd.atoms import EMT
    assert supports_hessian(EMT())
    with pytest.raises(ValueError, match='12'):
        EMT().hessian_vector_product(at, np.zeros(11))


def test_wrong_shapes_are_invalid_arguments(ctx):
    from ctypes import c_double
    from sella_amd import _lib
    from sella_amd._lib import ptr
    L = _lib.lib()
    INVALID = -1                                                       # SELLA_E_INVALID
    at = make_case('narrow')
    pos, par, shifts, rc, acut, cutoff, beta = emt_args(at)
    n, ns = len(pos), len(shifts)
    tail = (c_double(rc), c_double(acut), c_double(cutoff), c_double(beta))
    small, right = ctx.zeros(3 * n, 3 * n - 1), ctx.zeros(3 * n, 3 * n)
    assert L.sella_emt_hessian(ctx._h, n, ptr(pos), ptr(par), ns, ptr(shifts), *tail, small.handle) == INVALID
    assert L.sella_emt_hessian(ctx._h, n, ptr(pos), ptr(par), ns, ptr(shifts), *tail, -1) == INVALID
    assert L.sella_emt_hessian(ctx._h, 0, ptr(pos), ptr(par), ns, ptr(shifts), *tail, right.handle) == INVALID
    assert L.sella_emt_hessian(ctx._h, n, ptr(pos), ptr(par), 128, ptr(shifts), *tail, right.handle) == INVALID
    V, HV = np.zeros((1, 3 * n)), np.zeros((1, 3 * n))
    assert L.sella_emt_hvp(ctx._h, n, ptr(pos), ptr(par), ns, ptr(shifts), *tail, ptr(V), 0, ptr(HV)) == INVALID
    assert L.sella_emt_hvp(ctx._h, n, ptr(pos), ptr(par), ns, ptr(shifts), *tail, None, 1, ptr(HV)) == INVALID
    at.get_potential_energy()
    resident = at.calc.device_calculator()
    x = np.ascontiguousarray(pos).ravel()
    assert L.sella_calc_hessian(resident._h, ptr(x), small.handle) == INVALID
    assert L.sella_calc_hvp(resident._h, ptr(x), ptr(V), 0, ptr(HV)) == INVALID
    assert L.sella_emt_hessian(ctx._h, n, ptr(pos), ptr(par), ns, ptr(shifts), *tail, right.handle) == 0
    with pytest.raises(ValueError):
        ctx.emt_hvp(pos, par, shifts, rc, acut, cutoff, beta, np.zeros((2, 3 * n + 1)))
