"""The pair-potential calculators on the device (`Morse`, `LennardJones`; `sella_pair_*`, `sella_calc_pair_create`,
csrc/pair.hip): energy, gradient and virial, the dense Hessian, the products and the resident operator, the bounded
lists of the sweep, and the refusals.

Yardsticks: the host classes `PairLJ`, `MorseCluster` and `PeriodicMorse` where they cover the case, and an explicit image
sum in NumPy written here (`image_sum`) where they do not (a cell narrower than 2 rcut, per-atom quantities, the closed
form of the Hessian).  The closed form is itself held to the Richardson extrapolant of the HOST gradient.

Tolerances are forward-error bounds.  A per-atom sum of m_i visit terms is held to 2 (m_i + 8) EPS A_i, A_i the sum of the
absolute values of the uncancelled terms as the yardstick computes them (Morse: D (2 x + x^2), 2 D a (x + x^2), ... with
x = exp(-a (r - r0)); Lennard-Jones: both powers; the shift terms |phi(rc)| and |phi'(rc) (r - rc)| on top); the 8 covers
exp, sqrt, division and the products of a term on either side.  Quantities summed over the atoms on the host (the
energy, the virial) add n EPS times the sum of the absolute per-atom values.  Every comparison prints error / bound."""
import numpy as np
import pytest

from conftest import make_context
from test_cell_optimization import distorted, fcc_cubic, strain_derivatives
from test_emt_hessian import acoustic_residual, list_counts, richardson_hessian
from test_hvp_operator import assert_same_run, davidson_through_callback, every_seventh_pinned, product_bound

EPS = np.finfo(np.float64).eps
H_STEP = 1e-3
E_LJ13 = -44.326801420
R_LJ13 = 1.0818382886
MORSE_CU = dict(D=0.3429, a=1.3588, r0=2.866)           # PeriodicMorse's defaults


@pytest.fixture(scope='module')
def hip_ctx(request):
    """Hardware only, for the sizes of the device."""
    yield from make_context(request, 'hip')


# ---- geometries ---------------------------------------------------------------------------------------------------------------
def icosahedron(radius=R_LJ13):
    g = 0.5 * (1.0 + np.sqrt(5.0))
    v = [(0.0, s1, s2 * g) for s1 in (-1, 1) for s2 in (-1, 1)]
    v = np.array(v + [(b, c, a) for a, b, c in v] + [(c, a, b) for a, b, c in v])
    return np.vstack([np.zeros((1, 3)), radius * v / np.linalg.norm(v[0])])


def cluster(pos):
    from sella_amd.atoms import Atoms
    return Atoms(['X'] * len(pos), pos, pbc=False)


def c13(jitter=0.03, seed=1):
    pos = icosahedron()
    if jitter:
        pos = pos + jitter * np.random.RandomState(seed).normal(size=pos.shape)
    return cluster(pos)


def c257():
    grid = np.array([(i, j, k) for i in range(7) for j in range(7) for k in range(7)], dtype=float)[:257]
    return cluster(1.1 * grid + 0.03 * np.random.RandomState(2).normal(size=(257, 3)))


def wide():
    return distorted(np.random.RandomState(0))


def narrow():
    at = fcc_cubic('Cu', 3.6, 1)
    at.positions += 0.05 * np.random.RandomState(3).normal(size=at.positions.shape)
    return at


# name -> (atoms, form, parameters, rcut)
def make_case(name):
    if name == 'c13-lj':
        return c13(), 'lj', (1.0, 1.0), None
    if name == 'c13-morse':
        return c13(), 'morse', (1.0, 1.0, 1.0), None
    if name == 'c257-lj':
        return c257(), 'lj', (1.0, 1.0), None
    if name == 'c257-morse':
        return c257(), 'morse', (1.0, 1.0, 1.0), None
    if name == 'wide':
        return wide(), 'morse', tuple(MORSE_CU.values()), 3.3
    if name == 'narrow':
        return narrow(), 'morse', tuple(MORSE_CU.values()), 5.0
    raise KeyError(name)


CASES = ['c13-lj', 'c13-morse', 'c257-lj', 'c257-morse', 'wide', 'narrow']
SMALL = ['c13-lj', 'c13-morse', 'wide', 'narrow']


def device_calc(form, params, rcut):
    from sella_amd.atoms import LennardJones, Morse
    return Morse(*params, rcut=rcut) if form == 'morse' else LennardJones(*params, rcut=rcut)


def host_calc(name, form, params):
    """The host class that covers the case, or None (narrow: minimum image does not)."""
    from sella_amd.atoms import MorseCluster, PairLJ, PeriodicMorse
    if name == 'narrow':
        return None
    if name == 'wide':
        return PeriodicMorse(rcut=3.3)
    return MorseCluster(*params) if form == 'morse' else PairLJ(*params)


def shifts_of(at, rcut):
    from sella_amd.atoms import EMT
    return np.zeros((1, 3)) if rcut is None else EMT.image_shifts(at.cell, at.pbc, rcut)


# ---- the yardstick written here: an explicit image sum -------------------------------------------------------------------
def radial(form, params, r):
    """phi, phi', phi'' and the sums of the absolute values of their uncancelled terms."""
    if form == 'morse':
        D, a, r0 = params
        x = np.exp(-a * (r - r0))
        return (D * x * (x - 2), 2 * D * a * (x - x * x), 2 * D * a * a * (2 * x * x - x),
                D * (2 * x + x * x), 2 * D * a * (x + x * x), 2 * D * a * a * (2 * x * x + x))
    eps, sigma = params
    s6 = (sigma / r) ** 6
    s12 = s6 * s6
    return (4 * eps * (s12 - s6), 4 * eps * (6 * s6 - 12 * s12) / r, 4 * eps * (156 * s12 - 42 * s6) / r ** 2,
            4 * eps * (s12 + s6), 4 * eps * (6 * s6 + 12 * s12) / r, 4 * eps * (156 * s12 + 42 * s6) / r ** 2)


def shifted(form, params, rcut, r):
    phi, d1, d2, aphi, ad1, ad2 = radial(form, params, r)
    if rcut is None:
        return phi, d1, d2, aphi, ad1, ad2
    pc, dc = radial(form, params, np.float64(rcut))[:2]
    return (phi - pc - dc * (r - rcut), d1 - dc, d2, aphi + abs(pc) + np.abs(dc * (r - rcut)), ad1 + abs(dc), ad2)


VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
_SUMS = {}


def image_sum(name):
    """Everything the checks need of a case, summed visit by visit over the explicit images (computed once): per-atom
    energies e, gradient g, per-atom virials w, Hessian H; the absolute-term sums Ae, Ag, Aw, AH that go with them; the
    visit counts m (all visits of an atom), mh (n x n: visits per pair of different atoms); and the smallest distance of a
    pair distance from the cutoff."""
    if name in _SUMS:
        return _SUMS[name]
    at, form, params, rcut = make_case(name)
    pos, n = at.positions, len(at)
    cut = np.inf if rcut is None else rcut
    e, Ae, g, Ag = np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
    w, Aw = np.zeros((n, 6)), np.zeros((n, 6))
    H, AH = np.zeros((n, 3, n, 3)), np.zeros((n, 3, n, 3))
    m, mh = np.zeros(n, dtype=int), np.zeros((n, n), dtype=int)
    gap = np.inf
    eye = np.eye(3)
    for sft in shifts_of(at, rcut):
        d = pos[None, :, :] + sft - pos[:, None, :]                     # d[i, j] = x_j + S - x_i
        r = np.linalg.norm(d, axis=2)
        live = r > 1e-8
        gap = min(gap, float(np.abs(r[live] - cut).min()))
        i, j = np.nonzero(live & (r < cut))
        dd, rr = d[i, j], r[i, j]
        phi, d1, d2, aphi, ad1, ad2 = shifted(form, params, rcut, rr)
        u = dd / rr[:, None]
        np.add.at(e, i, 0.5 * phi)
        np.add.at(Ae, i, 0.5 * aphi)
        np.add.at(m, i, 1)
        for k, (a, b) in enumerate(VOIGT):
            np.add.at(w[:, k], i, 0.5 * d1 / rr * dd[:, a] * dd[:, b])
            np.add.at(Aw[:, k], i, 0.5 * ad1 / rr * np.abs(dd[:, a] * dd[:, b]))
        other = i != j                                                  # an own image moves no position block
        i, j, u, rr, d1, d2, ad1, ad2 = i[other], j[other], u[other], rr[other], d1[other], d2[other], ad1[other], ad2[other]
        np.add.at(g, i, -d1[:, None] * u)
        np.add.at(Ag, i, ad1[:, None] * np.abs(u))
        np.add.at(mh, (i, j), 1)
        uu = u[:, :, None] * u[:, None, :]
        K = d2[:, None, None] * uu + (d1 / rr)[:, None, None] * (eye - uu)
        AK = ad2[:, None, None] * np.abs(uu) + (ad1 / rr)[:, None, None] * (eye + np.abs(uu))
        for a in range(3):
            for b in range(3):
                np.add.at(H[:, a, :, b], (i, j), -K[:, a, b])
                np.add.at(H[:, a, :, b], (i, i), K[:, a, b])
                np.add.at(AH[:, a, :, b], (i, j), AK[:, a, b])
                np.add.at(AH[:, a, :, b], (i, i), AK[:, a, b])
    H = H.reshape(3 * n, 3 * n)
    out = dict(e=e, Ae=Ae, g=g, Ag=Ag, w=w, Aw=Aw, H=0.5 * (H + H.T), AH=AH.reshape(3 * n, 3 * n), m=m, mh=mh, gap=gap,
               nshift=len(shifts_of(at, rcut)))
    _SUMS[name] = out
    return out


def bounds(S):
    """The forward-error bounds of the module docstring for E, g (n, 3), the virial (6,) and H (3n, 3n)."""
    n = len(S['m'])
    per = 2 * (S['m'] + 8) * EPS
    bE = float((per * S['Ae']).sum() + n * EPS * np.abs(S['e']).sum())
    bg = per[:, None] * S['Ag']
    bw = (per[:, None] * S['Aw']).sum(axis=0) + n * EPS * np.abs(S['w']).sum(axis=0)
    # a block (i, j) sums the images of j, the diagonal block all visits of i; then (H + H^T) / 2
    terms = np.where(np.eye(n, dtype=bool), (S['m'] + 8)[:, None], S['mh'] + 8)
    bH = 2 * EPS * np.repeat(np.repeat(terms, 3, axis=0), 3, axis=1) * S['AH']
    bH = 0.5 * (bH + bH.T) + EPS * np.abs(S['H'])
    return bE, bg, bw, bH


def report(label, err, bound):
    err, bound = np.asarray(err, dtype=float), np.asarray(bound, dtype=float)
    ratio = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
    print(f'{label}: max error {float(err.max()):.3e}  error / bound {ratio:.3f}')
    assert np.all(err <= bound), label


def pair_args(name):
    at, form, params, rcut = make_case(name)
    return at.positions, form, params, shifts_of(at, rcut), rcut


# ---- 1. energy, gradient, virial ------------------------------------------------------------------------------------------
def test_lj13_energy(ctx):
    at = c13(jitter=0.0)
    at.calc = device_calc('lj', (1.0, 1.0), None)
    from sella_amd.atoms import PairLJ
    assert abs(PairLJ().energy_and_gradient(at.positions)[0] - E_LJ13) < 1e-8      # the geometry is the documented one
    pos = at.positions
    r = np.linalg.norm(pos[None] - pos[:, None], axis=2)[~np.eye(13, dtype=bool)].reshape(13, 12)
    A = 0.5 * radial('lj', (1.0, 1.0), r)[3].sum(axis=1)
    bound = float((2 * (12 + 8) * EPS * A).sum() + 13 * EPS * 2 * abs(E_LJ13)) + 5e-10   # + the nine decimals E_LJ13 is given to
    err = abs(at.get_potential_energy() - E_LJ13)
    report('E(LJ13)', err, bound)


@pytest.mark.parametrize('name', CASES)
def test_energy_gradient_virial(ctx, name):
    at, form, params, rcut = make_case(name)
    S = image_sum(name)
    bE, bg, bw, _ = bounds(S)
    args = pair_args(name)
    e, g = ctx.pair_eval(*args)
    e1, g1, w1 = ctx.pair_eval_stress(*args)
    assert e == e1 and np.array_equal(g, g1)                            # the same pass with and without the virial
    e2, g2, w2 = ctx.pair_eval_stress(*args)
    assert e2 == e1 and np.array_equal(g2, g1) and np.array_equal(w2, w1)          # and the same from run to run
    e3, g3 = ctx.pair_eval(*args)
    assert e3 == e and np.array_equal(g3, g)
    # against the image sum written here
    report(f'{name} E vs image sum', abs(e - S['e'].sum()), bE)
    report(f'{name} g vs image sum', np.abs(g - S['g']), bg)
    report(f'{name} W vs image sum', np.abs(w1 - S['w'].sum(axis=0)), bw)
    # against the host class
    host = host_calc(name, form, params)
    if host is not None:
        ref = at.copy()
        ref.calc = host
        eh, gh = ref.get_potential_energy(), -ref.get_forces()
        if name == 'wide':
            # PeriodicMorse's effective cutoff min(rcut, half the cell width) stays 3.3: the same function
            assert 0.5 / np.linalg.norm(np.linalg.pinv(ref.cell), axis=0).max() > 3.3
            report(f'{name} W vs PeriodicMorse', np.abs(w1 - ref.get_stress() * ref.get_volume()), bw)
        report(f'{name} E vs {type(host).__name__}', abs(e - eh), bE)
        report(f'{name} g vs {type(host).__name__}', np.abs(g - gh), bg)
    # the virial against the strain derivative of the yardstick's energy
    assert S['gap'] > 2 * 1e-5 * (rcut or 0.0)                         # a strain of 1e-5 moves a pair distance by 1e-5 r

    def energy(atoms):
        if host is not None:
            atoms = atoms.copy()
            atoms.calc = host_calc(name, form, params)
            return atoms.get_potential_energy()
        d = np.concatenate([atoms.positions[None, :, :] + sft - atoms.positions[:, None, :]
                            for sft in shifts_of(atoms, rcut)]).reshape(-1, 3)
        r = np.linalg.norm(d, axis=1)
        r = r[(r > 1e-8) & (r < rcut)]
        return 0.5 * shifted(form, params, rcut, r)[0].sum()
    np.testing.assert_allclose(w1, strain_derivatives(at, energy), rtol=1e-6, atol=1e-6)


def test_calculator_interface(ctx):
    """The `Calculator` methods: caching, the stress, and a change of the cell."""
    from sella_amd.atoms import supports_hessian, supports_stress
    at, form, params, rcut = make_case('wide')
    at.calc = device_calc(form, params, rcut)
    assert supports_stress(at.calc) and supports_hessian(at.calc) and at.calc.library_form
    assert at.calc.device_calculator() is None                         # nothing seen yet
    S = image_sum('wide')
    s = at.get_stress()
    assert at.calc.ncalls == 1
    np.testing.assert_allclose(s * at.get_volume(), S['w'].sum(axis=0), rtol=1e-12, atol=1e-12)
    e, f = at.get_potential_energy(), at.get_forces()
    assert at.calc.ncalls == 1                                         # energy, forces and stress from one evaluation
    dc = at.calc.device_calculator()
    e2, g2 = dc.eval(at.positions)
    assert e2 == e and np.array_equal(g2.reshape(-1, 3), -f)           # the library form: the same pass
    assert at.calc.ncalls == 2
    at.set_cell(at.cell * 1.01, scale_atoms=True)                      # the shifts follow the cell
    assert at.get_potential_energy() != e
    assert at.calc.device_calculator() is not dc


# ---- 2. dense Hessian ---------------------------------------------------------------------------------------------------------
def host_gradient(name):
    at, form, params, rcut = make_case(name)
    host = host_calc(name, form, params)
    if host is not None:
        ref = at.copy()
        ref.calc = host
        return ref, lambda atoms: -atoms.get_forces().ravel()
    sh = shifts_of(at, rcut)

    def gradient(atoms):                                                # narrow: the image sum's own gradient
        pos = atoms.positions
        g = np.zeros_like(pos)
        for sft in sh:
            d = pos[None, :, :] + sft - pos[:, None, :]
            r = np.linalg.norm(d, axis=2)
            i, j = np.nonzero((r > 1e-8) & (r < rcut))
            keep = i != j
            i, j = i[keep], j[keep]
            d1 = shifted(form, params, rcut, r[i, j])[1]
            np.add.at(g, i, -(d1 / r[i, j])[:, None] * d[i, j])
        return g.ravel()
    return at, gradient


@pytest.mark.parametrize('name', SMALL)
def test_closed_form_matches_richardson_of_host_gradient(name):
    """The yardstick of the Hessian checks, held to the rule of test_emt_hessian.py."""
    S = image_sum(name)
    assert S['gap'] > 2 * H_STEP
    at, gradient = host_gradient(name)
    R = richardson_hessian(at, gradient)
    est = float(np.abs(R - R.T).max())
    err = float(np.abs(S['H'] - R).max())
    print(f'{name}: max|H| {np.abs(R).max():.3f}  yardstick asymmetry {est:.2e}  max|H - R| {err:.2e}  ratio {err / est:.2f}')
    assert est < 1e-6 * np.abs(R).max()
    assert err <= 10 * est


@pytest.mark.parametrize('name', CASES)
def test_dense_hessian(ctx, name):
    at, form, params, rcut = make_case(name)
    at.calc = device_calc(form, params, rcut)
    S = image_sum(name)
    before = at.calc.ncalls
    H = at.calc.get_hessian(at)
    assert at.calc.ncalls == before and at.calc.nhessians == 1         # not a force call
    assert np.array_equal(H, H.T)
    report(f'{name} H vs closed form', np.abs(H - S['H']), bounds(S)[3])
    res, cap = acoustic_residual(H), (S['m'].max() + 8) * EPS * S['AH'].sum(axis=1).max()
    print(f'{name}: acoustic residual {res:.2e}  rounding of a row sum {cap:.2e}')
    assert res <= cap
    assert np.array_equal(ctx.pair_hessian(*pair_args(name)).numpy(), H)           # the same from run to run
    if name == 'narrow':
        assert S['nshift'] == 125 and S['m'].min() == 42 and abs(S['gap'] - 0.09) < 0.01    # own images among the 42
    if name == 'wide':
        assert S['nshift'] == 27 and (S['m'] == 12).all() and abs(S['gap'] - 0.17) < 0.01


# ---- 3. products --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SMALL + ['c257-morse'])
def test_products_with_host_vectors(ctx, name):
    at, form, params, rcut = make_case(name)
    at.calc = device_calc(form, params, rcut)
    H = at.calc.get_hessian(at)
    n = H.shape[0]
    rng = np.random.RandomState(5)
    before = at.calc.ncalls
    for k in (1, 3, 8, 17):
        V = rng.normal(size=(k, n))
        HV = at.calc.hessian_vector_product(at, V)
        assert HV.shape == (k, n)
        report(f'{name} k={k}', np.abs(HV - V @ H).max(axis=1), [product_bound(H, v) for v in V])
    v = rng.normal(size=n)
    assert np.array_equal(at.calc.hessian_vector_product(at, v), at.calc.hessian_vector_product(at, v[None])[0])
    assert at.calc.ncalls == before


def resident(name):
    at, form, params, rcut = make_case(name)
    at.calc = device_calc(form, params, rcut)
    H = at.calc.get_hessian(at)
    at.get_potential_energy()
    return at, H, at.calc.device_calculator()


@pytest.mark.parametrize('pinned', [False, True], ids=['all', 'pinned'])
@pytest.mark.parametrize('name', SMALL)
def test_operator(ctx, name, pinned):
    from sella_amd.device import DeviceHvpOperator
    at, H, dc = resident(name)
    n = H.shape[0]
    before = dc.ncalls
    free = every_seventh_pinned(n) if pinned else None
    sel = np.arange(n) if free is None else free
    Hs = H[sel][:, sel]
    op = DeviceHvpOperator(dc, at.positions.ravel(), free)
    assert op.shape == (len(sel), len(sel))
    rng = np.random.RandomState(6)
    for scale in (1.0, 1e-3):                                           # single products
        v = scale * rng.normal(size=len(sel))
        got = op.apply(v)
        report(f'{name} pinned={pinned} single', np.abs(got - Hs @ v).max(), product_bound(H, v))
        assert np.array_equal(op.apply(v), got)
    assert not op.apply(np.zeros(len(sel))).any()
    V = rng.normal(size=(16, len(sel)))                                 # a block of 16
    Y = op.apply_block(V)
    report(f'{name} pinned={pinned} block', np.abs(Y - V @ Hs).max(axis=1), [product_bound(H, v) for v in V])
    # a row does not depend on its companions, its slot or the number of rows
    assert np.array_equal(op.apply_block(V[5:6])[0], Y[5])
    W = rng.normal(size=(7, len(sel)))
    W[3] = V[5]
    assert np.array_equal(op.apply_block(W)[3], Y[5])
    assert np.array_equal(op.apply_block(np.vstack([V, V[:3]]))[16:], Y[:3])       # more rows than one block
    report(f'{name} pinned={pinned} diagonal', np.abs(op.diagonal() - np.diag(Hs)),
           2 * (image_sum(name)['m'].max() + 8) * EPS * np.diag(image_sum(name)['AH'])[sel])
    # the record: the single products of non-vanishing vectors, in full length
    Vs, AVs = op.Vs, op.AVs
    assert Vs.shape == (n, 4) and op.calls == 5 + 16 + 1 + 7 + 19
    assert not Vs[np.setdiff1d(np.arange(n), sel)].any()
    report(f'{name} pinned={pinned} record', np.abs(AVs - H @ Vs).max(axis=0), [product_bound(H, v) for v in Vs.T])
    assert dc.ncalls == before                                          # none of this is a force call


def test_davidson_on_the_device_equals_davidson_through_the_callback(ctx):
    from sella_amd.device import DeviceHvpOperator
    at, H, dc = resident('wide')
    n = H.shape[0]
    free = every_seventh_pinned(n)
    m = len(free)
    v0 = np.random.RandomState(13).normal(size=(m, 1))
    op, op2 = DeviceHvpOperator(dc, at.positions.ravel(), free), DeviceHvpOperator(dc, at.positions.ravel(), free)
    run = ctx.davidson(op, m, v0, 0.1, method='jd0', maxiter=6)
    ref = davidson_through_callback(ctx, op2, m, v0, 0.1, 'jd0', 6)
    assert_same_run(run, ref)
    lams, V, AV, nmatvec = run
    assert nmatvec == op.calls
    assert np.abs(AV - H[free][:, free] @ V).max() <= product_bound(H, V)
    assert np.abs(op.AVs - H @ op.Vs).max() <= product_bound(H, op.Vs)


# ---- 4. the bounded lists of the sweep ------------------------------------------------------------------------------------
OPENED = {'wide-open': ('wide', 6.0, 27), 'narrow-open': ('narrow', 7.0, 125)}


@pytest.mark.parametrize('name', ['wide', 'narrow', 'wide-open', 'narrow-open'])
def test_results_do_not_depend_on_the_lists(ctx, name):
    """`emt_hcap` = 1 against the default of 8, bit for bit, with the NumPy count of what each thread notes
    (test_emt_hessian.list_counts: candidate (image s, atom j) belongs to thread (s n + j) mod 256 and is noted if it lies
    inside the cutoff).  On `wide` (rcut 3.3) and `narrow` (rcut 5.0) the 13 and 43 candidates of an atom inside the cutoff
    fall on as many different threads — narrow's 500 candidates are two per thread, but a list holds hits, not candidates —
    so one slot overflows in neither (counted below: the largest list is 1) and the comparison there is lists against
    lists.  The same two cells with the cutoff opened to 6.0 and 7.0 (the same 27 and 125 images) are the cases where one
    slot overflows and eight do not: sweep against lists."""
    from sella_amd.device import DeviceCalculator, DeviceHvpOperator
    base, rcut_open, nimg = OPENED.get(name, (name, None, None))
    pos, form, params, shifts, rcut = args = pair_args(base)
    if rcut_open is not None:
        rcut = rcut_open
        args = (pos, form, params, shifts, rcut)
        assert len(shifts_of(make_case(base)[0], rcut)) == nimg == len(shifts)
    counts = list_counts(pos, shifts, rcut)
    print(f'{name}: largest list {counts.max()}, threads with more than one entry {(counts > 1).sum()}')
    assert counts.max() <= 8                                            # eight slots overflow nowhere
    assert (counts.max() >= 2) == (name in OPENED)                      # one slot does where the cutoff is opened
    if base == 'narrow':
        assert len(shifts) * len(pos) == 500 and counts.max() == (2 if name in OPENED else 1)
    rng = np.random.RandomState(8)
    V = rng.normal(size=(3, pos.size))

    def everything():
        dc = DeviceCalculator.pair(ctx, len(pos), form, params, shifts, rcut)
        op = DeviceHvpOperator(dc, pos.ravel())
        return (ctx.pair_eval_stress(*args), ctx.pair_hessian(*args).numpy(), ctx.pair_hvp(*args, V), dc.eval(pos.ravel()),
                op.apply(V[0]), op.apply_block(V), op.diagonal())
    full = everything()
    with ctx.options(emt_hcap=1):
        one = everything()

    def same(a, b):
        if isinstance(a, tuple):
            return all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(np.asarray(a), np.asarray(b))
    assert same(full, one)


# ---- 5. routes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pin', [True, False], ids=['pinned', 'default'])
def test_pes_takes_the_device_operator_when_an_atom_is_pinned(ctx, monkeypatch, pin):
    from sella_amd.internal import Constraints
    from sella_amd.peswrapper import PES
    from test_hvp_operator import Spy, check_diag
    at, form, params, rcut = make_case('c13-lj')
    at.calc = device_calc(form, params, rcut)
    H = at.calc.get_hessian(at)                                        # (not a force call: the PES makes the first one)
    kw = dict(hessian_vector_product=True)
    if pin:
        cons = Constraints(at)
        cons.fix_translation(0)
        kw.update(constraints=cons, proj_rot=False)
    spy = Spy(monkeypatch)
    pes = PES(at, **kw)
    check_diag(pes, at, H, spy, 'device' if pin else 'host')


def test_lowest_modes(ctx):
    from sella_amd.eigensolvers import lowest_modes
    from test_block_hvp import TOL, eig_tolerance
    at, H, dc = resident('c13-lj')
    free = np.arange(9, 39, dtype=np.int32)                             # atoms 0 - 2 pinned: no zero mode is left
    Hs = H[free][:, free]
    w, Q = np.linalg.eigh(Hs)
    before = at.calc.ncalls
    out = lowest_modes(at, nev=4, free=free, tol=TOL)
    assert out['nconv'] == 4 and at.calc.ncalls == before
    print(f'lowest modes {out["lams"]}  LAPACK {w[:4]}  niter {out["niter"]}')
    for h in range(4):
        assert abs(out['lams'][h] - w[h]) <= eig_tolerance(H, out['lams'][h])
    modes = out['modes'].reshape(4, -1)
    assert not modes[:, :9].any()
    assert np.abs(modes[:, free] @ modes[:, free].T - np.eye(4)).max() <= 1e-10


# ---- 7. refusals and arguments ----------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from sella_amd import Sella, _lib
    from sella_amd._lib import SellaHipError, ptr
    from sella_amd.atoms import LennardJones, Morse, supports_cell_hessian, supports_cell_hvp
    from sella_amd.device import DeviceCalculator, DeviceHvpOperator
    from sella_amd.eigensolvers import lowest_modes
    at = wide()
    at.calc = Morse(**MORSE_CU)                                        # rcut=None with periodic directions
    with pytest.raises(ValueError, match='cutoff'):
        at.get_potential_energy()
    with pytest.raises(ValueError):
        Morse(rcut=-1.0)
    with pytest.raises(ValueError):
        LennardJones(sigma=0.0)
    tight = fcc_cubic('Cu', 2.4, 1)                                    # rcut 6: 7^3 images
    tight.calc = Morse(**MORSE_CU, rcut=6.0)
    with pytest.raises(ValueError, match='127'):
        tight.get_potential_energy()
    at.calc = Morse(**MORSE_CU, rcut=3.3)
    e = at.get_potential_energy()
    # no second derivatives with respect to the cell
    assert not supports_cell_hessian(at.calc) and not supports_cell_hvp(at.calc)
    with pytest.raises(NotImplementedError):
        at.calc.get_cell_hessian(at)
    with pytest.raises(NotImplementedError):
        at.calc.cell_hessian_vector_product(at, np.zeros(96 + 9))
    with pytest.raises(NotImplementedError, match='Morse'):
        Sella(at, order=0, optimize_cell=True, cell_hessian_vector_product=True, logfile=None)
    with pytest.raises(NotImplementedError, match='Morse'):
        lowest_modes(at, nev=2, cell=True)
    # wrong shapes and values, through the Python layer and through the C ABI
    pos, form, params, shifts, rcut = pair_args('wide')
    with pytest.raises(ValueError):
        ctx.pair_eval(pos.ravel(), form, params, shifts, rcut)
    with pytest.raises(ValueError):
        ctx.pair_eval(pos, form, params[:2], shifts, rcut)
    with pytest.raises(ValueError):
        ctx.pair_eval(pos, 'buckingham', params, shifts, rcut)
    with pytest.raises(ValueError):
        ctx.pair_hvp(pos, form, params, shifts, rcut, np.zeros((2, 95)))
    with pytest.raises(SellaHipError, match='cutoff'):
        ctx.pair_eval(pos, form, params, shifts, None)                 # no cutoff with 27 images
    with pytest.raises(SellaHipError, match='127'):
        ctx.pair_eval(pos, form, params, np.zeros((128, 3)), rcut)
    L = _lib.lib()
    INVALID = -1
    P, X, S3 = np.array(params), np.ascontiguousarray(pos), np.ascontiguousarray(shifts)
    en, g = _lib.c_double(0.0), np.empty_like(X)
    n, ns = len(X), len(S3)
    assert L.sella_pair_eval(ctx._h, n, ptr(X), 0, ptr(P), ns, ptr(S3), 3.3, _lib.byref(en), None) == INVALID
    assert L.sella_pair_eval(ctx._h, n, ptr(X), 2, ptr(P), ns, ptr(S3), 3.3, _lib.byref(en), ptr(g)) == INVALID
    assert L.sella_pair_eval(ctx._h, 0, ptr(X), 0, ptr(P), ns, ptr(S3), 3.3, _lib.byref(en), ptr(g)) == INVALID
    assert L.sella_pair_eval(ctx._h, n, ptr(X), 0, ptr(P), ns, ptr(S3), float('nan'), _lib.byref(en), ptr(g)) == INVALID
    assert L.sella_pair_eval(ctx._h, n, ptr(X), 1, ptr(np.array([1.0, -1.0])), ns, ptr(S3), 3.3, _lib.byref(en), ptr(g)) == INVALID
    small = ctx.zeros(3 * n - 3, 3 * n - 3)
    assert L.sella_pair_hessian(ctx._h, n, ptr(X), 0, ptr(P), ns, ptr(S3), 3.3, small.handle) == INVALID
    assert L.sella_pair_hvp(ctx._h, n, ptr(X), 0, ptr(P), ns, ptr(S3), 3.3, ptr(X), 0, ptr(g)) == INVALID
    h = _lib.c_void_p()
    assert L.sella_calc_pair_create(ctx._h, n, 0, ptr(P), 128, ptr(np.zeros((128, 3))), 3.3, _lib.byref(h)) == INVALID
    assert L.sella_calc_pair_create(ctx._h, n, 0, ptr(P), ns, ptr(S3), 0.0, _lib.byref(h)) == INVALID
    # the operator of positions and cell does not exist for this kind, and says which kind it met
    dc = DeviceCalculator.pair(ctx, n, form, params, shifts, rcut)
    with pytest.raises(SellaHipError, match='pair-potential'):
        DeviceHvpOperator.for_cell(dc, pos.ravel(), at.cell, np.eye(9), np.zeros((9, 9)))
    # the context is usable after all of it
    at2 = wide()
    at2.calc = Morse(**MORSE_CU, rcut=3.3)
    assert at2.get_potential_energy() == e


# ---- 8. hardware only: beyond the LDS staging of the positions -------------------------------------------------------------
@pytest.mark.gpu
def test_bulk_beyond_the_staging_limit(hip_ctx):
    """N = 1100 > 1024: the sweep reads the positions from memory.  The gradient of one evaluation and one product, on a
    random subset of 64 atoms' rows, against the image sum (the bounds of the module docstring, on those rows)."""
    from sella_amd.atoms import EMT
    ctx = hip_ctx
    params, rcut = tuple(MORSE_CU.values()), 6.0
    at = fcc_cubic('Cu', 3.7, 7)
    keep = np.sort(np.random.RandomState(4).permutation(len(at))[:1100])
    pos = at.positions[keep] + 0.05 * np.random.RandomState(5).normal(size=(1100, 3))
    shifts = EMT.image_shifts(at.cell, at.pbc, rcut)
    assert len(shifts) == 27
    rows = np.sort(np.random.RandomState(6).permutation(1100)[:64])
    v = np.random.RandomState(7).normal(size=(1100, 3))
    g, Ag, hv, Ahv, m = np.zeros((64, 3)), np.zeros((64, 3)), np.zeros((64, 3)), np.zeros((64, 3)), np.zeros(64, dtype=int)
    for sft in shifts:
        d = pos[None, :, :] + sft - pos[rows][:, None, :]
        r = np.linalg.norm(d, axis=2)
        i, j = np.nonzero((r > 1e-8) & (r < rcut))
        keep_ = rows[i] != j
        i, j = i[keep_], j[keep_]
        rr = r[i, j]
        u = d[i, j] / rr[:, None]
        _, d1, d2, _, ad1, ad2 = shifted('morse', params, rcut, rr)
        np.add.at(m, i, 1)
        np.add.at(g, i, -d1[:, None] * u)
        np.add.at(Ag, i, ad1[:, None] * np.abs(u))
        dv = v[rows][i] - v[j]
        t = (u * dv).sum(axis=1)
        np.add.at(hv, i, (d1 / rr)[:, None] * dv + (d2 - d1 / rr)[:, None] * t[:, None] * u)
        np.add.at(Ahv, i, (ad1 / rr)[:, None] * np.abs(dv) + (ad2 + ad1 / rr)[:, None] * (np.abs(u) * np.abs(dv)).sum(axis=1)[:, None] * np.abs(u))
    e, gd = ctx.pair_eval(pos, 'morse', params, shifts, rcut)
    e1, gd1, _ = ctx.pair_eval_stress(pos, 'morse', params, shifts, rcut)
    assert e == e1 and np.array_equal(gd, gd1)
    per = 2 * (m + 8) * EPS
    report('N=1100 gradient rows', np.abs(gd[rows] - g), per[:, None] * Ag)
    hvd = ctx.pair_hvp(pos, 'morse', params, shifts, rcut, v.ravel()).reshape(-1, 3)
    report('N=1100 product rows', np.abs(hvd[rows] - hv), 2 * per[:, None] * Ahv)
