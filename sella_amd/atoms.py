"""Minimal stand-ins for the parts of ASE the path touches (ASE is not installable in the build
image; when `ase` imports, its own classes are used instead and these are bypassed).

  Atoms       positions / cell / pbc / calc, get_potential_energy(), get_forces()  — exactly the
              attributes `PES` reads (sella/peswrapper.py:294-303,332-338,413-418) — and get_cell(), set_cell(),
              get_volume(), get_stress(), get_pbc(), the subset of ASE's interface `CellCartesianPES` uses
  Optimizer   the run()/irun()/log()/converged() loop `Sella` inherits from
              ase.optimize.optimize.Optimizer (sella/optimize/optimize.py:10,177)
  calculators on the far side of the calculator boundary, for tests and benchmarks:
              QuadraticCubicModel (SURVEY.md §8d model PES), MorseCluster
              (tests/integration/test_morse_cluster.py), PairLJ — O(N^2) NumPy on the host, the yardsticks of
              Morse and LennardJones, the same pair potentials on the device (csrc/pair.hip) with stress, Hessian,
              Hessian-vector products and a library form; TIP3P, rigid three-site water on the device
              (csrc/tip3p.hip) with Hessian, products and a library form.
"""
import sys
import time

import numpy as np

try:                                                        # pragma: no cover - depends on the host
    from ase import Atoms as _AseAtoms                      # noqa: F401
    from ase.optimize.optimize import Optimizer as _AseOptimizer
    HAVE_ASE = True
except Exception:                                           # noqa: BLE001
    HAVE_ASE = False


# standard atomic weights of the elements the examples use (u); unknown symbols weigh 1
_MASSES = dict(H=1.008, C=12.011, N=14.007, O=15.999, F=18.998, Al=26.982, Si=28.085, P=30.974, S=32.06, Cl=35.45,
               Ar=39.948, Ni=58.693, Cu=63.546, Pd=106.42, Ag=107.868, Pt=195.084, Au=196.967, Xe=131.293)


# chemical symbols by atomic number ('X' = 0: a placeholder species, as in ase.data.chemical_symbols)
CHEMICAL_SYMBOLS = ('X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr '
                    'Rb Sr Y Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb '
                    'Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf '
                    'Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og').split()
_ATOMIC_NUMBER = {sym: z for z, sym in enumerate(CHEMICAL_SYMBOLS)}


class Atoms:
    def __init__(self, symbols=None, positions=None, cell=None, pbc=False, calculator=None,
                 numbers=None):
        self.positions = np.array(positions, dtype=np.float64).reshape((-1, 3))
        n = len(self.positions)
        if symbols is not None and len(symbols) and not isinstance(symbols[0], str):
            symbols, numbers = None, symbols                    # Atoms(numbers, positions), as read from a trajectory
        if symbols is None and numbers is not None:
            symbols = [CHEMICAL_SYMBOLS[int(z)] for z in numbers]
        self.symbols = list(symbols) if symbols is not None else ['X'] * n
        self.numbers = np.array(numbers if numbers is not None else [_ATOMIC_NUMBER.get(sym, 0) for sym in self.symbols],
                                dtype=int)
        self.cell = np.zeros((3, 3)) if cell is None else np.array(cell, dtype=np.float64).reshape(3, 3)
        self.pbc = np.array([pbc] * 3 if np.isscalar(pbc) else pbc, dtype=bool)
        self.calc = calculator
        self.constraints = []
        self.info = {}
        self.masses = np.array([_MASSES.get(sym, 1.0) for sym in self.symbols], dtype=np.float64)

    def __len__(self):
        return len(self.positions)

    def copy(self):
        new = Atoms(self.symbols, self.positions.copy(), self.cell.copy(), self.pbc.copy(), self.calc,
                    self.numbers.copy())
        new.info = dict(self.info)
        new.masses = self.masses.copy()
        return new

    def get_positions(self):
        return self.positions.copy()

    def set_positions(self, pos):
        self.positions = np.array(pos, dtype=np.float64).reshape((-1, 3))

    def get_atomic_numbers(self):
        return self.numbers.copy()

    def get_chemical_symbols(self):
        return list(self.symbols)

    def get_masses(self):
        return self.masses.copy()

    def set_masses(self, masses):
        self.masses = np.asarray(masses, dtype=np.float64).copy()

    def get_potential_energy(self):
        return float(self.calc.get_potential_energy(self))

    # ---- the cell (ase.Atoms.get_cell / set_cell / get_volume / get_pbc; get_cell hands out a plain array) ----------
    def get_cell(self):
        return self.cell.copy()

    def set_cell(self, cell, scale_atoms=False):
        """New lattice vectors (rows); with scale_atoms the positions keep their fractional coordinates."""
        cell = np.array(cell, dtype=np.float64).reshape(3, 3)
        if scale_atoms:
            self.positions = self.positions @ np.linalg.solve(self.cell, cell)
        self.cell = cell

    def get_volume(self):
        return float(abs(np.linalg.det(self.cell)))

    def get_pbc(self):
        return self.pbc.copy()

    def get_stress(self):
        """Stress in Voigt order (xx, yy, zz, yz, xz, xy), eV / Angstrom^3, from the calculator (ASE's convention:
        V sigma_ab = dE / d eps_ab under a homogeneous strain, negative diagonal for a compressed crystal)."""
        return np.asarray(self.calc.get_stress(self), dtype=np.float64).reshape(6)

    def get_forces(self):
        return np.asarray(self.calc.get_forces(self), dtype=np.float64).reshape((-1, 3))

    # `for atom in slab: atom.position, atom.index` (README.md:23-25 of the reference)
    def __getitem__(self, i):
        return _Atom(self, int(i) % len(self))

    def __iter__(self):
        return (_Atom(self, i) for i in range(len(self)))

    def extend(self, symbol, position):
        self.symbols.append(symbol)
        self.positions = np.vstack([self.positions, np.asarray(position, dtype=np.float64).reshape(1, 3)])
        self.numbers = np.append(self.numbers, _ATOMIC_NUMBER.get(symbol, 0))
        self.masses = np.append(self.masses, _MASSES.get(symbol, 1.0))


class _Atom:
    def __init__(self, atoms, index):
        self._atoms, self.index = atoms, index

    position = property(lambda self: self._atoms.positions[self.index])
    symbol = property(lambda self: self._atoms.symbols[self.index])


# ---- structure builders: the two ase.build functions the reference's README example uses -----------
def fcc111(symbol, size, a=3.61, vacuum=None):
    """Orthogonal-free hexagonal fcc(111) slab, size = (nx, ny, nlayers), ABC stacking, periodic in x, y."""
    nx, ny, nz = size
    d = a / np.sqrt(2.0)                       # nearest-neighbour distance
    a1 = np.array([d, 0.0, 0.0])
    a2 = np.array([0.5 * d, 0.5 * np.sqrt(3.0) * d, 0.0])
    dz = a / np.sqrt(3.0)                      # interlayer spacing
    shift = (a1 + a2) / 3.0                    # lateral offset between consecutive layers
    pos = []
    for k in range(nz):
        off = ((nz - 1 - k) % 3) * shift       # top layer unshifted, like ase.build.fcc111
        for j in range(ny):
            for i in range(nx):
                pos.append(i * a1 + j * a2 + off + np.array([0.0, 0.0, k * dz]))
    pos = np.array(pos)
    cell = np.array([nx * a1, ny * a2, [0.0, 0.0, (nz - 1) * dz]])
    if vacuum is not None:
        pos[:, 2] += vacuum
        cell[2, 2] += 2.0 * vacuum
    atoms = Atoms([symbol] * len(pos), pos, cell=cell, pbc=[True, True, False])
    atoms.info = dict(adsorbate_sites=dict(ontop=np.zeros(2), bridge=0.5 * a1[:2], fcc=(a1 + a2)[:2] / 3.0,
                                           hcp=2.0 * (a1 + a2)[:2] / 3.0))
    return atoms


def add_adsorbate(slab, symbol, height, position='ontop'):
    """Put one atom `height` above the top layer at a named site (or an (x, y) pair)."""
    xy = slab.info['adsorbate_sites'][position] if isinstance(position, str) else np.asarray(position, float)
    ztop = slab.positions[:, 2].max()
    slab.extend(symbol, [xy[0], xy[1], ztop + height])


class XYZTrajectory:
    """Extended-XYZ trajectory writer (one frame per call of write()), readable by ase.io.read(..., ':').
    Stands in for ase.io.Trajectory when a file NAME is passed as `trajectory=` (peswrapper.py:409-418 writes
    a frame at every energy/force evaluation); with ASE installed pass a real Trajectory object instead."""

    def __init__(self, filename, atoms, mode='w'):
        self.atoms = atoms
        self.f = open(filename, mode)
        self.nframes = 0

    def write(self, atoms=None):
        at = self.atoms if atoms is None else atoms
        cell = np.asarray(at.cell, dtype=float).ravel()
        calc = at.calc
        res = getattr(calc, '_res', None)
        have = res is not None and getattr(calc, '_key', None) == cache_key(at)
        head = 'Lattice="%s" Properties=species:S:1:pos:R:3%s pbc="%s"' % (
            ' '.join('%.10f' % v for v in cell), ':forces:R:3' if have else '',
            ' '.join('T' if b else 'F' for b in at.pbc))
        if have:
            head += ' energy=%.12f' % res[0]
        self.f.write('%d\n%s\n' % (len(at), head))
        for i, (sym, p) in enumerate(zip(at.symbols, at.positions)):
            line = '%-3s %18.10f %18.10f %18.10f' % (sym, p[0], p[1], p[2])
            if have:
                fr = -res[1][i]
                line += ' %18.10f %18.10f %18.10f' % (fr[0], fr[1], fr[2])
            self.f.write(line + '\n')
        self.f.flush()
        self.nframes += 1

    def close(self):
        if not self.f.closed:
            self.f.close()


def cache_key(atoms):
    """What a calculator's results are cached under: the positions and the cell (a probe of the cell alone is a new
    geometry)."""
    return np.ascontiguousarray(atoms.positions).tobytes() + np.asarray(atoms.cell, dtype=np.float64).tobytes()


def voigt_to_matrix(v):
    """3 x 3 symmetric tensor of a Voigt 6-vector (xx, yy, zz, yz, xz, xy)."""
    xx, yy, zz, yz, xz, xy = v
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=np.float64)


def supports_stress(calc):
    """Whether `calc` can produce a stress tensor: a calculator of this module that implements the virial, or a foreign
    (ASE) calculator with `get_stress` that lists 'stress' among its implemented properties (if it lists any)."""
    if calc is None:
        return False
    if isinstance(calc, Calculator):
        return type(calc).energy_gradient_virial is not Calculator.energy_gradient_virial
    if not callable(getattr(calc, 'get_stress', None)):
        return False
    props = getattr(calc, 'implemented_properties', None)
    return props is None or 'stress' in props


def supports_hessian(calc):
    """Whether `calc` can produce its own second derivatives (`get_hessian`, `get_device_hessian`,
    `hessian_vector_product`): a calculator of this module that implements `device_hessian`, or a foreign calculator
    with a `get_hessian` method."""
    if calc is None:
        return False
    if isinstance(calc, Calculator):
        return calc.has_hessian
    return callable(getattr(calc, 'get_hessian', None))


def supports_cell_hessian(calc):
    """Whether `calc` can produce the second derivatives of positions and cell together (`get_cell_hessian`,
    `get_device_cell_hessian`): a calculator of this module that implements `device_cell_hessian`, or a foreign
    calculator with a `get_cell_hessian` method."""
    if calc is None:
        return False
    if isinstance(calc, Calculator):
        return calc.has_cell_hessian
    return callable(getattr(calc, 'get_cell_hessian', None))


def supports_cell_hvp(calc):
    """Whether `calc` can multiply the Hessian of positions and cell into vectors without forming it
    (`cell_hessian_vector_product`): a calculator of this module that implements `cell_hessian_products`, or a foreign
    calculator with a `cell_hessian_vector_product` method."""
    if calc is None:
        return False
    if isinstance(calc, Calculator):
        return calc.has_cell_hvp
    return callable(getattr(calc, 'cell_hessian_vector_product', None))


class Calculator:
    """energy_and_gradient(positions (N,3)) -> (E, dE/dx (N,3)); results cached per geometry (positions and cell).
    A calculator that also has the virial implements energy_gradient_virial(positions) -> (E, dE/dx, W (6,)), W the
    derivative of E under a homogeneous strain in Voigt order; get_stress() is then W / V from the same evaluation.
    A calculator that has its second derivatives implements device_hessian(positions) -> (3N x 3N) `DeviceMatrix` and
    hessian_products(positions, V (k, 3N)) -> H V[q] (k, 3N); get_hessian(), get_device_hessian() and
    hessian_vector_product() are then available (and fit `Sella(..., hessian_function=)`).  They are not force calls:
    `ncalls` does not move, `nhessians` counts the evaluations.
    A calculator that also has the second derivatives with respect to the cell implements
    device_cell_hessian(positions, cell) -> (3N + 9)-square `DeviceMatrix` in the coordinates [positions; cell.ravel()]
    (lattice vectors in the rows of the cell, positions fixed while the cell varies); get_cell_hessian() and
    get_device_cell_hessian() are then available (and fit `Sella(..., optimize_cell=True, hessian_function=)`), cached
    and counted like the Hessian at fixed cell.  Its products without forming it are
    cell_hessian_products(positions, cell, V (k, 3N + 9)) -> (k, 3N + 9) in the same coordinates, behind
    cell_hessian_vector_product() (fits `Sella(..., optimize_cell=True, cell_hessian_vector_product=True)`); they are
    neither force calls nor Hessians: `ncellhvps` counts the batches."""

    def __init__(self):
        self._key = None
        self._res = None
        self._virial = None
        self._ncalls = 0
        self._hess = None                  # (cache key, DeviceMatrix, ndarray or None) of the last Hessian
        self._cell_hess = None             # the same of the last Hessian of positions and cell
        self.nhessians = 0                 # Hessians and batches of Hessian-vector products evaluated
        self.ncellhvps = 0                 # batches of products with the Hessian of positions and cell

    def _library_calls(self):
        dc = getattr(self, '_devcalc', None)
        dc = dc[1] if isinstance(dc, tuple) else dc
        return 0 if dc is None else dc.ncalls

    # force calls: through this object, plus those the library made on its own copy of the calculator
    ncalls = property(lambda self: self._ncalls + self._library_calls(),
                      lambda self, v: setattr(self, '_ncalls', v - self._library_calls()))

    def energy_and_gradient(self, pos):
        raise NotImplementedError

    # a calculator that also exists inside the library says so (`library_form`) and hands out that object
    # (`device_calculator()`; None until it can be built): sella_amd/search.py, PES._library_fd_operator
    library_form = False

    def device_calculator(self):
        return None

    def energy_gradient_virial(self, pos):
        raise NotImplementedError(f'{type(self).__name__} has no stress tensor')

    def device_hessian(self, pos):
        raise NotImplementedError(f'{type(self).__name__} has no analytic Hessian')

    def hessian_products(self, pos, V):
        raise NotImplementedError(f'{type(self).__name__} has no analytic Hessian')

    def device_cell_hessian(self, pos, cell):
        raise NotImplementedError(f'{type(self).__name__} has no analytic Hessian of positions and cell')

    def cell_hessian_products(self, pos, cell, V):
        raise NotImplementedError(f'{type(self).__name__} has no Hessian-vector product of positions and cell')

    has_hessian = property(lambda self: type(self).device_hessian is not Calculator.device_hessian)
    has_cell_hessian = property(lambda self: type(self).device_cell_hessian is not Calculator.device_cell_hessian)
    has_cell_hvp = property(lambda self: type(self).cell_hessian_products is not Calculator.cell_hessian_products)

    def _prepare(self, atoms):
        """Whatever depends on the species and the cell of `atoms` rather than on the positions (nothing here)."""

    def _drop_hessian(self):
        for hit in (self._hess, self._cell_hess):
            if hit is not None:
                hit[1].free()
        self._hess = self._cell_hess = None

    def _cached_hessian(self, atoms):
        if not self.has_hessian:
            raise NotImplementedError(f'{type(self).__name__} has no analytic Hessian')
        self._prepare(atoms)
        key = cache_key(atoms)
        if self._hess is None or self._hess[0] != key or self._hess[1].ctx._h is None:     # (or its context is gone)
            self._drop_hessian()
            self._hess = [key, self.device_hessian(atoms.positions), None]
            self.nhessians += 1
        return self._hess

    def get_device_hessian(self, atoms):
        """The Cartesian Hessian d2E/dx2 (3N x 3N) of the geometry of `atoms` as a `DeviceMatrix` of the caller's own (a
        device copy of the cached one: `ApproximateHessian.set_B` keeps what it is given)."""
        return self._cached_hessian(atoms)[1].copy()

    def get_hessian(self, atoms):
        """The same as an array (one download per geometry)."""
        hit = self._cached_hessian(atoms)
        if hit[2] is None:
            hit[2] = hit[1].numpy()
        return hit[2].copy()

    def _cached_cell_hessian(self, atoms):
        if not self.has_cell_hessian:
            raise NotImplementedError(f'{type(self).__name__} has no analytic Hessian of positions and cell')
        self._prepare(atoms)
        key = cache_key(atoms)
        hit = self._cell_hess
        if hit is None or hit[0] != key or hit[1].ctx._h is None:                         # (or its context is gone)
            if hit is not None:
                hit[1].free()
            self._cell_hess = None
            cell = np.array(atoms.cell, dtype=np.float64)
            self._cell_hess = [key, self.device_cell_hessian(atoms.positions, cell), None]
            self.nhessians += 1
        return self._cell_hess

    def get_device_cell_hessian(self, atoms):
        """The Hessian of positions and cell ((3N + 9) square, coordinates [positions; cell.ravel()], the positions fixed
        while the lattice vectors vary) of the geometry of `atoms` as a `DeviceMatrix` of the caller's own."""
        return self._cached_cell_hessian(atoms)[1].copy()

    def get_cell_hessian(self, atoms):
        """The same as an array (one download per geometry)."""
        hit = self._cached_cell_hessian(atoms)
        if hit[2] is None:
            hit[2] = hit[1].numpy()
        return hit[2].copy()

    def hessian_vector_product(self, atoms, V):
        """H v for one vector (3N,) or the rows of V (k, 3N), without forming H; the shape of V."""
        if not self.has_hessian:
            raise NotImplementedError(f'{type(self).__name__} has no analytic Hessian')
        self._prepare(atoms)
        V = np.ascontiguousarray(V, dtype=np.float64)
        n = 3 * len(atoms)
        if V.shape != (n,) and (V.ndim != 2 or V.shape[1] != n or V.shape[0] == 0):
            raise ValueError(f'expected vectors of length {n} as an array of shape ({n},) or (k, {n}), got {V.shape}')
        self.nhessians += 1
        return np.asarray(self.hessian_products(atoms.positions, V.reshape(-1, n))).reshape(V.shape)

    def cell_hessian_vector_product(self, atoms, V):
        """The Hessian of positions and cell times one vector (3N + 9,) or the rows of V (k, 3N + 9), each
        [v; W.ravel()] in the coordinates of `get_cell_hessian` (W the variation of the cell, lattice vectors in its rows),
        without forming it; the shape of V."""
        if not self.has_cell_hvp:
            raise NotImplementedError(f'{type(self).__name__} has no Hessian-vector product of positions and cell')
        self._prepare(atoms)
        V = np.ascontiguousarray(V, dtype=np.float64)
        n = 3 * len(atoms) + 9
        if V.shape != (n,) and (V.ndim != 2 or V.shape[1] != n or V.shape[0] == 0):
            raise ValueError(f'expected vectors of length {n} as an array of shape ({n},) or (k, {n}), got {V.shape}')
        self.ncellhvps += 1
        cell = np.array(atoms.cell, dtype=np.float64)
        return np.asarray(self.cell_hessian_products(atoms.positions, cell, V.reshape(-1, n))).reshape(V.shape)

    def _get(self, atoms, stress=False):
        """(E, dE/dx) of the geometry of `atoms`; with `stress`, the virial is cached alongside them from the same
        evaluation (energy and forces cached without it cost one more)."""
        key = cache_key(atoms)
        if key != self._key or (stress and self._virial is None):
            self._ncalls += 1
            if stress:
                e, g, w = self.energy_gradient_virial(atoms.positions)
                self._res, self._virial = (e, g), np.asarray(w, dtype=np.float64).copy()
            else:
                self._res, self._virial = self.energy_and_gradient(atoms.positions), None
            self._key = key
        return self._res

    def get_potential_energy(self, atoms):
        return self._get(atoms)[0]

    def get_forces(self, atoms):
        return -self._get(atoms)[1]

    def get_stress(self, atoms):
        """Stress (Voigt order xx, yy, zz, yz, xz, xy; eV / Angstrom^3) = virial / V."""
        self._get(atoms, stress=True)
        volume = abs(np.linalg.det(np.asarray(atoms.cell, dtype=np.float64)))
        if volume == 0.0:
            raise ValueError('stress needs a cell with a non-zero volume')
        return self._virial / volume


class QuadraticCubicModel(Calculator):
    """f(x) = 1/2 x^T A x + c/3 sum_j (u_j . x)^3 — gradient = one matvec + a few dots, so an
    optimizer step on it is linear-algebra bound.  `A` may be given as a numpy
    array (host matvec) or as a callable v -> A v (e.g. a device-resident matrix)."""

    def __init__(self, A, U, c=0.05, device_matrix=None):
        super().__init__()
        self.A = A
        self.U = np.asarray(U, dtype=np.float64)
        self.c = c
        self.device_matrix = device_matrix         # the DeviceMatrix behind a callable A: enables `device_calculator`

    library_form = property(lambda self: self.device_matrix is not None)

    def device_calculator(self):
        """The same function as a calculator inside the library (`sella_calc_model_*`), or None."""
        if self.device_matrix is None:
            return None
        if getattr(self, '_devcalc', None) is None:
            from .device import DeviceCalculator
            self._devcalc = DeviceCalculator.model(self.device_matrix.ctx, self.device_matrix, self.U, self.c)
        return self._devcalc

    # second derivatives A + 2 c sum_j (u_j . x) u_j u_j^T: through the library's copy of the calculator only
    has_hessian = property(lambda self: self.device_matrix is not None)

    def device_hessian(self, pos):
        return self.device_calculator().hessian(np.asarray(pos).ravel())

    def hessian_products(self, pos, V):
        return self.device_calculator().hvp(np.asarray(pos).ravel(), V)

    def energy_and_gradient(self, pos):
        x = pos.ravel()
        Ax = self.A(x) if callable(self.A) else self.A @ x
        p = self.U @ x
        e = 0.5 * x @ Ax + self.c / 3.0 * np.sum(p ** 3)
        g = Ax + self.U.T @ (self.c * p ** 2)
        return e, g.reshape(pos.shape)


class MorseCluster(Calculator):
    """Pairwise Morse potential, D (1 - exp(-a (r - r0)))^2 - D."""

    def __init__(self, D=1.0, a=1.0, r0=1.0):
        super().__init__()
        self.D, self.a, self.r0 = D, a, r0

    def energy_and_gradient(self, pos):
        n = len(pos)
        d = pos[:, None, :] - pos[None, :, :]
        r = np.linalg.norm(d, axis=2)
        iu = np.triu_indices(n, 1)
        rr = r[iu]
        ex = np.exp(-self.a * (rr - self.r0))
        e = np.sum(self.D * (1 - ex) ** 2 - self.D)
        de = 2 * self.D * self.a * (1 - ex) * ex
        g = np.zeros_like(pos)
        u = d[iu] / rr[:, None]
        np.add.at(g, iu[0], de[:, None] * u)
        np.add.at(g, iu[1], -de[:, None] * u)
        return e, g


class PeriodicMorse(Calculator):
    """Morse pair potential under the minimum-image convention of a (partially) periodic cell, in
    shifted-force form (energy and force continuous at `rcut`) — a stand-in for EMT on the far side of the calculator boundary (ASE's EMT is not
    available in this image).  Defaults: Girifalco-Weizer parameters for Cu (eV, Angstrom)."""

    def __init__(self, D=0.3429, a=1.3588, r0=2.866, rcut=6.0):
        super().__init__()
        self.D, self.a, self.r0, self.rcut = D, a, r0, rcut
        self.cell, self.pbc = None, None

    def _get(self, atoms, stress=False):
        self.cell, self.pbc = np.asarray(atoms.cell, dtype=float), np.asarray(atoms.pbc, dtype=bool)
        return super()._get(atoms, stress)

    def energy_and_gradient(self, pos):
        return self._evaluate(pos, False)

    def energy_gradient_virial(self, pos):
        """Energy, gradient and virial sum_pairs (dE/dr / r) d (x) d over the minimum-image pairs (Voigt order)."""
        return self._evaluate(pos, True)

    def _evaluate(self, pos, virial):
        n = len(pos)
        iu = np.triu_indices(n, 1)
        d = pos[iu[0]] - pos[iu[1]]
        rcut = self.rcut
        if self.pbc is not None and self.pbc.any():
            per = np.where(self.pbc)[0]
            C = self.cell[per]                                   # periodic lattice vectors (rows)
            Cinv = np.linalg.pinv(C)
            d = d - np.round(d @ Cinv) @ C
            # the minimum image is unique (and the energy smooth) only inside half the cell width
            rcut = min(rcut, 0.5 / np.linalg.norm(Cinv, axis=0).max())
        rr = np.linalg.norm(d, axis=1)
        m = rr < rcut
        d, rr, i0, i1 = d[m], rr[m], iu[0][m], iu[1][m]
        # shifted-force form: energy AND force go to zero continuously at the cutoff
        ex = np.exp(-self.a * (rr - self.r0))
        exc = np.exp(-self.a * (rcut - self.r0))
        vc = self.D * (1 - exc) ** 2
        dvc = 2 * self.D * self.a * (1 - exc) * exc
        e = np.sum(self.D * (1 - ex) ** 2 - vc - dvc * (rr - rcut))
        de = 2 * self.D * self.a * (1 - ex) * ex - dvc
        g = np.zeros_like(pos)
        u = d / rr[:, None]
        np.add.at(g, i0, de[:, None] * u)
        np.add.at(g, i1, -de[:, None] * u)
        if not virial:
            return e, g
        W = np.einsum('p,pa,pb->ab', de / rr, d, d)
        return e, g, np.array([W[0, 0], W[1, 1], W[2, 2], W[1, 2], W[0, 2], W[0, 1]])


class EMT(Calculator):
    """Effective-medium theory in the functional form and with the parameter table of ASE's `ase.calculators.emt`
    (Jacobsen, Stoltze, Norskov, Surf. Sci. 366, 394 (1996)) for Al, Cu, Ag, Au, Ni, Pd, Pt, evaluated on the
    device (csrc/emt.hip: all-pairs density / cohesive / force kernels, deterministic in-block reductions).
    ASE is not installable in the build image, so this restates the published algorithm: **unpinned** against
    ASE; checked against the NumPy restatement in oracle/ and finite differences of its own energy.  Periodic
    directions are handled by an explicit sum over the periodic images: ceil(cutoff / height) of them on either side
    along each periodic direction (one while the cell is at least a cutoff, ~5.3 A for Cu, wide), 127 images at most.
    get_stress() takes energy, forces and the virial from one device evaluation (`sella_emt_eval_stress`);
    get_hessian() / get_device_hessian() / hessian_vector_product() are the analytic second derivatives
    (`sella_emt_hessian`, `sella_emt_hvp`), get_cell_hessian() / get_device_cell_hessian() those of positions and cell
    together (`sella_emt_cell_hessian`), cell_hessian_vector_product() their products without the matrix
    (`sella_emt_cell_hvp`)."""
    #              E0     s0    V0     eta2   kappa  lambda n0        (eV, bohr, eV, 1/bohr, 1/bohr, 1/bohr, 1/bohr^3)
    _PAR = dict(Al=(-3.28, 3.00, 1.493, 1.240, 2.000, 1.169, 0.00700), Cu=(-3.51, 2.67, 2.476, 1.652, 2.740, 1.906, 0.00910),
                Ag=(-2.96, 3.01, 2.132, 1.652, 2.790, 1.892, 0.00547), Au=(-3.80, 3.00, 2.321, 1.674, 2.873, 2.182, 0.00703),
                Ni=(-4.44, 2.60, 3.673, 1.669, 2.757, 1.948, 0.01030), Pd=(-3.90, 2.87, 2.773, 1.818, 3.107, 2.155, 0.00688),
                Pt=(-5.85, 2.90, 4.067, 1.812, 3.145, 2.192, 0.00802))
    _BETA = 1.809                      # (16 pi / 3)^(1/3) / sqrt(2), historical rounding
    _BOHR = 0.529177210903

    def __init__(self):
        super().__init__()
        self._setup = None

    def _prepare(self, atoms):
        key = (tuple(atoms.symbols), np.asarray(atoms.cell, dtype=float).tobytes(), tuple(atoms.pbc))
        if self._setup is None or self._setup[0] != key:
            self._setup = (key, self._initialize(atoms))
            self._key = None                       # results cached for the old cell / species are stale
            self._drop_hessian()

    def _get(self, atoms, stress=False):
        self._prepare(atoms)
        return super()._get(atoms, stress)

    def _initialize(self, atoms):
        b, beta = self._BOHR, self._BETA
        par = {}
        for k in sorted(set(atoms.symbols)):
            if k not in self._PAR:
                raise ValueError(f'EMT has no parameters for {k}')
            E0, s0, V0, eta2, kappa, lam, n0 = self._PAR[k]
            par[k] = dict(E0=E0, s0=s0 * b, V0=V0, eta2=eta2 / b, kappa=kappa / b, lam=lam / b, n0=n0 / b ** 3)
        maxseq = max(p['s0'] for p in par.values())
        rc = beta * maxseq * 0.5 * (np.sqrt(3.0) + 2.0)
        rr = rc * 2.0 * 2.0 / (np.sqrt(3.0) + 2.0)
        acut = np.log(9999.0) / (rr - rc)
        for p in par.values():
            g1 = g2 = 0.0
            for i, nn in enumerate((12, 6, 24)):
                r = p['s0'] * beta * np.sqrt(i + 1.0)
                x = nn / (12.0 * (1.0 + np.exp(acut * (r - rc))))
                g1 += x * np.exp(-p['eta2'] * (r - beta * p['s0']))
                g2 += x * np.exp(-p['kappa'] / beta * (r - beta * p['s0']))
            p['gamma1'], p['gamma2'] = g1, g2
        table = np.array([[par[s][name] for s in atoms.symbols]
                          for name in ('E0', 's0', 'V0', 'eta2', 'kappa', 'lam', 'n0', 'gamma1', 'gamma2')])
        cutoff = rc + 0.5
        shifts = self.image_shifts(atoms.cell, atoms.pbc, cutoff)
        return dict(par=np.ascontiguousarray(table), rc=rc, acut=acut, cutoff=cutoff, shifts=shifts)

    _MAX_IMAGES = 127                  # the packing limit of the device's neighbour lists (csrc/emt.hip, emt_pack)

    @classmethod
    def image_shifts(cls, cell, pbc, cutoff):
        """Lattice translations of the periodic images to sum over: k = -m_d .. m_d along each periodic direction d,
        m_d = ceil(cutoff / height_d) (height_d: distance between the lattice planes the other periodic vectors span),
        nested in the order x, y, z.  A cell at least one cutoff wide in every periodic direction gives the 3^d list."""
        cell = np.asarray(cell, dtype=float)
        per = [d for d in range(3) if pbc[d]]
        m = {}
        if per:
            dual = np.linalg.pinv(cell[per])                     # columns: dual vectors within the periodic lattice
            for k, d in enumerate(per):
                norm = np.linalg.norm(dual[:, k])
                if not np.isfinite(norm) or norm == 0.0:
                    raise ValueError('EMT: degenerate periodic cell')
                m[d] = int(np.ceil(cutoff * norm))
        count = int(np.prod([2 * m[d] + 1 for d in per])) if per else 1
        if count > cls._MAX_IMAGES:
            raise ValueError(f'EMT: the cell needs {count} periodic images within the cutoff ({cutoff:.3f} A), more than '
                             f'{cls._MAX_IMAGES}')
        shifts = [np.zeros(3)]
        for d in per:
            shifts = [sft + k * cell[d] for sft in shifts for k in range(-m[d], m[d] + 1)]
        return np.array(shifts)

    def energy_and_gradient(self, pos):
        from .device import get_context
        S = self._setup[1]
        return get_context().emt_eval(pos, S['par'], S['shifts'], S['rc'], S['acut'], S['cutoff'], self._BETA)

    def energy_gradient_virial(self, pos):
        from .device import get_context
        S = self._setup[1]
        return get_context().emt_eval_stress(pos, S['par'], S['shifts'], S['rc'], S['acut'], S['cutoff'], self._BETA)

    def _emt_args(self, pos):
        S = self._setup[1]
        return pos, S['par'], S['shifts'], S['rc'], S['acut'], S['cutoff'], self._BETA

    def device_hessian(self, pos):
        """The analytic Hessian (csrc/emt_hessian.hip: pair blocks per atom, the embedding term as one rank-N product)."""
        from .device import get_context
        return get_context().emt_hessian(*self._emt_args(pos))

    def hessian_products(self, pos, V):
        from .device import get_context
        return get_context().emt_hvp(*self._emt_args(pos), V)

    def device_cell_hessian(self, pos, cell):
        """The analytic Hessian of positions and cell (csrc/emt_hessian.hip: the cell enters through the image
        translations, so the same pair quantities contracted with the image indices)."""
        from .device import get_context
        pos, par, shifts, *tail = self._emt_args(pos)
        return get_context().emt_cell_hessian(pos, par, shifts, cell, *tail)

    def cell_hessian_products(self, pos, cell, V):
        from .device import get_context
        pos, par, shifts, *tail = self._emt_args(pos)
        return get_context().emt_cell_hvp(pos, par, shifts, cell, *tail, V)

    library_form = True

    def device_calculator(self):
        """This potential, for the species and cell it was last set up for, as a calculator inside the library
        (`sella_calc_emt_*`); None before the first evaluation."""
        if self._setup is None:
            return None
        hit = getattr(self, '_devcalc', None)
        if hit is None or hit[0] is not self._setup:
            from .device import DeviceCalculator, get_context
            S = self._setup[1]
            hit = (self._setup, DeviceCalculator.emt(get_context(), S['par'].shape[1], S['par'], S['shifts'], S['rc'],
                                                     S['acut'], S['cutoff'], self._BETA))
            self._devcalc = hit
        return hit[1]


class _DevicePairPotential(Calculator):
    """A pair potential E = 1/2 sum over ordered pairs of phi(r) on the device (csrc/pair.hip), with everything a
    calculator of the library has: energy and forces, the virial (`get_stress`), the analytic Hessian and its products
    (`get_hessian`, `get_device_hessian`, `hessian_vector_product`), and its library form (`device_calculator()`:
    whole searches, cohorts, the finite-difference and the exact Hessian-vector operators).

    rcut=None sums plain phi over all pairs and is for systems without a periodic direction (ValueError otherwise).  With
    a cutoff the pair function is the shifted-force form phi(r) - phi(rcut) - phi'(rcut) (r - rcut) inside rcut and zero
    beyond, as `PeriodicMorse` uses; periodic directions are an explicit image sum (`EMT.image_shifts`), so cells narrower
    than 2 rcut work, up to 127 images.  One parameter set per calculator.  There are no second derivatives with respect
    to the cell: `get_cell_hessian` and `cell_hessian_vector_product` raise NotImplementedError."""
    _form = None

    def __init__(self, params, rcut):
        super().__init__()
        self._params = np.array(params, dtype=np.float64)
        self.rcut = None if rcut is None else float(rcut)
        if not np.all(np.isfinite(self._params)) or (self.rcut is not None and not (np.isfinite(self.rcut) and self.rcut > 0.0)):
            raise ValueError(f'{type(self).__name__}: the parameters must be finite and rcut positive (or None)')
        self._setup = None

    def _prepare(self, atoms):
        key = (len(atoms), np.asarray(atoms.cell, dtype=float).tobytes(), tuple(bool(p) for p in atoms.pbc))
        if self._setup is None or self._setup[0] != key:
            if self.rcut is None:
                if np.any(atoms.pbc):
                    raise ValueError(f'{type(self).__name__}: a periodic system needs a cutoff (rcut=None sums over all pairs)')
                shifts = np.zeros((1, 3))
            else:
                shifts = EMT.image_shifts(atoms.cell, atoms.pbc, self.rcut)
            self._setup = (key, dict(natoms=len(atoms), shifts=np.ascontiguousarray(shifts)))
            self._key = None                       # results cached for the old cell are stale
            self._drop_hessian()

    def _get(self, atoms, stress=False):
        self._prepare(atoms)
        return super()._get(atoms, stress)

    def _pair_args(self, pos):
        if self._setup is None:
            raise RuntimeError(f'{type(self).__name__}: no atoms seen yet (evaluate through an Atoms object first)')
        return pos, self._form, self._params, self._setup[1]['shifts'], self.rcut

    def energy_and_gradient(self, pos):
        from .device import get_context
        return get_context().pair_eval(*self._pair_args(pos))

    def energy_gradient_virial(self, pos):
        from .device import get_context
        return get_context().pair_eval_stress(*self._pair_args(pos))

    def device_hessian(self, pos):
        """The analytic Hessian (csrc/pair.hip: the pair blocks K = phi'' u u^T + (phi'/r)(I - u u^T) per atom)."""
        from .device import get_context
        return get_context().pair_hessian(*self._pair_args(pos))

    def hessian_products(self, pos, V):
        from .device import get_context
        return get_context().pair_hvp(*self._pair_args(pos), V)

    library_form = True

    def device_calculator(self):
        """This potential, for the cell it was last set up for, as a calculator inside the library
        (`sella_calc_pair_create`); None before the first evaluation."""
        if self._setup is None:
            return None
        hit = getattr(self, '_devcalc', None)
        if hit is None or hit[0] is not self._setup:
            from .device import DeviceCalculator, get_context
            S = self._setup[1]
            hit = (self._setup, DeviceCalculator.pair(get_context(), S['natoms'], self._form, self._params, S['shifts'],
                                                      self.rcut))
            self._devcalc = hit
        return hit[1]


class Morse(_DevicePairPotential):
    """phi = D (1 - exp(-a (r - r0)))^2 - D on the device: `MorseCluster`'s function with rcut=None, `PeriodicMorse`'s
    shifted-force form with a cutoff (there under the minimum image, here as an image sum)."""
    _form = 'morse'

    def __init__(self, D=1.0, a=1.0, r0=1.0, rcut=None):
        super().__init__((D, a, r0), rcut)
        self.D, self.a, self.r0 = float(D), float(a), float(r0)


class LennardJones(_DevicePairPotential):
    """phi = 4 eps ((sigma / r)^12 - (sigma / r)^6) on the device: `PairLJ`'s function with rcut=None."""
    _form = 'lj'

    def __init__(self, eps=1.0, sigma=1.0, rcut=None):
        super().__init__((eps, sigma), rcut)
        if not self._params[1] > 0.0:
            raise ValueError('LennardJones: sigma must be positive')
        self.eps, self.sigma = float(eps), float(sigma)


# TIP3P (Jorgensen et al., J. Chem. Phys. 79, 926 (1983)) as ase/calculators/tip3p.py states it; the two unit factors
# from the CODATA 2014 values ase.units uses, named here and nowhere else: 0.1521 kcal/mol in eV, and the Coulomb constant
# Hartree x Bohr = e^2 / (4 pi eps0) in eV Angstrom
qH = 0.417
sigma0 = 3.15061
epsilon0 = 0.00659568020328023
_COULOMB = 14.399645351950547
rOH = 0.9572
angleHOH = 104.52


class TIP3P(Calculator):
    """Rigid three-site TIP3P water on the device (csrc/tip3p.hip), the model of ASE's `ase.calculators.tip3p.TIP3P`:
    atoms in consecutive triples, one molecule each, `O H H` or `H H O`; Lennard-Jones (`sigma0`, `epsilon0`) between the
    oxygens, Coulomb between all sites of different molecules (`qH`, q_O = -2 qH), every molecule pair multiplied by a
    switch of the O-O distance that falls from 1 at rc - width to 0 at rc.  Nothing acts inside a molecule: the geometry
    (`rOH`, `angleHOH`) is held by constraints.  Periodic directions need a diagonal cell with edges of at least 2 rc
    (minimum image, one shift per molecule pair); ValueError otherwise.

    Energy and forces, the analytic Hessian and its products (`get_hessian`, `get_device_hessian`,
    `hessian_vector_product`), and the library form (`device_calculator()`: whole searches, cohorts, the finite-difference
    and the exact Hessian-vector operators).  No virial: `get_stress` raises NotImplementedError, and there are no second
    derivatives with respect to the cell."""

    def __init__(self, rc=5.0, width=1.0):
        super().__init__()
        self.rc, self.width = float(rc), float(width)
        if not (np.isfinite(self.rc) and np.isfinite(self.width) and 0.0 < self.width <= self.rc):
            raise ValueError('TIP3P: 0 < width <= rc is required')
        self._params = np.array([qH, sigma0, epsilon0, _COULOMB, self.rc, self.width])
        self._setup = None

    def _prepare(self, atoms):
        cell = np.asarray(atoms.cell, dtype=float)
        pbc = tuple(bool(p) for p in atoms.pbc)
        key = (tuple(int(z) for z in atoms.numbers), cell.tobytes(), pbc)
        if self._setup is not None and self._setup[0] == key:
            return
        n = len(atoms)
        if n == 0 or n % 3:
            raise ValueError(f'TIP3P: {n} atoms are not a whole number of three-site molecules')
        z = np.asarray(atoms.numbers).reshape(-1, 3)
        if (z == (8, 1, 1)).all():
            o = 0
        elif (z == (1, 1, 8)).all():
            o = 2
        else:
            raise ValueError('TIP3P: the atoms must be consecutive molecules, all O H H or all H H O')
        box = np.zeros(3)
        for k in range(3):
            if not pbc[k]:
                continue
            if np.any(np.delete(cell[k], k) != 0.0) or np.any(np.delete(cell[:, k], k) != 0.0) or not cell[k, k] > 0.0:
                raise ValueError('TIP3P: the cell must be diagonal in its periodic directions (orthorhombic box)')
            if cell[k, k] < 2.0 * self.rc:
                raise ValueError(f'TIP3P: the periodic edge {cell[k, k]:.3f} is shorter than 2 rc = {2.0 * self.rc:.3f} '
                                 f'(minimum image only)')
            box[k] = cell[k, k]
        self._setup = (key, dict(nmol=n // 3, o=o, box=box))
        self._key = None                           # results cached for the old cell are stale
        self._drop_hessian()

    def _get(self, atoms, stress=False):
        self._prepare(atoms)
        return super()._get(atoms, stress)

    def _tip3p_args(self, pos):
        if self._setup is None:
            raise RuntimeError('TIP3P: no atoms seen yet (evaluate through an Atoms object first)')
        S = self._setup[1]
        return pos, S['o'], S['box'], self._params

    def energy_and_gradient(self, pos):
        from .device import get_context
        return get_context().tip3p_eval(*self._tip3p_args(pos))

    def device_hessian(self, pos):
        """The analytic Hessian (csrc/tip3p.hip: 9 x 9 blocks per pair of molecules, the switch terms included)."""
        from .device import get_context
        return get_context().tip3p_hessian(*self._tip3p_args(pos))

    def hessian_products(self, pos, V):
        from .device import get_context
        return get_context().tip3p_hvp(*self._tip3p_args(pos), V)

    library_form = True

    def device_calculator(self):
        """This potential, for the molecules and cell it was last set up for, as a calculator inside the library
        (`sella_calc_tip3p_create`); None before the first evaluation."""
        if self._setup is None:
            return None
        hit = getattr(self, '_devcalc', None)
        if hit is None or hit[0] is not self._setup:
            from .device import DeviceCalculator, get_context
            S = self._setup[1]
            hit = (self._setup, DeviceCalculator.tip3p(get_context(), S['nmol'], S['o'], S['box'], self._params))
            self._devcalc = hit
        return hit[1]


class PairLJ(Calculator):
    def __init__(self, eps=1.0, sigma=1.0):
        super().__init__()
        self.eps, self.sigma = eps, sigma

    def energy_and_gradient(self, pos):
        n = len(pos)
        d = pos[:, None, :] - pos[None, :, :]
        iu = np.triu_indices(n, 1)
        rr = np.linalg.norm(d[iu], axis=1)
        s6 = (self.sigma / rr) ** 6
        e = np.sum(4 * self.eps * (s6 ** 2 - s6))
        de = 4 * self.eps * (-12 * s6 ** 2 + 6 * s6) / rr
        g = np.zeros_like(pos)
        u = d[iu] / rr[:, None]
        np.add.at(g, iu[0], de[:, None] * u)
        np.add.at(g, iu[1], -de[:, None] * u)
        return e, g


class _MiniOptimizer:
    """The subset of ase.optimize.optimize.Optimizer that `Sella` relies on."""

    def __init__(self, atoms, restart=None, logfile='-', trajectory=None, master=None):
        self.atoms = atoms
        self.optimizable = atoms
        self.restart = restart
        if logfile == '-':
            self.logfile = sys.stdout
            self._own_log = False
        elif logfile is None:
            self.logfile = None
            self._own_log = False
        elif isinstance(logfile, str):
            self.logfile = open(logfile, 'a')
            self._own_log = True
        else:
            self.logfile = logfile
            self._own_log = False
        self.nsteps = 0
        self.max_steps = 0
        self.fmax = None
        self.observers = []
        self._closers = []
        if trajectory is not None:
            # ase/optimize/optimize.py: a name opens a Trajectory writer owned by the optimizer; either way its
            # write() becomes an observer (one image per step)
            if isinstance(trajectory, str):
                from .trajectory import Trajectory
                trajectory = self.closelater(Trajectory(trajectory, 'w', atoms, master=master))
            self.attach(trajectory.write)
            self.trajectory = trajectory

    def closelater(self, obj):
        self._closers.append(obj)
        return obj

    def attach(self, function, interval=1, *args, **kwargs):
        self.observers.append((function, interval, args, kwargs))

    def call_observers(self):
        for function, interval, args, kwargs in self.observers:
            if interval > 0 and self.nsteps % interval == 0:
                function(*args, **kwargs)

    def irun(self, fmax=0.05, steps=100000000):
        self.fmax = fmax
        self.max_steps = self.nsteps + steps
        # ASE's order (ase/optimize/optimize.py irun): convergence is evaluated first, so that log() reports
        # the fmax / cmax of the geometry whose energy it prints
        conv = self.converged()
        self.log()
        self.call_observers()
        if conv:
            yield True
            return
        while self.nsteps < self.max_steps:
            self.step()
            self.nsteps += 1
            conv = self.converged()
            self.log()
            self.call_observers()
            if conv:
                yield True
                return
            yield False

    def run(self, fmax=0.05, steps=100000000):
        conv = False
        for conv in self.irun(fmax=fmax, steps=steps):
            pass
        return conv

    def close(self):
        for obj in self._closers:
            if hasattr(obj, 'close'):
                obj.close()
        if self._own_log and self.logfile is not None:
            self.logfile.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def converged(self, forces=None):
        raise NotImplementedError

    def log(self, forces=None):
        raise NotImplementedError

    def step(self):
        raise NotImplementedError


Optimizer = _AseOptimizer if HAVE_ASE else _MiniOptimizer
