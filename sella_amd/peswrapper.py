"""`PES` — the potential-energy-surface wrapper of the saddle-point loop, drop-in for the Cartesian
class of sella/peswrapper.py:214-607 (same constructor, getters, `diag()`, `kick()`,
`converged()`), built on the device-resident `ApproximateHessian`.

The calculator boundary is untouched: `eval()` calls `atoms.get_potential_energy()` /
`atoms.get_forces()` exactly like peswrapper.py:413-418.  Everything n x n happens on the
MI355X: B·s products, U^T B U projections, the eigendecomposition shared by the Davidson
preconditioner / TS-BFGS / P-RFO, the Davidson loop and the quasi-Newton updates.
Host-side (as in the reference, outside its accelerator seam): the rank-revealing pivoted QR
of the (ncons x n) constraint Jacobian and O(n) vector algebra.

Also here: `InternalPES` (redundant internal coordinates) and `CellCartesianPES` (positions and unit cell together,
for minima).  Not restated: CellInternalPES.
"""
import numpy as np
from scipy.linalg import eigh, qr

from .atoms import Atoms  # noqa: F401  (re-export for users without ASE)
from .device import get_context
from .eigensolvers import rayleigh_ritz
from .hessian_update import symmetrize_Y
from .internal import Constraints, DuplicateInternalError
from .linalg import AnalyticHessian, ApproximateHessian, NumericalHessian
from .utilities.math import register_selection, selection_of, is_identity, shared_identity


class _LRU2:
    """Two-entry cache keyed by the geometry hash (peswrapper.py:24-48)."""

    def __init__(self):
        self._entries = [None, None]
        self._next = 0

    def get(self, key):
        for e in self._entries:
            if e is not None and e[0] == key:
                return e[1]
        return None

    def put(self, key, value):
        if self.get(key) is not None:
            return
        self._entries[self._next] = (key, value)
        self._next = 1 - self._next


def _pinned_coordinates(drdx):
    """(column index, value) per row when every constraint pins exactly one distinct Cartesian coordinate
    (fix_translation on single atoms), else None.  For such constraints the least-squares solves of the glue
    code (multipliers, linear constraint correction, peswrapper.py:429-438, 475-479) are componentwise divisions."""
    if drdx.shape[0] == 0:
        return None
    memo = _pinned_memo[0]                           # ONE read of ONE slot: (drdx, out) is published atomically, so
    if memo is not None and memo[0] is drdx:         # threads driving different replicas never mix key and value
        return memo[1]
    nz = drdx != 0.0
    if not np.all(nz.sum(axis=1) == 1):
        out = None
    else:
        cidx = nz.argmax(axis=1)
        out = None if len(np.unique(cidx)) != len(cidx) else (cidx, drdx[np.arange(len(cidx)), cidx])
    if not drdx.flags.writeable:                     # read-only Jacobian of a translation-only constraint set
        _pinned_memo[0] = (drdx, out)
    return out


_pinned_memo = [None]


def _split_cons_subspace(drdx, tol_factor=1e-6):
    """(Ucons, Ufree): row space of the constraint Jacobian and its orthogonal complement by
    rank-revealing pivoted QR of drdx^T (peswrapper.py:51-69)."""
    n = drdx.shape[1]
    if drdx.shape[0] == 0:
        return np.zeros((n, 0)), shared_identity(n)
    # Constraints that each pin one Cartesian coordinate (fix_translation on single atoms, the README slab) span a
    # coordinate subspace: the bases are columns of the identity and no O(n^3) full QR is needed.  Any
    # orthonormal basis of the same subspaces gives the same projected problem.
    nz = drdx != 0.0
    if np.all(nz.sum(axis=1) == 1):
        cols = np.flatnonzero(nz.any(axis=0))
        if len(cols) == drdx.shape[0]:
            free = np.setdiff1d(np.arange(n), cols)
            eye = shared_identity(n)
            # (fancy indexing along axis 1 returns a Fortran-ordered array: make the C copy once, not at every upload)
            return (register_selection(np.ascontiguousarray(eye[:, cols]), cols),
                    register_selection(np.ascontiguousarray(eye[:, free]), free))
    Q, R, _ = qr(drdx.T, mode='full', pivoting=True, check_finite=False)
    diag = np.abs(np.diag(R))
    # A Jacobian that vanishes to rounding constrains nothing: rigid-body constraints seen from internal coordinates that
    # are themselves invariant under translation and rotation (rows of ~1e-16: the relative rule alone counted them all)
    ncons = int(np.sum(diag > tol_factor * diag[0])) if diag.size and diag[0] > 1e-12 else 0
    return Q[:, :ncons], Q[:, ncons:]


def open_trajectory(name, atoms, append=False):
    """A file NAME passed as `trajectory=` (peswrapper.py:257-261, optimize.py:144-150 of the reference): an ASE
    `.traj` file (sella_amd/trajectory.py) like the reference writes — or, for names ending in .xyz / .extxyz, the
    extended-XYZ text writer."""
    if name.lower().endswith(('.xyz', '.extxyz')):
        from .atoms import XYZTrajectory
        return XYZTrajectory(name, atoms, mode='a' if append else 'w')
    from .trajectory import Trajectory
    return Trajectory(name, 'a' if append else 'w', atoms)


class PES:
    n_cell_dof = 0
    # `hessian_vector_product=`: exact products for the iterative diagonalisation, Cartesian coordinates only (the
    # subclasses for internal coordinates and for the cell refuse the keyword)
    _accepts_hvp = True
    _hvp_hint = ''

    def __init__(self, atoms, H0=None, constraints=None, eigensolver='jd0', trajectory=None,
                 eta=1e-4, v0=None, proj_trans=None, proj_rot=None, hessian_function=None, hessian_vector_product=None):
        self.atoms = atoms
        self._hvp, self._hvp_from_calc = self._resolve_hvp(atoms, hessian_vector_product), hessian_vector_product is True
        self.nhvp = 0                                        # Hessian-vector products taken (`neval` counts force calls only)
        self.cons = self._constraint_set(atoms, constraints, proj_trans, proj_rot)
        self.eigensolver, self.eta, self.v0 = eigensolver, eta, v0
        self.hessian_function = hessian_function
        self.traj = open_trajectory(trajectory, atoms) if isinstance(trajectory, str) else trajectory
        # coordinate system: Cartesian here (subclasses set `int` / `dummies` and the sizes themselves)
        self.int = self.dummies = None
        self.dim = self.ncart = 3 * len(atoms)
        # the cached point and its predecessor (plain dicts: the IRC driver swaps them in and out), counters
        self.curr = dict.fromkeys(('x', 'f', 'g'))
        self.last = dict(self.curr)
        self.savepoint = dict.fromkeys(('apos', 'dpos'))
        self.neval = 0
        self.first_diag = True
        self._basis_cache = _LRU2()
        self.set_H(H0, initialized=H0 is not None)

    def _resolve_hvp(self, atoms, hvp):
        """`V (k, 3N) -> H V[q] (k, 3N)` at the geometry the atoms have when it is called, from the keyword
        `hessian_vector_product`: True takes the calculator's own, a callable f(atoms, V) is taken as it is."""
        if hvp is None or hvp is False:
            return None
        if not self._accepts_hvp:
            raise NotImplementedError(f'hessian_vector_product is not implemented for {type(self).__name__}: the products '
                                      f'exist in Cartesian coordinates at fixed cell only{self._hvp_hint}')
        if hvp is True:
            from .atoms import supports_hessian
            calc = getattr(atoms, 'calc', None)
            own = getattr(calc, 'hessian_vector_product', None)
            if not supports_hessian(calc) or not callable(own):
                raise NotImplementedError(f'hessian_vector_product=True needs a calculator with its own Hessian-vector '
                                          f'product, and {type(calc).__name__} has none')
            return lambda V: own(self.atoms, V)
        if not callable(hvp):
            raise TypeError('hessian_vector_product must be True or a callable f(atoms, V (k, 3N)) -> (k, 3N)')
        return lambda V: hvp(self.atoms, V)

    @staticmethod
    def _constraint_set(atoms, constraints, proj_trans, proj_rot):
        """The constraints a search runs under (peswrapper.py:226-253): the user's, plus — unless they already say
        something about it or the caller decides otherwise — a fixed centre of the system and, for non-periodic
        systems, fixed global rotations.  The rotation constraint is the LINEARISED one (infinitesimal generators about
        the centroid, internal.py Constraints.fix_rotation): the three rotational soft modes leave the Davidson / P-RFO
        subspace exactly as in the reference."""
        cons = Constraints(atoms) if constraints is None else constraints
        want_trans = (not cons.internals['translations']) if proj_trans is None else proj_trans
        want_rot = (not np.any(atoms.pbc)) if proj_rot is None else proj_rot
        if want_trans:
            try:
                cons.fix_translation(replace_ok=False)
            except DuplicateInternalError:
                pass                                             # some component is pinned already
        if want_rot and not cons.internals['rotations']:
            cons.fix_rotation()
        return cons

    apos = property(lambda self: self.atoms.positions.copy())
    dpos = property(lambda self: None)

    def _state_hash(self):
        """Key of everything cached per geometry: the bytes of the positions and, if there is one, of the cell."""
        parts = [np.ascontiguousarray(self.atoms.positions).tobytes()]
        cell = np.asarray(self.atoms.cell, dtype=float)
        if cell.any():
            parts.append(cell.tobytes())
        return b''.join(parts)

    def save(self):
        self.savepoint = {'apos': self.apos, 'dpos': self.dpos}

    def restore(self):
        kept = self.savepoint['apos']
        if kept is None:
            raise AssertionError('PES.restore() without a saved geometry')
        self.atoms.positions = kept

    def close(self):
        if self.traj is not None:
            self.traj.close()
            self.traj = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ---- positions -------------------------------------------------------------------------
    def set_x(self, target):
        diff = target - self.get_x()
        self.atoms.positions = target.reshape((-1, 3))
        g = self.curr.get('g')
        return diff, diff, (np.zeros_like(diff) if g is None else g)

    def get_x(self):
        return self.apos.ravel().copy()

    # ---- Hessians ----------------------------------------------------------------------------
    def get_H(self):
        return self.H

    def set_H(self, target, *args, **kwargs):
        self.H = ApproximateHessian(self.dim, self.ncart, target, *args, **kwargs)

    def get_Hc(self):
        """Constraint curvature contracted with the multipliers, sum_k L_k d2 r_k / dx2."""
        multipliers = self.curr.get('L')
        if multipliers is None:
            raise RuntimeError("PES.get_Hc() called with L=None.")
        return self.cons.hessian().ldot(multipliers)

    def get_HL(self):
        """Hessian of the Lagrangian as a lazy sum (linalg.MatrixSum semantics)."""
        return self.H + (-self.get_Hc())

    def _has_curved_constraints(self):
        c = self.cons
        return (c.nbonds + c.nangles + c.ndihedrals) > 0

    def get_HL_projected(self, U):
        """ApproximateHessian(U^T (B - Hc) U) without forming HL (peswrapper.py:363-386).

        The result is cached per (Hessian version, basis): the optimizer asks for the same
        projection from the step solve and from the curvature test of one iteration.  Without
        curved constraints and with an identity basis the projection *is* B, and the object
        returned is the PES Hessian itself, so its device eigendecomposition is computed once and
        shared with the quasi-Newton update."""
        H = self.get_H()
        n = U.shape[1]
        if H._is_none:
            return ApproximateHessian(n, 0, None, H.update_method, H.symm)
        L = self.curr.get('L')
        curved = L is not None and L.size > 0 and self._has_curved_constraints()
        if is_identity(U) and not curved:
            return H
        selection = (not curved) and getattr(self, '_pinned_basis', None) is not None and U is self._pinned_basis[2]
        if selection:
            view = H.principal_view(U)
            if view is not None:
                return view
        key = (id(H), H.version, id(U), None if not curved else L.tobytes())
        hit = getattr(self, '_hlproj_cache', None)
        if hit is not None and hit[0] == key and hit[1] is U:
            return hit[2]
        ctx = get_context()
        if is_identity(U):
            Bproj = H._get_B_gpu().copy()
        else:
            Bproj = ctx.project_dev(H._get_B_gpu(), ctx.resident(U))
        if curved:
            Hc = self.get_Hc()          # zero for translation-only constraints: skipped above
            dHc = ctx.upload(U.T @ Hc @ U)
            Bnew = ctx.axpby(1.0, Bproj, -1.0, dHc)
            Bproj.free()
            dHc.free()
            Bproj = Bnew
        out = ApproximateHessian(n, 0, Bproj, H.update_method, H.symm)
        self._hlproj_cache = (key, U, out)
        if selection:
            H.register_view(U, out)          # from now on updated together with H (linalg.ApproximateHessian.update)
        return out

    # ---- constraints ------------------------------------------------------------------------
    def get_res(self):
        return self.cons.residual()

    def get_drdx(self):
        return self.cons.jacobian()

    def _calc_basis(self):
        key = self._state_hash()
        cached = self._basis_cache.get(key)
        if cached is not None:
            return cached
        drdx = self.get_drdx()
        pinned = _pinned_coordinates(drdx)
        self._pinned_cache = (key, pinned)
        if pinned is not None:
            # coordinate-pinning constraints: the bases depend on the constraint set only, so the SAME arrays are
            # handed out at every geometry (downstream caches and device uploads key on the object)
            sig = pinned[0].tobytes()
            hit = getattr(self, '_pinned_basis', None)
            if hit is None or hit[0] != sig:
                Ucons, Ufree = _split_cons_subspace(drdx)
                hit = (sig, Ucons, Ufree)
                self._pinned_basis = hit
            Ucons, Ufree = hit[1], hit[2]
        else:
            Ucons, Ufree = _split_cons_subspace(drdx)
        result = (drdx, Ucons, shared_identity(self.dim), Ufree)
        self._basis_cache.put(key, result)
        return result

    def write_traj(self):
        if self.traj is not None:
            self.traj.write()

    # ---- the calculator boundary (peswrapper.py:413-418) ----------------------------------------
    def eval(self):
        self.neval += 1
        f = self.atoms.get_potential_energy()
        g = -np.asarray(self.atoms.get_forces()).ravel()
        self.write_traj()
        return f, g

    def _calc_eg(self, x):
        self.save()
        self.set_x(x)
        f, g = self.eval()
        self.restore()
        return f, g

    def get_scons(self):
        """Minimum-norm linear correction towards the constraint manifold (peswrapper.py:429-438)."""
        Ucons = self.get_Ucons()
        if Ucons.shape[1] == 0:
            return np.zeros(self.dim)
        pinned = self._pinned()
        if pinned is not None and self.int is None:
            s = np.zeros(self.dim)
            s[pinned[0]] = -self.get_res() / pinned[1]
            return s
        return -Ucons @ np.linalg.lstsq(self.get_drdx() @ Ucons, self.get_res(), rcond=None)[0]

    def _pinned(self):
        """Cached `_pinned_coordinates` of the current constraint Jacobian (it only depends on the constraint
        set for translation constraints, but is keyed on the geometry like the basis)."""
        key = self._state_hash()
        hit = getattr(self, '_pinned_cache', None)
        if hit is None or hit[0] != key:
            hit = (key, _pinned_coordinates(PES.get_drdx(self)) if self.int is None else None)
            self._pinned_cache = hit
        return hit[1]

    # ---- the cached point: geometry -> (basis, energy, gradient, multipliers) ---------------------------------------
    # `curr` / `last` are plain dicts because callers swap them in and out (IRC, sella/optimize/irc.py:62-75); what
    # fills them is organised around ONE question — does the cache describe the geometry the atoms have now?
    def _cache_status(self, want_energy):
        """'fresh': nothing to do; 'energy': same geometry, energy / gradient still missing; 'moved': new geometry."""
        here = self._state_hash()
        if self.curr['x'] is None or here != self.curr.get('state_hash'):
            return 'moved', here
        if want_energy and self.curr['f'] is None:
            return 'energy', here
        return 'fresh', here

    def _update(self, feval=True):
        status, here = self._cache_status(feval)
        if status == 'fresh':
            return False
        basis = self._calc_basis()
        energy, gradient = self.eval() if feval else (None, None)
        if status == 'moved':
            self.last = self.curr.copy()          # the previous point becomes the reference of the next secant pair
        self.curr.update(x=self.get_x(), state_hash=here, f=energy, g=gradient)
        self._update_basis(basis)
        return True

    def _multipliers(self, drdx, g):
        """Lagrange multipliers of the constraint forces: least-squares solution of drdx^T L = g (peswrapper.py:475-479);
        a division per constraint when every constraint pins one coordinate."""
        if g is None:
            return None
        if drdx.shape[0] == 0:
            return np.zeros(0)
        pinned = self._pinned()
        if pinned is not None:
            return g[pinned[0]] / pinned[1]
        return np.linalg.lstsq(drdx.T, g, rcond=None)[0]

    def _update_basis(self, basis=None):
        drdx, Ucons, Unred, Ufree = self._calc_basis() if basis is None else basis
        self.curr.update(drdx=drdx, Ucons=Ucons, Unred=Unred, Ufree=Ufree, L=self._multipliers(drdx, self.curr['g']))

    def _update_H(self, dx, dg):
        if self.last['x'] is None or self.last['g'] is None:
            return
        self.H.update(dx, dg)

    def _point_getter(name, needs_energy, copy=False):      # noqa: N805 — class-body helper, not a method
        """Accessor of one entry of the cached point: bring the cache up to date (with or without a force call), hand
        the entry out (a copy where callers modify what they get)."""
        def getter(self):
            self._update(needs_energy)
            value = self.curr[name]
            return value.copy() if copy else value
        getter.__name__ = 'get_' + name
        return getter

    get_f = _point_getter('f', True)
    get_g = _point_getter('g', True, copy=True)
    get_Unred = _point_getter('Unred', False)
    get_Ufree = _point_getter('Ufree', False)
    get_Ucons = _point_getter('Ucons', False)
    del _point_getter

    # ---- iterative diagonalisation (peswrapper.py:508-556) ----------------------------------------
    def diag(self, gamma=0.1, threepoint=False, maxiter=None):
        self._update(True)                                  # energy and gradient of the point the operator is built at
        Ufree = self.get_Ufree()
        if Ufree.shape[1] == 0:
            return
        P = self.get_HL_projected(Ufree)
        P_is_none = P._is_none
        # start vector (peswrapper.py:521-529): only while there is no curvature information to start from — the user's
        # v0, else the projected gradient, unless that vanishes
        v0 = None
        if P_is_none or self.first_diag:
            v0 = self.v0
            if v0 is None:
                g = self.get_g()
                v0 = g if is_identity(Ufree) else g @ Ufree
            if np.linalg.norm(v0) < 1e-12:
                v0 = None
        if self._hvp is not None:
            # exact products (`hessian_vector_product=`): no displacement, so `threepoint` has no meaning here
            Hproj = self._library_hvp_operator(Ufree)
            if Hproj is None:
                Hproj = AnalyticHessian(self._hvp, self.dim, Ufree)
        else:
            Hproj = self._library_fd_operator(Ufree, threepoint)
            if Hproj is None:
                Hproj = NumericalHessian(self._calc_eg, self.get_x(), self.get_g(), self.eta, threepoint, Ufree)
        A = Hproj
        Hc = None
        if self._has_curved_constraints():
            Hc = self.get_Hc()
            A = Hproj + (-(Ufree.T @ Hc @ Ufree))
        # P is handed over as the ApproximateHessian itself: its device eigendecomposition is the
        # preconditioner of the JD correction (sella_amd/csrc/davidson.hip)
        rayleigh_ritz(A, gamma, None if P_is_none else P, v0=v0, method=self.eigensolver, maxiter=maxiter)

        Vs, AVs = Hproj.Vs, Hproj.AVs
        if self._hvp is not None:
            self._count_products(Hproj)
        elif not isinstance(Hproj, NumericalHessian):
            self.neval += Hproj.calls * (2 if threepoint else 1)     # force calls the library made itself
        # Ritz vectors of the collected full-space iterates (peswrapper.py:545-551)
        Atilde = Vs.T @ symmetrize_Y(Vs, AVs, symm=2)
        if Hc is not None:
            Atilde = Atilde - Vs.T @ Hc @ Vs
        _, X = eigh(Atilde)
        self.H.update(Vs @ X, AVs @ X)
        self.first_diag = False

    def _count_products(self, Hproj):
        self.nhvp += Hproj.calls                                     # products, not force calls

    def _library_fd_operator(self, Ufree, threepoint):
        """The finite-difference Hessian as a library object (`sella_fd_*`) when the calculator itself lives in the
        library (`atoms.calc.device_calculator()`): the force calls of the Davidson run are then library calls, with no
        interpreter frame between them.  Needs a basis that is the identity or a selection of coordinates, no curved
        constraints, and nobody listening per force call (a trajectory writes one image per call, peswrapper.py:409-418)."""
        route = self._library_route(Ufree)
        if route is None:
            return None
        from .device import DeviceFdOperator
        return DeviceFdOperator(route[0], self.get_x(), self.get_g(), self.eta, threepoint, route[1])

    def _library_route(self, Ufree):
        """(the calculator's library form, free coordinates or None for all) when an operator of the library can stand
        for the Hessian seen through Ufree, else None (the conditions in `_library_fd_operator`)."""
        calc = getattr(self.atoms, 'calc', None)
        maker = getattr(calc, 'device_calculator', None)
        if maker is None or self.traj is not None or self._has_curved_constraints() or type(self) is not PES:
            return None
        if getattr(self, 'use_library_calculator', True) is False:
            return None
        free = None
        if not is_identity(Ufree):
            free = selection_of(Ufree)
            if free is None:
                return None
        dc = maker()
        if dc is None:
            return None
        return dc, free

    def _library_hvp_operator(self, Ufree):
        """The analytic Hessian as a library object (`sella_hvp_*`, `DeviceHvpOperator`) under the conditions of
        `_library_fd_operator`, when the products are the calculator's own (`hessian_vector_product=True`): its state at
        this geometry is built once, and the products of the Davidson run never leave the device."""
        if not self._hvp_from_calc:
            return None
        route = self._library_route(Ufree)
        if route is None:
            return None
        from .device import DeviceHvpOperator
        return DeviceHvpOperator(route[0], self.get_x(), route[1])

    def get_projected_forces(self):
        g = self.get_g()
        Ufree = self.get_Ufree()
        if is_identity(Ufree):
            return -g.reshape((-1, 3))
        hit = getattr(self, '_pinned_basis', None)
        if hit is not None and Ufree is hit[2]:
            # columns of the identity: the projection keeps the free components and zeroes the pinned ones
            if len(hit) < 4:
                sel = selection_of(Ufree)
                hit = self._pinned_basis = hit + (Ufree.argmax(axis=0) if sel is None else sel,)
            out = np.zeros_like(g)
            out[hit[3]] = g[hit[3]]
            return -out.reshape((-1, 3))
        return -(Ufree @ (Ufree.T @ g)).reshape((-1, 3))

    def converged(self, fmax, cmax=1e-5):
        """(done, largest projected force on an atom, norm of the constraint residual)."""
        per_atom = self.get_projected_forces()
        worst_force = np.sqrt(np.einsum('ij,ij->i', per_atom, per_atom).max())
        violation = np.linalg.norm(self.get_res())
        return bool(worst_force < fmax and violation < cmax), worst_force, violation

    def wrap_dx(self, dx):
        return dx

    def get_df_pred(self, dx, g, H):
        """Energy change of the quadratic model along dx (one Hessian-vector product on the device)."""
        return None if H is None else float(g @ dx + 0.5 * (dx @ (H @ dx)))

    # ---- step + update (peswrapper.py:578-602) -------------------------------------------------------
    def kick(self, dx, diag=False, **diag_kwargs):
        """Take the step dx: returns the ratio of the actual to the predicted energy change (None when no prediction
        is possible), after teaching the approximate Hessian the new secant pair and — if asked — refreshing its
        lowest modes by iterative diagonalisation."""
        before = dict(x=self.get_x(), f=self.get_f(), g=self.get_g())
        dx_asked, dx_taken, g_transported = self.set_x(before['x'] + dx)
        # quadratic model of the energy change along the step that was asked for (B dx on the device)
        predicted = self.get_df_pred(dx_asked, before['g'], self.H)
        secant_dg = self.get_g() - g_transported
        actual = self.get_f() - before['f']
        ratio = actual / predicted if (predicted is not None and abs(predicted) >= 1e-14) else None
        self._update_H(dx_taken, secant_dg)
        if diag:
            if self.hessian_function is not None:
                self.calculate_hessian()
            else:
                self.diag(**diag_kwargs)
        return ratio

    def calculate_hessian(self):
        assert self.hessian_function is not None
        self.H.set_B(self.hessian_function(self.atoms))


# ------------------------------------------------------------------------------------------------
# InternalPES — optimisation in redundant internal coordinates with geodesic steps
# (sella/peswrapper.py:609-1288; Hermes et al., J. Chem. Phys. 155, 094105 (2021)).
#
# Scope of this build: translations / bonds / angles / dihedrals / rotations given as an `InternalCoordinates`
# object (or found automatically from covalent radii), Cartesian constraints expressed through the usual
# `Constraints` object.  Dummy atoms at linear centres are extra Cartesian degrees of freedom of this class
# (:641-667, 756-834, 967-991, 1124-1127): the Cartesian vector is [atoms; dummies], 3 (N + D) long; the
# calculator, the trajectory, the forces and `converged()` concern the N real atoms.  Not built: carrying the
# approximate Hessian across a re-generation of the internals (`update_internals`, :1126-1172 — `Sella` builds a
# fresh PES instead), cell degrees of freedom.
# The heavy pieces run on the device: B-matrix rows and D(v) = H_i v (csrc/internals.hip), the range basis
# and pseudo-inverse of B through the device eigensolver (`_BFactor`, in place of the reference's
# `_gpu_qr` + SVD, :691-709), the Hessian algebra as for `PES`.
# Parity: the reference class needs ASE + JAX and cannot be imported in the build container, so this
# restatement is property-tested only (tests/test_internal_pes.py) — unpinned.
# ------------------------------------------------------------------------------------------------
from scipy.integrate import LSODA  # noqa: E402

from .internal import InternalCoordinates  # noqa: E402


class _BFactor:
    """B = dq/dx (nint x 3N) held sparse together with the spectral factor of its Gram matrix.

    The reference takes an economy QR of the dense B and, because B never has full column rank without
    TRIC coordinates (the rigid-body motions are in its null space), falls through to a dense SVD
    (peswrapper.py:674-709) to get the range basis Q and the pseudo-inverse.  Both follow from the
    eigendecomposition of the small Gram matrix — G = B^T B = V L V^T (3N x 3N) when nint >= 3N, else
    G = B B^T — which is assembled from the sparse rows and diagonalised by the device eigensolver:

        Q = B V_r L_r^-1/2   R = L_r^1/2 V_r^T   B^+ = M B^T,  M = V_r L_r^-1 V_r^T   (device resident)

    (singular values s_i = sqrt(l_i) > 1e-6 kept, like `Si > 1e-6` in the reference).  B^+ y is then one
    sparse product and one symmetric matrix-panel product on the device; nothing of size nint x 3N is
    formed unless a caller asks for the dense pseudo-inverse.  The pseudo-inverse is unique, Q is one of
    the (equally arbitrary) orthonormal bases of range(B)."""

    def __init__(self, Bs, tol=1e-6):
        ctx = get_context()
        self.Bs = Bs.tocsr()
        self.BsT = Bs.T.tocsr()
        nint, nx = Bs.shape
        self.shape = (nint, nx)
        self.left = nint < nx                       # Gram matrix on the short side
        G = ((self.Bs @ self.BsT) if self.left else (self.BsT @ self.Bs)).toarray()
        n = G.shape[0]
        if n == 0:
            self.rank, self.s, self.M, self._N0 = 0, np.zeros(0), None, None
            self._Q, self._R, self.BinvQ, self._dense = np.zeros((nint, 0)), np.zeros((0, nx)), np.zeros((nx, 0)), None
            return
        hG = ctx.upload(G)
        w, V, Vt = ctx.eigh(hG)
        hG.free()
        V.free()
        floor = max(tol * tol, 64 * n * np.finfo(float).eps * max(w[-1], 0.0))
        keep = np.flatnonzero(w > floor)[::-1]                    # descending singular values
        Vall = Vt.numpy()
        Vr = Vall[keep]                                           # (r, n): eigenvectors as rows
        # null space of the Gram matrix = null(B) on the Cartesian side (rigid-body motions): its basis lets
        # `pinv_dot_moved` return the MINIMUM-NORM solution at a nearby geometry
        self._N0 = None if self.left else np.ascontiguousarray(Vall[np.setdiff1d(np.arange(n), keep)].T)
        Vt.free()
        self.s = np.sqrt(w[keep])
        self.rank = len(keep)
        X = np.ascontiguousarray(Vr / self.s[:, None])            # rows v_i / s_i
        hX = ctx.upload(X)
        self.M = ctx.zeros(n, n)
        ctx.gemm(hX, hX, self.M, transA=True)                     # M = V_r L_r^-1 V_r^T
        hX.free()
        self._Vr = Vr
        self.BinvQ = None if self.left else np.ascontiguousarray(X.T)        # B^+ Q = V_r L_r^-1/2
        self._Q = self._R = self._dense = None
        if self.left:
            self._Q = np.ascontiguousarray(Vr.T)                  # left singular vectors
            self._R = np.ascontiguousarray((self.BsT @ self._Q).T)          # Q^T B
            self.BinvQ = np.ascontiguousarray(self._R.T / (self.s ** 2)[None, :])

    @property
    def Q(self):
        """Orthonormal basis of range(B), (nint, rank) — dense, formed on first use."""
        if self._Q is None:
            self._Q = np.ascontiguousarray(self.Bs @ self.BinvQ)
        return self._Q

    @property
    def R(self):
        if self._R is None:
            self._R = self.s[:, None] * self._Vr
        return self._R

    def pinv_dot(self, Y):
        """B^+ Y for Y (nint,) or (nint, k)."""
        if self.M is None or np.size(Y) == 0:
            return np.zeros((self.shape[1],) + np.shape(Y)[1:])
        ctx = get_context()
        if self.left:
            return self.BsT @ ctx.symm_mm(self.M, Y)
        return ctx.symm_mm(self.M, self.BsT @ Y)

    _NULL_MAX = 16          # more null directions than this: not a rigid-body null space, factorise anew

    def pinv_dot_moved(self, Bs_new, Y, tol=1e-11, maxit=30):
        """B_new^+ Y for the Jacobian of a NEARBY geometry, without a new factorisation: preconditioned conjugate
        gradients on the normal equations (B_new^T B_new) x = B_new^T Y with this factor's M = (B^T B)^+ as the
        preconditioner — M B_new^T B_new is the projector onto range(B^T) plus a perturbation of the size of the
        geometry change, so a handful of iterations (two sparse products and one device panel product each) reach
        1e-11.  The CG iterates stay in range(B^T) of the OLD geometry, so what converges is a least-squares solution
        that differs from the minimum-norm one by a null vector of B_new (the null space — rigid rotations of a
        molecule — has turned with the geometry).  The same solve therefore carries d extra columns B_new N0 (N0 = this
        factor's null basis, d = 3 ... 6): N0 - C spans null(B_new), and the solution is projected onto its
        orthogonal complement, which makes it B_new^+ Y exactly (the reference applies the pseudo-inverse of the
        current point, peswrapper.py:1200-1221).  Returns None if CG does not converge or the null space is not
        a small rigid-body one (the caller then factorises anew)."""
        if self.M is None or self.left or np.size(Y) == 0:
            return None
        ctx = get_context()
        Y2 = Y[:, None] if np.ndim(Y) == 1 else Y
        ny = Y2.shape[1]
        N0 = self._N0
        d = 0 if N0 is None else N0.shape[1]
        if d > self._NULL_MAX:
            return None
        if d:
            Y2 = np.column_stack((Y2, np.asarray(Bs_new @ N0)))
        BT_new = Bs_new.T.tocsr()
        R = np.asarray(BT_new @ Y2)
        X = np.zeros_like(R)
        Z = ctx.symm_mm(self.M, R)
        P = Z.copy()
        rz = np.einsum('ij,ij->j', R, Z)
        rz0 = np.where(rz > 0, rz, 1.0)
        # (null directions that B_new barely sees start with a residual at rounding level: relative to the scale
        # of the data columns they are converged from the start)
        floor = tol * tol * max(float(rz0[:ny].max()), 1e-300) * 1e-6
        for _ in range(maxit):
            AP = np.asarray(BT_new @ (Bs_new @ P))
            pap = np.einsum('ij,ij->j', P, AP)
            live = (rz > np.maximum(tol * tol * rz0, floor)) & (pap > 0)
            if not live.any():
                break
            alpha = np.where(live, rz / np.where(pap > 0, pap, 1.0), 0.0)
            X += alpha * P
            R -= alpha * AP
            Z = ctx.symm_mm(self.M, R)
            rz_new = np.einsum('ij,ij->j', R, Z)
            P = Z + np.where(live, rz_new / np.where(rz != 0, rz, 1.0), 0.0) * P
            rz = rz_new
        else:
            return None
        sol = X[:, :ny]
        if d:
            Nn, _ = np.linalg.qr(N0 - X[:, ny:])                 # orthonormal basis of null(B_new)
            sol = sol - Nn @ (Nn.T @ sol)
        return sol[:, 0] if np.ndim(Y) == 1 else sol

    def pinvT_dot(self, Y):
        """(B^+)^T Y for Y (3N,) or (3N, k) — e.g. the Cartesian gradient -> internal gradient."""
        if self.M is None or np.size(Y) == 0:
            return np.zeros((self.shape[0],) + np.shape(Y)[1:])
        ctx = get_context()
        if self.left:
            return ctx.symm_mm(self.M, self.Bs @ Y)
        return self.Bs @ ctx.symm_mm(self.M, Y)

    def pinv(self):
        """Dense B^+ (3N x nint)."""
        if self._dense is None:
            if self.M is None:
                self._dense = np.zeros(self.shape[::-1])
            else:
                M = self.M.numpy()
                self._dense = np.asarray(self.BsT @ M) if self.left else np.ascontiguousarray(np.asarray(self.Bs @ M).T)
        return self._dense

    def project_diag(self, h):
        """P diag(h) P with P = Q Q^T the projector onto range(B) (`_range_space_projector`,
        peswrapper.py:72-82, applied as in :644-650): three device GEMMs."""
        nint = self.shape[0]
        if self.rank == 0:
            return np.zeros((nint, nint))
        ctx = get_context()
        hQ = ctx.upload(self.Q)
        hQh = ctx.upload(self.Q * np.asarray(h)[:, None])
        hT = ctx.zeros(self.rank, self.rank)
        ctx.gemm(hQ, hQh, hT, transA=True)
        hQh.free()
        hZ = ctx.zeros(nint, self.rank)
        ctx.gemm(hQ, hT, hZ)
        hT.free()
        hH = ctx.zeros(nint, nint)
        ctx.gemm(hZ, hQ, hH, transB=True)
        H = hH.numpy()
        for hnd in (hQ, hZ, hH):
            hnd.free()
        return 0.5 * (H + H.T)


class InternalPES(PES):
    _accepts_hvp = False

    def __init__(self, atoms, internals, *args, H0=None, iterative_stepper=0, auto_find_internals=True,
                 exact_geodesic=False, **kwargs):
        if internals is None or internals is True:
            internals = InternalCoordinates.from_atoms(atoms, cons=kwargs.pop('constraints', None))
        self.int_orig = internals
        new_int = internals.copy()
        if new_int.cons is None:
            new_int.cons = Constraints(atoms, dummies=new_int._dummies)
        kwargs.pop('constraints', None)
        # global translations / rotations are never projected out in internal space (peswrapper.py:633-641): a
        # caller's `Sella(internal=True, proj_rot=...)` must not collide with the explicit keywords below
        kwargs.pop('proj_trans', None)
        kwargs.pop('proj_rot', None)
        self._factor_cache = _LRU2()
        self._real_factor_cache = _LRU2()
        self._Hc_cache = _LRU2()
        PES.__init__(self, atoms, *args, constraints=new_int.cons, H0=None, proj_trans=False, proj_rot=False,
                     **kwargs)
        self.int = new_int
        self.dim = len(self.get_x())
        self.ncart = self.int.ndof
        if H0 is None:
            # guess Hessian with the components in the infeasible (redundant) subspace zeroed, :644-650
            self.set_H(self._get_factor().project_diag(self.int.guess_hessian(diagonal_only=True)), initialized=False)
        else:
            self.set_H(H0, initialized=True)
        self.bad_int = None
        self.exact_geodesic = exact_geodesic
        self.iterative_stepper = iterative_stepper

    # ---- B = dq/dx: range basis and pseudo-inverse from one factorisation (:674-736) -------------------
    def _get_factor(self):
        key = self._state_hash()
        cached = self._factor_cache.get(key)
        if cached is None:
            cached = _BFactor(self.int.jacobian_csr())
            self._factor_cache.put(key, cached)
        return cached

    def _get_jacobian_qr(self):
        fac = self._get_factor()
        return fac.Q, fac.R

    def _get_Binv(self):
        return self._get_factor().pinv()

    # ---- dummy atoms: extra Cartesian degrees of freedom (:641-667, 872-875) -------------------------------------
    dpos = property(lambda self: None if self.int is None else self.int.dummies.copy())

    def _state_hash(self):
        h = PES._state_hash(self)
        if self.int is not None and self.int.ndummies:
            h += np.ascontiguousarray(self.int.dummies).tobytes()
        return h

    def restore(self):
        PES.restore(self)
        kept = self.savepoint.get('dpos')
        if kept is not None and len(kept):
            self.int.dummies = kept

    def _all_positions(self):
        return np.array(self.int.all_positions, dtype=np.float64)

    # ---- geodesic position update (:840-880, :1200-1221) ----------------------------------------------
    def _q_ode(self, t, y):
        nx = self.int.ndof
        x, dxdt, g = y.reshape((3, nx))
        dydt = np.zeros((3, nx))
        dydt[0] = dxdt
        self.int.set_all_positions(x)
        # rows of D(dxdt) are H_i dxdt (one device launch per kind); only D @ [dxdt, g] is needed
        rhs = self.int.hessian_rdot_mult(dxdt, np.column_stack((dxdt, g)))
        fac = self._ode_factor
        if self.exact_geodesic:
            # pseudo-inverse AT THE CURRENT POINT of the path (peswrapper.py:1200-1221 re-evaluates it at every
            # right-hand side): carried from the factor of the starting point by a few preconditioned CG
            # iterations on the sparse Jacobian instead of a new spectral factorisation per right-hand side
            # (130 ms each at 1024 atoms); a new factor is taken — and becomes the carrier — only if that stalls
            sol = fac.pinv_dot_moved(self.int.jacobian_csr(), rhs)
            if sol is None:
                fac = self._ode_factor = self._get_factor()
                sol = fac.pinv_dot(rhs)
            out = -sol
        else:
            out = -fac.pinv_dot(rhs)                                                          # (nx, 2)
        dydt[1] = out[:, 0]
        dydt[2] = out[:, 1]
        return dydt.ravel()

    def _set_x_ode(self, target):
        dx = self.wrap_dx(target - self.get_x())
        fac = self._get_factor()
        self._ode_factor = fac
        g_int = self.curr.get('g')
        if g_int is None:
            g_int = np.zeros_like(dx)
        y0 = np.hstack((self._all_positions().ravel(), fac.pinv_dot(np.column_stack((dx, g_int))).T.ravel()))
        ode = LSODA(self._q_ode, 0.0, y0, t_bound=1.0, atol=1e-6)
        t0, y = 0.0, y0
        while ode.status == 'running':
            ode.step()
            y, t0 = ode.y, ode.t
            self.bad_int = self.int.check_for_bad_internals()
            if self.bad_int is not None:
                break
            if ode.nfev > 1000:
                raise RuntimeError("Geometry update ODE is taking too long to converge!")
        if ode.status == 'failed':
            raise RuntimeError("Geometry update ODE failed to converge!")
        y = y.reshape((3, self.int.ndof))
        self.int.set_all_positions(y[0])
        B = self.int.jacobian_csr()
        return t0 * dx, t0 * (B @ y[1]), B @ y[2]

    def _set_x_iterative(self, target, max_iter=20):
        """Newton back-transformation q(x) = target (peswrapper.py:749-839): faster than the geodesic for small
        feasible steps; returns None — positions restored — when it does not settle, and `set_x` integrates the
        geodesic instead.  Acceptance rules as in the reference: root-mean-square residual below 1e-8, or a
        stagnated iteration that at least halved it and ends below 1e-6; a residual that doubles, a stagnation
        above half the initial residual or an internal coordinate turning degenerate abort.  The Newton correction
        is B^+ (target - q) with the pseudo-inverse of the CURRENT geometry (spectral factor, cached per geometry)."""
        start = self._all_positions()
        q0 = self.get_x()
        dq_wanted = target - q0
        g_int = self.curr.get('g')
        g_cart = self._get_factor().pinv_dot(g_int if g_int is not None else np.zeros_like(dq_wanted))

        def give_up():
            self.int.set_all_positions(start)
            return None

        first = previous = None
        stalled = 0
        for sweep in range(max_iter):
            miss = self.wrap_dx(target - self.get_x())
            rms = float(np.sqrt(miss @ miss / len(miss)))
            first = rms if first is None else first
            if rms < 1e-8:
                break
            if rms > 2.0 * first:
                return give_up()
            if sweep > 3 and rms > 0.95 * previous:
                stalled += 1
                if stalled >= 3:
                    if rms > 0.5 * first:
                        return give_up()
                    break
            elif sweep > 3:
                stalled = 0
            previous = rms
            self.int.set_all_positions(self._all_positions() + self._get_factor().pinv_dot(miss).reshape((-1, 3)))
            if self.int.check_for_bad_internals() is not None:
                return give_up()
        miss = self.wrap_dx(target - self.get_x())
        if np.sqrt(miss @ miss / len(dq_wanted)) > 1e-6:
            return give_up()
        return dq_wanted, self.get_x() - q0, self.int.jacobian_csr() @ g_cart

    def set_x(self, target):
        res = self._set_x_iterative(target) if self.iterative_stepper else None
        dx_initial, dx_final_ode, g_final = res if res is not None else self._set_x_ode(target)
        q_after = self.int.calc().copy()
        moved = self._project_to_constraints()
        return dx_initial, self._add_proj_delta(dx_final_ode, q_after, moved), g_final

    def _add_proj_delta(self, dx_int_final, q_after_ode, proj_moved):                 # :903-926
        if not proj_moved:
            return dx_int_final
        return dx_int_final + self.int.wrap(self.int.calc() - q_after_ode)

    def _project_to_constraints(self, target_tol=1e-7, max_iter=8, safety_limit=0.05):  # :928-994
        if self.cons.residual().size == 0:
            return False
        moved = False
        for _ in range(max_iter):
            r = self.cons.residual()
            if np.linalg.norm(r, ord=np.inf) < target_tol:
                return moved
            drdx, Ucons, _, _ = self._compute_basis_int()
            if Ucons.shape[1] == 0:
                return moved
            s = np.linalg.lstsq(drdx @ Ucons, -r, rcond=None)[0]
            dx = self._get_factor().pinv_dot(Ucons @ s)
            if np.linalg.norm(dx, ord=np.inf) > safety_limit:
                return moved
            self.int.set_all_positions(self._all_positions() + dx.reshape(-1, 3))
            moved = True
        return moved

    def get_x(self):
        x = self.int.calc()
        nd = self.int.ndihedrals
        if self.curr['x'] is not None and nd:
            # keep dihedrals continuous with the previous point instead of jumping by 2 pi (:996-1008); they sit
            # between the angles and the rotations
            sl = self.int._dihedral_slice()
            dx = x[sl] - self.curr['x'][sl]
            x[sl] = self.curr['x'][sl] + (dx + np.pi) % (2 * np.pi) - np.pi
        return x

    def wrap_dx(self, dx):
        return self.int.wrap(dx)

    # ---- constraints in internal space (:1011-1122) ------------------------------------------------------
    def _compute_Hc_int(self):
        if self.curr['L'] is None:
            raise RuntimeError("InternalPES.get_Hc() called with L=None.")
        fac = self._get_factor()
        n_dof = fac.shape[0]
        if self.curr['L'].size == 0:
            return np.zeros((n_dof, n_dof))
        D_cons = self.cons.hessian().ldot(self.curr['L'])
        L_int = fac.pinvT_dot(self.curr['L'] @ self.cons.jacobian())
        D_int = self.int.hessian().ldot(L_int)
        # Binv^T D Binv with D symmetric (3N x 3N)
        return fac.pinvT_dot(fac.pinvT_dot(D_cons - D_int).T)

    def get_Hc(self):
        key = self._state_hash()
        cached = self._Hc_cache.get(key)
        if cached is None:
            cached = self._compute_Hc_int()
            self._Hc_cache.put(key, cached)
        return cached

    def _has_curved_constraints(self):
        return True                      # in internal space even a fixed translation has a curvature term

    def get_drdx(self):
        return self._get_factor().pinvT_dot(PES.get_drdx(self).T).T     # dr/dq = dr/dx dx/dq

    def _compute_basis_int(self):
        fac = self._get_factor()
        Unred = Q = fac.Q
        n_int = Q.shape[0]
        cons_jac = self.cons.jacobian()
        if cons_jac.shape[0] == 0:
            return np.zeros((0, n_int)), np.zeros((n_int, 0)), Unred, Unred
        drdxnred = cons_jac @ fac.BinvQ                    # dr/dx B^+ Q
        Vcons, Vfree = _split_cons_subspace(drdxnred)
        if Vcons.shape[1] == 0:
            # constraints the internal coordinates cannot violate (a fixed centre and orientation seen from bonds and
            # angles): no constrained direction, and no multipliers from a Jacobian that is rounding noise
            return np.zeros((0, n_int)), np.zeros((n_int, 0)), Unred, Unred
        return drdxnred @ Q.T, Unred @ Vcons, Unred, Unred @ Vfree

    def _calc_basis(self):
        key = self._state_hash()
        cached = self._basis_cache.get(key)
        if cached is None:
            cached = self._compute_basis_int()
            self._basis_cache.put(key, cached)
        return cached

    # ---- calculator boundary: Cartesian gradient -> internal (:1124-1127) ---------------------------------
    def eval(self):
        f, g_cart = PES.eval(self)
        if self.int.ndummies:
            # the calculator knows no dummies: no force on them (`Binv[:len(g_cart)]`, :1124-1127)
            g_cart = np.concatenate([g_cart, np.zeros(3 * self.int.ndummies)])
        return f, self._get_factor().pinvT_dot(g_cart)

    def get_df_pred(self, dx, g, H):                                                    # :1174-1181
        if H is None:
            return None
        # dx_r . (Unred^T H Unred) . dx_r = p . H p with p = Unred Unred^T dx: two thin products and ONE
        # Hessian-vector product instead of the reference's projected matrix
        Unred = self.get_Unred()
        dx_r, g_r = dx @ Unred, g @ Unred
        p = Unred @ dx_r
        return g_r @ dx_r + (p @ (H @ p)) / 2.

    def get_projected_forces(self):                                                     # :1183-1192
        g = self.get_g()
        Ufree = self.get_Ufree()
        B = self.curr.get('B')
        if B is None:
            B = self.int.jacobian_csr()
        return -np.asarray((Ufree @ (Ufree.T @ g)) @ B).reshape((-1, 3))[:len(self.atoms)]      # real atoms

    def _update(self, feval=True):
        if not PES._update(self, feval=feval):
            return
        self.curr.update(B=self._get_factor().Bs)
        return True

    # ---- exact Hessians: hessian_function in internal coordinates (:1247-1288) -----------------------------------
    def _get_real_factor(self):
        """The spectral factor of B[:, :3N], the columns of the real atoms (the PES's own factor without dummies)."""
        if not self.int.ndummies:
            return self._get_factor()
        key = self._state_hash()
        cached = self._real_factor_cache.get(key)
        if cached is None:
            cached = _BFactor(self.int.jacobian_csr()[:, :3 * len(self.atoms)])
            self._real_factor_cache.put(key, cached)
        return cached

    def _convert_cartesian_hessian_to_internal(self, Hcart, consume=False):
        """The internal-coordinate Hessian of the Cartesian Hessian Hcart (3N x 3N, real atoms) as a `DeviceMatrix`
        (nint x nint): with B = B[:, :3N] = U_r S_r V_r^T (singular values above 1e-6), X = V_r S_r^-1 and Q = U_r,
        Hnred = X^T (Hcart - sum_i g_i d2q_i/dx2) X and lambda_bar the geometric mean of |eig(Hnred)|, the result is
        Q Hnred Q^T + lambda_bar (I - Q Q^T) — the reference's Unred Hnred Unred^T + lambda_bar Ured Ured^T.  lambda_bar is
        taken from the eigenvalues of the symmetric part of Hnred, which for an asymmetric Hcart (finite differences)
        differ from those of the one triangle the reference's eigh reads.  Runs on the device
        (`sella_hessian_cart_to_int`); dummy degrees of freedom enter as zero rows and columns of Hcart and zero rows of
        X.  Hcart may be a `DeviceMatrix` (a calculator's own): it is not taken to the host and back.  The conversion
        overwrites its input, so it works on a device copy — unless `consume` hands the matrix over, which is then used
        as it is and freed."""
        from .device import DeviceMatrix
        n, nx = 3 * len(self.atoms), self.int.ndof
        on_device = isinstance(Hcart, DeviceMatrix)        # (a calculator's own, e.g. EMT.get_device_hessian: not copied
        if not on_device:                                  # to the host and back)
            Hcart = np.asarray(Hcart, dtype=np.float64)
        if Hcart.shape != (n, n):
            raise ValueError(f'hessian_function must return the {n} x {n} Cartesian Hessian of the {len(self.atoms)} '
                             f'atoms, got an array of shape {Hcart.shape}')
        fac = self._get_real_factor()
        X, Q = fac.BinvQ, fac.Q
        ctx = get_context()
        given = Hcart if on_device and consume else None
        if on_device and nx != n:                          # dummy atoms: the zero frame around it is put on on the host
            Hcart, on_device = Hcart.numpy(), False
        if on_device:
            hH = Hcart if consume else Hcart.copy()
        if nx != n:
            Hcart = np.pad(Hcart, ((0, nx - n), (0, nx - n)))
            X = np.pad(X, ((0, nx - n), (0, 0)))
        g = self.get_g()
        hess = self.int.sparse_hessians()                  # B and the d2q_i/dx2 of this geometry, on the device
        if not on_device:
            hH = ctx.upload(Hcart)
        hX, hQ = ctx.upload(X), ctx.upload(Q)
        try:
            out, _ = ctx.hessian_cart_to_int(hess._device(), g, hH, hX, hQ)
        finally:
            for h in (hH, hX, hQ):
                h.free()
            if given is not None:
                given.free()                               # (no-op if it was hH)
        return out

    def _convert_internal_hessian_to_cartesian(self, Hint):
        """B^T Hint B + sum_i g_i d2q_i/dx2 over all Cartesian degrees of freedom, dummies included (3(N + D) square), as
        a `DeviceMatrix`; Hint (nint x nint) a `DeviceMatrix` or an array (`sella_hessian_int_to_cart`)."""
        from .device import DeviceMatrix
        ctx = get_context()
        g = self.get_g()
        own = not isinstance(Hint, DeviceMatrix)
        hI = ctx.upload(np.asarray(Hint, dtype=np.float64)) if own else Hint
        try:
            return ctx.hessian_int_to_cart(self.int.sparse_hessians()._device(), g, hI)
        finally:
            if own:
                hI.free()

    def calculate_hessian(self):
        assert self.hessian_function is not None
        # what the hessian_function returns is the PES's from here on, as in `PES.calculate_hessian` (set_B keeps it)
        self.H.set_B(self._convert_cartesian_hessian_to_internal(self.hessian_function(self.atoms), consume=True))

    def kick(self, dx, diag=False, **diag_kwargs):
        # A geodesic that runs into a degenerate internal coordinate (an angle close to 0 or pi) stops there:
        # `bad_int` stays set and the caller — `Sella.step`, optimize.py:384-410 — rebuilds the coordinate system
        # from the geometry reached.
        return PES.kick(self, dx, diag=diag, **diag_kwargs)


# ------------------------------------------------------------------------------------------------
# CellCartesianPES — atomic positions and the unit cell together, for minima (sella/peswrapper.py:2376-2935).
#
# Coordinates x = [positions (3N), masked entries of L = logm(F) * exp_cell_factor], F = cell . orig_cell^-1 (the
# log-deformation of ASE's FrechetCellFilter).  The gradient of the cell coordinates comes from the calculator's stress:
# dE/dC = C^-T (V sigma + r^T f) at fixed Cartesian positions, dE/dF = dE/dC C0^T, and dE/dL through the Frechet
# derivative of expm (Daleckii-Krein form).  The cell coordinates carry no constraints; the search runs through the
# general driver (the fused step, the library finite-difference operator and the library search loop are for `PES`
# itself).
# ------------------------------------------------------------------------------------------------
from scipy.linalg import expm, expm_frechet, logm  # noqa: E402

from .atoms import voigt_to_matrix  # noqa: E402


def logm_3x3(F):
    """Principal logarithm of a real 3 x 3 matrix with positive eigenvalues, V diag(log lam) V^-1 from its
    eigendecomposition; scipy's `logm` when the eigenvector matrix is ill-conditioned (nearly defective F)."""
    lam, V = np.linalg.eig(F)
    if np.linalg.cond(V) > 1e10:
        return np.real(logm(F))
    return np.real(V @ np.diag(np.log(lam.astype(complex))) @ np.linalg.inv(V))


def expm_frechet_3x3_contracted(U, G):
    """g_mn = sum_ab G_ab [D expm(U)[E_mn]]_ab for all nine unit directions E_mn: the gradient with respect to U of a
    function whose gradient with respect to F = expm(U) is G.  For diagonalisable U = V diag(lam) V^-1 the Frechet
    derivative is D expm(U)[E] = V (f o (V^-1 E V)) V^-1 with the divided differences f_ij = (e^lam_i - e^lam_j) /
    (lam_i - lam_j) (e^lam_i on the diagonal and for equal eigenvalues; Daleckii-Krein), which contracts to
    g = V^-T (f o (V^T G V^-T)) V^T.  U ~ 0 gives the identity map; an ill-conditioned eigenbasis falls back to
    scipy's `expm_frechet`, direction by direction."""
    if np.linalg.norm(U) < 1e-10:
        return np.array(G, dtype=np.float64)
    lam, V = np.linalg.eig(U)
    if np.linalg.cond(V) > 1e10:
        g = np.zeros((3, 3))
        for m in range(3):
            for n in range(3):
                E = np.zeros((3, 3))
                E[m, n] = 1.0
                g[m, n] = np.sum(expm_frechet(U, E, compute_expm=False) * G)
        return g
    Vinv = np.linalg.inv(V)
    el = np.exp(lam)
    diff = lam[:, None] - lam[None, :]
    distinct = np.abs(diff) > 1e-12 * max(np.abs(lam).max(), 1.0)
    f = np.where(distinct, (el[:, None] - el[None, :]) / np.where(distinct, diff, 1.0), el[:, None])
    return np.real(Vinv.T @ (f * (V.T @ G @ Vinv.T)) @ V.T)


def _dEdC(atoms, stress, forces, scalar_pressure):
    """(dE/dC (3 x 3, p V included) at fixed Cartesian positions, C) from the stress and the forces."""
    sigma = voigt_to_matrix(stress) if np.size(stress) == 6 else np.asarray(stress, dtype=np.float64).reshape(3, 3)
    sigma = sigma + scalar_pressure * np.eye(3)
    C = np.array(atoms.get_cell(), dtype=np.float64)
    volume = abs(np.linalg.det(C))
    pos = np.asarray(atoms.positions, dtype=np.float64)
    return np.linalg.solve(C.T, volume * sigma + pos.T @ forces), C


def _masked_expm_derivatives(U, cell_mask):
    """(D1 (m, 3, 3), D2 (m, m, 3, 3)): the first and second Frechet derivatives D expm(U)[E_m] and
    D2 expm(U)[E_m, E_q] along the masked unit directions, from one 9 x 9 exponential per ordered pair: in
    expm([[U, E1, 0], [0, U, E2], [0, 0, U]]) the (1,2) block is D expm(U)[E1] and the (1,3) block the E1-before-E2
    half of the second derivative, which is that block plus the one with E1 and E2 swapped."""
    dirs = []
    for r, c in zip(*np.nonzero(cell_mask)):                         # row-major, the order of L[cell_mask]
        E = np.zeros((3, 3))
        E[r, c] = 1.0
        dirs.append(E)
    m = len(dirs)
    D1, half = np.zeros((m, 3, 3)), np.zeros((m, m, 3, 3))
    big = np.zeros((9, 9))
    for k in range(3):
        big[3 * k:3 * k + 3, 3 * k:3 * k + 3] = U
    for i, E1 in enumerate(dirs):
        for j, E2 in enumerate(dirs):
            big[0:3, 3:6], big[3:6, 6:9] = E1, E2
            X = expm(big)
            half[i, j] = X[0:3, 6:9]
            if j == 0:
                D1[i] = X[0:3, 3:6]
    return D1, half + half.transpose(1, 0, 2, 3)


def cell_param_maps(atoms, orig_cell, cell_mask, exp_cell_factor, scalar_pressure, derivatives=_masked_expm_derivatives):
    """(J (9, m), G0 (m, m), P (9, 9) or None) of `CellCartesianPES._cell_param_maps` at the geometry of `atoms`, for the
    log-deformation about `orig_cell` times `exp_cell_factor` at the entries of `cell_mask` (3 x 3 bools), with p V of
    `scalar_pressure`: one stress and force evaluation and m^2 9 x 9 exponentials."""
    stress = np.asarray(atoms.get_stress(), dtype=np.float64)
    forces = np.asarray(atoms.get_forces(), dtype=np.float64).reshape((-1, 3))
    dEdC, C = _dEdC(atoms, stress, forces, scalar_pressure)
    P = None
    if scalar_pressure != 0.0:
        Ci = np.linalg.inv(C)
        # d2 det C / dC_ab dC_cd = det C (C^-1_ba C^-1_dc - C^-1_da C^-1_bc)
        d2 = np.einsum('ba,dc->abcd', Ci, Ci) - np.einsum('da,bc->abcd', Ci, Ci)
        P = scalar_pressure * abs(np.linalg.det(C)) * d2.reshape(9, 9)
    U = logm_3x3(C @ np.linalg.inv(orig_cell))
    D1, D2 = derivatives(U, cell_mask)
    J = (D1 @ orig_cell).reshape(len(D1), 9).T / exp_cell_factor    # (9, m)
    dEdF = dEdC @ orig_cell.T
    G0 = np.einsum('ab,mqab->mq', dEdF, D2) / exp_cell_factor ** 2
    return J, G0, P


class CellCartesianPES(PES):
    """`PES` with the unit cell as extra coordinates (Cartesian positions + masked log-deformation of the cell).

    exp_cell_factor (default N) scales the log-deformation; cell_mask (3 x 3 bools, default all) selects the free
    entries; scalar_pressure (eV / A^3) adds p V to the energy.  The initial Hessian is the user's H0, else 70 I on the
    positions and 1 I on the cell; refine_initial_hessian fills the cell columns by central differences (2 n_cell_dof
    evaluations, step hessian_delta; not run with a hessian_function); save_hessian names an .npy file for it.
    hessian_function(atoms) returns the (3N + 9)-square Hessian in the coordinates [positions; cell.ravel()] (lattice
    vectors in the rows of the cell, positions fixed while the cell varies), as an array or a `DeviceMatrix`, e.g.
    `EMT.get_device_cell_hessian`; `calculate_hessian` carries it into the PES's own coordinates.
    cell_hessian_vector_product (True: the calculator's own, e.g. `EMT.cell_hessian_vector_product`; or a callable
    f(atoms, V (k, 3N + 9)) -> (k, 3N + 9) in the same coordinates) gives the iterative diagonalisation exact products
    instead of finite differences of the gradient: `diag` carries every vector into [x; C.ravel()] and the product back
    (`_cell_hvp`), without a force call.  `hessian_vector_product=` (products of 3N) stays refused, like a 3N x 3N
    `hessian_function`."""
    _accepts_hvp = False
    _hvp_hint = ' (a cell run takes cell_hessian_vector_product=)'

    def __init__(self, atoms, H0=None, constraints=None, eigensolver='jd0', trajectory=None, eta=1e-4, v0=None,
                 proj_trans=None, proj_rot=None, hessian_function=None, exp_cell_factor=None, cell_mask=None,
                 scalar_pressure=0.0, refine_initial_hessian=False, hessian_delta=1e-5, save_hessian=None,
                 hessian_vector_product=None, cell_hessian_vector_product=None):
        self._resolve_hvp(atoms, hessian_vector_product)            # (refused: products of 3N say nothing about the cell)
        cell_hvp = self._resolve_cell_hvp(atoms, cell_hessian_vector_product)
        self.orig_cell = np.array(atoms.get_cell(), dtype=np.float64)
        self.exp_cell_factor = float(len(atoms)) if exp_cell_factor is None else float(exp_cell_factor)
        mask = np.ones((3, 3), dtype=bool) if cell_mask is None else np.asarray(cell_mask, dtype=bool).reshape((3, 3))
        self.cell_mask = mask
        self.n_cell_dof = int(mask.sum())
        self.scalar_pressure = float(scalar_pressure)
        PES.__init__(self, atoms, H0=None, constraints=constraints, eigensolver=eigensolver, trajectory=trajectory,
                     eta=eta, v0=v0, proj_trans=proj_trans, proj_rot=proj_rot, hessian_function=hessian_function)
        nc = self.ncart
        self.dim = nc + self.n_cell_dof
        self._cell_hvp_source, self._cell_maps_cache = cell_hvp, _LRU2()
        self._cell_hvp_from_calc = cell_hessian_vector_product is True
        if cell_hvp is not None:
            self._hvp = self._cell_hvp                           # what `PES.diag` takes its products from
        if H0 is not None:
            H0 = np.asarray(H0, dtype=np.float64)
            if H0.shape == (nc, nc):                             # positions only: the cell block as by default
                full = np.eye(self.dim)
                full[:nc, :nc] = H0
                H0 = full
        else:
            H0 = np.eye(self.dim)
            H0[:nc, :nc] *= 70.0
            # (with a hessian_function the exact Hessian replaces H0 at the first step: no finite differences for it)
            if refine_initial_hessian and hessian_function is None:
                cols = self._cell_hessian_columns(hessian_delta)
                H0[:nc, nc:] = cols[:nc]
                H0[nc:, :nc] = cols[:nc].T
                H0[nc:, nc:] = 0.5 * (cols[nc:] + cols[nc:].T)
        if save_hessian is not None:
            np.save(save_hessian, H0)
        self.set_H(H0, initialized=True)

    def _cell_hessian_columns(self, delta):
        """Hessian columns of the cell coordinates by central differences of the gradient (dim x n_cell_dof)."""
        nc = self.ncart
        cols = np.zeros((self.dim, self.n_cell_dof))
        x0 = self.get_x()
        self.save()
        for k in range(self.n_cell_dof):
            gs = []
            for sign in (1.0, -1.0):
                x = x0.copy()
                x[nc + k] += sign * delta
                self.set_x(x)
                gs.append(self.eval()[1])
                self.restore()
            cols[:, k] = (gs[0] - gs[1]) / (2.0 * delta)
        self.curr = dict.fromkeys(('x', 'f', 'g'))
        self.last = dict(self.curr)
        return cols

    # ---- cell coordinates --------------------------------------------------------------------------------------------
    def _cell(self):
        return np.array(self.atoms.get_cell(), dtype=np.float64)

    def _log_deform(self):
        """L = logm(cell . orig_cell^-1) * exp_cell_factor (3 x 3)."""
        return logm_3x3(self._cell() @ np.linalg.inv(self.orig_cell)) * self.exp_cell_factor

    def _set_cell_params(self, params):
        L = self._log_deform()
        L[self.cell_mask] = params
        self.atoms.set_cell(expm(L / self.exp_cell_factor) @ self.orig_cell, scale_atoms=False)

    def get_x(self):
        return np.concatenate([self.apos.ravel(), self._log_deform()[self.cell_mask]])

    def set_x(self, target):
        """The cell first, then the Cartesian positions (not scaled with the cell)."""
        nc = self.ncart
        x0 = self.get_x()
        self._set_cell_params(target[nc:])
        self.atoms.positions = target[:nc].reshape((-1, 3))
        dx = target - x0
        g = self.curr.get('g')
        return dx, dx.copy(), (np.zeros(self.dim) if g is None else g.copy())

    def save(self):
        PES.save(self)
        self.savepoint['cell'] = self._cell()

    def restore(self):
        kept = self.savepoint.get('cell')
        if kept is not None:
            self.atoms.set_cell(kept, scale_atoms=False)
        PES.restore(self)

    # ---- the calculator boundary -------------------------------------------------------------------------------------
    def eval(self):
        """Energy (+ p V) and gradient [dE/dr, dE/dparams]; the stress is asked for first, so that a calculator that
        computes everything in one go (EMT) is called once."""
        self.neval += 1
        stress = np.asarray(self.atoms.get_stress(), dtype=np.float64)
        f = float(self.atoms.get_potential_energy())
        forces = np.asarray(self.atoms.get_forces(), dtype=np.float64).reshape((-1, 3))
        if self.scalar_pressure != 0.0:
            f += self.scalar_pressure * self.atoms.get_volume()
        g = np.concatenate([-forces.ravel(), self._cell_gradient(stress, forces)])
        self.write_traj()
        return f, g

    def _dEdC(self, stress, forces):
        """(dE/dC (3 x 3, p V included) at fixed Cartesian positions, C) from the stress and the forces."""
        return _dEdC(self.atoms, stress, forces, self.scalar_pressure)

    def _cell_gradient(self, stress, forces):
        dEdC, C = self._dEdC(stress, forces)
        dEdF = dEdC @ self.orig_cell.T                                   # C = F C0
        U = logm_3x3(C @ np.linalg.inv(self.orig_cell))
        g = expm_frechet_3x3_contracted(U, dEdF)
        return g[self.cell_mask] / self.exp_cell_factor

    # ---- exact Hessians: hessian_function in the coordinates [x; C.ravel()] -------------------------------------
    def _expm_derivatives(self, U):
        """`_masked_expm_derivatives` along the directions of this PES's mask."""
        return _masked_expm_derivatives(U, self.cell_mask)

    def _cell_param_maps(self):
        """(J (9, m), G0 (m, m), P (9, 9) or None) of the current geometry, what carries second derivatives from
        [x; C.ravel()] into the PES's coordinates: with U = L / exp_cell_factor, C = expm(U) C0 and the masked unit
        directions E_m, J[:, m] = vec(D expm(U)[E_m] C0) / exp_cell_factor, G0[m, q] = sum_ab dEdC_ab
        (D2 expm(U)[E_m, E_q] C0)_ab / exp_cell_factor^2 (symmetric up to rounding), and P = p d2|det C|/dC2, which p V adds
        to H_CC (its first derivative is part of dEdC).  Computed once per geometry (m^2 9 x 9 exponentials): the dense
        conversion and every product of `_cell_hvp` share them."""
        key = (self._state_hash(), self.orig_cell.tobytes())             # (`load_state` replaces the reference cell)
        hit = self._cell_maps_cache.get(key)
        if hit is not None:
            return hit
        out = cell_param_maps(self.atoms, self.orig_cell, self.cell_mask, self.exp_cell_factor, self.scalar_pressure,
                              derivatives=lambda U, _mask: self._expm_derivatives(U))
        self._cell_maps_cache.put(key, out)
        return out

    def _cell_block_to_params(self, rows):
        """The cell rows of the Hessian in the PES's own coordinates, (m, 3N + m), from the nine cell rows `rows`
        (9, 3N + 9) of the Hessian in [x; C.ravel()], with J, G0 and P of `_cell_param_maps`: H_px = J^T H_Cx and
        H_pp = J^T (H_CC + P) J + G0, symmetrised."""
        nc = self.ncart
        J, G0, P = self._cell_param_maps()
        H_Cx, H_CC = rows[:, :nc], rows[:, nc:].copy()
        if P is not None:
            H_CC += P
        H_pp = J.T @ H_CC @ J + G0
        return np.hstack([J.T @ H_Cx, 0.5 * (H_pp + H_pp.T)])

    # ---- exact products: cell_hessian_vector_product in the coordinates [x; C.ravel()] -----------------------------------
    def _resolve_cell_hvp(self, atoms, hvp):
        """`f(atoms, V (k, 3N + 9)) -> (k, 3N + 9)` from the keyword `cell_hessian_vector_product`: True takes the
        calculator's own, a callable is taken as it is."""
        if hvp is None or hvp is False:
            return None
        if hvp is True:
            from .atoms import supports_cell_hvp
            calc = getattr(atoms, 'calc', None)
            if not supports_cell_hvp(calc):
                raise NotImplementedError(f'cell_hessian_vector_product=True needs a calculator with its own Hessian-vector '
                                          f'product of positions and cell, and {type(calc).__name__} has none')
            return calc.cell_hessian_vector_product
        if not callable(hvp):
            raise TypeError('cell_hessian_vector_product must be True or a callable f(atoms, V (k, 3N + 9)) -> (k, 3N + 9)')
        return hvp

    def _cell_hvp(self, V):
        """H V[q] for the rows [v_x; v_p] of V (k, dim) in the PES's own coordinates: W = J v_p is the variation of the
        cell, [y_x; y_C] the product in [x; C.ravel()] (p V adds P W to y_C), and y_p = J^T y_C + G v_p with
        G = (G0 + G0^T) / 2 — row by row what `_convert_cell_hessian` does to the matrix."""
        nc = self.ncart
        V = np.asarray(V, dtype=np.float64).reshape(-1, self.dim)
        J, G0, P = self._cell_param_maps()
        Vp = V[:, nc:]
        W = Vp @ J.T                                                       # (k, 9)
        Y = np.asarray(self._cell_hvp_source(self.atoms, np.hstack([V[:, :nc], W])), dtype=np.float64)
        if Y.shape != (V.shape[0], nc + 9):
            raise ValueError(f'cell_hessian_vector_product must return {V.shape[0]} x {nc + 9} products of the '
                             f'{len(self.atoms)} atoms and the nine cell entries, got {" x ".join(str(k) for k in Y.shape)}')
        yC = Y[:, nc:]
        if P is not None:
            yC = yC + W @ P.T
        return np.hstack([Y[:, :nc], yC @ J + Vp @ (0.5 * (G0 + G0.T)).T])

    def _library_hvp_operator(self, Ufree):
        """The Hessian of positions and cell as a library object (`sella_hvp_create_cell`, `DeviceHvpOperator.for_cell`)
        when the products are the calculator's own (`cell_hessian_vector_product=True`) and the calculator lives in the
        library as EMT: the state of this geometry, with J, G and P of `_cell_param_maps`, is built once and the products of
        the Davidson run never leave the device.  Needs what `PES._library_fd_operator` needs: nobody listening per
        evaluation, no curved constraints, `use_library_calculator` not False, and a basis that selects coordinates (its
        cell part is always the identity).  Else None: the host operator over `_cell_hvp`."""
        from .atoms import EMT
        calc = getattr(self.atoms, 'calc', None)
        if not self._cell_hvp_from_calc or not isinstance(calc, EMT) or self.traj is not None:
            return None
        maker = calc.device_calculator
        if self._has_curved_constraints() or getattr(self, 'use_library_calculator', True) is False:
            return None
        # constraints that each pin one coordinate make the basis a selection of position coordinates with the identity of
        # the cell behind it (`_split_cons_subspace`); none make it the identity; any other basis mixes coordinates
        free = None
        if PES.get_drdx(self).shape[0] > 0:
            pinned = self._pinned()
            if pinned is None:
                return None
            free = np.setdiff1d(np.arange(self.ncart), pinned[0])
        dc = maker()
        if dc is None:
            return None
        from .device import DeviceHvpOperator
        J, G0, P = self._cell_param_maps()
        return DeviceHvpOperator.for_cell(dc, self.apos.ravel(), self._cell(), J, 0.5 * (G0 + G0.T), P, free=free)

    def _count_products(self, Hproj):
        """`PES._count_products`; the calculator counts every product of the device route as a batch of one (`ncellhvps`),
        as it would through the host."""
        from .device import DeviceHvpOperator
        PES._count_products(self, Hproj)
        if isinstance(Hproj, DeviceHvpOperator):
            self.atoms.calc.ncellhvps += Hproj.calls

    def _convert_cell_hessian(self, H, consume=False):
        """The Hessian in the PES's coordinates [x; p] of what a `hessian_function` returns in a cell run: the
        (3N + 9)-square Hessian in [x; C.ravel()] (lattice vectors in the rows of C, positions fixed while C varies), as
        an array or a `DeviceMatrix`; the result is of the same kind.  The 3N x 3N block is carried over as it is — on the
        device it never leaves it: only the nine cell rows are taken to the host, transformed there and sent back.
        `consume` hands a `DeviceMatrix` over (freed here)."""
        from .device import DeviceMatrix
        nc, m = self.ncart, self.n_cell_dof
        on_device = isinstance(H, DeviceMatrix)
        if not on_device:
            H = np.asarray(H, dtype=np.float64)
        if H.shape != (nc + 9, nc + 9):
            shape = ' x '.join(str(k) for k in H.shape)
            if on_device and consume:
                H.free()
            hint = (f': {nc} x {nc} is the Hessian at fixed cell; a cell run needs the (3N+9)-square one, e.g. '
                    f'`calc.get_device_cell_hessian`') if H.shape == (nc, nc) else ''
            raise ValueError(f'hessian_function must return the {nc + 9} x {nc + 9} Hessian of the {len(self.atoms)} atoms '
                             f'and the nine cell entries in a cell run, got {shape}{hint}')
        if not on_device:
            low = self._cell_block_to_params(H[nc:])
            out = np.empty((nc + m, nc + m))
            out[:nc, :nc] = H[:nc, :nc]
            out[nc:] = low
            out[:nc, nc:] = low[:, :nc].T
            return out
        ctx = H.ctx
        rows = ctx.mat_rows(H, nc, 9)
        try:
            low = self._cell_block_to_params(rows.numpy())
        finally:
            rows.free()
        out = ctx.zeros(nc + m, nc + m)
        hlow = ctx.upload(low)
        hcol = hlow.transpose()
        try:
            ctx.mat_copy_block(H, 0, 0, nc, nc, out, 0, 0)
            ctx.mat_copy_block(hlow, 0, 0, m, nc + m, out, nc, 0)
            ctx.mat_copy_block(hcol, 0, 0, nc, m, out, 0, nc)
        finally:
            hlow.free()
            hcol.free()
            if consume:
                H.free()
        return out

    def calculate_hessian(self):
        assert self.hessian_function is not None
        # what the hessian_function returns is the PES's from here on, as in `PES.calculate_hessian`
        self.H.set_B(self._convert_cell_hessian(self.hessian_function(self.atoms), consume=True))

    # ---- constraints: they act on the positions only ------------------------------------------------------------
    def get_drdx(self):
        drdx = PES.get_drdx(self)
        out = np.zeros((drdx.shape[0], self.dim))
        out[:, :self.ncart] = drdx
        return out

    def get_Hc(self):
        Hc = PES.get_Hc(self)
        out = np.zeros((self.dim, self.dim))
        out[:self.ncart, :self.ncart] = Hc
        return out

    def _calc_basis(self):
        key = self._state_hash()
        cached = self._basis_cache.get(key)
        if cached is not None:
            return cached
        nc, ncell = self.ncart, self.n_cell_dof
        Ucons_c, Ufree_c = _split_cons_subspace(PES.get_drdx(self))
        Ucons = np.zeros((self.dim, Ucons_c.shape[1]))
        Ucons[:nc] = Ucons_c
        Ufree = np.zeros((self.dim, Ufree_c.shape[1] + ncell))
        Ufree[:nc, :Ufree_c.shape[1]] = Ufree_c
        Ufree[nc:, Ufree_c.shape[1]:] = np.eye(ncell)
        result = (self.get_drdx(), Ucons, shared_identity(self.dim), Ufree)
        self._basis_cache.put(key, result)
        return result

    def get_projected_forces(self):
        g = self.get_g()[:self.ncart]
        Uc = self.get_Ufree()[:self.ncart]
        return -(Uc @ (Uc.T @ g)).reshape((-1, 3))

    def converged(self, fmax, smax=None, cmax=1e-5):
        """(done, largest projected force on an atom, norm of the constraint residual, largest |cell gradient|) —
        the reference's order; smax defaults to fmax."""
        smax = fmax if smax is None else smax
        per_atom = self.get_projected_forces()
        worst_force = float(np.sqrt(np.einsum('ij,ij->i', per_atom, per_atom).max()))
        g_cell = self.get_g()[self.ncart:]
        worst_cell = float(np.abs(g_cell).max()) if g_cell.size else 0.0
        violation = float(np.linalg.norm(self.get_res()))
        return (bool(worst_force < fmax and worst_cell < smax and violation < cmax), worst_force, violation,
                worst_cell)
