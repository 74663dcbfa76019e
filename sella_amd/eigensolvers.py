"""Davidson / Rayleigh-Ritz partial diagonalisation — drop-in for sella/eigensolvers.py
(`exact` :9-28, `rayleigh_ritz` :31-112; the correction methods of `expand` :115-153 are
selected by the same `method` strings).  The whole loop runs inside libsella_hip
(sella_amd/csrc/davidson.hip); only the operator A may call back into Python, because the
finite-difference Hessian lives behind the calculator boundary.
"""
import numpy as np

from .device import DeviceFdOperator, DeviceHvpOperator, DeviceMatrix, get_context
from .linalg import ApproximateHessian


def _is_identity(P):
    n = P.shape[0]
    if P.shape != (n, n) or P[0, 0] != 1.0:
        return False
    return np.count_nonzero(P) == n and bool(np.all(P.diagonal() == 1.0))


def _dense_from_operator(A, probes):
    """B = sum_i p_i (A p_i)^T over the ROWS p_i of `probes`, symmetrised (eigensolvers.py:22-26)."""
    n = A.shape[0]
    B = np.zeros((n, n))
    for i in range(n):
        p = probes[i]
        B += np.outer(p, np.asarray(A.dot(p)).ravel())
    return 0.5 * (B + B.T)


def exact(A, gamma=None, P=None):
    """Full diagonalisation on the device; returns (lams, vecs, lams * vecs)."""
    ctx = get_context()
    if isinstance(A, DeviceMatrix):
        dA, own = A, False
    elif isinstance(A, np.ndarray):
        dA, own = ctx.upload(A), True
    else:
        probes = np.eye(A.shape[0]) if P is None else exact(P)[1]
        dA, own = ctx.upload(_dense_from_operator(A, probes)), True
    lams, V, Vt = ctx.eigh(dA)
    vecs = V.numpy()
    V.free()
    Vt.free()
    if own:
        dA.free()
    return lams, vecs, lams[np.newaxis, :] * vecs


def _preconditioner(P):
    """-> dict(Pvecs, PvecsT, pevals, pscale), owned handles to free afterwards."""
    ctx = get_context()
    if P is None:
        return dict(pscale=1.0), []
    if isinstance(P, ApproximateHessian):
        if P._is_none:
            return dict(pscale=1.0), []
        lr = P.device_eig_lr()
        if lr is not None:
            # structured P = lam0 (I - W^T W) + W^T diag(mu) W: r explicit pairs, lam0 on the complement
            if lr['r'] == 0:
                return dict(pscale=float(lr['lam0'])), []
            Wt = ctx.mat_rows(lr['Wt'], 0, lr['r'])
            W = Wt.transpose()
            return dict(Pvecs=W, PvecsT=Wt, pevals=lr['mu'][:lr['r']].copy(), pscale=float(lr['lam0'])), [W, Wt]
        w, V, Vt = P.device_eig()
        return dict(Pvecs=V, PvecsT=Vt, pevals=w), []
    P = np.asarray(P, dtype=np.float64)
    if _is_identity(P):
        return dict(pscale=1.0), []
    dP = ctx.upload(P)
    w, V, Vt = ctx.eigh(dP)
    dP.free()
    return dict(Pvecs=V, PvecsT=Vt, pevals=w), [V, Vt]


def rayleigh_ritz(A, gamma, P, B=None, v0=None, vref=None, vreftol=0.99,
                  method='jd0', maxiter=None):
    """Same contract as the reference: returns (lams, V, AV) with the columns of V rotated
    into the Ritz basis.  `A` may be a numpy array, a DeviceMatrix or any object with
    `.shape` and `.dot(v)` (e.g. NumericalHessian); `P` a numpy array or an
    ApproximateHessian (whose cached device eigendecomposition is then reused)."""
    n, _ = A.shape
    if B is not None and not _is_identity(np.asarray(B)):
        return _rayleigh_ritz_metric(A, gamma, P, np.asarray(B, dtype=np.float64), v0, vref, vreftol, method, maxiter)
    if maxiter is None:
        maxiter = 2 * n + 1
    if gamma <= 0:
        return exact(A, gamma, P)

    ctx = get_context()
    pre, owned = _preconditioner(P)
    try:
        if v0 is not None:
            start = np.asarray(v0, dtype=np.float64).reshape((n, -1))
        else:
            # leading eigenvectors of P span the start block (eigensolvers.py:46-50)
            if 'Pvecs' in pre:
                P_lams = pre['pevals']
                nneg = max(1, int(np.sum(P_lams < 0)))
                start = pre['PvecsT'].numpy()[:nneg].T
            else:
                start = np.eye(n)[:, :1]
        own_A = False
        if isinstance(A, np.ndarray):
            op, own_A = ctx.upload(A), True
        elif isinstance(A, (DeviceMatrix, DeviceFdOperator, DeviceHvpOperator)):
            op = A
        else:
            def op(v, _A=A):
                return np.asarray(_A.dot(v)).ravel()
        lams, V, AV, _ = ctx.davidson(op, n, np.ascontiguousarray(start), gamma, method=method,
                                      maxiter=maxiter, vref=vref, vreftol=vreftol, **pre)
        if own_A:
            op.free()
    finally:
        for h in owned:
            h.free()
    return lams, V, AV


class _Congruent:
    """x -> S (A (S x)) for an operator A that only offers `.dot` (S symmetric, resident)."""

    def __init__(self, A, S):
        self.A, self.S, self.shape = A, S, A.shape

    def dot(self, v):
        ctx = get_context()
        inner = ctx.symm_mm(self.S, np.asarray(v, dtype=np.float64).ravel())
        return ctx.symm_mm(self.S, np.asarray(self.A.dot(inner), dtype=np.float64).ravel())


def _rayleigh_ritz_metric(A, gamma, P, B, v0, vref, vreftol, method, maxiter):
    """Generalised problem A x = theta B x (sella/eigensolvers.py:35-36, 58, 70; no caller of the reference passes a metric).
    Reduced to the standard one by the congruence with S = B^-1/2 from the device eigendecomposition of B:
    (S A S) y = theta y, x = S y, and the standard device path runs on (S A S, S P S).  Returned as the reference returns
    them: Ritz values, V with V^T B V = I, AV = A V.
    Deviation: the reference keeps a Euclidean-orthonormal basis and solves a generalised Rayleigh-Ritz problem in it, so its
    search space after k steps is not this one and its convergence test |A x - theta B x| is |S^-1 (residual here)|;
    converged pairs agree, trajectories do not."""
    ctx = get_context()
    n = B.shape[0]
    dB = ctx.upload(0.5 * (B + B.T))
    wB, VB, VBt = ctx.eigh(dB)
    dB.free()
    if not wB[0] > 0.0:
        VB.free()
        VBt.free()
        raise ValueError('rayleigh_ritz: the metric B must be positive definite')
    Q = VB.numpy()
    VB.free()
    VBt.free()
    # S = B^-1/2 resident, B^1/2 applied on the host to single vectors / narrow panels only (O(n^2 k))
    dQs, dQt, S = ctx.upload(Q * wB ** -0.5), ctx.upload(np.ascontiguousarray(Q.T)), ctx.zeros(n, n)
    ctx.gemm(dQs, dQt, S)
    dQs.free()
    dQt.free()

    def sqrtB(X):
        return Q @ ((wB ** 0.5)[:, None] * (Q.T @ X.reshape((n, -1))))

    owned = [S]
    try:
        def congruent(M):
            dM = M if isinstance(M, DeviceMatrix) else ctx.upload(np.asarray(M, dtype=np.float64))
            tmp, out = ctx.zeros(n, n), ctx.zeros(n, n)
            ctx.gemm(S, dM, tmp)
            ctx.gemm(tmp, S, out)
            tmp.free()
            if dM is not M:
                dM.free()
            return out
        if isinstance(A, (np.ndarray, DeviceMatrix)):
            At = congruent(A)
            owned.append(At)
        else:
            At = _Congruent(A, S)
        Pt = None
        if P is not None:
            Pn = P.B if isinstance(P, ApproximateHessian) else np.asarray(P, dtype=np.float64)
            if Pn is not None:
                dPt = congruent(Pn)
                Pt = dPt.numpy()
                Pt = 0.5 * (Pt + Pt.T)
                dPt.free()
        v0t = None if v0 is None else sqrtB(np.asarray(v0, dtype=np.float64)).ravel()
        vreft = None if vref is None else ctx.symm_mm(S, np.asarray(vref, dtype=np.float64).ravel())
        lams, Vt_, AVt = rayleigh_ritz(At, gamma, Pt, None, v0t, vreft, vreftol, method, maxiter)
        V = ctx.symm_mm(S, np.ascontiguousarray(Vt_))
        return lams, V, sqrtB(np.ascontiguousarray(AVt))
    finally:
        for h in owned:
            h.free()


def block_davidson(A, nev, P=None, tol=1e-8, block=16, maxiter=500, maxvec=0, v0=None):
    """Lowest `nev` eigenpairs of a dense symmetric A by block Davidson (`sella_davidson_block`: `block` <= 16 new
    vectors per iteration, A streamed once per block on the matrix cores — BASELINE configs[4]).  The reference has
    no block method (one vector per iteration, eigensolvers.py:111-112); the result matches `exact(A)` truncated.
    P: approximate operator whose eigenbasis preconditions the corrections ('gd', eigensolvers.py:119-121),
    an ApproximateHessian, or None (diagonal of A).  Returns (lams (nev,), V (n, nev), residual norms (nev,))."""
    ctx = get_context()
    own = []
    if isinstance(A, DeviceMatrix):
        dA, diag = A, None
    else:
        A = np.asarray(A, dtype=np.float64)
        dA, diag = ctx.upload(A), np.ascontiguousarray(A.diagonal())
        own.append(dA)
    n = dA.shape[0]
    kw = {}
    if P is not None:
        pk, owned = _preconditioner(P)
        own += owned
        if 'Pvecs' in pk:
            kw = dict(Pvecs=pk['Pvecs'], PvecsT=pk['PvecsT'], pevals=pk['pevals'])
    if not kw and diag is not None:
        kw = dict(diag=diag)
    out = ctx.davidson_block(dA, n, nev, block=block, tol=tol, maxiter=maxiter, maxvec=maxvec, V0=v0, **kw)
    for m in own:
        m.free()
    if out['nconv'] < nev:
        raise RuntimeError(f'block_davidson: {out["nconv"]} of {nev} pairs converged in {out["niter"]} iterations')
    return out['lams'], out['V'], out['res']


def _free_coordinates(atoms, constraints, free):
    """Ascending free Cartesian coordinates (int32) of `lowest_modes`, or None when nothing is pinned."""
    n = 3 * len(atoms)
    if free is not None and constraints is not None:
        raise ValueError('lowest_modes: give the free coordinates as `free` or as `constraints`, not both')
    if free is not None:
        free = np.asarray(free)
        if free.ndim != 1 or free.size == 0 or not np.issubdtype(free.dtype, np.integer):
            raise ValueError('lowest_modes: `free` must be a non-empty list of coordinate indices')
        if free[0] < 0 or free[-1] >= n or np.any(np.diff(free) <= 0):
            raise ValueError(f'lowest_modes: `free` must be ascending indices below {n}')
        return free.astype(np.int32)
    if constraints is None:
        return None
    from .peswrapper import _pinned_coordinates
    from .search import _only_translations
    c = constraints
    if not _only_translations(c):
        raise NotImplementedError('lowest_modes: only constraints that pin Cartesian coordinates (fix_translation on single '
                                  'atoms) select coordinates; curved or inequality constraints are not covered')
    drdx = c.jacobian()
    if drdx.shape[0] == 0:
        return None
    pinned = _pinned_coordinates(drdx)
    if pinned is None:
        raise NotImplementedError('lowest_modes: the constraints are not a selection of Cartesian coordinates')
    return np.setdiff1d(np.arange(n), pinned[0]).astype(np.int32)


def lowest_modes(atoms, nev=1, constraints=None, free=None, tol=1e-8, block=None, maxiter=500, maxvec=0, V0=None,
                 allow_unconverged=False, cell=False, cell_mask=None, exp_cell_factor=None, scalar_pressure=0.0):
    """The `nev` lowest curvatures and modes of the Hessian of `atoms` over its free coordinates, without the 3N x 3N
    matrix: block Davidson (`sella_davidson_block_hvp`) on the analytic Hessian-vector operator of a calculator that lives
    in the library (device `EMT`, `QuadraticCubicModel` with a device matrix), preconditioned with the operator's diagonal.

    The free coordinates are `free` (ascending indices into the 3N Cartesian coordinates) or what a `Constraints` object
    that pins coordinates (`fix_translation`) leaves; default: all.  V0: (m, k <= 16) start block over the free coordinates.
    Returns dict(lams (nev,), modes (nev, N, 3), res, niter, nmatvec, nconv); `modes` are orthonormal and zero on the
    pinned coordinates.

    A pair counts as converged when |r| <= tol |theta|: the rule is RELATIVE, so an exact zero mode never converges.  A
    system that has them — nothing pinned in a periodic cell (three translations), a free cluster (six) — should have
    atoms pinned, which removes them; otherwise `nconv < nev` raises RuntimeError unless `allow_unconverged=True`.

    cell=True: the lowest curvatures over [free positions; cell], the cell in the coordinates of `CellCartesianPES`: the
    log-deformation about the current cell, times `exp_cell_factor` (default N), at the entries `cell_mask` (3 x 3 bools,
    default all) selects, with p V of `scalar_pressure` in the energy (device `EMT` in a fully periodic cell; block Davidson
    on `DeviceHvpOperator.for_cell`, preconditioned with its diagonal).  V0 then has the mask's entries behind the free
    coordinates, and the result one more key, `cell_modes` (nev, 3, 3): the cell part of every mode at the mask's
    positions, zero elsewhere; `modes` and `cell_modes` TOGETHER are orthonormal.  Zero modes there: the three translations
    unless an atom is pinned, and, with the full mask at a minimum (no stress), the three rotations of cell and atoms
    together — use a triangular mask there, which leaves the cell no rotation."""
    if cell:
        return _lowest_cell_modes(atoms, nev, constraints, free, tol, block, maxiter, maxvec, V0, allow_unconverged, cell_mask,
                                  exp_cell_factor, scalar_pressure)
    from .atoms import supports_hessian
    calc = getattr(atoms, 'calc', None)
    if not (supports_hessian(calc) and getattr(calc, 'library_form', False)):
        raise NotImplementedError(f'lowest_modes: {type(calc).__name__} has no analytic Hessian-vector operator in the library '
                                  '(device EMT and QuadraticCubicModel with a device matrix have)')
    n = 3 * len(atoms)
    sel = _free_coordinates(atoms, constraints, free)
    m = n if sel is None else len(sel)
    nev = int(nev)
    if nev < 1 or nev > m:
        raise ValueError(f'lowest_modes: nev = {nev} with {m} free coordinates')
    if block is None:
        block = min(16, max(nev, 4))
    atoms.get_potential_energy()                                       # the evaluation the library calculator is made at
    dc = calc.device_calculator()
    op = DeviceHvpOperator(dc, np.asarray(atoms.positions, dtype=np.float64).ravel(), sel)
    out = dc.ctx.davidson_block(op, None, nev, block=min(int(block), m), tol=tol, maxiter=maxiter, maxvec=maxvec, V0=V0,
                                diag=op.diagonal())
    if out['nconv'] < nev and not allow_unconverged:
        raise RuntimeError(f'lowest_modes: nconv = {out["nconv"]} of {nev} pairs converged in {out["niter"]} iterations '
                           '(the stopping rule is relative: zero modes do not converge; pin atoms)')
    modes = np.zeros((nev, n))
    modes[:, np.arange(n) if sel is None else sel] = out['V'].T
    return dict(lams=out['lams'], modes=modes.reshape(nev, len(atoms), 3), res=out['res'], niter=out['niter'],
                nmatvec=out['nmatvec'], nconv=out['nconv'])


def _lowest_cell_modes(atoms, nev, constraints, free, tol, block, maxiter, maxvec, V0, allow_unconverged, cell_mask,
                       exp_cell_factor, scalar_pressure):
    """`lowest_modes(cell=True)`."""
    from .atoms import EMT
    from .peswrapper import cell_param_maps
    calc = getattr(atoms, 'calc', None)
    if not (isinstance(calc, EMT) and calc.has_cell_hvp and getattr(calc, 'library_form', False)):
        raise NotImplementedError(f'lowest_modes: {type(calc).__name__} has no Hessian-vector operator of positions and cell in '
                                  'the library (device EMT has)')
    if not np.all(atoms.pbc):
        raise NotImplementedError('lowest_modes: cell=True needs a cell that is periodic in all three directions')
    mask = np.ones((3, 3), dtype=bool) if cell_mask is None else np.asarray(cell_mask, dtype=bool).reshape((3, 3))
    mc = int(mask.sum())
    if mc == 0:
        raise ValueError('lowest_modes: cell=True with an empty cell_mask')
    n = 3 * len(atoms)
    sel = _free_coordinates(atoms, constraints, free)
    mx = n if sel is None else len(sel)
    m = mx + mc
    nev = int(nev)
    if nev < 1 or nev > m:
        raise ValueError(f'lowest_modes: nev = {nev} with {mx} free coordinates and {mc} of the cell')
    if block is None:
        block = min(16, max(nev, 4))
    atoms.get_potential_energy()                                       # the evaluation the library calculator is made at
    cell0 = np.array(atoms.get_cell(), dtype=np.float64)             # the log-deformation is taken about the current cell
    factor = float(len(atoms)) if exp_cell_factor is None else float(exp_cell_factor)
    J, G0, P = cell_param_maps(atoms, cell0, mask, factor, float(scalar_pressure))
    dc = calc.device_calculator()
    op = DeviceHvpOperator.for_cell(dc, np.asarray(atoms.positions, dtype=np.float64).ravel(),
                                    cell0, J, 0.5 * (G0 + G0.T), P, free=sel)
    out = dc.ctx.davidson_block(op, None, nev, block=min(int(block), m), tol=tol, maxiter=maxiter, maxvec=maxvec, V0=V0,
                                diag=op.diagonal())
    if out['nconv'] < nev and not allow_unconverged:
        raise RuntimeError(f'lowest_modes: nconv = {out["nconv"]} of {nev} pairs converged in {out["niter"]} iterations '
                           '(the stopping rule is relative: zero modes do not converge; pin an atom, and at a minimum take a '
                           'triangular cell_mask)')
    V = out['V']
    modes = np.zeros((nev, n))
    modes[:, np.arange(n) if sel is None else sel] = V[:mx].T
    cell_modes = np.zeros((nev, 3, 3))
    cell_modes[:, mask] = V[mx:].T
    return dict(lams=out['lams'], modes=modes.reshape(nev, len(atoms), 3), cell_modes=cell_modes, res=out['res'],
                niter=out['niter'], nmatvec=out['nmatvec'], nconv=out['nconv'])
