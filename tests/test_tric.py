"""TRIC fragment coordinates: the rotation kernel (csrc/tric.hip) against closed forms, finite differences and a NumPy
restatement; the fragment topology of `InternalCoordinates.from_atoms(..., allow_fragments=True)`; and whole searches
with `Sella(internal=True, allow_fragments=True)` (sella/internal.py:1030-1078, :3085-3144, :3366-3455)."""
import numpy as np
import pytest

from sella_amd.atoms import Atoms, MorseCluster

WATER = np.array([[0.0, 0.0, 0.1193], [0.0, 0.7632, -0.4770], [0.0, -0.7632, -0.4770]])   # test_molecules.py
MORSE = dict(D=1.2, a=1.6, r0=1.05)


def rotmat(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


# ---- NumPy restatement of the formulas (numpy.linalg.eigh) -----------------------------------------------------------
def _F(R):
    tr = np.trace(R)
    y = np.array([R[1, 2] - R[2, 1], R[2, 0] - R[0, 2], R[0, 1] - R[1, 0]])
    F = np.empty((4, 4))
    F[0, 0], F[0, 1:], F[1:, 0] = tr, y, y
    F[1:, 1:] = R + R.T - tr * np.eye(3)
    return F


def _asinc(x):
    if x < 0.97:
        om = 1 - x * x
        s = np.arccos(x) / np.sqrt(om)
        s1 = (x * s - 1) / om
        return s, s1, (s + 3 * x * s1) / om
    a = np.array([1, -1 / 3, 2 / 15, -2 / 35, 8 / 315, -8 / 693, 16 / 3003, -16 / 6435, 128 / 109395, -128 / 230945])
    y, n = x - 1.0, np.arange(10)
    return (a @ y ** n, (n[1:] * a[1:]) @ y ** (n[1:] - 1), (n[2:] * (n[2:] - 1) * a[2:]) @ y ** (n[2:] - 2))


def np_rotation(pos, ref, q_prev, tangent=None):
    """(values (3,), gradient (3, 3m), H t (3, 3m), Hessian (3, 3m, 3m), new quaternion) of one fragment."""
    m = len(pos)
    dx = pos - pos.mean(0)
    F = _F(dx.T @ ref)
    w, V = np.linalg.eigh(F)
    lam = w[-1]
    top = V[:, lam - w < 1e-10]
    q = top @ (top.T @ q_prev)
    q = V[:, -1].copy() if np.linalg.norm(q) < 1e-14 else q / np.linalg.norm(q)
    c = -q if q[0] < 0 else q
    gap = w - lam
    ig = np.where(np.abs(gap) > 1e-14, 1.0 / np.where(np.abs(gap) > 1e-14, gap, 1.0), 0.0)
    P = (V * ig) @ V.T
    Fa = np.zeros((3 * m, 4, 4))
    for a in range(3 * m):
        R = np.zeros((3, 3))
        R[a % 3] = ref[a // 3]
        Fa[a] = _F(R)
    Fac = Fa @ c                                        # (3m, 4)
    ca = -(Fac @ P)
    lama = Fac @ c
    s, s1, s2 = _asinc(c[0])
    val = 2 * c[1:] * s
    grad = 2 * (ca[:, 1:].T * s + np.outer(c[1:], ca[:, 0]) * s1)
    u = (np.einsum('aij,bj->abi', Fa, ca) - lama[:, None, None] * ca[None, :, :])
    u = u + u.transpose(1, 0, 2)
    cab = -(u @ P) - c[None, None, :] * (ca @ ca.T)[:, :, None]
    H = 2 * (cab[:, :, 1:].transpose(2, 0, 1) * s
             + s1 * (ca[:, 1:].T[:, :, None] * ca[None, :, 0] + ca[:, 1:].T[:, None, :] * ca[:, 0][None, :, None])
             + c[1:, None, None] * (s2 * np.outer(ca[:, 0], ca[:, 0]) + s1 * cab[:, :, 0]))
    hv = None if tangent is None else H @ tangent.ravel()
    return val, grad, hv, H, c


def tric(ctx, frags, pos, refs, q, tangent=None, hessian=False):
    fp = np.concatenate([[0], np.cumsum([len(f) for f in frags])])
    return ctx.tric_eval(fp, np.concatenate(frags), pos, np.concatenate(refs), q, tangent=tangent, hessian=hessian)


def one(ctx, pos, ref, q=None, **kw):
    m = len(pos)
    q = np.array([[1.0, 0, 0, 0]]) if q is None else q
    val, g, hv, H = tric(ctx, [np.arange(m)], pos, [ref], q, **kw)
    return (val[0], g.reshape(3, 3 * m), None if hv is None else hv.reshape(3, 3 * m),
            None if H is None else H.reshape(3, 3 * m, 3 * m), q[0])


def fragment(m, seed):
    ref = np.random.RandomState(seed).normal(size=(m, 3)) * 1.2
    return ref - ref.mean(0)


# ---- 1. closed form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mag', [1e-9, 0.3, 3.0])
def test_rigid_motion_gives_rotation_vector(ctx, mag):
    """A rigid rotation R(w) plus a shift: the three rotation values are the rotation vector that takes the current
    geometry back onto the reference (-w, the reference's convention), the translations the centroid shift."""
    from sella_amd.internal import InternalCoordinates
    rng = np.random.RandomState(int(mag * 1e3) + 11)
    ref = fragment(5, 3) + np.array([0.3, -1.0, 2.0])
    for _ in range(4):
        axis = rng.normal(size=3)
        w = mag * axis / np.linalg.norm(axis)
        shift = rng.normal(size=3)
        at = Atoms(['C'] * 5, ref.copy())
        ic = InternalCoordinates(at)
        ic.add_translation(np.arange(5))
        ic.add_rotation(np.arange(5))
        cen = ref.mean(0)
        at.positions = (ref - cen) @ rotmat(w).T + cen + shift
        q = ic.calc()
        assert ic.ntrans == 3 and ic.nrotations == 3 and len(q) == 6
        assert np.abs(q[:3] - (cen + shift)).max() < 1e-12
        assert np.abs(q[3:] + w).max() < 1e-12, (q[3:], w)


# ---- 2. branch continuity -------------------------------------------------------------------------------------------
def test_branch_continuity_and_diatomic(ctx):
    from sella_amd.internal import InternalCoordinates
    ref = fragment(4, 5)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    at = Atoms(['C'] * 4, ref.copy())
    ic = InternalCoordinates(at)
    ic.add_rotation(np.arange(4))
    proj = []
    for th in np.linspace(0.0, 3.0, 31):
        at.positions = ref @ rotmat(th * axis).T
        proj.append(-ic.calc() @ axis)
    proj = np.array(proj)
    assert np.all(np.diff(proj) > 0.09) and np.all(np.diff(proj) < 0.11)
    assert abs(proj[-1] - 3.0) < 1e-10
    # diatomic: a degenerate top eigenspace; finite everywhere, no NaN in any output
    d = np.array([[0.0, 0.0, -0.55], [0.0, 0.0, 0.55]])
    q = np.array([[1.0, 0, 0, 0]])
    rng = np.random.RandomState(0)
    for th in np.linspace(0.0, 3.0, 31):
        pos = d @ rotmat(th * np.array([1.0, 0.0, 0.0])).T + 0.01 * rng.normal(size=(2, 3))
        val, g, hv, H = tric(ctx, [np.arange(2)], pos, [d], q, tangent=rng.normal(size=(2, 3)), hessian=True)
        for arr in (val, g, hv, H, q):
            assert np.all(np.isfinite(arr))
        assert abs(np.linalg.norm(q) - 1.0) < 1e-12 and q[0, 0] >= 0


# ---- 3. derivatives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [3, 5, 40])
def test_derivatives_against_finite_differences(ctx, m):
    rng = np.random.RandomState(m)
    ref = fragment(m, m + 1)
    pos = ref @ rotmat(rng.normal(size=3) * 0.7).T + 0.15 * rng.normal(size=(m, 3)) + 2.0
    t = rng.normal(size=(m, 3))
    val, g, hv, H, c = one(ctx, pos, ref, tangent=t, hessian=True)
    h = 1e-5
    gfd, Hfd = np.zeros_like(g), np.zeros_like(H)
    for a in range(3 * m):
        e = np.zeros(3 * m)
        e[a] = h
        vp, gp, *_ = one(ctx, pos + e.reshape(m, 3), ref, q=c[None].copy())
        vm, gm, *_ = one(ctx, pos - e.reshape(m, 3), ref, q=c[None].copy())
        gfd[:, a] = (vp - vm) / (2 * h)
        Hfd[:, :, a] = (gp - gm) / (2 * h)
    scale = max(1.0, np.abs(H).max())
    assert np.abs(g - gfd).max() < 1e-8 * max(1.0, np.abs(g).max())
    assert np.abs(H - Hfd).max() < 1e-7 * scale
    assert np.abs(H - H.transpose(0, 2, 1)).max() <= 1e-14 * scale
    assert np.abs(hv - H @ t.ravel()).max() < 1e-12 * scale
    hvfd = np.einsum('kab,b->ka', Hfd, t.ravel())
    assert np.abs(hv - hvfd).max() < 1e-6 * scale * np.abs(t).sum()


# ---- 4. batch layout --------------------------------------------------------------------------------------------------
def test_batch_against_numpy_restatement(ctx):
    rng = np.random.RandomState(7)
    sizes = [3] * 64 + [40]
    frags, refs, pos = [], [], []
    start = 0
    for k, m in enumerate(sizes):
        ref = fragment(m, 100 + k)
        frags.append(np.arange(start, start + m))
        refs.append(ref)
        pos.append(ref @ rotmat(rng.normal(size=3)).T + 0.1 * rng.normal(size=(m, 3)) + 3.0 * rng.normal(size=3))
        start += m
    pos = np.concatenate(pos)
    t = rng.normal(size=pos.shape)
    q = np.tile([1.0, 0, 0, 0], (len(sizes), 1))
    q0 = q.copy()
    val, g, hv, H = tric(ctx, frags, pos, refs, q, tangent=t, hessian=True)
    go = ho = 0
    for f, (ix, ref) in enumerate(zip(frags, refs)):
        m = len(ix)
        v_, g_, hv_, H_, c_ = np_rotation(pos[ix], ref, q0[f], t[ix])
        gs = g[go:go + 9 * m].reshape(3, 3 * m)
        hs = hv[go:go + 9 * m].reshape(3, 3 * m)
        Hs = H[ho:ho + 27 * m * m].reshape(3, 3 * m, 3 * m)
        go, ho = go + 9 * m, ho + 27 * m * m
        assert np.abs(val[f] - v_).max() <= 1e-12 * max(1.0, np.abs(v_).max())
        assert np.abs(q[f] - c_).max() <= 1e-12
        assert np.abs(gs - g_).max() <= 1e-12 * max(1.0, np.abs(g_).max())
        assert np.abs(hs - hv_).max() <= 1e-10 * max(1.0, np.abs(hv_).max())
        assert np.abs(Hs - H_).max() <= 1e-10 * max(1.0, np.abs(H_).max())
    assert go == len(g) and ho == len(H)


def test_invalid_fragment_indices_are_refused(ctx):
    from sella_amd._lib import SellaHipError
    q = np.array([[1.0, 0, 0, 0]])
    with pytest.raises(SellaHipError):
        ctx.tric_eval([0, 2], [0, 5], np.zeros((3, 3)), np.zeros((2, 3)), q)


# ---- 5. topology ------------------------------------------------------------------------------------------------------
def water_cluster(seed=1):
    rng = np.random.RandomState(seed)
    pos, sym = [], []
    for c in [(0, 0, 0), (3, 0, 0), (0, 3, 0), (3, 3, 0)]:
        pos += list(WATER @ rotmat(rng.normal(size=3)).T + np.array(c, float))
        sym += ['O', 'H', 'H']
    pos.append([1.5, 1.5, 2.6])
    sym.append('Ar')
    at = Atoms(sym, np.array(pos), pbc=False)
    at.calc = MorseCluster(**MORSE)
    return at


def test_fragment_topology(ctx):
    from sella_amd.internal import InternalCoordinates, _fragments
    at = water_cluster()
    ic = InternalCoordinates.from_atoms(at, allow_fragments=True)
    b = ic.idx['bonds']
    lab = _fragments(len(at), b)
    assert np.all(lab[b[:, 0]] == lab[b[:, 1]])                         # no bond between fragments
    assert len(np.unique(lab)) == 5
    assert ic.ntrans == 15 and ic.nrotations == 12 and ic.nbonds == 8 and ic.nangles == 4
    assert ic.nint == 15 + 8 + 4 + 12 == len(ic.calc())
    assert ic.trans[0][0].tolist() == [12]                              # the lone atom's translations first
    J = ic.jacobian()
    assert np.linalg.matrix_rank(J) == 3 * len(at)
    assert np.abs(ic.jacobian_csr().toarray() - J).max() == 0.0
    assert np.abs(ic.sparse_jacobian().asarray() - J).max() == 0.0
    Hd = ic.hessian().asarray()
    assert np.abs(np.asarray(ic.sparse_hessians().asarray()) - Hd).max() == 0.0
    v = np.random.RandomState(0).normal(size=3 * len(at))
    assert np.abs(ic.hessian_rdot(v) - Hd @ v).max() < 1e-13
    W = np.random.RandomState(1).normal(size=(3 * len(at), 2))
    assert np.abs(ic.hessian_rdot_mult(v, W) - (Hd @ v) @ W).max() < 1e-12
    h0 = ic.guess_hessian(diagonal_only=True)
    assert len(h0) == ic.nint and np.allclose(h0[:15], 0.05 * 27.211386245988) and np.allclose(h0[-12:], h0[0])
    # dihedral wrap by offset: only the dihedral block wraps
    vec = np.full(ic.nint, 7.0)
    assert np.array_equal(ic.wrap(vec), vec)
    # copy round-trips, quaternion state and reference positions included
    at.positions = at.positions + 0.05 * np.random.RandomState(2).normal(size=at.positions.shape)
    q1 = ic.calc()
    cp = ic.copy()
    assert np.array_equal(cp.frag_q, ic.frag_q) and cp.frag_q is not ic.frag_q
    assert all(np.array_equal(a, b) for a, b in zip(cp.frag_ref, ic.frag_ref))
    assert cp.trans is not ic.trans and [(t.tolist(), d) for t, d in cp.trans] == [(t.tolist(), d) for t, d in ic.trans]
    assert np.array_equal(cp.calc(), ic.calc()) and np.array_equal(cp.jacobian(), ic.jacobian())
    assert np.abs(cp.calc() - q1).max() < 1e-14


def test_without_flag_topology_is_unchanged(ctx):
    """The same structure without the flag: bonds grown until connected, no fragment coordinates — the arrays a build
    without fragment support gives (pinned here by recomputing them with the search's own rule)."""
    from sella_amd.internal import InternalCoordinates
    at = water_cluster()
    ic = InternalCoordinates.from_atoms(at)
    assert ic.ntrans == 0 and ic.nrotations == 0 and ic.trans == [] and ic.rot == []
    assert ic.nint == ic.nbonds + ic.nangles + ic.ndihedrals == len(ic.calc())
    assert ic.nbonds > 8                                                # bonds between the fragments
    explicit = InternalCoordinates(at, ic.idx['bonds'], ic.idx['angles'], ic.idx['dihedrals'], ic.ncv['bonds'],
                                   ic.ncv['angles'], ic.ncv['dihedrals'])
    assert np.array_equal(explicit.calc(), ic.calc()) and np.array_equal(explicit.jacobian(), ic.jacobian())
    assert not InternalCoordinates.from_atoms(at, allow_fragments=False).allow_fragments


def test_add_translation_and_rotation(ctx):
    from sella_amd.internal import DuplicateInternalError, InternalCoordinates
    at = water_cluster()
    ic = InternalCoordinates(at)
    ic.add_translation(3, dim=1)
    ic.add_rotation([0, 1, 2], axis=2)
    ic.add_rotation([0, 1, 2], axis=0)                  # the same fragment: one reference, one quaternion state
    ic.add_rotation([0, 1, 2], axis=1)
    with pytest.raises(DuplicateInternalError):
        ic.add_rotation([0, 1, 2], axis=2)
    with pytest.raises(DuplicateInternalError):
        ic.add_translation([3], dim=1)
    with pytest.raises(ValueError):
        ic.add_rotation([4])
    assert ic.ntrans == 1 and ic.nrotations == 3 and len(ic.frags) == 1
    q = ic.calc()
    assert q[0] == at.positions[3, 1] and np.abs(q[1:]).max() < 1e-12


# ---- 6. end to end ----------------------------------------------------------------------------------------------------
def fd_hessian(at, h=1e-4):
    x0 = at.positions.copy()
    n = x0.size
    H = np.zeros((n, n))
    for i in range(n):
        d = np.zeros(n)
        d[i] = h
        at.positions = (x0.ravel() + d).reshape(-1, 3)
        gp = -at.get_forces().ravel()
        at.positions = (x0.ravel() - d).reshape(-1, 3)
        gm = -at.get_forces().ravel()
        H[:, i] = (gp - gm) / (2 * h)
    at.positions = x0
    return 0.5 * (H + H.T)


@pytest.mark.emu_heavy
def test_cluster_minimum_and_saddle(ctx):
    from sella_amd import Sella
    at = water_cluster()
    opt = Sella(at, internal=True, allow_fragments=True, order=0, logfile=None)
    assert opt.pes.int.nrotations == 12 and opt.pes.int.ntrans == 15
    assert opt.run(fmax=1e-3, steps=400)
    assert np.abs(at.get_forces()).max() < 1e-3
    w, V = np.linalg.eigh(fd_hessian(at))
    assert w[0] > -1e-4, w[:8]
    # order 1 from the minimum pushed along its softest internal mode
    soft = V[:, 6]
    at.positions = at.positions + 0.3 * soft.reshape(-1, 3)
    opt = Sella(at, internal=True, allow_fragments=True, order=1, logfile=None)
    assert opt.run(fmax=1e-3, steps=400)
    assert np.abs(at.get_forces()).max() < 1e-3
    w = np.linalg.eigvalsh(fd_hessian(at))
    assert int(np.sum(w < -1e-4)) == 1, w[:8]


# ---- 7. rebuild ----------------------------------------------------------------------------------------------------
def test_rebuild_keeps_fragment_coordinates(ctx, monkeypatch):
    from sella_amd import Sella
    from sella_amd.internal import InternalCoordinates
    at = water_cluster()
    opt = Sella(at, order=0, internal=True, allow_fragments=True, logfile=None, exact_geodesic=False)
    opt.run(fmax=1e-9, steps=1)
    first = opt.pes
    calls = {'n': 0}
    real = InternalCoordinates.check_for_bad_internals

    def once_bad(self):
        calls['n'] += 1
        return np.array([0]) if calls['n'] == 1 else real(self)
    monkeypatch.setattr(InternalCoordinates, 'check_for_bad_internals', once_bad)
    opt.step()
    assert opt.pes is not first and not opt.initialized
    assert opt.pes.int.ntrans == 15 and opt.pes.int.nrotations == 12 and opt.pes.int.allow_fragments


def test_cartesian_accepts_the_flag(ctx):
    from sella_amd import Sella
    at = water_cluster()
    opt = Sella(at, order=0, allow_fragments=True, logfile=None)
    assert opt.pes.int is None
