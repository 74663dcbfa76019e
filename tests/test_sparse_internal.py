"""sella_amd.linalg.SparseInternalJacobian / SparseInternalHessian / SparseInternalHessiansSkeleton /
SparseInternalHessians (sella/linalg.py:362-646) on the device (csrc/sparse_internal.hip): the pinned reference fixture
g11 through the public classes, skeleton reuse, device-filled topologies of InternalCoordinates, and the 1024-atom slab
on the hardware."""
import time

import numpy as np
import pytest

from conftest import load_golden


def _slab(size):
    from sella_amd.atoms import fcc111
    slab = fcc111('Cu', size, vacuum=6.0)
    rng = np.random.RandomState(3)
    slab.positions += 0.05 * rng.normal(size=slab.positions.shape)
    return slab


def group_order_ldot(natoms, indices, vals, v):
    """sum_i v_i H_i summed as the reference does: size groups in order of first appearance, each group's sum from
    zero (coordinates in order, then local (a, b, i, j) order, every product rounded), added to the running total."""
    ndof = 3 * natoms
    sizes = [len(ix) for ix in indices]
    total = np.zeros(ndof * ndof)
    for m in dict.fromkeys(sizes):
        members = [c for c in range(len(indices)) if sizes[c] == m]
        part = np.zeros(ndof * ndof)
        if m:
            ix = np.array([np.asarray(indices[c]) for c in members])                    # (batch, m)
            dof = 3 * ix[:, :, None] + np.arange(3)                                      # (batch, a, i)
            flat = dof[:, :, None, :, None] * ndof + dof[:, None, :, None, :]            # (batch, a, b, i, j)
            prod = np.array([np.asarray(vals[c]).transpose(0, 2, 1, 3) for c in members]) * v[members][:, None, None,
                                                                                                        None, None]
            np.add.at(part, flat.ravel(), prod.ravel())
        total += part
    return total.reshape(ndof, ndof)


def _random_case(rng, natoms, sizes):
    indices = [rng.choice(natoms, size=m, replace=False) for m in sizes]
    hvals = []
    for m in sizes:
        h = rng.normal(size=(3 * m, 3 * m))
        hvals.append((0.5 * (h + h.T)).reshape(m, 3, m, 3))
    return indices, hvals


def test_golden_through_public_classes(ctx, manifest):
    """g11 (generated from the reference's own classes) through the public classes, fed with the reference's
    constructor arguments in the fixture's mixed order; case 1 carries a coordinate that repeats an atom."""
    from sella_amd.linalg import SparseInternalHessian, SparseInternalHessians, SparseInternalJacobian
    g = load_golden('g11_sparse_internal')
    for case in manifest['g11_sparse_internal']:
        i, natoms, sizes = case['id'], case['natoms'], case['sizes']
        indices = [g[f'c{i}_idx{k}'] for k in range(len(sizes))]
        gvals = [g[f'c{i}_g{k}'] for k in range(len(sizes))]
        hvals = [g[f'c{i}_h{k}'] for k in range(len(sizes))]
        x, u, y = g[f'c{i}_x'], g[f'c{i}_u'], g[f'c{i}_y']
        J = SparseInternalJacobian(natoms, [list(ix) for ix in indices], [list(v) for v in gvals])
        hs = [SparseInternalHessian(natoms, list(ix), hv) for ix, hv in zip(indices, hvals)]
        Hs = SparseInternalHessians(hs, 3 * natoms)
        assert np.array_equal(Hs.ldot(y), g[f'c{i}_ldot']), i
        assert np.array_equal(J.rmatvec(y), g[f'c{i}_JTy']), i
        np.testing.assert_allclose(J.asarray(), g[f'c{i}_J'], atol=1e-14)
        np.testing.assert_allclose(Hs.asarray(), g[f'c{i}_Hall'], atol=1e-14)
        np.testing.assert_allclose(np.asarray(Hs), g[f'c{i}_Hall'], atol=1e-14)
        np.testing.assert_allclose(hs[0].asarray(), g[f'c{i}_H0'], atol=1e-14)
        np.testing.assert_allclose(J.matvec(x), g[f'c{i}_Jx'], atol=1e-13)
        np.testing.assert_allclose(Hs.rdot(x), g[f'c{i}_rdot'], atol=1e-13)
        np.testing.assert_allclose(Hs.ddot(u, x), g[f'c{i}_ddot'], atol=1e-13)
        np.testing.assert_allclose(hs[0].matvec(x), g[f'c{i}_H0x'], atol=1e-13)
        assert np.array_equal(Hs.ldot_dev(y).numpy(), g[f'c{i}_ldot'])
        np.testing.assert_allclose(Hs.rdot_dev(x).numpy(), g[f'c{i}_rdot'], atol=1e-13)


def test_skeleton_reuse_and_mismatch(ctx):
    """A skeleton reused with new values computes what a fresh build does, and the values of the first user survive
    the second (they are uploaded again when it computes next); a skeleton of another (n_hess, natoms) is refused."""
    from sella_amd.linalg import SparseInternalHessian, SparseInternalHessians
    rng = np.random.RandomState(7)
    natoms, sizes = 10, (3, 2, 4, 2, 3, 3, 2, 4)
    ind, va = _random_case(rng, natoms, sizes)
    vb = [rng.normal(size=h.shape) for h in va]
    v, x, u = rng.normal(size=len(sizes)), rng.normal(size=3 * natoms), rng.normal(size=3 * natoms)
    A = SparseInternalHessians([SparseInternalHessian(natoms, ix, h) for ix, h in zip(ind, va)], 3 * natoms)
    hb = [SparseInternalHessian(natoms, ix, h) for ix, h in zip(ind, vb)]
    B = SparseInternalHessians(hb, 3 * natoms, skeleton=A._skeleton)
    fresh = SparseInternalHessians(hb, 3 * natoms)
    assert B._skeleton is A._skeleton
    assert np.array_equal(B.ldot(v), fresh.ldot(v))
    assert np.array_equal(B.rdot(x), fresh.rdot(x))
    assert np.array_equal(B.ddot(u, x), fresh.ddot(u, x))
    assert np.array_equal(B.asarray(), fresh.asarray())
    assert np.array_equal(A.ldot(v), group_order_ldot(natoms, ind, va, v))
    assert np.array_equal(B.ldot(v), group_order_ldot(natoms, ind, vb, v))
    with pytest.raises(ValueError):
        SparseInternalHessians(hb[:-1], 3 * natoms, skeleton=A._skeleton)
    with pytest.raises(ValueError):
        SparseInternalHessians(hb, 3 * (natoms + 1), skeleton=A._skeleton)


def test_empty_and_wide_coordinates(ctx):
    """Zero coordinates, coordinates of no atoms between the others, and one coordinate over 40 atoms."""
    from sella_amd.linalg import SparseInternalHessian, SparseInternalHessians, SparseInternalJacobian
    natoms = 45
    ndof = 3 * natoms
    none = SparseInternalHessians([], ndof)
    assert np.array_equal(none.ldot(np.zeros(0)), np.zeros((ndof, ndof)))
    assert none.rdot(np.ones(ndof)).shape == (0, ndof)
    assert none.ddot(np.ones(ndof), np.ones(ndof)).shape == (0,)
    assert none.asarray().shape == (0, ndof, ndof)
    J0 = SparseInternalJacobian(natoms, [], [])
    assert J0.asarray().shape == (0, ndof)
    assert np.array_equal(J0.rmatvec(np.zeros(0)), np.zeros(ndof))

    rng = np.random.RandomState(11)
    sizes = (2, 0, 42, 3, 0, 2)
    ind, hv = _random_case(rng, natoms, sizes)
    gv = [rng.normal(size=(m, 3)) for m in sizes]
    hs = [SparseInternalHessian(natoms, ix, h) for ix, h in zip(ind, hv)]
    H = SparseInternalHessians(hs, ndof)
    J = SparseInternalJacobian(natoms, ind, gv)
    v, x, u = rng.normal(size=len(sizes)), rng.normal(size=ndof), rng.normal(size=ndof)
    dense = np.array([h.asarray() for h in hs])
    Jd = np.zeros((len(sizes), natoms, 3))
    for k, (ix, g) in enumerate(zip(ind, gv)):
        np.add.at(Jd[k], ix, g)
    Jd = Jd.reshape(len(sizes), ndof)
    assert np.array_equal(H.ldot(v), group_order_ldot(natoms, ind, hv, v))
    np.testing.assert_allclose(H.asarray(), dense, atol=1e-14)
    np.testing.assert_allclose(H.rdot(x), dense @ x, atol=1e-12)
    np.testing.assert_allclose(H.ddot(u, x), (dense @ x) @ u, atol=1e-12)
    np.testing.assert_allclose(J.asarray(), Jd, atol=1e-14)
    np.testing.assert_allclose(J.matvec(x), Jd @ x, atol=1e-13)
    np.testing.assert_allclose(J.rmatvec(v), Jd.T @ v, atol=1e-13)


def test_device_filled_topology(ctx):
    """ic.sparse_hessians() / sparse_jacobian() — blocks evaluated on the device into the object's buffers — against
    ic.hessian() / ic.jacobian() on a periodic slab with bonds, angles, dihedrals and a bond to an atom's own image;
    the cached skeleton is reused after the atoms move, and the values of the earlier object survive that."""
    from sella_amd.internal import InternalCoordinates
    slab = _slab((2, 2, 2))
    full = InternalCoordinates.from_atoms(slab)
    assert len(full.idx['dihedrals'])
    b, a, d = full.idx['bonds'], full.idx['angles'][:40], full.idx['dihedrals'][:24]
    bncv, ancv, dncv = full.ncv['bonds'], full.ncv['angles'][:40], full.ncv['dihedrals'][:24]
    b = np.vstack([b, [[0, 0]]])                                          # atom 0 bonded to its own image along a
    bncv = np.concatenate([bncv, [[[1.0, 0.0, 0.0]]]])
    ic = InternalCoordinates(slab, bonds=b, angles=a, dihedrals=d, bond_ncvecs=bncv, angle_ncvecs=ancv,
                             dihedral_ncvecs=dncv)
    rng = np.random.RandomState(5)
    v, x, u = rng.normal(size=ic.nint), rng.normal(size=ic.ndof), rng.normal(size=ic.ndof)

    H, Hh = ic.sparse_hessians(), ic.hessian()
    J, Jh = ic.sparse_jacobian(), ic.jacobian()
    assert H.shape == Hh.shape
    np.testing.assert_allclose(H.asarray(), Hh.asarray(), atol=1e-12)
    np.testing.assert_allclose(H.ldot(v), Hh.ldot(v), atol=1e-12)
    np.testing.assert_allclose(H.rdot(x), Hh.rdot(x), atol=1e-12)
    np.testing.assert_allclose(H.ddot(u, x), Hh.ddot(u, x), atol=1e-12)
    np.testing.assert_allclose(J.asarray(), Jh, atol=1e-12)
    np.testing.assert_allclose(J.matvec(x), Jh @ x, atol=1e-12)
    np.testing.assert_allclose(J.rmatvec(v), Jh.T @ v, atol=1e-12)
    L = H.ldot(v)
    assert np.array_equal(H.ldot_dev(v).numpy(), L)
    assert np.array_equal(L, group_order_ldot(len(slab), [h.indices for h in H.hessians], [h.vals for h in H.hessians],
                                              v))

    slab.positions += 0.02 * rng.normal(size=slab.positions.shape)
    H2, J2 = ic.sparse_hessians(), ic.sparse_jacobian()
    assert H2._skeleton is H._skeleton
    np.testing.assert_allclose(H2.asarray(), ic.hessian().asarray(), atol=1e-12)
    np.testing.assert_allclose(J2.asarray(), ic.jacobian(), atol=1e-12)
    assert np.array_equal(H.ldot(v), L)                                   # the first object's values were kept
    np.testing.assert_allclose(J.asarray(), Jh, atol=1e-12)


def test_config_scale_slab(ctx):
    """The 1024-atom Cu slab with bonds + angles (3N = 3072, 57,600 coordinates): ldot bit for bit against the
    group-order sum, rdot against the host stack; timings printed, not asserted."""
    if ctx.backend != 'hip':
        pytest.skip('config scale: device only')
    from sella_amd.internal import InternalCoordinates, angles_from_bonds, neighbour_bonds
    slab = _slab((16, 16, 4))
    bonds, bncv = neighbour_bonds(slab, 1.25 * 3.61 / np.sqrt(2))
    angles, ancv = angles_from_bonds(bonds, bncv)
    ic = InternalCoordinates(slab, bonds=bonds, angles=angles, bond_ncvecs=bncv, angle_ncvecs=ancv)
    rng = np.random.RandomState(9)
    v, x = rng.normal(size=ic.nint), rng.normal(size=ic.ndof)
    t0 = time.perf_counter()
    H = ic.sparse_hessians()
    t1 = time.perf_counter()
    L = H.ldot(v)
    t2 = time.perf_counter()
    hs = H.hessians
    assert np.array_equal(L, group_order_ldot(len(slab), [h.indices for h in hs], [h.vals for h in hs], v))
    t3 = time.perf_counter()
    R = H.rdot(x)
    t4 = time.perf_counter()
    Rh = ic.hessian().rdot(x)
    np.testing.assert_allclose(R, Rh, rtol=1e-12, atol=1e-12 * np.abs(Rh).max())
    print(f'\n1024-atom slab, {ic.nint} coordinates: sparse_hessians() {1e3 * (t1 - t0):.1f} ms (first: skeleton '
          f'upload), ldot {1e3 * (t2 - t1):.1f} ms (first: pair index), rdot {1e3 * (t4 - t3):.1f} ms')
