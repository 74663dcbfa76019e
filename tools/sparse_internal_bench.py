"""Device-resident sparse internal-coordinate Hessians (sella_amd.linalg.SparseInternalHessians, csrc/sparse_internal.hip)
against the host stacks of InternalCoordinates.hessian() (`_HessianStack`) on the 1024-atom Cu(111) slab, bonds + angles
(3N = 3072, 57,600 coordinates).

    python tools/sparse_internal_bench.py [--reps 20] [--atoms 16,16,4]

Device times: host clock around the call, which ends in a device synchronisation (every entry point returns complete
results).  `ldot_dev` / `rdot_dev` write into preallocated device matrices; `ldot` / `rdot` include the download and
the numpy array (72 MB / 1.4 GB).  Kernel times: run under `rocprofv3 --kernel-trace --stats` separately."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps, sync=None):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--atoms', default='16,16,4')
    ap.add_argument('--host-reps', type=int, default=3)
    args = ap.parse_args()

    from sella_amd.atoms import fcc111
    from sella_amd.device import get_context
    from sella_amd.internal import InternalCoordinates, angles_from_bonds, neighbour_bonds

    ctx = get_context()
    slab = fcc111('Cu', tuple(int(s) for s in args.atoms.split(',')), vacuum=6.0)
    slab.positions += 0.05 * np.random.RandomState(3).normal(size=slab.positions.shape)
    bonds, bncv = neighbour_bonds(slab, 1.25 * 3.61 / np.sqrt(2))
    angles, ancv = angles_from_bonds(bonds, bncv)
    ic = InternalCoordinates(slab, bonds=bonds, angles=angles, bond_ncvecs=bncv, angle_ncvecs=ancv)
    rng = np.random.RandomState(0)
    v, x, u = rng.normal(size=ic.nint), rng.normal(size=ic.ndof), rng.normal(size=ic.ndof)
    print(f'{len(slab)} atoms, 3N = {ic.ndof}, {len(bonds)} bonds + {len(angles)} angles on {ctx.name}', flush=True)

    t0 = time.perf_counter()
    H = ic.sparse_hessians()
    first_fill = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    H.ldot(v)
    first_ldot = 1e3 * (time.perf_counter() - t0)
    Lout, Rout = ctx.zeros(ic.ndof, ic.ndof), ctx.zeros(ic.nint, ic.ndof)
    rows = [('sparse_hessians() fill', median_ms(ic.sparse_hessians, args.reps)),
            ('ldot_dev', median_ms(lambda: H.ldot_dev(v, Lout), args.reps)),
            ('rdot_dev', median_ms(lambda: H.rdot_dev(x, Rout), args.reps)),
            ('ddot', median_ms(lambda: H.ddot(u, x), args.reps)),
            ('ldot (numpy out)', median_ms(lambda: H.ldot(v), args.reps)),
            ('rdot (numpy out)', median_ms(lambda: H.rdot(x), max(2, args.reps // 4)))]
    Rout.free()
    host = ic.hessian()
    hrows = [('hessian() fill', median_ms(ic.hessian, args.host_reps)),
             ('ldot', median_ms(lambda: host.ldot(v), args.host_reps)),
             ('rdot', median_ms(lambda: host.rdot(x), args.host_reps)),
             ('ddot', median_ms(lambda: host.ddot(u, x), args.host_reps))]
    # the device result against the host stack (ldot: the host sums in coordinate order, the device in the reference's
    # group order; a few ulps apart)
    L, Lh = H.ldot(v), host.ldot(v)
    print(f'ldot max |device - host| = {np.abs(L - Lh).max():.2e} (max |entry| {np.abs(Lh).max():.2e})')
    print(f'first sparse_hessians() {first_fill:.1f} ms (skeleton built and uploaded), first ldot {first_ldot:.1f} ms '
          f'(pair index built)')
    print(f'{"device":<26}{"ms":>10}')
    for name, ms in rows:
        print(f'{name:<26}{ms:>10.3f}')
    print(f'{"host stack":<26}{"ms":>10}')
    for name, ms in hrows:
        print(f'{name:<26}{ms:>10.3f}')
    Lout.free()


if __name__ == '__main__':
    main()
