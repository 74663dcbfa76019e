#!/usr/bin/env python3
"""Time the conversion of a Cartesian Hessian into internal coordinates (`InternalPES.calculate_hessian` with a
`hessian_function`) on the device against a NumPy restatement of the reference's dense path on the host
(sella/peswrapper.py:1247-1275: dense B, full SVD, sum_i g_i d2q_i/dx2, two products, eigh), 16 BLAS threads.

    python tools/hessconv_bench.py [--sizes 20 60 200] [--reps 5] [--out FILE]

The molecules are zigzag chains with a Morse calculator, built here; Hcart is random and symmetric.  Device time: the
whole method call (curvature blocks evaluated on the device, uploads, `sella_hessian_cart_to_int`, result left on the
device) with the spectral factor of B already cached for the geometry, as it is in a search (the PES factors B at every
new point anyway).  The factor's own time is reported beside it.  Both results are compared.
"""
import argparse
import json
import os
import sys
import time

for var in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):
    os.environ.setdefault(var, '16')

import numpy as np  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def chain(natoms, seed=0):
    """A zigzag chain (C-C 1.05 A, 112 degrees) twisted a little out of plane, so that dihedrals are defined."""
    from sella_amd.atoms import Atoms, MorseCluster
    rng = np.random.RandomState(seed)
    half = np.radians(112.0) / 2
    pos = np.zeros((natoms, 3))
    for k in range(1, natoms):
        pos[k] = pos[k - 1] + 1.05 * np.array([np.sin(half), (-1) ** k * np.cos(half), 0.0])
    pos += 0.03 * rng.normal(size=pos.shape)
    at = Atoms(['C'] * natoms, pos, pbc=False)
    at.calc = MorseCluster(D=1.2, a=1.6, r0=1.05)
    return at


def host_reference(B, Hc, Hcart):
    """The reference's dense path (peswrapper.py:1254-1275) in NumPy."""
    U, S, Vt = np.linalg.svd(B, full_matrices=True)
    r = int(np.sum(S > 1e-6))
    X = Vt[:r].T / S[:r]
    Hnred = X.T @ (Hcart - Hc) @ X
    lam = np.exp(np.log(np.abs(np.linalg.eigvalsh(Hnred))).mean())
    return U[:, :r] @ Hnred @ U[:, :r].T + lam * U[:, r:] @ U[:, r:].T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[20, 60, 200])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from sella_amd.device import get_context
    from sella_amd.internal import InternalCoordinates
    from sella_amd.peswrapper import InternalPES, _BFactor
    ctx = get_context()
    rows = []
    for natoms in args.sizes:
        at = chain(natoms)
        pes = InternalPES(at, InternalCoordinates.from_atoms(at))
        n, nint = 3 * natoms, len(pes.get_x())
        A = np.random.RandomState(1).normal(size=(n, n))
        Hcart = A + A.T
        pes._convert_cartesian_hessian_to_internal(Hcart).free()              # warm-up of every shape
        dev = []
        for _ in range(args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            out = pes._convert_cartesian_hessian_to_internal(Hcart)
            ctx.sync()
            dev.append(time.perf_counter() - t0)
        H_dev = out.numpy()
        out.free()
        fac = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _BFactor(pes.int.jacobian_csr())
            ctx.sync()
            fac.append(time.perf_counter() - t0)
        host = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            B = np.asarray(pes.int.jacobian())
            Hc = np.asarray(pes.int.hessian().ldot(pes.get_g()))
            H_ref = host_reference(B, Hc, Hcart)
            host.append(time.perf_counter() - t0)
        rel = float(np.linalg.norm(H_dev - H_ref) / np.linalg.norm(H_ref))
        row = dict(natoms=natoms, ncart=n, nint=nint, device_ms=1e3 * float(np.median(dev)),
                   factor_ms=1e3 * float(np.median(fac)), host_numpy_ms=1e3 * float(np.median(host)), rel_diff=rel)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(device=ctx.name, blas_threads=os.environ.get('OMP_NUM_THREADS'), rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
