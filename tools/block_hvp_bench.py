#!/usr/bin/env python3
"""Time the block form of the device-resident Hessian-vector operator (`sella_hvp_apply_block`, `sella_davidson_block_hvp`,
`sella_amd.lowest_modes`) against what it stands in for; prints one JSON line per slab.

    python tools/block_hvp_bench.py [--reps R] [--warmup W] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/block_hvp_bench.py --trace     # kernel times, a run of its own

On the Cu(111) slabs fcc111('Cu', (8, 8, 16)) (1024 atoms, 3N = 3072) and (10, 10, 11) (1100 atoms), lower half pinned atom
by atom as in tools/hvp_operator_bench.py.  Every window is a host clock around work that ends in a stream synchronisation;
all variants are warmed up first and then alternated in one process, `reps` windows each; medians with min / max /
interquartile range.

(a) 16 products of the same 16 vectors (host panels in, host panels out):
  single16_ms      the baseline: 16 x `sella_hvp_matvec` (the single-vector kernels; 16 uploads, read-backs and waits)
  block_ms         one `sella_hvp_apply_block` (one upload, read-back and wait)
  panel16_dense_ms the same 16 products from the resident dense Hessian: `sella_symm_mm` with 16 right-hand sides, i.e.
                   one `launch_panel16` over the 3N x 3N matrix (full-length vectors up, full-length products back)
  diagonal_ms      `sella_hvp_diag` (one launch that sweeps all atoms through all images per atom: O(N^2 images))
(b) the four lowest modes of the free block, tol 1e-8, end to end:
  lowest_modes_ms  `lowest_modes(nev=4)`: operator, its diagonal, `sella_davidson_block_hvp`
  dense_*_ms       the route before the operator had a block form: `sella_calc_hessian` (build), the free block cut out on
                   the host and uploaded (cut), `Context.davidson_block` on it with its diagonal (solve); dense_ms their sum
  eigh_ms          `Context.eigh` of the same free block (after build and cut)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sella_amd import _lib, lowest_modes  # noqa: E402
from sella_amd._lib import ptr  # noqa: E402
from sella_amd.atoms import EMT  # noqa: E402
from sella_amd.device import DeviceHvpOperator, get_context  # noqa: E402
from tools.emt_slab_opt import make_slab  # noqa: E402  (bench.py's slab)
from tools.hvp_operator_bench import alternate, pinned_lower_half, spread  # noqa: E402

SIZES = [(8, 8, 16), (10, 10, 11)]


def setup(size):
    slab = make_slab(size)
    slab.calc = EMT()
    slab.get_potential_energy()
    dc = slab.calc.device_calculator()
    x0 = slab.positions.ravel().copy()
    cons = pinned_lower_half(slab)
    free = np.setdiff1d(np.arange(x0.size), np.flatnonzero((cons.jacobian() != 0.0).any(axis=0))).astype(np.int32)
    return slab, dc, x0, free


def measure(ctx, size, a):
    slab, dc, x0, free = setup(size)
    n, m = x0.size, len(free)
    V = np.random.RandomState(0).normal(size=(16, m))
    V /= np.linalg.norm(V, axis=1)[:, None]
    out_m = np.empty(m)
    L = _lib.lib()
    single = DeviceHvpOperator(dc, x0, free)

    def single16():
        for v in V:
            L.sella_hvp_matvec(single._h, ptr(v), ptr(out_m), m)

    block = DeviceHvpOperator(dc, x0, free)
    dH = dc.hessian(x0)
    Xfull = np.zeros((n, 16))
    Xfull[free] = V.T
    calls = dict(single16=single16, block=lambda: block.apply_block(V), panel16_dense=lambda: ctx.symm_mm(dH, Xfull),
                 diagonal=block.diagonal)
    samples = alternate(ctx, calls, a.warmup, a.reps)
    out = dict(device=ctx.name, natoms=n // 3, n=n, nfree=m, reps=a.reps)
    for name in calls:
        out[f'{name}_ms'] = spread(np.array(samples[name]))
    dH.free()
    # (b) end to end
    info = {}

    def modes():
        info['modes'] = lowest_modes(slab, nev=4, free=free, tol=1e-8)

    def dense_parts():
        t0 = time.perf_counter()
        dH = dc.hessian(x0)
        ctx.sync()
        t1 = time.perf_counter()
        Hs = np.ascontiguousarray(dH.numpy()[free][:, free])
        dH.free()
        dA = ctx.upload(Hs)
        ctx.sync()
        t2 = time.perf_counter()
        return dA, Hs, t1 - t0, t2 - t1, t2

    parts = dict(dense_build=[], dense_cut=[], dense_solve=[], dense=[], eigh=[], lowest_modes=[])
    for rep in range(a.warmup + a.reps):
        ctx.sync()
        t0 = time.perf_counter()
        modes()
        ctx.sync()
        tm = time.perf_counter() - t0
        dA, Hs, tb, tc, t2 = dense_parts()
        info['dense'] = ctx.davidson_block(dA, m, 4, block=4, tol=1e-8, diag=np.ascontiguousarray(np.diag(Hs)))
        ctx.sync()
        ts = time.perf_counter() - t2
        t3 = time.perf_counter()
        w = ctx.eigh(dA, vectors=False)
        ctx.sync()
        te = time.perf_counter() - t3
        info['w'] = np.asarray(w[0] if isinstance(w, tuple) else w)[:4]
        dA.free()
        if rep >= a.warmup:
            for key, t in (('dense_build', tb), ('dense_cut', tc), ('dense_solve', ts), ('dense', tb + tc + ts), ('eigh', te),
                           ('lowest_modes', tm)):
                parts[key].append(t)
    for key, ts in parts.items():
        out[f'{key}_ms'] = spread(np.array(ts))
    mo, de = info['modes'], info['dense']
    out['lowest_modes_run'] = dict(lams=list(mo['lams']), niter=mo['niter'], nmatvec=mo['nmatvec'], nconv=mo['nconv'])
    out['dense_run'] = dict(lams=list(de['lams']), niter=de['niter'], nmatvec=de['nmatvec'], nconv=de['nconv'])
    out['eigh_lams'] = list(info['w'])
    return out


def trace(ctx, a):
    """A few products of each kind at the 1024-atom slab, for `rocprofv3 --kernel-trace --stats`."""
    slab, dc, x0, free = setup(SIZES[0])
    m = len(free)
    V = np.random.RandomState(0).normal(size=(16, m))
    single = DeviceHvpOperator(dc, x0, free)
    for _ in range(5):
        for v in V:
            single.apply(v)
        DeviceHvpOperator(dc, x0, free).apply_block(V)
    ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--trace', action='store_true', help='only a few products of each kind (under rocprofv3)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = get_context()
    if a.trace:
        trace(ctx, a)
        return
    results = []
    for size in SIZES:
        res = measure(ctx, size, a)
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
