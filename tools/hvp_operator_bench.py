#!/usr/bin/env python3
"""Time the device-resident Hessian-vector operator (`sella_hvp_*`, `sella_davidson_hvp`) against the finite-difference
operator it stands in for; prints one JSON line per slab.

    python tools/hvp_operator_bench.py [--reps R] [--warmup W] [--products P] [--maxiter M] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/hvp_operator_bench.py --trace     # kernel times, a run of its own

On the Cu(111) slabs fcc111('Cu', (8, 8, 16)) (1024 atoms, 3N = 3072) and (10, 10, 11) (1100 atoms), lower half pinned
atom by atom as in bench.py.  Every window is a host clock around work that ends in a stream synchronisation; all variants
are warmed up first and then alternated in one process, `reps` windows each; medians, and for the baseline the spread
(min, max, interquartile range).

Per product (a window is P products):
  fd_ms        (a) `sella_fd_matvec`, one-sided: the baseline — upload of the displaced point, density and force pass, read-back
               of the gradient, wait, the quotient on the host
  hvp_k1_ms    (b) `sella_emt_hvp` with k = 1: density pass, F2, the two product passes on a group of 8 vectors, upload,
               read-back, wait
  op_host_ms   `sella_hvp_matvec`: upload of v, the operator's device product, read-back, wait
Per ADDED Davidson iteration at fixed start vector, (time(maxiter = M) - time(maxiter = M / 2)) / (M / 2), gamma so small that
no call converges; the iterations of the three operator kinds differ by their products only:
  iter_fd_ms   `sella_davidson` over `sella_fd_matvec`
  iter_cb_ms   `sella_davidson` over `sella_hvp_matvec` (host callback)
  iter_dev_ms  (c) `sella_davidson_hvp` (the device branch: no copy, no wait, no callback frame per product)
  dev_minus_fd_ms = iter_dev_ms - iter_fd_ms: what one product gains or loses inside the eigensolver
Per `PES.diag(maxiter = M)` on a fresh PES whose point is already evaluated: wall time, force calls and products, without
and with `hessian_vector_product=True`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sella_amd import Constraints, _lib  # noqa: E402
from sella_amd._lib import ptr  # noqa: E402
from sella_amd.atoms import EMT  # noqa: E402
from sella_amd.device import DeviceFdOperator, DeviceHvpOperator, get_context  # noqa: E402
from sella_amd.peswrapper import PES  # noqa: E402
from tools.emt_slab_opt import make_slab  # noqa: E402  (bench.py's slab)

SIZES = [(8, 8, 16), (10, 10, 11)]


def pinned_lower_half(slab):
    cons = Constraints(slab)
    for atom in slab:
        if atom.position[2] < slab.cell[2, 2] / 2.:
            cons.fix_translation(atom.index)
    return cons


def spread(ts):
    q1, q3 = np.percentile(ts, [25, 75])
    return dict(median=1e3 * float(np.median(ts)), min=1e3 * float(np.min(ts)), max=1e3 * float(np.max(ts)),
                iqr=1e3 * float(q3 - q1))


def alternate(ctx, calls, warmup, reps):
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    samples = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            samples[name].append(time.perf_counter() - t0)
    return samples


def measure(ctx, size, a):
    slab = make_slab(size)
    calc = EMT()
    slab.calc = calc
    g0 = -slab.get_forces().ravel()
    S = calc._setup[1]
    dc = calc.device_calculator()
    pos = slab.positions.copy()
    x0 = pos.ravel().copy()
    n = x0.size
    args = (S['par'], S['shifts'], S['rc'], S['acut'], S['cutoff'], EMT._BETA)
    cons = pinned_lower_half(slab)
    free = np.setdiff1d(np.arange(n), np.flatnonzero((cons.jacobian() != 0.0).any(axis=0))).astype(np.int32)
    m = len(free)
    rng = np.random.RandomState(0)
    V = rng.normal(size=(a.products, m))
    V /= np.linalg.norm(V, axis=1)[:, None]
    Vfull = np.zeros((a.products, n))
    Vfull[:, free] = V
    out_m = np.empty(m)
    L = _lib.lib()

    def fd_products():
        op = DeviceFdOperator(dc, x0, g0, 1e-4, False, free)
        for v in V:
            L.sella_fd_matvec(op._h, ptr(v), ptr(out_m), m)

    def hvp_k1_products():
        for v in Vfull:
            ctx.emt_hvp(pos, *args, v)

    hop = DeviceHvpOperator(dc, x0, free)

    def op_host_products():
        for v in V:
            L.sella_hvp_matvec(hop._h, ptr(v), ptr(out_m), m)

    v0 = V[0].copy()
    M, M0 = a.maxiter, a.maxiter // 2

    def dav(kind, maxiter):
        def run():
            if kind == 'fd':
                op = DeviceFdOperator(dc, x0, g0, 1e-4, False, free)
            else:
                op = DeviceHvpOperator(dc, x0, free, through_host=kind == 'cb')
            ctx.davidson(op, m, v0, 1e-12, method='jd0', maxiter=maxiter)
        return run

    def diag(keyword):
        def run():
            run.pes.diag(maxiter=M)

        def fresh():
            run.pes = PES(slab, constraints=cons, hessian_vector_product=keyword)
            run.pes.get_g()
        run.fresh = fresh
        return run

    calls = dict(fd=fd_products, hvp_k1=hvp_k1_products, op_host=op_host_products)
    for kind in ('fd', 'cb', 'dev'):
        calls[f'dav_{kind}_{M}'] = dav(kind, M)
        calls[f'dav_{kind}_{M0}'] = dav(kind, M0)
    samples = alternate(ctx, calls, a.warmup, a.reps)
    out = dict(device=ctx.name, natoms=n // 3, n=n, nfree=m, nimages=len(S['shifts']), products=a.products, reps=a.reps,
               maxiter=M)
    for name in ('fd', 'hvp_k1', 'op_host'):
        per = np.array(samples[name]) / a.products
        out[f'{name}_ms'] = 1e3 * float(np.median(per))
    out['fd_ms_spread'] = spread(np.array(samples['fd']) / a.products)
    for kind in ('fd', 'cb', 'dev'):
        hi, lo = np.array(samples[f'dav_{kind}_{M}']), np.array(samples[f'dav_{kind}_{M0}'])
        out[f'dav_{kind}_{M}_ms'] = 1e3 * float(np.median(hi))
        out[f'dav_{kind}_{M0}_ms'] = 1e3 * float(np.median(lo))
        out[f'iter_{kind}_ms'] = 1e3 * float(np.median(hi) - np.median(lo)) / (M - M0)
        if kind == 'fd':
            out['iter_fd_ms_spread'] = spread((hi - lo) / (M - M0))
    out['dev_minus_fd_ms'] = out['iter_dev_ms'] - out['iter_fd_ms']
    out['dev_minus_cb_ms'] = out['iter_dev_ms'] - out['iter_cb_ms']
    # PES.diag with and without the keyword, alternated; the PES is made (and its point evaluated) outside the window
    runs = dict(diag_fd=diag(None), diag_hvp=diag(True))
    ts = {name: [] for name in runs}
    counts = {}
    for rep in range(a.warmup + a.reps):
        for name, fn in runs.items():
            fn.fresh()
            before = calc.ncalls
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            dt = time.perf_counter() - t0
            if rep >= a.warmup:
                ts[name].append(dt)
            counts[name] = dict(force_calls=calc.ncalls - before, products=fn.pes.nhvp)
    for name in runs:
        out[f'{name}_ms'] = 1e3 * float(np.median(ts[name]))
        out[f'{name}_counts'] = counts[name]
    out['diag_fd_ms_spread'] = spread(ts['diag_fd'])
    return out


def trace(ctx, a):
    """A few calls of each kind at the 1024-atom slab, for `rocprofv3 --kernel-trace --stats`."""
    slab = make_slab(SIZES[0])
    slab.calc = EMT()
    g0 = -slab.get_forces().ravel()
    dc = slab.calc.device_calculator()
    x0 = slab.positions.ravel().copy()
    n = x0.size
    v0 = np.random.RandomState(0).normal(size=n)
    for _ in range(3):
        ctx.davidson(DeviceFdOperator(dc, x0, g0, 1e-4, False, None), n, v0, 1e-12, method='jd0', maxiter=a.maxiter)
        ctx.davidson(DeviceHvpOperator(dc, x0, None), n, v0, 1e-12, method='jd0', maxiter=a.maxiter)
    ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--products', type=int, default=64, help='products per timed window')
    ap.add_argument('--maxiter', type=int, default=24)
    ap.add_argument('--trace', action='store_true', help='only a few eigensolver calls of each kind (under rocprofv3)')
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
