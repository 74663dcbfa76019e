#!/usr/bin/env python3
"""Time the analytic EMT Hessian and Hessian-vector product against the force call and against the central-difference
Hessian they replace; prints one JSON line.

    python tools/emt_hessian_bench.py [--reps R] [--warmup W] [--k K] [--fd-columns C] [--out FILE]

On the 1024-atom Cu(111) slab of bench.py (9 periodic images), host clock around calls that end in a stream
synchronisation, all of them alternated in one process after a warm-up of each:

  force_ms        one `sella_emt_eval` (upload, density and force pass, read-back)
  hessian_ms      one `sella_emt_hessian` (density pass, F2, pair blocks + G, rank-N product, symmetrisation; the result
                  stays on the device), and its parts from the library's own launch profile: the product
                  (`gemm_ms`, PROF_GEMM) against everything else
  hvp_ms          one `sella_emt_hvp` with K vectors (upload of V, three passes, read-back of H V)
  cell_hessian_ms one `sella_emt_cell_hessian` (the passes of the Hessian into the (3N + 9)-wide result, then the cell
                  pass, the 3N x N x 9 product and the finishing launch); `cell_over_hessian` is its ratio to
                  hessian_ms of the same run
  refine_ms       the 18 `sella_emt_eval_stress` calls that `refine_initial_hessian` spends on the nine cell columns
                  (central differences of force + stress), as one sample
  fd_hessian_ms   the central-difference Hessian: 2 x 3N calls of `sella_emt_eval` at displaced geometries, the
                  difference quotients written into a host array, symmetrised and uploaded.  With --fd-columns C < 3N
                  only C columns are measured and the total is C-column time x 3N / C (the calls are identical in
                  cost); the default measures all 3N.
The analytic Hessian is checked against the measured columns of the central-difference one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sella_amd.atoms import EMT  # noqa: E402
from sella_amd.device import get_context  # noqa: E402
from tools.emt_slab_opt import make_slab  # noqa: E402  (bench.py's 1024-atom slab)

PROF_GEMM = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--fd-columns', type=int, default=0, help='columns of the central-difference Hessian to measure (0: all)')
    ap.add_argument('--fd-step', type=float, default=1e-3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = get_context()
    slab = make_slab()
    calc = EMT()
    slab.calc = calc
    slab.get_potential_energy()                            # set-up (parameter table, shift list)
    S = calc._setup[1]
    pos = slab.positions.copy()
    args = (S['par'], S['shifts'], S['rc'], S['acut'], S['cutoff'], EMT._BETA)
    n = pos.size
    V = np.random.RandomState(0).normal(size=(a.k, n))

    def hessian():
        ctx.emt_hessian(pos, *args).free()

    cell = np.array(slab.cell, dtype=np.float64)

    def cell_hessian():
        ctx.emt_cell_hessian(pos, args[0], args[1], cell, *args[2:]).free()

    def refine():
        for _ in range(18):
            ctx.emt_eval_stress(pos, *args)

    calls = dict(force=lambda: ctx.emt_eval(pos, *args), hessian=hessian, hvp=lambda: ctx.emt_hvp(pos, *args, V),
                 cell_hessian=cell_hessian, refine=refine)
    for fn in calls.values():
        for _ in range(a.warmup):
            fn()
    samples = {name: [] for name in calls}
    for _ in range(a.reps):                                # alternated: all see the same machine state
        for name, fn in calls.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            samples[name].append(time.perf_counter() - t0)
    out = dict(device=ctx.name, natoms=n // 3, nimages=len(S['shifts']), k=a.k, reps=a.reps)
    for name, ts in samples.items():
        out[f'{name}_ms'] = 1e3 * float(np.median(ts))
        out[f'{name}_ms_min'] = 1e3 * float(np.min(ts))
    # the rank-N product inside the Hessian, from the launch profile (kernel time of the dispatch itself)
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(a.reps):
        hessian()
    ctx.sync()
    gemm = ctx.prof_get(PROF_GEMM)
    ctx.prof_enable(False)
    out['gemm_ms'] = gemm['ms'] / max(gemm['launches'], 1)
    out['gemm_tflops'] = 1e-9 * gemm['flops'] / gemm['ms'] if gemm['ms'] > 0 else None
    # the central-difference Hessian on the force call alone
    cols = n if a.fd_columns <= 0 else min(a.fd_columns, n)
    pick = np.arange(n) if cols == n else np.sort(np.random.RandomState(1).choice(n, cols, replace=False))
    Hfd = np.zeros((n, cols))
    x = pos.ravel().copy()
    ctx.sync()
    t0 = time.perf_counter()
    for q, i in enumerate(pick):
        x[i] += a.fd_step
        gp = ctx.emt_eval(x.reshape(-1, 3), *args)[1].ravel()
        x[i] -= 2 * a.fd_step
        gm = ctx.emt_eval(x.reshape(-1, 3), *args)[1].ravel()
        x[i] = pos.ravel()[i]
        Hfd[:, q] = (gp - gm) / (2 * a.fd_step)
    t_cols = time.perf_counter() - t0
    t_up = 0.0
    if cols == n:
        t0 = time.perf_counter()
        ctx.upload(0.5 * (Hfd + Hfd.T)).free()
        ctx.sync()
        t_up = time.perf_counter() - t0
    out['fd_columns'] = int(cols)
    out['fd_hessian_ms'] = 1e3 * (t_cols * n / cols + t_up)
    out['fd_upload_ms'] = 1e3 * t_up if cols == n else None
    H = ctx.emt_hessian(pos, *args)
    Hn = H.numpy()
    H.free()
    out['max_abs_hessian'] = float(np.abs(Hn).max())
    out['max_diff_vs_fd'] = float(np.abs(Hn[:, pick] - Hfd).max())
    out['hvp_over_force'] = out['hvp_ms'] / out['force_ms']
    out['hessian_over_force'] = out['hessian_ms'] / out['force_ms']
    out['fd_over_hessian'] = out['fd_hessian_ms'] / out['hessian_ms']
    out['cell_over_hessian'] = out['cell_hessian_ms'] / out['hessian_ms']
    out['cell_over_hessian_min'] = out['cell_hessian_ms_min'] / out['hessian_ms_min']
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
