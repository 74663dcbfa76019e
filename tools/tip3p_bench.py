#!/usr/bin/env python3
"""Time the TIP3P water calculator (`sella_tip3p_*`, the resident Hessian-vector operator of kind 3) next to the
Lennard-Jones pair potential at the same number of sites; prints one JSON line per size.

    python tools/tip3p_bench.py [--reps R] [--warmup W] [--calls P] [--out FILE]

256 (4 x 8 x 8) and 1000 (10 x 10 x 10) waters on a cubic lattice of spacing 3.104 A (liquid density) in a periodic box,
random orientations, jitter 0.05 A; rc = 5, width = 1.  `LennardJones(rcut=5)` runs on the same 768 / 3000 positions
(27 images).  Every window is a host clock around P calls that each end in a stream synchronisation; all variants are
warmed up first and then alternated in one process, `reps` windows each; per call the median and the spread (min, max,
interquartile range).  The dense Hessians are timed in windows of one call.

  tip3p_eval / lj_eval        the force call: upload of the positions, one pass, read-back, wait
  tip3p_hess / lj_hess        the dense Hessian, left on the device (allocation and release of the matrix included)
  tip3p_hvp16 / lj_hvp16      16 host vectors through `sella_tip3p_hvp` / `sella_pair_hvp` (the state built per call)
  tip3p_op1 / lj_op1          `sella_hvp_matvec` on the resident operator: upload of v, one pass over the kept visits, read-back
  tip3p_op16 / lj_op16        `sella_hvp_apply_block` with 16 rows on the resident operator
  host_numpy                  the force call of the NumPy yardstick of tests/test_tip3p.py, for context (one call)

`visits` counts the ordered molecule pairs inside rc; a product reads 548 bytes per visit (csrc/tip3p.h), `op1_GBps` and
`op16_GBps` are that traffic over the median time of a product (the 16 rows of a block share it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from sella_amd import _lib  # noqa: E402
from sella_amd._lib import ptr  # noqa: E402
from sella_amd.atoms import TIP3P, Atoms, LennardJones  # noqa: E402
from sella_amd.device import DeviceHvpOperator, get_context  # noqa: E402

SIZES = [(4, 8, 8), (10, 10, 10)]
SPACING = 3.104
RC, WIDTH = 5.0, 1.0
BYTES_PER_VISIT = 548


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


def liquid(shape):
    from sella_amd.atoms import angleHOH, rOH
    rng = np.random.RandomState(1)
    h = 0.5 * np.radians(angleHOH)
    mol = rOH * np.array([[0.0, 0.0, 0.0], [np.sin(h), np.cos(h), 0.0], [-np.sin(h), np.cos(h), 0.0]])
    pos = []
    for i in range(shape[0]):
        for j in range(shape[1]):
            for k in range(shape[2]):
                Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
                pos.append(mol @ Q.T + (np.array([i, j, k]) + 0.5) * SPACING)
    pos = np.concatenate(pos)
    pos += 0.05 * rng.uniform(-1.0, 1.0, size=pos.shape)
    box = np.array(shape, dtype=float) * SPACING
    return Atoms(['O', 'H', 'H'] * (len(pos) // 3), pos, cell=np.diag(box), pbc=True), box


def count_visits(pos, box):
    ox = pos[::3]
    d = ox[None, :, :] - ox[:, None, :]
    d -= box * np.rint(d / box)
    return int(((d * d).sum(axis=2) < RC * RC).sum() - len(ox))


def measure(ctx, shape, a):
    at, box = liquid(shape)
    pos = at.positions.copy()
    x0 = pos.ravel().copy()
    n = x0.size
    water, lj = at.copy(), at.copy()
    water.calc, lj.calc = TIP3P(rc=RC, width=WIDTH), LennardJones(rcut=RC)
    water.get_potential_energy()
    lj.get_potential_energy()
    targs, largs = water.calc._tip3p_args(pos), lj.calc._pair_args(pos)
    ops = dict(tip3p=DeviceHvpOperator(water.calc.device_calculator(), x0), lj=DeviceHvpOperator(lj.calc.device_calculator(), x0))
    rng = np.random.RandomState(1)
    v, V16 = rng.normal(size=n), rng.normal(size=(16, n))
    out1, out16 = np.empty(n), np.empty((16, n))
    L = _lib.lib()
    P = a.calls

    def repeat(fn):
        def window():
            for _ in range(P):
                fn()
        return window

    calls = dict(
        tip3p_eval=repeat(lambda: ctx.tip3p_eval(*targs)), lj_eval=repeat(lambda: ctx.pair_eval(*largs)),
        tip3p_hvp16=repeat(lambda: ctx.tip3p_hvp(*targs, V16)), lj_hvp16=repeat(lambda: ctx.pair_hvp(*largs, V16)),
        tip3p_op1=repeat(lambda: L.sella_hvp_matvec(ops['tip3p']._h, ptr(v), ptr(out1), n)),
        lj_op1=repeat(lambda: L.sella_hvp_matvec(ops['lj']._h, ptr(v), ptr(out1), n)),
        tip3p_op16=repeat(lambda: L.sella_hvp_apply_block(ops['tip3p']._h, ptr(V16), 16, ptr(out16))),
        lj_op16=repeat(lambda: L.sella_hvp_apply_block(ops['lj']._h, ptr(V16), 16, ptr(out16))),
    )
    samples = alternate(ctx, calls, a.warmup, a.reps)
    dense = dict(tip3p_hess=lambda: ctx.tip3p_hessian(*targs).free(), lj_hess=lambda: ctx.pair_hessian(*largs).free())
    dense_samples = alternate(ctx, dense, 1, a.dense_reps)
    visits = count_visits(pos, box)
    res = dict(device=ctx.name, waters=len(at) // 3, sites=len(at), box=box.tolist(), rc=RC, width=WIDTH, visits=visits,
               bytes_per_visit=BYTES_PER_VISIT, lj_images=len(largs[3]), calls_per_window=P, reps=a.reps,
               dense_reps=a.dense_reps)
    for name, ts in samples.items():
        res[f'{name}_ms'] = spread(np.array(ts) / P)
    for name, ts in dense_samples.items():
        res[f'{name}_ms'] = spread(np.array(ts))
    traffic = BYTES_PER_VISIT * visits
    res['op1_GBps'] = traffic / (1e-3 * res['tip3p_op1_ms']['median']) / 1e9
    res['op16_GBps'] = traffic / (1e-3 * res['tip3p_op16_ms']['median']) / 1e9
    if a.host:
        from test_tip3p import yardstick_calculator
        host = yardstick_calculator()(0, box, RC, WIDTH)
        t0 = time.perf_counter()
        host.energy_and_gradient(pos)
        res['host_numpy_ms'] = 1e3 * (time.perf_counter() - t0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--dense-reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=16, help='calls per timed window')
    ap.add_argument('--no-host', dest='host', action='store_false', help='skip the NumPy force call')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = get_context()
    results = []
    for shape in SIZES:
        res = measure(ctx, shape, a)
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
