#!/usr/bin/env python3
"""Time the pair-potential calculator (`sella_pair_eval`, the resident Hessian-vector operator of kind 2) next to EMT on
the same geometry; prints one JSON line per size.

    python tools/pair_bench.py [--reps R] [--warmup W] [--calls P] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pair_bench.py --trace      # kernel times, a run of its own

fcc Cu bulk, a = 3.6, jitter 0.05 A: 4 x 4 x 4 conventional cells (256 atoms) and 4 x 8 x 8 (1024), periodic, 27 images
for both potentials; Morse with `PeriodicMorse`'s parameters and rcut = 6.  Every window is a host clock around P calls that
each end in a stream synchronisation; all variants are warmed up first and then alternated in one process, `reps` windows
each; per call the median and the spread (min, max, interquartile range).

  pair_eval    `sella_pair_eval`: upload of the positions, one pass, read-back, wait
  emt_eval     `sella_emt_eval`: the same with the density and the force pass
  pair_op1     `sella_hvp_matvec` on the pair operator: upload of v, one gather pass on the kept visits, read-back, wait
  emt_op1      the same on the EMT operator (dots and gather pass)
  pair_op16    `sella_hvp_apply_block` with 16 rows on the pair operator
  emt_op16     the same on the EMT operator
  host_morse   `PeriodicMorse.energy_and_gradient` (NumPy on the host, minimum image), for context; `--host-reps` windows of one call
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sella_amd import _lib  # noqa: E402
from sella_amd._lib import ptr  # noqa: E402
from sella_amd.atoms import EMT, Atoms, Morse, PeriodicMorse  # noqa: E402
from sella_amd.device import DeviceHvpOperator, get_context  # noqa: E402

SIZES = [(4, 4, 4), (4, 8, 8)]
MORSE = dict(D=0.3429, a=1.3588, r0=2.866)
RCUT = 6.0


def bulk(reps, a=3.6, jitter=0.05, seed=0):
    basis = np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])
    pos = np.array([(b + [i, j, k]) * a for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2]) for b in basis])
    pos += jitter * np.random.RandomState(seed).normal(size=pos.shape)
    return Atoms(['Cu'] * len(pos), pos, cell=np.diag(np.array(reps, dtype=float) * a), pbc=True)


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


def setup(ctx, reps):
    at = bulk(reps)
    pair_at, emt_at = at.copy(), at.copy()
    pair_at.calc, emt_at.calc = Morse(**MORSE, rcut=RCUT), EMT()
    pair_at.get_potential_energy()
    emt_at.get_potential_energy()
    return at, pair_at, emt_at


def measure(ctx, reps, a):
    at, pair_at, emt_at = setup(ctx, reps)
    pos = at.positions.copy()
    x0 = pos.ravel().copy()
    n = x0.size
    pair_args = pair_at.calc._pair_args(pos)
    S = emt_at.calc._setup[1]
    emt_args = (pos, S['par'], S['shifts'], S['rc'], S['acut'], S['cutoff'], EMT._BETA)
    ops = dict(pair=DeviceHvpOperator(pair_at.calc.device_calculator(), x0), emt=DeviceHvpOperator(emt_at.calc.device_calculator(), x0))
    rng = np.random.RandomState(1)
    v = rng.normal(size=n)
    V16 = rng.normal(size=(16, n))
    out1, out16 = np.empty(n), np.empty((16, n))
    L = _lib.lib()
    P = a.calls

    def repeat(fn):
        def window():
            for _ in range(P):
                fn()
        return window

    calls = dict(
        pair_eval=repeat(lambda: ctx.pair_eval(*pair_args)),
        emt_eval=repeat(lambda: ctx.emt_eval(*emt_args)),
        pair_op1=repeat(lambda: L.sella_hvp_matvec(ops['pair']._h, ptr(v), ptr(out1), n)),
        emt_op1=repeat(lambda: L.sella_hvp_matvec(ops['emt']._h, ptr(v), ptr(out1), n)),
        pair_op16=repeat(lambda: L.sella_hvp_apply_block(ops['pair']._h, ptr(V16), 16, ptr(out16))),
        emt_op16=repeat(lambda: L.sella_hvp_apply_block(ops['emt']._h, ptr(V16), 16, ptr(out16))),
    )
    samples = alternate(ctx, calls, a.warmup, a.reps)
    res = dict(device=ctx.name, natoms=len(at), nimages_pair=len(pair_args[3]), nimages_emt=len(S['shifts']), rcut=RCUT,
               emt_cutoff=float(S['cutoff']), calls_per_window=P, reps=a.reps)
    for name, ts in samples.items():
        res[f'{name}_ms'] = spread(np.array(ts) / P)
    host = PeriodicMorse(rcut=RCUT)
    host.cell, host.pbc = np.asarray(at.cell, dtype=float), np.asarray(at.pbc, dtype=bool)
    ts = []
    for _ in range(a.host_reps + 1):
        t0 = time.perf_counter()
        host.energy_and_gradient(pos)
        ts.append(time.perf_counter() - t0)
    res['host_morse_ms'] = spread(np.array(ts[1:]))
    return res


def trace(ctx, a):
    """A few calls of each kind at 1024 atoms, for `rocprofv3 --kernel-trace --stats`."""
    at, pair_at, emt_at = setup(ctx, SIZES[1])
    x0 = at.positions.ravel().copy()
    pair_op = DeviceHvpOperator(pair_at.calc.device_calculator(), x0)
    emt_op = DeviceHvpOperator(emt_at.calc.device_calculator(), x0)
    rng = np.random.RandomState(1)
    v, V16 = rng.normal(size=x0.size), rng.normal(size=(16, x0.size))
    for _ in range(5):
        pair_at.calc.energy_and_gradient(at.positions)
        emt_at.calc.energy_and_gradient(at.positions)
        for op in (pair_op, emt_op):
            op.apply(v)
            op.apply_block(V16)
    ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=32, help='calls per timed window')
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--trace', action='store_true', help='only a few calls of each kind (under rocprofv3)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = get_context()
    if a.trace:
        trace(ctx, a)
        return
    results = []
    for reps in SIZES:
        res = measure(ctx, reps, a)
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
