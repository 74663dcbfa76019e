#!/usr/bin/env python3
"""Time the exact Hessian-vector product of positions and cell against the routes a cell run had before it; prints one
JSON line per size and a markdown table.

    python tools/cell_hvp_bench.py [--reps R] [--warmup W] [--k K] [--sizes 4,6] [--out FILE]

On jittered bulk Cu (rep^3 conventional fcc cells, 27 periodic images; rep = 4: N = 256, rep = 6: N = 864), host clock
around calls that end in a stream synchronisation, all of them alternated in one process after a warm-up of each:

  cell_hvp    (a) `calc.cell_hessian_vector_product` with K vectors (`sella_emt_cell_hvp`: upload of V and the image
                  tables, density pass, F2, dots, gather, finish, read-back)
  cell_hvp_1      the same K products one vector at a time through `CellCartesianPES._hvp`, the way `PES.diag` asks for
                  them (J and G of the geometry cached)
  hvp         (b) `calc.hessian_vector_product` with K vectors: the product at fixed cell, the floor
  fd          (c) K finite-difference products through `CellCartesianPES`: `NumericalHessian` over `_calc_eg` (set_x ->
                  expm -> set_cell, a fresh image set-up, one force-and-virial pass per product), the route `diag` took
                  in a cell run before
  dense       (d) `calc.get_device_cell_hessian` of a geometry not seen before (the dense (3N + 9)-square Hessian)
Each sample is the time of the whole batch of K products (or the one dense Hessian); median, minimum, maximum and the
quartiles over the repetitions are reported.  The products of (a) are checked against the dense Hessian of (d)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sella_amd.atoms import EMT, Atoms  # noqa: E402
from sella_amd.device import get_context  # noqa: E402
from sella_amd.linalg import NumericalHessian  # noqa: E402
from sella_amd.peswrapper import CellCartesianPES  # noqa: E402


def bulk(rep, a=3.6, jitter=0.05, seed=1):
    basis = np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])
    pos = np.array([(b + [i, j, k]) * a for i in range(rep) for j in range(rep) for k in range(rep) for b in basis])
    at = Atoms(['Cu'] * len(pos), pos, cell=np.eye(3) * a * rep, pbc=True)
    at.positions += jitter * np.random.RandomState(seed).normal(size=at.positions.shape)
    at.calc = EMT()
    return at


def measure(rep, k, reps, warmup):
    ctx = get_context()
    at = bulk(rep)
    calc = at.calc
    n = at.positions.size
    rng = np.random.RandomState(0)
    V = rng.normal(size=(k, n + 9))
    pes = CellCartesianPES(at, cell_hessian_vector_product=True)
    pes.get_g()
    Ufree = pes.get_Ufree()
    Vp = rng.normal(size=(k, pes.dim))
    Vfree = rng.normal(size=(k, Ufree.shape[1]))
    pes._hvp(Vp[:1])                                       # J, G of this geometry
    x0 = at.positions.copy()
    moved = [0]

    def fd():
        op = NumericalHessian(pes._calc_eg, pes.get_x(), pes.get_g(), pes.eta, False, Ufree)
        for v in Vfree:
            op.dot(v)

    def dense():
        moved[0] += 1                                      # a geometry of its own: the calculator caches per geometry
        at.positions = x0 + 1e-9 * moved[0]
        calc.get_device_cell_hessian(at).free()
        at.positions = x0

    def one_at_a_time():
        for v in Vp:
            pes._hvp(v[None, :])

    calls = dict(cell_hvp=lambda: calc.cell_hessian_vector_product(at, V), cell_hvp_1=one_at_a_time,
                 hvp=lambda: calc.hessian_vector_product(at, V[:, :n]), fd=fd, dense=dense)
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    samples = {name: [] for name in calls}
    for _ in range(reps):                                  # alternated: all see the same machine state
        for name, fn in calls.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            samples[name].append(time.perf_counter() - t0)
    out = dict(device=ctx.name, natoms=n // 3, nimages=len(calc._setup[1]['shifts']), k=k, reps=reps, warmup=warmup)
    for name, ts in samples.items():
        ts = 1e3 * np.array(ts)
        q1, med, q3 = np.percentile(ts, [25, 50, 75])
        out[name] = dict(median_ms=float(med), min_ms=float(ts.min()), max_ms=float(ts.max()), q1_ms=float(q1), q3_ms=float(q3))
    H = calc.get_cell_hessian(at)
    HV = calc.cell_hessian_vector_product(at, V)
    out['max_abs_err_vs_dense'] = float(np.abs(HV - V @ H).max())
    out['err_bound'] = float(2 * (n + 9) * np.finfo(float).eps * np.abs(H).sum(axis=1).max() * np.abs(V).max())
    med = {name: out[name]['median_ms'] for name in calls}
    out['fd_over_cell_hvp'] = med['fd'] / med['cell_hvp']
    out['fd_over_cell_hvp_1'] = med['fd'] / med['cell_hvp_1']
    out['cell_hvp_over_hvp'] = med['cell_hvp'] / med['hvp']
    out['dense_over_cell_hvp'] = med['dense'] / med['cell_hvp']
    return out


def table(results):
    names = ('cell_hvp', 'cell_hvp_1', 'hvp', 'fd', 'dense')
    lines = ['| N | k | ' + ' | '.join(f'{name} ms (min .. max; quartiles)' for name in names) + ' | fd / cell_hvp | cell_hvp / hvp | dense / cell_hvp |',
             '|---|---|' + '---|' * (len(names) + 3)]
    for r in results:
        cells = [f"{r[m]['median_ms']:.3f} ({r[m]['min_ms']:.3f} .. {r[m]['max_ms']:.3f}; {r[m]['q1_ms']:.3f}, {r[m]['q3_ms']:.3f})"
                 for m in names]
        lines.append(f"| {r['natoms']} | {r['k']} | " + ' | '.join(cells)
                     + f" | {r['fd_over_cell_hvp']:.1f} | {r['cell_hvp_over_hvp']:.2f} | {r['dense_over_cell_hvp']:.2f} |")
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--sizes', default='4,6', help='conventional cells per edge (4: N = 256, 6: N = 864)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    results = []
    for rep in (int(s) for s in a.sizes.split(',')):
        results.append(measure(rep, a.k, a.reps, a.warmup))
        print(json.dumps(results[-1]), flush=True)
    print(table(results), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(results, f, indent=1)
    slower = [r['natoms'] for r in results if not r['cell_hvp']['median_ms'] < r['fd']['median_ms']]
    if slower:
        sys.exit(f'the exact product is not faster than the finite-difference route at N = {slower}')


if __name__ == '__main__':
    main()
