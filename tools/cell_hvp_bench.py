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
  op_1        (e) K single products through the resident operator of positions and cell (`DeviceHvpOperator.for_cell`,
                  `sella_hvp_matvec` with host vectors), the operator made once outside the clock
  op_create       making that operator: density pass, F2, the image indices, J, G and P uploaded — once per geometry
  op_block    (f) one block product of K rows on it (`sella_hvp_apply_block`)
  diag_dev    (g) one whole `CellCartesianPES.diag(maxiter=K)` (at most K products) with
                  the first atom pinned, on the device route ...
  diag_host       ... and on the host route (`use_library_calculator = False`); two PES objects that see the same sequence
                  of calls, so repetition r of the one answers repetition r of the other
Each sample is the time of the whole batch of K products (or the one dense Hessian, operator or diagonalisation); median,
minimum, maximum and the quartiles over the repetitions are reported.  The products of (a) are checked against the dense
Hessian of (d), those of (f) against the same Hessian carried into the coordinates of the PES."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sella_amd.atoms import EMT, Atoms  # noqa: E402
from sella_amd.device import DeviceHvpOperator, get_context  # noqa: E402
from sella_amd.internal import Constraints  # noqa: E402
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

    J, G0, P = pes._cell_param_maps()
    dc = calc.device_calculator()
    op_args = (dc, at.positions.ravel().copy(), np.array(at.cell, dtype=float), J, 0.5 * (G0 + G0.T), P)
    op = DeviceHvpOperator.for_cell(*op_args)
    out1 = np.empty(pes.dim)

    def op_single():
        for v in Vp:
            out1[:] = op.apply(v)

    def pinned_pes(library):
        atoms = bulk(rep)
        cons = Constraints(atoms)
        cons.fix_translation(0)
        p = CellCartesianPES(atoms, cell_hessian_vector_product=True, constraints=cons)
        p.use_library_calculator = library
        p.get_g()
        return p
    pes_dev, pes_host = pinned_pes(True), pinned_pes(False)

    calls = dict(cell_hvp=lambda: calc.cell_hessian_vector_product(at, V), cell_hvp_1=one_at_a_time,
                 hvp=lambda: calc.hessian_vector_product(at, V[:, :n]), fd=fd, dense=dense,
                 op_1=op_single, op_create=lambda: DeviceHvpOperator.for_cell(*op_args), op_block=lambda: op.apply_block(Vp),
                 diag_dev=lambda: pes_dev.diag(maxiter=k), diag_host=lambda: pes_host.diag(maxiter=k))
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
    Hp = pes._convert_cell_hessian(H)
    out['op_block_max_abs_err_vs_dense'] = float(np.abs(op.apply_block(Vp) - Vp @ Hp).max())
    out['op_block_err_bound'] = float(2 * (pes.dim + 18) * np.finfo(float).eps * np.abs(Hp).sum(axis=1).max() * np.abs(Vp).max())
    out['diag_products'] = dict(dev=pes_dev.nhvp, host=pes_host.nhvp, calls=reps + warmup)
    med = {name: out[name]['median_ms'] for name in calls}
    out['cell_hvp_1_over_op_1'] = med['cell_hvp_1'] / med['op_1']
    out['diag_host_over_diag_dev'] = med['diag_host'] / med['diag_dev']
    out['fd_over_cell_hvp'] = med['fd'] / med['cell_hvp']
    out['fd_over_cell_hvp_1'] = med['fd'] / med['cell_hvp_1']
    out['cell_hvp_over_hvp'] = med['cell_hvp'] / med['hvp']
    out['dense_over_cell_hvp'] = med['dense'] / med['cell_hvp']
    return out


def table(results):
    names = ('cell_hvp', 'cell_hvp_1', 'hvp', 'fd', 'dense', 'op_1', 'op_create', 'op_block', 'diag_dev', 'diag_host')
    lines = ['| N | k | ' + ' | '.join(f'{name} ms (min .. max; quartiles)' for name in names) + ' | fd / cell_hvp | cell_hvp / hvp | dense / cell_hvp | cell_hvp_1 / op_1 | diag_host / diag_dev |',
             '|---|---|' + '---|' * (len(names) + 5)]
    for r in results:
        cells = [f"{r[m]['median_ms']:.3f} ({r[m]['min_ms']:.3f} .. {r[m]['max_ms']:.3f}; {r[m]['q1_ms']:.3f}, {r[m]['q3_ms']:.3f})"
                 for m in names]
        lines.append(f"| {r['natoms']} | {r['k']} | " + ' | '.join(cells)
                     + f" | {r['fd_over_cell_hvp']:.1f} | {r['cell_hvp_over_hvp']:.2f} | {r['dense_over_cell_hvp']:.2f}"
                     + f" | {r['cell_hvp_1_over_op_1']:.1f} | {r['diag_host_over_diag_dev']:.2f} |")
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
    # the resident operator: its single products against the one-at-a-time route (the spreads must not touch), and the whole
    # diagonalisation against the host route
    slower = [r['natoms'] for r in results if not r['op_1']['max_ms'] < r['cell_hvp_1']['min_ms']]
    if slower:
        sys.exit(f'single products on the resident operator are not clear of the one-at-a-time route at N = {slower}')
    slower = [r['natoms'] for r in results if not r['diag_dev']['median_ms'] < r['diag_host']['median_ms']]
    if slower:
        sys.exit(f'diag() on the device route is not faster than on the host route at N = {slower}')


if __name__ == '__main__':
    main()
