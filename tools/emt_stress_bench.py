"""EMT with and without the virial, and a full cell relaxation; prints one JSON line.

    python tools/emt_stress_bench.py [--reps R] [--warmup W]

  emt_eval / emt_eval_stress  ms per call on the 1024-atom Cu(111) slab of bench.py and on a 4 x 4 x 4 fcc Cu bulk
                              (256 atoms), the two alternated in one process after a warm-up of each (host clock around
                              calls that end in a stream synchronise: sella_emt_eval* wait for their read-back)
  cell relaxation             Sella(order=0, optimize_cell=True) on the 256-atom bulk from a strained, jittered start:
                              steps, ms per optimizer step, final stress
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sella_amd import Sella  # noqa: E402
from sella_amd.atoms import EMT, Atoms  # noqa: E402
from sella_amd.device import get_context  # noqa: E402
from tools.emt_slab_opt import make_slab  # noqa: E402  (bench.py's 1024-atom slab)


def fcc_bulk(a, rep):
    basis = np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])
    pos = np.array([(b + [i, j, k]) * a for i in range(rep) for j in range(rep) for k in range(rep) for b in basis])
    return Atoms(['Cu'] * len(pos), pos, cell=np.eye(3) * a * rep, pbc=True)


def time_calls(atoms, reps, warmup):
    ctx = get_context()
    calc = EMT()
    atoms.calc = calc
    atoms.get_potential_energy()                           # set-up (parameter table, shift list)
    S = calc._setup[1]
    args = (atoms.positions, S['par'], S['shifts'], S['rc'], S['acut'], S['cutoff'], EMT._BETA)
    calls = dict(emt_eval=lambda: ctx.emt_eval(*args), emt_eval_stress=lambda: ctx.emt_eval_stress(*args))
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    total = dict.fromkeys(calls, 0.0)
    for _ in range(reps):                                  # alternated: both see the same machine state
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            total[name] += time.perf_counter() - t0
    e0, g0 = calls['emt_eval']()
    e1, g1, _ = calls['emt_eval_stress']()
    return {f'{k}_ms': 1e3 * v / reps for k, v in total.items()} | dict(
        natoms=len(atoms), nimages=len(S['shifts']), same_energy_gradient=bool(e0 == e1 and np.array_equal(g0, g1)))


def relax(seed=0):
    rng = np.random.RandomState(seed)
    at = fcc_bulk(3.70, 4)
    eps = 0.01 * rng.normal(size=(3, 3))
    at.set_cell(at.cell @ (np.eye(3) + 0.5 * (eps + eps.T)).T, scale_atoms=True)
    at.positions += 0.02 * rng.normal(size=at.positions.shape)
    at.calc = EMT()
    opt = Sella(at, order=0, optimize_cell=True, logfile=None)
    opt.converged()                                        # first force call outside the timed window
    t0 = time.perf_counter()
    conv = opt.run(fmax=1e-3, steps=300)
    dt = time.perf_counter() - t0
    return dict(converged=bool(conv), steps=int(opt.nsteps), ms_per_step=1e3 * dt / max(opt.nsteps, 1),
                force_calls=int(at.calc.ncalls), max_abs_stress=float(np.abs(at.get_stress()).max()),
                edge=float(np.linalg.norm(at.cell, axis=1).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    out = dict(device=get_context().name)
    out['slab1024'] = time_calls(make_slab(), a.reps, a.warmup)
    out['bulk256'] = time_calls(fcc_bulk(3.61, 4), a.reps, a.warmup)
    out['relax_bulk256'] = relax()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
