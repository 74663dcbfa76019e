"""Whole searches on the device pair potentials (`Morse`, `LennardJones`; csrc/pair.hip, calc.hip kind 2): the reference's
integration case (tests/integration/test_morse_cluster.py) with its own assertions, the library loop on the LJ13
cluster, a cell run, and a cohort — the routes a calculator gets by living in the library."""
import numpy as np
import pytest

from test_cell_optimization import fcc_cubic
from test_pair_potential import E_LJ13, c13

KB = 8.617333262e-5
XE = dict(D=226.9 * KB, a=1.099 / 4.73, r0=4.73)        # DOI 10.1515/zna-1987-0505, as the reference's test has them


def xe4(calc):
    from sella_amd.atoms import Atoms
    at = Atoms(['Xe'] * 4, np.random.RandomState(4).normal(size=(4, 3), scale=3.0), pbc=False)
    at.calc = calc
    return at


def run_reference_case(at, internal, order, **kw):
    """The reference's test body; returns (optimizer, energy, negative projected eigenvalues)."""
    from sella_amd import Sella
    from sella_amd.internal import Constraints
    cons = Constraints(at)
    cons.fix_translation()
    cons.fix_rotation()
    opt = Sella(at, order=order, internal=internal, gamma=1e-3, constraints=cons, logfile=None, **kw)
    opt.run(fmax=1e-3)
    Ufree = opt.pes.get_Ufree()
    np.testing.assert_allclose(opt.pes.get_g() @ Ufree, 0, atol=5e-3)
    opt.pes.diag(gamma=1e-16)
    H = opt.pes.get_HL().project(Ufree)
    nneg = int(np.sum(H.evals < 0))
    assert nneg == order, H.evals
    return opt, at.get_potential_energy(), nneg


# ---- 6a. the reference's integration case -------------------------------------------------------------------------------
HEAVY = pytest.mark.emu_heavy                            # 25 - 60 s each fibre by fibre; (False, 0) stays on the emulator


@pytest.mark.parametrize('internal,order', [(False, 0), pytest.param(False, 1, marks=HEAVY), pytest.param(True, 0, marks=HEAVY),
                                            pytest.param(True, 1, marks=HEAVY)])
def test_morse_cluster(ctx, internal, order):
    from sella_amd.atoms import Morse, MorseCluster
    opt, e, nneg = run_reference_case(xe4(Morse(**XE)), internal, order)
    # the same run on the host calculator, on the same backend
    opt_h, e_h, nneg_h = run_reference_case(xe4(MorseCluster(**XE)), internal, order)
    print(f'internal={internal} order={order}: E {e:.10f} (host {e_h:.10f})  steps {opt.nsteps} ({opt_h.nsteps})  '
          f'force calls {opt.pes.neval} ({opt_h.pes.neval})')
    assert abs(e - e_h) <= 1e-8 and nneg == nneg_h


@HEAVY
def test_morse_saddle_with_exact_products(ctx):
    from sella_amd.atoms import Morse
    fd, e_fd, _ = run_reference_case(xe4(Morse(**XE)), False, 1)
    assert fd.pes.nhvp == 0
    hvp, e_hvp, _ = run_reference_case(xe4(Morse(**XE)), False, 1, hessian_vector_product=True)
    print(f'finite differences: {fd.pes.neval} force calls; exact products: {hvp.pes.neval} force calls, {hvp.pes.nhvp} products')
    assert hvp.pes.nhvp > 0
    assert hvp.pes.neval <= fd.pes.neval


# ---- 6b. the library loop on LJ13 -----------------------------------------------------------------------------------------
@pytest.fixture
def structured_from_39():
    from sella_amd import linalg
    old = linalg.LR_MIN_DIM
    linalg.LR_MIN_DIM = 39
    yield
    linalg.LR_MIN_DIM = old


def lj13_minimisation(lib, seed=1):
    from sella_amd import Sella
    from sella_amd.atoms import LennardJones
    from sella_amd.internal import Constraints
    at = c13(seed=seed)
    at.calc = LennardJones()
    # (no constraint on the centre or the orientation: the library loop covers pinned coordinates only)
    opt = Sella(at, order=0, logfile=None, constraints=Constraints(at), proj_trans=False, proj_rot=False)
    assert opt._lib_kw is not None                                     # qualifies for the library loop
    opt.use_library_loop = lib
    return at, opt


@pytest.mark.emu_heavy
def test_lj13_in_and_out_of_the_library_loop(ctx, structured_from_39, monkeypatch):
    from sella_amd.search import LibrarySearch
    entered = []
    real = LibrarySearch.run
    monkeypatch.setattr(LibrarySearch, 'run', lambda self, *a, **k: entered.append(self.atoms) or real(self, *a, **k))
    a1, o1 = lj13_minimisation(True)
    a2, o2 = lj13_minimisation(False)
    assert o1.run(fmax=1e-4, steps=200) and o2.run(fmax=1e-4, steps=200)
    assert entered == [a1] and o2._lib is None                         # one ran inside the library, the other never did
    n1, n2 = o1.nsteps, o2.nsteps
    print(f'steps {n1} / {n2}  force calls {a1.calc.ncalls} / {a2.calc.ncalls}  E {a1.get_potential_energy():.9f}')
    assert n1 == n2 and a1.calc.ncalls == a2.calc.ncalls
    assert o1.pes.neval == o2.pes.neval
    assert abs(a1.get_potential_energy() - E_LJ13) <= 1e-6 and abs(a2.get_potential_energy() - E_LJ13) <= 1e-6


# ---- 6c. a cell run ---------------------------------------------------------------------------------------------------------
@HEAVY
def test_cell_run_on_morse_bulk(ctx, monkeypatch):
    """fcc bulk of the Morse potential with `PeriodicMorse`'s parameters (rcut 6, 27 images), 2 x 2 x 2 conventional cells,
    the lattice constant 3 % above 3.6: positions and cell relax together, the stress served by the device
    (`sella_pair_eval_stress`)."""
    from sella_amd import Sella
    from sella_amd.atoms import Morse
    from sella_amd.device import Context
    from test_pair_potential import MORSE_CU
    served = []
    real = Context.pair_eval_stress
    monkeypatch.setattr(Context, 'pair_eval_stress', lambda self, *a: served.append(1) or real(self, *a))
    at = fcc_cubic('Cu', 1.03 * 3.6, 2)
    at.positions += 0.02 * np.random.RandomState(9).normal(size=at.positions.shape)
    at.calc = Morse(**MORSE_CU, rcut=6.0)
    e0, s0 = at.get_potential_energy(), at.get_stress()
    smax = 1e-3
    opt = Sella(at, order=0, optimize_cell=True, smax=smax, logfile=None)
    assert opt.run(fmax=1e-3, steps=300)
    done, worst_force, _, worst_cell = opt.pes.converged(1e-3, smax=smax)
    stress = at.get_stress()
    print(f'steps {opt.nsteps}  E {e0:.6f} -> {at.get_potential_energy():.6f}  a {at.cell[0, 0] / 2:.5f}  '
          f'largest cell gradient {worst_cell:.2e}  stress {s0[:3]} -> {stress[:3]}')
    assert done and worst_cell < smax                                   # smax is met
    assert np.abs(stress[:3]).max() < smax < np.abs(s0[:3]).max()
    assert len(served) >= opt.nsteps                                    # get_stress was served by the device
    assert np.abs(at.get_forces()).max() < 1e-3 and at.get_potential_energy() < e0


# ---- 6d. a cohort -----------------------------------------------------------------------------------------------------------
def _member(i):
    from sella_amd.atoms import LennardJones
    from sella_amd.internal import Constraints
    at = c13(seed=11 + i)
    at.calc = LennardJones()
    return at, dict(constraints=Constraints(at))


@pytest.mark.emu_heavy
def test_cohort_of_four_lj13_members(ctx, structured_from_39):
    """Four LJ13 clusters from different jitters advanced in lockstep (one batched launch of the pair kernels for all of
    them): every member's summary and geometry equal its solo run's, bit for bit."""
    from sella_amd import ensemble
    kw = dict(order=0, proj_trans=False, proj_rot=False)
    steps = 6
    alone = [ensemble.run_one(_member(i), 0.0, steps, kw) for i in range(4)]
    with ensemble.EnsembleCohort(4) as cohort:
        res = ensemble.run_ensemble(_member, 4, fmax=0.0, steps=steps, sella_kwargs=kw, cohort=cohort)
        st = cohort.stats()
    for i in range(4):
        np.testing.assert_array_equal(res['summary'][i], alone[i][0])
        np.testing.assert_array_equal(res['positions'][i], alone[i][1])
    assert len({round(e, 9) for e in res['summary'][:, 2]}) == 4
    assert st['launches_issued'] < st['launches_asked']                 # the members' launches were merged
