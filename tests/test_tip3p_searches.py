"""The reference's second integration case (tests/integration/test_tip3p_cluster.py) on the device `TIP3P` calculator
(csrc/tip3p.hip, calc.hip kind 3): eight rigid waters — both O-H bonds and the H-O-H angle of every molecule held at their
targets, net translation and rotation removed — minimised in TRIC internal coordinates with fragments and in Cartesian
coordinates, rattled and minimised again, with the reference's own assertions at the end.

The same case runs on the NumPy yardstick of test_tip3p.py.  A water octamer has many minima, so the two runs need not end
in the same one: instead the device calculator is evaluated at the geometry the yardstick run ends at, and energy and
gradient are held to the forward-error bounds of test_tip3p.py there.

The reference's body is transcribed with its `opt.delta = 0.05` and ASE's default second rattle.  The run ends by the largest
projected Cartesian force on an atom, while the final assertion bounds the components of the gradient in the TRIC
coordinates, where a fragment's rotation collects the torque of its three atoms: the two measures are the reference's own
and differ by a factor of 0.5 to 1.5 between runs.

Measured, internal: 80 + 2 steps and 126 force calls on both calculators and both backends, E = -2.64237925 eV, max
|g @ Ufree| 6.9e-4 (device calculator) and 7.8e-4 (yardstick) on the device, 7.6e-4 and 7.7e-4 on the emulator.  Cartesian, on
the device: 58 + 4 steps, 106 force calls, E = -2.69320422 eV, max |g @ Ufree| 4.5e-4 and 4.4e-4."""
import numpy as np
import pytest

from test_tip3p import bounds, case_atoms, make_case, report, yardstick

HEAVY = pytest.mark.emu_heavy                            # whole searches: tens of seconds each fibre by fibre


def constrained(at):
    from sella_amd.atoms import angleHOH, rOH
    from sella_amd.internal import Constraints, DuplicateConstraintError
    cons = Constraints(at)
    for i in range(len(at) // 3):
        cons.fix_bond((3 * i, 3 * i + 1), target=rOH)
        cons.fix_bond((3 * i, 3 * i + 2), target=rOH)
        cons.fix_angle((3 * i + 1, 3 * i, 3 * i + 2), target=angleHOH)
    for fix in (cons.fix_translation, cons.fix_rotation):               # tolerated, as in the reference
        try:
            fix()
        except DuplicateConstraintError:
            pass
    return cons


def optimizer(at, internal):
    """The reference's optimizer for the case: order 0, eta 1e-6, delta0 1e-2, and its `opt.delta = 0.05` before the run."""
    from sella_amd import Sella
    from sella_amd.internal import InternalCoordinates
    cons = constrained(at)
    kw = dict(order=0, eta=1e-6, delta0=1e-2, logfile=None)
    if internal:
        kw['internal'] = InternalCoordinates.from_atoms(at, cons=cons, allow_fragments=True)
    else:
        kw['constraints'] = cons
    opt = Sella(at, **kw)
    opt.delta = 0.05
    return opt


def run_reference_case(at, internal):
    """The reference's test body (it runs order 0 only); returns the optimizer.  The jitter of 0.01 of `w8` is its
    `rattle(0.01)` before the first run; the second rattle is ASE's default one, 0.001 from RandomState(42)."""
    opt = optimizer(at, internal)
    opt.run(fmax=1e-3)
    first = opt.nsteps
    at.set_positions(at.positions + 0.001 * np.random.RandomState(42).normal(size=at.positions.shape))
    opt.run(fmax=1e-3)
    Ufree = opt.pes.get_Ufree()
    g = opt.pes.get_g() @ Ufree
    print(f'{type(at.calc).__name__} internal={internal}: steps {first} + {opt.nsteps - first}  '
          f'max |g @ Ufree| {np.abs(g).max():.3e}')
    np.testing.assert_allclose(g, 0, atol=1e-3)
    opt.pes.diag(gamma=1e-16)
    H = opt.pes.get_HL().project(Ufree)
    assert np.sum(H.evals < 0) == 0, H.evals
    opt.first_run = first
    return opt


@pytest.mark.parametrize('internal,steps', [(False, 3), (True, 2)], ids=['cartesian', 'internal'])
def test_first_steps_follow_the_yardstick(ctx, internal, steps):
    """The lighter test that stays on the emulator: the first steps of the same case on the device calculator and on the
    yardstick (two in internal coordinates, where a step takes ten seconds fibre by fibre).  Both are the same algorithm on
    energies and gradients that agree to rounding, so the geometries agree far below the step length afterwards, the energy
    has gone down and the constraints are closer to their targets."""
    at = case_atoms('w8')
    ref = make_case('w8')[0]
    ref.calc = yardstick('w8')
    e0 = at.get_potential_energy()
    opts = [optimizer(a, internal) for a in (at, ref)]
    res0 = float(np.linalg.norm(opts[0].pes.get_res()))
    for opt in opts:
        opt.run(fmax=1e-3, steps=steps)
    res = float(np.linalg.norm(opts[0].pes.get_res()))
    moved = float(np.abs(at.positions - make_case('w8')[0].positions).max())
    apart = float(np.abs(at.positions - ref.positions).max())
    print(f'internal={internal}: {steps} steps moved an atom by up to {moved:.3e}, device and yardstick runs {apart:.3e} apart; '
          f'E {e0:.6f} -> {at.get_potential_energy():.6f}  constraint residual {res0:.2e} -> {res:.2e}')
    assert opts[0].nsteps == opts[1].nsteps == steps and opts[0].pes.neval == opts[1].pes.neval
    assert moved > 1e-3 and apart < 1e-8
    assert at.get_potential_energy() < e0 and res < res0


@pytest.mark.parametrize('internal', [pytest.param(False, marks=HEAVY, id='cartesian'),
                                      pytest.param(True, marks=HEAVY, id='internal')])
def test_tip3p_cluster(ctx, internal):
    from sella_amd.atoms import angleHOH, rOH
    at = case_atoms('w8')
    opt = run_reference_case(at, internal)
    pos = at.positions.reshape(-1, 3, 3)
    oh = np.linalg.norm(pos[:, 1:] - pos[:, :1], axis=2)
    cosang = ((pos[:, 1] - pos[:, 0]) * (pos[:, 2] - pos[:, 0])).sum(axis=1) / (oh[:, 0] * oh[:, 1])
    assert np.abs(oh - rOH).max() < 1e-4 and np.abs(np.degrees(np.arccos(cosang)) - angleHOH).max() < 1e-2
    # the same run on the yardstick, on the same backend
    ref = make_case('w8')[0]
    ref.calc = yardstick('w8')
    opt_h = run_reference_case(ref, internal)
    print(f'internal={internal}: E {at.get_potential_energy():.8f} (yardstick run {ref.get_potential_energy():.8f})  '
          f'steps {opt.nsteps} ({opt_h.nsteps}), of them before the rattle {opt.first_run} ({opt_h.first_run})  '
          f'force calls {opt.pes.neval} ({opt_h.pes.neval})')
    # the device calculator where the yardstick run ended
    S = ref.calc.sums(ref.positions, second=False)
    bE, bg, _ = bounds(S)
    probe = case_atoms('w8')
    probe.set_positions(ref.positions)
    report(f'internal={internal} E at the yardstick minimum', abs(probe.get_potential_energy() - S['e'].sum()), bE)
    report(f'internal={internal} g at the yardstick minimum', np.abs(-probe.get_forces() - S['g']), bg)
