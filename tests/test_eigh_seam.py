"""The panel seam of the blocked tridiagonalisation carried by the trailing update.

Where the rank-2nb update of a panel runs through the streaming kernels on the full block (`rank2k_stream = 1`, 16-byte
aligned block origin), the workgroups that own row 0 of the updated block also leave that row in `u`, its diagonal entry in
`d` and one partial of its sum of squares per tile column — and the next panel starts with its matvec, without the row
launch of its first column.  Every other case (`rank2k_stream = 0`, an odd block origin, the triangle-only update) keeps
the row launch, which is how the old seam is reached here at run time.  `eigh_upd_max = 0, eigh_tail_lds = 0` keep the
blocked chain running down to the last column at these small sizes.

Bounds: those of `test_eigh.check` against LAPACK; new seam against old seam 1e-12 max|w| (the same quantities, the sum of
squares added up in another order); run to run and between the two update kernels identical bits (fixed summation order,
one shared epilogue).

On the card every shape runs every panel width (4, 16, 24, 32 and the odd 5) with the second run.  The emulator runs fibre
by fibre (1 s per factorisation at n = 34, 4 s at 70, 14 s at 147, 25 s at 201, 45 s at 290), so there — a departure from
the full matrix of shapes and widths — every width and the odd one run at n = 34 and 70, the generic-kernel width 24
and the odd one with the second run at the multi-tile size 147, and one width each at 201 (32) and 290 (16)
without the second run."""
import numpy as np
import pytest

from test_eigh import check

BLOCKED = dict(eigh_upd_max=0, eigh_tail_lds=0)          # the blocked chain all the way down
WIDTHS = (4, 16, 24, 32)


def sym(n, seed):
    A = np.random.RandomState(seed).normal(size=(n, n))
    return A + A.T


def seam_against_old(ctx, A, rerun=True, **opts):
    """New seam: LAPACK bounds and (rerun) a second run with identical bits; then the eigenvalues of the three-launch seam on
    the same matrix."""
    dA = ctx.upload(A)
    with ctx.options(rank2k_stream=1, **opts):
        w = check(ctx, A)
        if rerun:
            np.testing.assert_array_equal(w, ctx.eigh(dA, vectors=False)[0])
    with ctx.options(rank2k_stream=0, **opts):
        ref = ctx.eigh(dA, vectors=False)[0]
    np.testing.assert_allclose(w, ref, rtol=0, atol=1e-12 * max(np.abs(ref).max(), np.finfo(float).tiny))
    return w


def widths(ctx, emu):
    return WIDTHS + (5,) if ctx.backend == 'hip' else emu


def test_two_panels_one_tile(ctx):
    """n = 34: two panels, everything inside one 32 x 128 tile; every panel width, and an odd one (odd block origins take
    the old seam, even ones the new: both in one factorisation)."""
    A = sym(34, 34)
    for nb in WIDTHS + (5,):
        seam_against_old(ctx, A, eigh_nb=nb, **BLOCKED)


def test_baseline_size(ctx):
    A = sym(70, 70)
    for nb in WIDTHS + (5,):
        seam_against_old(ctx, A, rerun=ctx.backend == 'hip' or nb == 16, eigh_nb=nb, **BLOCKED)


def test_second_tile_column_nearly_empty(ctx):
    A = sym(147, 147)
    for nb in widths(ctx, (24, 5)):
        seam_against_old(ctx, A, eigh_nb=nb, **BLOCKED)


def test_ragged_tile_column(ctx):
    A = sym(201, 201)
    for nb in widths(ctx, (32,)):
        seam_against_old(ctx, A, rerun=ctx.backend == 'hip', eigh_nb=nb, **BLOCKED)


def test_three_tile_columns(ctx):
    """n = 290: three tile columns, the block origin crosses a tile edge on the way down; larger blocks on the card."""
    for n in (290,) if ctx.backend == 'emu' else (290, 530, 1100):
        A = sym(n, n)
        for nb in widths(ctx, (16,)):
            seam_against_old(ctx, A, rerun=ctx.backend == 'hip', eigh_nb=nb, **BLOCKED)


def test_both_update_kernels_through_the_seam(ctx):
    """`rank2k_stream_fixed_kernel<16 / 32>` and the generic loop kernel write the same row, diagonal entry and partials:
    eigenvalues bit for bit (n = 201 with panels of 16 on the emulator: test_eigh.py::test_trailing_update_kernels_agree)."""
    for n in (70,) if ctx.backend == 'emu' else (70, 201, 530):
        dA = ctx.upload(sym(n, 3 * n))
        for nb in (16, 32):
            out = []
            for fixed in (0, 1):
                with ctx.options(rank2k_stream=1, rank2k_fixed=fixed, eigh_nb=nb, **BLOCKED):
                    out.append(ctx.eigh(dA, vectors=False)[0])
            np.testing.assert_array_equal(out[0], out[1])


def degenerate(n, rng):
    u = rng.normal(size=(n, 3))
    T = np.diag(rng.normal(size=n)) + np.diag(rng.normal(size=n - 1), 1)
    yield 'zero', np.zeros((n, n))                        # tau = 0 and sum u^2 = 0 in the partials of the epilogue
    yield 'identity', np.eye(n)
    yield 'diagonal', np.diag(rng.normal(size=n))
    yield 'tridiagonal', T + T.T
    yield 'identity + low rank', 2.5 * np.eye(n) + u @ u.T - 0.3 * np.outer(u[:, 0] + 1, u[:, 0] + 1)


def test_degenerate_inputs_through_the_seam(ctx):
    rng = np.random.RandomState(5)
    for n in (40, 72):
        for name, A in degenerate(n, rng):
            seam_against_old(ctx, A, rerun=ctx.backend == 'hip', eigh_nb=16, **BLOCKED)


def test_hand_over_to_the_other_stages(ctx):
    """Where the one-launch chain or the LDS tail follows an update, the seam outputs are not written and nothing depends
    on them: the blocked chain handing over behind a seam, and (on the card: n > 201) the library's defaults."""
    seam_against_old(ctx, sym(201, 7), rerun=ctx.backend == 'hip', eigh_nb=16, eigh_upd_max=64, eigh_tail_lds=128)
    if ctx.backend == 'hip':
        seam_against_old(ctx, sym(301, 8))


def test_more_than_64_partials(ctx):
    """n = 4200: 68 partials of sum u^2 per column at the start, the loop behind the matvec's first 64."""
    if ctx.backend == 'emu':
        pytest.skip('more than 64 partials need n > 4096: card only')
    with ctx.options(eigh_upd_max=0):
        check(ctx, sym(4200, 4200))


def test_the_new_seam_is_taken(ctx):
    """The launches themselves, through the profiling slots: with profiling on every 4th column is sampled, and with panels
    of 16 the first column of every panel is one of them.  n = 70 has updates in front of the panels at 16, 32, 48 and 64
    (the one behind the last panel has no panel behind it): four launches in slot 3 (row kernels and the rest) with the
    three-launch seam that the new seam does not make; the same five updates in slot 2 and matvecs in slot 5 either way."""
    dA = ctx.upload(sym(70, 70))
    counts = []
    for stream in (1, 0):
        with ctx.options(rank2k_stream=stream, eigh_nb=16, **BLOCKED):
            ctx.prof_reset()
            ctx.prof_enable(True)
            try:
                ctx.eigh(dA, vectors=False)
            finally:
                ctx.prof_enable(False)
            counts.append([ctx.prof_get(k)['launches'] for k in (3, 2, 5)])
    assert counts[1][0] - counts[0][0] == 4, counts
    assert counts[0][1] == counts[1][1] == 5, counts
    assert counts[0][2] == counts[1][2] == len(range(0, 68, 4)), counts
