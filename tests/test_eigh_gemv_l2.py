"""The alternating sweep of the blocked chain's matvec (`trd_gemv_kernel<NCH>`, NCH > 0, `a.desc`).

Where the trailing block is larger than `SELLA_EIGH_L2_BYTES` (default: 24 MiB, so from 1774 rows up) every second column
takes the row pairs from the far end: workgroup b of a grid rounded up to a multiple of eight takes slot
(G8 - 1 - b/8) * 8 + (b & 7).  Only the assignment of row pairs to workgroups changes, so `w` and `V` must be the bits of
the loop form (`eigh_gemv_flat = 0`), which never descends and is the reference of every case here.  The resident /
non-temporal split of rows that was measured beside the sweep (profiles/trd_gemv_l2.md) lost and is not in the library:
`SELLA_EIGH_L2_BYTES` is the size from which the sweep engages and nothing else.

`eigh_upd_max = 0, eigh_tail_lds = 0` keep the blocked chain running down to the last column.  Two thresholds per size:
1 byte (the sweep runs down to the last column) and the size of the block at n/2 rows (the sweep ends in the middle of the
factorisation, the ascending geometry takes over).  Sizes: 5 (fewer than eight workgroups), 18 (one full group of eight and
a ragged one), 33 and 70 (several panels: the alignment pad runs through 0 ... 15, up to 30 panel rows are appended, the
seam is taken), 131 (odd n, odd block origins), 290 (two chunks per row); on the card also 1100, 2070 and 2600 (NCH = 4
and 6) with the default threshold, where the sweep engages by itself at the two larger sizes.

The emulator runs fibre by fibre (a factorisation with vectors takes seconds from n = 70 and tens of seconds at 290, as in
test_eigh.py::test_trailing_matvec_all_loads_up_front), so there 131 and 290 run one combination (1 byte, sweep on)
against the reference, and every combination runs at 5, 18, 33 and 70."""
import numpy as np
import pytest

from test_eigh import check

BLOCKED = dict(eigh_upd_max=0, eigh_tail_lds=0)
SIZES = (5, 18, 33, 70, 131, 290)
CARD_SIZES = (1100, 2070, 2600)
_reference = {}


def sym(n, border=False):
    A = np.random.RandomState(1000 + n).normal(size=(n, n))
    A = A + A.T
    if border:
        # one extra leading row and column without coupling: column 0 has nothing to eliminate and the factorisation of A
        # starts at the odd column 1 — the other parity of every column against the sweep
        B = np.zeros((n + 1, n + 1))
        B[0, 0] = 0.37
        B[1:, 1:] = A
        A = B
    return A


def eigh(ctx, A, flat):
    with ctx.options(eigh_gemv_flat=flat, **BLOCKED):
        w, V, _ = ctx.eigh(ctx.upload(A))
    return np.array(w), V.numpy()


def reference(ctx, n, border=False):
    """The loop form (computed once per backend and matrix, shared, never modified)."""
    key = (ctx.backend, n, border)
    if key not in _reference:
        w, V = eigh(ctx, sym(n, border), 0)
        w.setflags(write=False)
        V.setflags(write=False)
        _reference[key] = (w, V)
    return _reference[key]


def same_bits(ctx, n, border=False):
    w, V = eigh(ctx, sym(n, border), 1)
    wr, Vr = reference(ctx, n, border)
    np.testing.assert_array_equal(w, wr)
    np.testing.assert_array_equal(V, Vr)


def thresholds(n):
    return (1, 8 * (n // 2) ** 2)


@pytest.mark.parametrize('n', SIZES)
def test_sweep_against_the_loop_form(ctx, monkeypatch, n):
    full = ctx.backend == 'hip' or n <= 70
    for nbytes in thresholds(n) if full else (1,):
        for sweep in (1, 0) if full else (1,):
            monkeypatch.setenv('SELLA_EIGH_L2_BYTES', str(nbytes))
            monkeypatch.setenv('SELLA_EIGH_L2_SWEEP', str(sweep))
            same_bits(ctx, n)


@pytest.mark.parametrize('n', CARD_SIZES)
def test_sweep_engages_by_itself(ctx, monkeypatch, n):
    """Default threshold: ascending throughout at 1100, descending even columns above 1774 rows at 2070 (NCH = 4 and 6) and
    2600 (NCH = 6)."""
    if ctx.backend == 'emu':
        pytest.skip('n >= 1100: card only')
    monkeypatch.delenv('SELLA_EIGH_L2_BYTES', raising=False)
    monkeypatch.delenv('SELLA_EIGH_L2_SWEEP', raising=False)
    same_bits(ctx, n)


@pytest.mark.parametrize('n', SIZES)
def test_switched_off_is_the_ascending_geometry(ctx, monkeypatch, n):
    """`SELLA_EIGH_L2_BYTES=0`, `SELLA_EIGH_L2_SWEEP=0`: the override path itself."""
    monkeypatch.setenv('SELLA_EIGH_L2_BYTES', '0')
    monkeypatch.setenv('SELLA_EIGH_L2_SWEEP', '0')
    same_bits(ctx, n)


@pytest.mark.parametrize('n', (18, 70))
@pytest.mark.parametrize('border', (False, True))
def test_padded_grid_both_parities(ctx, monkeypatch, n, border):
    """The grid of a descending launch is rounded up to a multiple of eight; the workgroups beyond the last slot leave at
    once (the row kernel adds the same `nblkB` partials either way).  Even columns descend: with the bordered matrix the
    columns of A have the other parity.  Bounds of `test_eigh.check` against LAPACK come with it."""
    monkeypatch.setenv('SELLA_EIGH_L2_BYTES', '1')
    monkeypatch.setenv('SELLA_EIGH_L2_SWEEP', '1')
    same_bits(ctx, n, border)
    with ctx.options(eigh_gemv_flat=1, **BLOCKED):
        w = check(ctx, sym(n, border))
    np.testing.assert_array_equal(w, reference(ctx, n, border)[0])
