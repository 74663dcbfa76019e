"""Block Davidson (`sella_davidson_block`, BASELINE configs[4]): the reference has no block method
(one vector per iteration, sella/eigensolvers.py:111-112), so the parity target is exact()
(sella/eigensolvers.py:9-28): converged eigenpairs equal LAPACK's / the oracle's to 1e-10."""
import numpy as np
import pytest

from conftest import hessian_like

import oracle.sella_oracle as orc


def check_pairs(A, out, nev, tol=1e-10):
    w, Z, _ = orc.exact(A)
    assert out['nconv'] == nev, out
    np.testing.assert_allclose(out['lams'], w[:nev], atol=tol * max(1.0, np.abs(w).max()))
    V = out['V']
    np.testing.assert_allclose(V.T @ V, np.eye(nev), atol=1e-10)
    R = A @ V - V * out['lams']
    assert np.abs(R).max() < 1e-6 * max(1.0, np.abs(w).max())
    # eigenvectors up to sign where the gap to the neighbours is healthy
    gaps = np.diff(w[:nev + 1])
    for j in range(nev):
        g = min(gaps[j], gaps[j - 1] if j else np.inf)
        if g > 1e-3:
            assert abs(abs(V[:, j] @ Z[:, j]) - 1.0) < 1e-8, j


@pytest.mark.parametrize('n,nev,block', [(96, 4, 4), (128, 16, 16), (100, 20, 16)])
def test_block_davidson_eigenbasis_preconditioner(ctx, n, nev, block):
    A, P, g = hessian_like(n, seed=n, nneg=2)
    dA, dP = ctx.upload(A), ctx.upload(P)
    w, Q, Qt = ctx.eigh(dP)
    out = ctx.davidson_block(dA, n, nev, block=block, tol=1e-8, maxiter=200, Pvecs=Q, PvecsT=Qt, pevals=w)
    check_pairs(A, out, nev)
    assert out['niter'] < 60


def test_block_davidson_diagonal_and_restart(ctx):
    """Diagonally dominant operator (Davidson's home ground), diagonal preconditioner, a basis limit small
    enough to force several thick restarts."""
    n, nev = 300, 6
    rng = np.random.RandomState(7)
    N = rng.normal(size=(n, n))
    A = np.diag(np.arange(1, n + 1) * 0.5) + 0.02 * (N + N.T)
    dA = ctx.upload(A)
    out = ctx.davidson_block(dA, n, nev, block=6, tol=1e-9, maxiter=400, maxvec=24, diag=np.diag(A).copy())
    check_pairs(A, out, nev)
    # no preconditioner, explicit start block: still converges (block Lanczos with restarts)
    out2 = ctx.davidson_block(dA, n, 3, block=8, tol=1e-8, maxiter=2000, maxvec=64, V0=rng.normal(size=(n, 8)))
    check_pairs(A, out2, 3)


def test_block_davidson_row_sharded_callback(ctx):
    """The row-sharded product path with a single rank: the all-gather callback sees device buffers and a stream
    (what ncclAllGather takes); here it is a device-to-device copy through the library."""
    import ctypes
    n, nev = 96, 5
    A, P, g = hessian_like(n, seed=11)
    dA, dP = ctx.upload(A), ctx.upload(P)
    w, Q, Qt = ctx.eigh(dP)
    calls = []

    def gather(send, recv, nbytes, stream):
        ctx.sync()
        calls.append(nbytes)
        ctx.copy_device(recv, send, nbytes)

    out = ctx.davidson_block(dA, n, nev, tol=1e-8, Pvecs=Q, PvecsT=Qt, pevals=w, row0=0, world=1, allgather=gather)
    check_pairs(A, out, nev)
    assert calls and all(b == 16 * n * 8 for b in calls)


def test_block_davidson_split_panel_products(ctx):
    """The short-and-wide panel products of the iteration (basis <= 64 rows against the block: projections, Gram blocks)
    through the split-index kernels (`panel_small_*`, on by default from 2048 columns; forced here at test size) and
    through the row-parallel MFMA kernel: same converged pairs."""
    n, nev = 160, 6
    A, P, g = hessian_like(n, seed=5, nneg=2)
    dA, dP = ctx.upload(A), ctx.upload(P)
    w, Q, Qt = ctx.eigh(dP)
    outs = {}
    for flag in (64, 0):
        with ctx.options(panel_small=flag):
            outs[flag] = ctx.davidson_block(dA, n, nev, block=8, tol=1e-9, maxiter=200, maxvec=32, Pvecs=Q, PvecsT=Qt, pevals=w)
        check_pairs(A, outs[flag], nev)
    np.testing.assert_allclose(outs[64]['lams'], outs[0]['lams'], atol=1e-11)
    assert outs[64]['niter'] == outs[0]['niter']


@pytest.mark.parametrize('precond', ['eigenbasis', 'diagonal'])
def test_block_davidson_pipelined_against_general_loop(ctx, precond):
    """Option bd_pipeline (default 1): A applied to the raw correction block while the host orthonormalises it, the same
    small coefficients transforming T and A T, two polled waits per iteration — against the general loop (0): the same
    converged pairs (no trajectory to match: the reference has no block method)."""
    nev = 16
    if precond == 'eigenbasis':
        n = 128
        A, P, g = hessian_like(n, seed=n, nneg=2)
        dA, dP = ctx.upload(A), ctx.upload(P)
        w, Q, Qt = ctx.eigh(dP)
        kw = dict(Pvecs=Q, PvecsT=Qt, pevals=w)
    else:
        n = 300
        N = np.random.RandomState(11).normal(size=(n, n))
        A = np.diag(np.arange(1, n + 1) * 0.5) + 0.02 * (N + N.T)        # diagonally dominant: Davidson's home ground
        dA = ctx.upload(A)
        kw = dict(diag=np.diag(A).copy())
    outs = {}
    for flag in (1, 0):
        with ctx.options(bd_pipeline=flag):
            outs[flag] = ctx.davidson_block(dA, n, nev, block=16, tol=1e-8, maxiter=400, **kw)
        check_pairs(A, outs[flag], nev)
    np.testing.assert_allclose(outs[1]['lams'], outs[0]['lams'], atol=1e-10)


@pytest.mark.parametrize('early', [1, 0])
@pytest.mark.parametrize('seed', [102, 103])
def test_block_davidson_pipelined_random_start_block(ctx, seed, early):
    """The hard regime: a start block of RANDOM vectors under a diagonal preconditioner (corrections that lie almost
    entirely inside the basis: projections cancel four to ten digits, every block takes the second Gram-Schmidt pass).
    The pipelined driver must get through it like the general loop does (84 - 91 iterations on sixteen such starts)."""
    n = 300
    N = np.random.RandomState(3).normal(size=(n, n))
    A = np.diag(np.arange(1, n + 1) * 0.5) + 0.02 * (N + N.T)
    dA = ctx.upload(A)
    V0 = np.random.RandomState(seed).normal(size=(n, 7))
    with ctx.options(bd_early_matvec=early):
        out = ctx.davidson_block(dA, n, 5, block=16, tol=1e-9, maxiter=200, V0=V0, diag=np.diag(A).copy())
    check_pairs(A, out, 5)
    assert out['niter'] < 120          # (84 - 91 in the general loop; 71 - 77 here since the restart keeps 2 nev vectors)


def test_block_davidson_early_matrix_pass(ctx):
    """Option bd_early_matvec (default 1): A applied to the raw correction block while the host orthonormalises it, A T
    transformed by the coefficients that transform T, under the per-row error budget — same converged pairs as with A
    applied to the final block (0)."""
    n, nev = 300, 16
    N = np.random.RandomState(11).normal(size=(n, n))
    A = np.diag(np.arange(1, n + 1) * 0.5) + 0.02 * (N + N.T)
    dA = ctx.upload(A)
    outs = {}
    for flag in (1, 0):
        with ctx.options(bd_early_matvec=flag):
            outs[flag] = ctx.davidson_block(dA, n, nev, block=16, tol=1e-9, maxiter=400, diag=np.diag(A).copy())
        check_pairs(A, outs[flag], nev)
    np.testing.assert_allclose(outs[1]['lams'], outs[0]['lams'], atol=1e-10)


def test_block_davidson_pipelined_restarts_and_small_blocks(ctx):
    """The pipelined driver with thick restarts in every iteration (maxvec at its minimum), with nev < block, and with a
    start block that leaves fewer than 16 vectors."""
    n = 300
    rng = np.random.RandomState(3)
    N = rng.normal(size=(n, n))
    A = np.diag(np.arange(1, n + 1) * 0.5) + 0.02 * (N + N.T)
    dA = ctx.upload(A)
    out = ctx.davidson_block(dA, n, 6, block=6, tol=1e-9, maxiter=400, maxvec=18, diag=np.diag(A).copy())
    check_pairs(A, out, 6)
    out = ctx.davidson_block(dA, n, 3, block=8, tol=1e-9, maxiter=400, diag=np.diag(A).copy())
    check_pairs(A, out, 3)
    V0 = np.eye(n)[:, :7] + 0.05 * rng.normal(size=(n, 7))            # (a start block the caller supplies: 7 < 16 vectors)
    out = ctx.davidson_block(dA, n, 5, block=16, tol=1e-9, maxiter=400, V0=V0, diag=np.diag(A).copy())
    check_pairs(A, out, 5)
