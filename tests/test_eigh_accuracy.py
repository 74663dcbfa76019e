"""Accuracy of the symmetric eigensolver and of the carried eigendecompositions in units of the norm of the matrix they
were given, at every scale: LAPACK's test ratios, against LAPACK's own ratios on the same matrix.

Measures (eps = 2^-52, n = A.shape[0], |A|_1 the largest absolute row sum; products in np.longdouble, 64-bit mantissa, or
in mpmath where the host's long double is no wider than double):

    res  = max|A V - V diag(w)| / (n eps |A|_1)
    orth = max|V^T V - I|       / (n eps)
    val  = max|w - w_ref|       / (n eps |A|_1)

Limit: every ratio <= max(1, 8 x the same ratio of numpy.linalg.eigh on the same matrix).  One unit of n eps |A| is what
backward stability means; the factor 8 over LAPACK allows for other summation orders and matrix-core accumulation.  The
zero matrix is the one special case: w == 0 exactly and V orthonormal.

Reference eigenvalues: closed forms (Toeplitz (-1, 2, -1): 2 - 2 cos(k pi / (n + 1)); Clement: +-(n - 1), +-(n - 3), ...),
mpmath's eigsy at 30 digits for the other tridiagonal matrices up to n = 64, numpy.linalg.eigvalsh for dense matrices (and
the one tridiagonal case above n = 64).  A matrix scaled by 2^k has the eigenvalues 2^k w_ref, exactly.  References are
computed once per module and shared by the two backends.

This file is the accuracy gate for work on eigh.hip: the bounds of test_eigh.py are absolute at unit scale and allow the
loss of two or three digits; these do not.  Every test prints its largest ratios (`accuracy-max ...`, pytest -s)."""
import functools

import numpy as np
import pytest

from test_eigh import cases
from test_eigh_seam import BLOCKED, WIDTHS

EPS = 2.0 ** -52
WIDE = np.finfo(np.longdouble).eps < 1e-18


def _products(A, w, V):
    """(max|A V - V diag(w)|, max|V^T V - I|) with the products formed in extended precision."""
    n = A.shape[0]
    if WIDE:
        L = np.longdouble
        A_, V_, w_ = A.astype(L), V.astype(L), np.asarray(w).astype(L)
        return float(np.abs(A_ @ V_ - V_ * w_).max()), float(np.abs(V_.T @ V_ - np.eye(n, dtype=L)).max())
    import mpmath
    with mpmath.workdps(30):
        A_, V_ = mpmath.matrix(A.tolist()), mpmath.matrix(V.tolist())
        R = A_ * V_ - V_ * mpmath.diag([mpmath.mpf(float(x)) for x in w])
        G = V_.T * V_ - mpmath.eye(n)
        return float(max(abs(x) for x in R)), float(max(abs(x) for x in G))


def ratios(A, w, V, w_ref):
    """LAPACK's test ratios (res, orth, val) of the eigenpairs (w, columns of V) of A."""
    n = A.shape[0]
    anorm = float(np.abs(A).sum(axis=1).max())
    r, o = _products(A, w, V)
    if anorm == 0.0:                                     # the zero matrix: nothing to divide by
        return (0.0 if r == 0.0 else np.inf), o / (n * EPS), (0.0 if not np.any(w) else np.inf)
    if WIDE:
        dv = float(np.abs(np.asarray(w).astype(np.longdouble) - np.asarray(w_ref).astype(np.longdouble)).max())
    else:
        dv = float(np.abs(np.asarray(w) - np.asarray(w_ref)).max())
    return r / (n * EPS * anorm), o / (n * EPS), dv / (n * EPS * anorm)


class Worst:
    """Largest ratios seen by one test, printed before the test's last assertion has a chance to fail."""

    def __init__(self, test, backend):
        self.test, self.backend, self.max, self.bad = test, backend, [0.0, 0.0, 0.0], []

    def take(self, label, A, w, V, w_ref):
        got = ratios(A, w, V, w_ref)
        wl, Vl = np.linalg.eigh(A)
        ref = ratios(A, wl, Vl, w_ref)
        assert np.all(np.diff(w) >= 0), label
        self.max = [max(a, b) for a, b in zip(self.max, got)]
        for name, g, l in zip(('res', 'orth', 'val'), got, ref):
            print(f'accuracy {self.test}[{self.backend}] {label}: {name} {g:.3g} (LAPACK {l:.3g})')
            if not g <= max(1.0, 8.0 * l):
                self.bad.append(f'{label}: {name} = {g:.3g} > max(1, 8 x {l:.3g})')

    def close(self):
        print(f'accuracy-max {self.test}[{self.backend}] res {self.max[0]:.3g} orth {self.max[1]:.3g} val {self.max[2]:.3g}')
        assert not self.bad, '\n'.join(self.bad)


def solve(ctx, A):
    w, V, Vt = ctx.eigh(ctx.upload(A))
    Vn = V.numpy()
    np.testing.assert_array_equal(Vt.numpy().T, Vn)
    return w, Vn


# ---- matrices and their reference eigenvalues ------------------------------------------------------------------------
def tridiag(d, e):
    return np.diag(np.asarray(d, float)) + np.diag(np.asarray(e, float), 1) + np.diag(np.asarray(e, float), -1)


def wilkinson(n):
    m = (n - 1) // 2
    return tridiag(np.abs(np.arange(n) - m), np.ones(n - 1))


def glued_wilkinson(copies, glue, m=21):
    n = copies * m
    e = np.ones(n - 1)
    e[m - 1::m] = glue
    return tridiag(np.tile(np.abs(np.arange(m) - (m - 1) // 2), copies), e)


def toeplitz(n):
    return tridiag(np.full(n, 2.0), np.full(n - 1, -1.0))


def clement(n):
    k = np.arange(1, n)
    return tridiag(np.zeros(n), np.sqrt(k * (n - k)))


def graded(n, r):
    d = float(r) ** np.arange(n)
    return tridiag(d, 0.5 * np.sqrt(d[:-1] * d[1:]))


def dense_random(n, seed):
    A = np.random.RandomState(seed).normal(size=(n, n))
    return A + A.T


def mp_eigenvalues(A):
    import mpmath
    with mpmath.workdps(30):
        E = mpmath.eigsy(mpmath.matrix(A.tolist()), eigvals_only=True)
        return np.sort(np.array([np.longdouble(mpmath.nstr(x, 25)) for x in E]))


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(A, w_ref) of a named case at scale 1; computed once, never modified (both backends read the same arrays)."""
    kind, _, arg = name.partition(' ')
    if kind == 'wilkinson':
        A = wilkinson(int(arg))
        w = mp_eigenvalues(A)
    elif kind == 'glued':
        copies, glue = arg.split(' x ')
        A = glued_wilkinson(int(copies), float(glue))
        w = mp_eigenvalues(A) if A.shape[0] <= 64 else np.linalg.eigvalsh(A)
    elif kind == 'toeplitz':
        n = int(arg)
        A = toeplitz(n)
        pi = 4 * np.arctan(np.longdouble(1))
        w = 2.0 - 2.0 * np.cos(np.arange(1, n + 1, dtype=np.longdouble) * pi / (n + 1))
    elif kind == 'clement':
        n = int(arg)
        A = clement(n)
        w = np.arange(-(n - 1), n, 2).astype(float)
    elif kind == 'graded':
        A = graded(60, float(arg))
        w = mp_eigenvalues(A)
    elif kind == 'random':
        n, seed = (int(x) for x in arg.split(' seed '))
        A = dense_random(n, seed)
        w = np.linalg.eigvalsh(A)
    elif kind == 'zero':
        A = np.zeros((int(arg), int(arg)))
        w = np.zeros(int(arg))
    else:                                                # a spectrum of test_eigh.cases at n = 40
        A = dict(cases(40, np.random.RandomState(1)))[name]
        A = 0.5 * (A + A.T)
        w = np.linalg.eigvalsh(A)
    A.setflags(write=False)
    w.setflags(write=False)
    return A, w


def scaled(name, k):
    A, w = matrix(name)
    return np.ldexp(A, k), np.ldexp(w, k)


# ---- 1 ------------------------------------------------------------------------------------------------------------
TRIDIAGONALS = ['wilkinson 21', 'wilkinson 41', 'glued', 'toeplitz 70', 'clement 60', 'graded 0.5', 'graded 2', 'zero 40']


@pytest.mark.parametrize('name', TRIDIAGONALS)
def test_hard_tridiagonals(ctx, name):
    """The classical hard tridiagonal matrices straight through divide & conquer (a tridiagonal input gives tau = 0
    reflectors): Wilkinson 21 and 41, three of W21 glued with 1e-14 (five with 1e-8, n = 105, on the card), Toeplitz
    (-1, 2, -1) n = 70, Clement n = 60, graded d_i = r^i, e_i = sqrt(d_i d_i+1) / 2 with r = 1/2 and 2 (n = 60), and the
    zero matrix; leaves of 4 and 32, both divide & conquer schedules.

    Largest ratios measured (res, orth, val): emulator 0.081, 0.25, 0.070; MI355X (with the n = 105 case) 0.066, 0.35, 0.081."""
    names = [name]
    if name == 'glued':
        names = ['glued 3 x 1e-14'] + (['glued 5 x 1e-8'] if ctx.backend == 'hip' else [])
    worst = Worst('test_hard_tridiagonals', ctx.backend)
    for name in names:
        A, w_ref = matrix(name)
        for leaf in (4, 32):
            for pipe in (0, 1):
                with ctx.options(eigh_leaf=leaf, eigh_dc_pipeline=pipe):
                    worst.take(f'{name} leaf {leaf} pipeline {pipe}', A, *solve(ctx, A), w_ref)
    worst.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------
SCALES = (-200, -60, -20, -10, 10, 60, 200)


@pytest.mark.parametrize('name', ['wilkinson 41', 'random 70 seed 70', 'identity + low rank', 'clusters', 'toeplitz 70'])
def test_scale_invariance(ctx, name):
    """A times 2^k, k = -200 ... 200: the same ratios as at scale 1.  Before a T of max-norm below one was scaled up to one in front
    of divide & conquer, deflation compared rho |z_i| (units of A) with 8 eps max(|D|max, |z|max) of a unit-norm z, and
    the residual of Wilkinson 41 times 2^-20 was 722 units, that of Toeplitz 70 times 2^-60 7.9e12.

    Largest ratios measured (res, orth, val): emulator 0.040, 0.14, 0.048; MI355X 0.030, 0.21, 0.033 — for every matrix the
    same figures at all seven k."""
    worst = Worst('test_scale_invariance', ctx.backend)
    for k in SCALES:
        A, w_ref = scaled(name, k)
        worst.take(f'{name} 2^{k}', A, *solve(ctx, A), w_ref)
    worst.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------
PATHS = [('blocked chain', BLOCKED),
         ('one-launch chain, 2 rows', dict(eigh_upd_max=4096, eigh_upd_rows=2, eigh_tail_lds=0)),
         ('one-launch chain, 8 rows', dict(eigh_upd_max=4096, eigh_upd_rows=8, eigh_tail_lds=0)),
         ('LDS tail', dict(eigh_upd_max=0, eigh_tail_lds=128)),
         ('LDS tail behind the one-launch chain', dict(eigh_upd_max=4096, eigh_tail_lds=128)),
         ('symmetric-aware matvec', dict(eigh_symv_min=1, **BLOCKED)),
         ('rank2k_fixed 0', dict(rank2k_fixed=0, **BLOCKED)),
         ('rank2k_fixed 1', dict(rank2k_fixed=1, **BLOCKED)),
         ('gemv_flat 0', dict(eigh_gemv_flat=0, **BLOCKED)),
         ('gemv_flat 1', dict(eigh_gemv_flat=1, **BLOCKED)),
         ('nb 4', dict(eigh_nb=4)), ('nb 16', dict(eigh_nb=16)), ('nb 24', dict(eigh_nb=24))]
PATHS += [(f'seam nb {nb}', dict(rank2k_stream=1, eigh_nb=nb, **BLOCKED)) for nb in WIDTHS + (5,)]
PATHS += [('three-launch seam', dict(rank2k_stream=0, eigh_nb=16, **BLOCKED)),
          ('wy_mfma 0', dict(eigh_wy_mfma=0)), ('wy_mfma 1', dict(eigh_wy_mfma=1)),
          ('wy 64 reflectors', dict(eigh_wy_nb64_min=1)),
          ('wy strip', dict(eigh_wy_nb64_min=1, eigh_wy_strip=2))]


@pytest.mark.parametrize('path,n', [(p[0], n) for p in PATHS for n in ((64,) if p[0] == 'wy strip' else (67, 70))])
def test_every_tridiagonalisation_path_at_scale(ctx, path, n):
    """One dense random matrix per size at scale 1 and 2^-20 through every stage of the tridiagonalisation and of the
    back-transformation, reached with the options the other eigh tests use: sizes 67 and 70 (and 141 on the card, with the
    case of 70), which put the panel, tile and tail edges where those tests put them; the strip kernel at n = 64 instead of
    both (it needs a multiple of 64).

    Largest ratios measured (res, orth, val): emulator 0.011, 0.18, 0.053; MI355X 0.012, 0.13, 0.053."""
    opts = dict(PATHS)[path]
    sizes = (70, 141) if n == 70 and ctx.backend == 'hip' else (n,)
    worst = Worst('test_every_tridiagonalisation_path_at_scale', ctx.backend)
    with ctx.options(**opts):
        for m in sizes:
            for k in (0, -20):
                A, w_ref = scaled(f'random {m} seed {m}', k)
                worst.take(f'{path} n {m} 2^{k}', A, *solve(ctx, A), w_ref)
    worst.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------
UPDATE_SCALES = (-30, -10, 0, 20)


@pytest.mark.parametrize('k', UPDATE_SCALES)
@pytest.mark.parametrize('kind', ['dense', 'scaled identity', 'identity + low rank'])
def test_update_carries_eigendecomposition_at_scale(ctx, kind, k):
    """The set-up of test_hessian_update.py::test_update_carries_eigendecomposition with B and Y times 2^k: the (w, V)
    carried by `update_h_eig` through every update formula meet the limits against the updated B read back from the device,
    after every update (the rank-one merges share the deflation of divide & conquer).

    Largest ratios measured (res, orth, val): emulator (n = 36) 0.073, 0.25, 0.19; MI355X (n = 150) 0.014, 0.11, 0.032."""
    rng = np.random.RandomState(5)
    n = 36 if ctx.backend == 'emu' else 150
    if kind == 'dense':
        A = rng.normal(size=(n, n))
        B = A + A.T
    elif kind == 'scaled identity':
        B = 2.5 * np.eye(n)
    else:
        u = rng.normal(size=(n, 3))
        B = 1.7 * np.eye(n) + u @ u.T - np.outer(u[:, 0] + 1, u[:, 0] + 1)
    H = rng.normal(size=(n, n))
    H = H + H.T
    dB = ctx.upload(np.ldexp(B, k))
    w, V, Vt = ctx.eigh(dB)
    worst = Worst('test_update_carries_eigendecomposition_at_scale', ctx.backend)
    total = 0
    for step, method in enumerate(['TS-BFGS', 'PSB', 'SR1', 'BFGS_auto', 'DFP', 'Greenstadt', 'TS-BFGS', 'TS-BFGS']):
        kk = 2 if step % 4 == 3 else 1
        S = rng.normal(size=(n, kk)) * 0.1
        Y = np.ldexp(H @ S + 0.05 * rng.normal(size=(n, kk)), k)
        w, nr = ctx.update_h_eig(dB, S, Y, w, V, Vt, method=method, symm=2, max_rank=8)
        if k == 0:
            assert nr >= 0, (method, nr)                          # carried: the test cannot pass by skipping the path
        if nr < 0:
            w, V, Vt = ctx.eigh(dB)
            continue
        total += nr
        Bn = dB.numpy()
        np.testing.assert_array_equal(Vt.numpy().T, V.numpy())
        worst.take(f'{kind} 2^{k} step {step} {method}', Bn, w, V.numpy(), np.linalg.eigvalsh(Bn))
    if k == 0:
        assert total > 0
    worst.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', UPDATE_SCALES)
def test_structured_update_at_scale(ctx, k):
    """The structured path (`update_h_lr`: lam0 I + rank r, merged by the same `eig_rank1_update` and deflation on r + 1
    rows): B = lam0 I + W^T diag(mu - lam0) W with negative, clustered and near-lam0 eigenvalues, times 2^k; one secant
    pair (the closed-form pair terms), a block of three (Gram-Schmidt) and a block of four (Cholesky-QR).  The explicit
    pairs completed by an orthonormal basis of the complement of span(W) for lam0 meet the limits against the dense B that
    the same call updated, read back from the device.

    Largest ratios measured (res, orth, val): emulator (n = 60) 0.011, 0.085, 0.034; MI355X (n = 150) 0.0054, 0.064, 0.0055.
    Before the merge was scaled the emulator gave res 4.7 and val 2.9 at k = -30."""
    n, r = (60, 12) if ctx.backend == 'emu' else (150, 40)
    rng = np.random.RandomState(77)
    lam0 = np.ldexp(0.7, k)
    mu = np.sort(np.concatenate(([-2.5, -0.3, 1.3, 1.3 + 4e-11, 1.3 + 8e-11, 0.7 - 6e-10, 0.7 + 5e-10, 1e-4, 1e3],
                                 np.exp(rng.uniform(np.log(1e-3), np.log(1e2), r - 9)))))
    cap = r + 4 * 8 + 8
    W = np.zeros((cap, n))
    W[:r] = np.linalg.qr(rng.normal(size=(n, r)))[0].T
    mus = np.zeros(cap)
    mus[:r] = np.ldexp(mu, k)
    lr = dict(Wt=ctx.upload(W), r=r, mu=mus, lam0=lam0)
    dB = ctx.zeros(n, n)
    ctx.lr_materialize(dB, lr['Wt'], r, mus, lam0)
    worst = Worst('test_structured_update_at_scale', ctx.backend)
    total = 0
    for kk in (1, 3, 4):
        B0 = dB.numpy()
        S = 0.3 * rng.normal(size=(n, kk)) / np.sqrt(n)
        Y = B0 @ S + 0.05 * rng.normal(size=(n, kk)) * np.linalg.norm(B0 @ S, axis=0) / np.sqrt(n)
        nr, _ = ctx.update_h_lr(dB, S, Y, lr)
        assert nr >= 0
        total += nr
        rr = lr['r']
        Wn = lr['Wt'].numpy()[:rr]
        Q = np.linalg.qr(Wn.T, mode='complete')[0][:, rr:]               # the eigenspace of lam0
        w = np.concatenate((lr['mu'][:rr], np.full(n - rr, lam0)))
        order = np.argsort(w, kind='stable')
        Bn = dB.numpy()
        assert np.all(np.diff(lr['mu'][:rr]) >= 0)
        worst.take(f'2^{k} block of {kk}', Bn, w[order], np.hstack((Wn.T, Q))[:, order], np.linalg.eigvalsh(Bn))
    assert total > 0
    worst.close()
