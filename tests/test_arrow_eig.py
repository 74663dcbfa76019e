"""`sella::hostm::arrow_eig` (csrc/host_math.h) — the arrowhead eigensolver behind the Davidson loop's O(k^2)
Rayleigh-Ritz update, reached otherwise only through whole Davidson trajectories — as a stand-alone program
(tests/hostmath/arrow_main.cpp, its own main) built with AddressSanitizer and UBSan: nothing is loaded into Python and
no GPU is touched.  Checked against NumPy on the dense arrowhead, the two exterior eigenvalues also against the 60-digit
secular root (tests/secular_reference.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import secular_reference as sr
from conftest import REPO

EPS = np.finfo(float).eps
SIZES = (0, 1, 2, 30, 64)


def _families(m, rng):
    """[(name, D, z, alpha)]"""
    D = rng.uniform(-1.0, 3.0, m)                                  # unsorted
    z = rng.normal(size=m)
    a = float(rng.normal())
    out = [('generic', D, z, a)]
    for f in (1e-12, 1e-160):
        out.append((f'border_x{f:g}', D, z * f, a))
    out.append(('border_zero', D, np.zeros(m), a))
    out.append(('triples', np.repeat(rng.uniform(-1.0, 3.0, m // 3 + 1), 3)[:m][rng.permutation(m)], z, a))
    pairs = np.repeat(rng.uniform(-1.0, 3.0, m // 2 + 1), 2)[:m]
    pairs[1::2] += 1e-10
    out.append(('pairs_1e-10', pairs, z, a))
    out.append(('border_graded', D, z * np.exp(np.linspace(-40.0, 0.0, m)), a))
    out.append(('alpha_far_above', D, z, 1e3))
    out.append(('alpha_far_below', D, z, -1e3))
    out.append(('alpha_inside', D, z, float(np.median(D)) if m else 0.0))
    for f in (1e-100, 1e100):
        out.append((f'scaled_{f:g}', D * f, z * f, a * f))
    return out


def _cases():
    rng = np.random.RandomState(17)
    return [(f'm{m}_{name}', D, z, a) for m in SIZES for name, D, z, a in _families(m, rng)]


@pytest.fixture(scope='module')
def arrow_results(tmp_path_factory):
    """All cases through ONE run of the sanitized program: {name: (rc, lam, W)}."""
    sys.path.insert(0, os.path.join(REPO, 'tests', 'hostemu'))
    import build_emu
    exe = str(tmp_path_factory.mktemp('arrow') / 'arrow_main')
    subprocess.check_call([build_emu.CXX, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
                           '-I', os.path.join(REPO, 'tests', 'hostemu', 'include'),
                           '-I', os.path.join(REPO, 'sella_amd', 'csrc'), '-I', os.path.join(REPO, 'include'),
                           os.path.join(REPO, 'tests', 'hostmath', 'arrow_main.cpp'), '-o', exe])
    cases = _cases()
    text = ''.join(f'{len(D)}\n{" ".join(map(repr, map(float, D)))}\n{" ".join(map(repr, map(float, z)))}\n{a!r}\n'
                   for _, D, z, a in cases)
    run = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr.decode(errors='replace')[-4000:]   # sanitizers silent
    lines = run.stdout.decode().split('\n')
    assert len(lines) >= 3 * len(cases)
    out = {}
    for k, (name, D, z, a) in enumerate(cases):
        M = len(D) + 1
        lam = np.array(lines[3 * k + 1].split(), dtype=float)
        W = np.array(lines[3 * k + 2].split(), dtype=float)
        assert lam.shape == (M,) and W.shape == (M * M,), name
        out[name] = (int(lines[3 * k]), lam, W.reshape(M, M))
    return out


def _dense(D, z, a):
    m = len(D)
    A = np.zeros((m + 1, m + 1))
    A[np.arange(m), np.arange(m)] = D
    A[m, :m] = A[:m, m] = z
    A[m, m] = a
    return A


@pytest.mark.parametrize('m', SIZES)
def test_arrow_eig_against_dense(arrow_results, m):
    """rc = 0, ascending eigenvalues to 1e-14 max|A| of eigvalsh, orthonormal vectors to 1e-14, residual to 1e-14 max|A|.
    (Worst measured over all cases, m = 64: 3.0e-15, 1.1e-15 and 1.8e-15.)"""
    worst = np.zeros(3)
    for name, D, z, a in _cases():
        if len(D) != m:
            continue
        rc, lam, W = arrow_results[name]
        A = _dense(D, z, a)
        scale = np.abs(A).max() or 1.0
        assert rc == 0 and np.isfinite(lam).all() and np.isfinite(W).all(), name
        assert (np.diff(lam) >= 0).all(), name
        e_val = np.abs(lam - np.linalg.eigvalsh(A)).max() / scale
        e_orth = np.abs(W.T @ W - np.eye(m + 1)).max()
        # (the products of entries near 1e100 are kept in range by scaling the matrix first)
        e_res = np.abs((A / scale) @ W - W * (lam / scale)).max()
        worst = np.maximum(worst, (e_val, e_orth, e_res))
        assert e_val <= 1e-14 and e_orth <= 1e-14 and e_res <= 1e-14, (name, e_val, e_orth, e_res)
    print(f'MEASURED arrow_eig m = {m}: eigenvalues {worst[0]:.2e} orthogonality {worst[1]:.2e} residual {worst[2]:.2e}')


@pytest.mark.parametrize('m', [s for s in SIZES if s > 0])
def test_arrow_eig_exterior_eigenvalues_against_60_digits(arrow_results, m):
    """The lowest and the highest eigenvalue to 4 ulp of max(max |lam|, max |D|), lam the whole spectrum: the solver
    works on D - alpha, so an alpha of 1e3 next to poles of order 1 costs the small end of the spectrum eps |alpha| —
    accuracy in units of the matrix, as in the dense comparison, but forty times tighter and against exact roots."""
    worst = 0.0
    for name, D, z, a in _cases():
        if len(D) != m:
            continue
        rc, lam, W = arrow_results[name]
        for got, top in ((lam[0], False), (lam[-1], True)):
            ref = sr.exterior_eigenvalue(D, z, a, top)
            unit = EPS * max(np.abs(lam).max(), np.abs(D).max())
            worst = max(worst, abs(got - ref) / unit)
            assert abs(got - ref) <= 4 * unit, (name, top, got, ref)
    print(f'MEASURED arrow_eig m = {m}: exterior eigenvalues within {worst:.2f} ulp')
