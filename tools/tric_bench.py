#!/usr/bin/env python3
"""TRIC rotation coordinates (csrc/tric.hip, `sella_internals_tric_eval`) against a NumPy restatement of the same
formulas on the host, for two shapes: 512 three-atom fragments and 8 fragments of 200 atoms.  Times per call:
value + gradient, value + gradient + H t, and value + gradient + Hessian blocks (API call, host copies included; the
first launch also as the kernel time of the profiler), and the largest difference from the host restatement.
One JSON line per (case, operation).

Periodic images (`sella_internals_tric_eval_shifted`): one Cu(111) slab fragment of 256 and of 1024 atoms, every member
with a random integer image, timed through the shifted entry against the unshifted entry on the same positions, and
one `InternalCoordinates._rot_eval(hessian=True)` of the 256-atom fragment.  `--shifted` runs only this part."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sella_amd import device as _dev  # noqa: E402
from sella_amd.device import Context  # noqa: E402


def _F(R):
    """F(R) for a stack of 3x3 matrices (..., 3, 3) -> (..., 4, 4)."""
    tr = np.trace(R, axis1=-2, axis2=-1)
    y = np.stack([R[..., 1, 2] - R[..., 2, 1], R[..., 2, 0] - R[..., 0, 2], R[..., 0, 1] - R[..., 1, 0]], -1)
    F = np.zeros(R.shape[:-2] + (4, 4))
    F[..., 0, 0] = tr
    F[..., 0, 1:] = y
    F[..., 1:, 0] = y
    F[..., 1:, 1:] = R + np.swapaxes(R, -1, -2) - tr[..., None, None] * np.eye(3)
    return F


def _asinc(x):
    if x < 0.97:
        om = 1 - x * x
        s = np.arccos(x) / np.sqrt(om)
        s1 = (x * s - 1) / om
        return s, s1, (s + 3 * x * s1) / om
    a = np.array([1, -1 / 3, 2 / 15, -2 / 35, 8 / 315, -8 / 693, 16 / 3003, -16 / 6435, 128 / 109395, -128 / 230945])
    y, n = x - 1.0, np.arange(10)
    return a @ y ** n, (n[1:] * a[1:]) @ y ** (n[1:] - 1), (n[2:] * (n[2:] - 1) * a[2:]) @ y ** (n[2:] - 2)


def host_fragment(pos, ref, qp, tangent=None, hessian=False):
    """Value (3,), gradient (3, 3m)[, H t (3, 3m)][, Hessian (3, 3m, 3m)] of one fragment, NumPy."""
    m = len(pos)
    w, V = np.linalg.eigh(_F((pos - pos.mean(0)).T @ ref))
    lam = w[-1]
    top = V[:, lam - w < 1e-10]
    q = top @ (top.T @ qp)
    q = V[:, -1] if np.linalg.norm(q) < 1e-14 else q / np.linalg.norm(q)
    c = -q if q[0] < 0 else q
    gap = w - lam
    P = (V * np.where(np.abs(gap) > 1e-14, 1.0 / np.where(np.abs(gap) > 1e-14, gap, 1.0), 0.0)) @ V.T
    R = np.zeros((m, 3, 3, 3))
    for d in range(3):
        R[:, d, d, :] = ref
    Fa = _F(R).reshape(3 * m, 4, 4)                       # dof a = 3 atom + d
    Fac = Fa @ c
    ca = -(Fac @ P)
    s, s1, s2 = _asinc(c[0])
    out = [2 * c[1:] * s, 2 * (ca[:, 1:].T * s + np.outer(c[1:], ca[:, 0]) * s1)]
    lama = Fac @ c
    if tangent is not None:
        Ft = _F(np.einsum('id,ie->de', tangent, ref))
        ct = -(P @ (Ft @ c))
        u = (Fa @ ct - lama[:, None] * ct) + (ca @ Ft.T - (c @ Ft @ c) * ca)
        cat = -(u @ P) - c[None, :] * (ca @ ct)[:, None]
        out.append(2 * (cat[:, 1:].T * s + s1 * (ca[:, 1:].T * ct[0] + np.outer(ct[1:], ca[:, 0]))
                        + c[1:, None] * (s2 * ca[:, 0] * ct[0] + s1 * cat[:, 0])))
    if hessian:
        u = np.einsum('aij,bj->abi', Fa, ca) - lama[:, None, None] * ca[None]
        u = u + u.transpose(1, 0, 2)
        cab = -(u @ P) - c[None, None, :] * (ca @ ca.T)[:, :, None]
        out.append(2 * (np.moveaxis(cab[:, :, 1:], 2, 0) * s
                        + s1 * (ca[:, 1:].T[:, :, None] * ca[None, :, 0] + ca[:, 1:].T[:, None, :] * ca[:, 0][None, :, None])
                        + c[1:, None, None] * (s2 * np.outer(ca[:, 0], ca[:, 0]) + s1 * cab[:, :, 0])))
    return out


def case(nf, m, seed=0):
    rng = np.random.RandomState(seed)
    refs, pos = [], []
    for _ in range(nf):
        r = rng.normal(size=(m, 3)) * (1.0 if m < 10 else 4.0)
        r -= r.mean(0)
        refs.append(r)
        w = rng.normal(size=3)
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        Q = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        pos.append(r @ Q.T + 0.05 * rng.normal(size=(m, 3)) + 10.0 * rng.normal(size=3))
    return np.arange(0, nf * m + 1, m), np.arange(nf * m), np.concatenate(pos), np.concatenate(refs), rng.normal(
        size=(nf * m, 3))


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main(cases=((512, 3), (8, 200))):
    ctx = Context()
    _dev._default = ctx
    for nf, m in cases:
        fp, fa, pos, ref, tan = case(nf, m)
        q0 = np.tile([1.0, 0.0, 0.0, 0.0], (nf, 1))
        for op, kw in (('value+grad', {}), ('value+grad+Ht', dict(tangent=tan)), ('value+grad+hessian',
                                                                                  dict(hessian=True))):
            reps = 20 if op != 'value+grad+hessian' or m < 10 else 5
            ctx.prof_reset()
            ctx.prof_enable(True)
            dt, dev = timed(lambda: ctx.tric_eval(fp, fa, pos, ref, q0.copy(), **kw), reps)
            ctx.prof_enable(False)
            p = ctx.prof_get(3)
            kernel_us = 1e3 * p['ms'] / max(1, p['launches'])

            def host():
                return [host_fragment(pos[fp[f]:fp[f + 1]], ref[fp[f]:fp[f + 1]], q0[f],
                                      tangent=tan[fp[f]:fp[f + 1]] if 'tangent' in kw else None,
                                      hessian=bool(kw.get('hessian'))) for f in range(nf)]
            dth, hres = timed(host, 1 if m > 10 and kw.get('hessian') else 3)
            val, g, hv, H = dev
            diff = max(np.abs(val - np.array([h[0] for h in hres])).max(),
                       np.abs(g - np.concatenate([h[1].ravel() for h in hres])).max())
            if hv is not None:
                diff = max(diff, np.abs(hv - np.concatenate([h[2].ravel() for h in hres])).max())
            if H is not None:
                diff = max(diff, np.abs(H - np.concatenate([h[-1].ravel() for h in hres])).max() / max(1.0, np.abs(H).max()))
            print(json.dumps(dict(case=f'{nf} x {m} atoms', op=op, device_call_us=round(1e6 * dt, 1),
                                  first_launch_kernel_us=round(kernel_us, 2), host_numpy_us=round(1e6 * dth, 1),
                                  speedup=round(dth / dt, 1), max_diff=float(f'{diff:.2e}'))), flush=True)
    ctx.close()


def slab_fragment(nx, ny, nz, seed=0):
    """(positions (m, 3), cell, integer images (m, 3)) of a Cu(111) slab fragment, periodic in x and y."""
    from sella_amd.atoms import fcc111
    slab = fcc111('Cu', (nx, ny, nz), vacuum=7.0)
    rng = np.random.RandomState(seed)
    img = np.zeros((len(slab), 3), dtype=np.int64)
    img[:, :2] = rng.randint(-1, 2, size=(len(slab), 2))
    return slab.positions + 0.05 * rng.normal(size=slab.positions.shape), np.asarray(slab.cell), img


def shifted(reps=20):
    from sella_amd.atoms import Atoms
    from sella_amd.internal import InternalCoordinates
    ctx = Context()
    _dev._default = ctx
    for size in ((8, 8, 4), (16, 16, 4)):
        pos, cell, img = slab_fragment(*size)
        m = len(pos)
        fp, fa = np.array([0, m]), np.arange(m)
        sh = img @ cell
        ref = pos + sh
        ref = ref - ref.mean(0)
        tan = np.random.RandomState(1).normal(size=pos.shape)
        q0 = np.array([[1.0, 0.0, 0.0, 0.0]])
        for op, kw in (('value+grad', {}), ('value+grad+Ht', dict(tangent=tan))):
            row = dict(case=f'slab fragment {m} atoms', op=op)
            for name, extra in (('unshifted', {}), ('shifted', dict(shift=sh))):
                ctx.prof_reset()
                ctx.prof_enable(True)
                dt, _ = timed(lambda: ctx.tric_eval(fp, fa, pos, ref, q0.copy(), **kw, **extra), reps)
                ctx.prof_enable(False)
                p = ctx.prof_get(3)
                row[f'{name}_call_us'] = round(1e6 * dt, 1)
                row[f'{name}_kernel_us'] = round(1e3 * p['ms'] / max(1, p['launches']), 2)
            print(json.dumps(row), flush=True)
        if m == 256:
            at = Atoms(['Cu'] * m, pos, cell=cell, pbc=[True, True, False])
            ic = InternalCoordinates(at)
            ic.add_rotation(np.arange(m), ncvecs=img)
            dt, _ = timed(lambda: ic._rot_eval(hessian=True), 5)
            print(json.dumps(dict(case=f'slab fragment {m} atoms', op='_rot_eval(hessian=True)',
                                  call_ms=round(1e3 * dt, 2))), flush=True)
    ctx.close()


if __name__ == '__main__':
    if '--shifted' in sys.argv:
        shifted()
    else:
        main()
