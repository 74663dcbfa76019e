"""60-digit reference for the step families in the eigenbasis of the Hessian (TEST INFRASTRUCTURE).

The RFO / P-RFO step at a trial alpha is an eigenvector of the scaled augmented matrix
    [[alpha^2 diag(lam), alpha ghat], [alpha ghat^T, 0]]                        (stepper.py:128-137)
whose eigenvalues are the roots of  f(mu) = mu + sum_i b_i^2 / (D_i - mu),  D = alpha^2 lam,  b = alpha ghat.
float64 `eigh` of that matrix has no relative accuracy for tiny roots and is roundoff-defined in clusters, so the
root is found here by bisection in `decimal` arithmetic (60 digits) on the distance to the nearest pole, from the
float64 inputs taken exactly.  Coincident poles are merged (weights summed), exactly-zero weights are dropped: both
leave the selected eigenvector's step unchanged unless the weightless pole IS the selected eigenvalue, which raises.

`dsda` of the library reproduces the reference implementation's formula, which is NOT the derivative of the step
(it divides by L_j - L_o where perturbation theory has L_o - L_j): `dsda_formula_ref` evaluates that same formula at
60 digits, and nothing here offers a true derivative to compare with.
"""
from decimal import Decimal, localcontext

import numpy as np

PREC = 60
CLAMP = Decimal('1e-12')                  # stepper.py:134-137
_SCAN = Decimal(10) ** -8                 # scale search towards the pole, factor per probe
_RTOL = Decimal(10) ** -45                # bisection stops at this relative width of the distance to the pole


class WeightlessPole(ValueError):
    """The selected eigenvalue is a pole with an exactly zero weight (the true hard case with b = 0): its eigenvector
    is a unit vector with last component 0, and the step is whatever the implementation's clamp makes of it."""


def _dec(x):
    return Decimal(float(x))              # exact


def _merged(lam, ghat, alpha):
    """(poles ascending, weights b^2 > 0, index of each input mode's pole or -1 for a weightless mode, weightless poles)."""
    a = _dec(alpha)
    D = [a * a * _dec(x) for x in lam]
    b = [a * _dec(x) for x in ghat]
    poles, weights, where, idle = [], [], [-1] * len(D), []
    for i in sorted(range(len(D)), key=lambda i: D[i]):
        if b[i] == 0:
            idle.append(D[i])
            continue
        if poles and poles[-1] == D[i]:
            weights[-1] += b[i] * b[i]
        else:
            poles.append(D[i])
            weights.append(b[i] * b[i])
        where[i] = len(poles) - 1
    return D, b, poles, weights, where, idle


def _from_pole(h, hi):
    """Root t in (0, hi] of an increasing h with h(0+) = -inf and h(hi) >= 0."""
    lo = hi
    for _ in range(400):
        lo = lo * _SCAN
        if h(lo) < 0:
            break
        hi = lo
    else:
        raise ArithmeticError('no sign change next to the pole')
    while hi - lo > _RTOL * lo:
        mid = (lo + hi) / 2
        if h(mid) < 0:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def _root(poles, weights, j):
    """Root number j (ascending, 0 .. len(poles)) as (origin pole, signed offset): mu = origin + offset."""
    n = len(poles)

    def f(origin, off):
        s = origin + off
        for p, w in zip(poles, weights):
            s += w / ((p - origin) - off)
        return s

    if j == 0 or j == n:
        sg = -1 if j == 0 else 1
        e = poles[0] if j == 0 else poles[-1]
        # |mu| <= max |D| + |b| (norm of the matrix), so the distance to the edge pole is below twice that
        reach = 4 * max(abs(p) for p in poles) + 2 * sum(weights).sqrt()
        return e, sg * _from_pole(lambda t: sg * f(e, sg * t), reach)
    lo, hi = poles[j - 1], poles[j]
    half = (hi - lo) / 2
    if f(lo, half) >= 0:
        return lo, _from_pole(lambda t: f(lo, t), half)
    return hi, -_from_pole(lambda t: -f(hi, -t), half)


def _block(lam, ghat, j, alpha):
    """Step of eigenpair j of one block, as floats.  Exterior roots (j = 0 or j = len(lam)) accept coincident poles
    and zero weights; an interior root needs distinct poles with nonzero weights."""
    mm = len(lam)
    if mm == 0:
        return np.zeros(0)
    with localcontext() as ctx:
        ctx.prec = PREC
        a = _dec(alpha)
        D, b, poles, weights, where, idle = _merged(lam, ghat, alpha)
        if 0 < j < mm:
            if idle or len(poles) != mm:
                raise ValueError('interior roots: distinct poles with nonzero weights only')
            origin, off = _root(poles, weights, j)
        elif not poles:
            origin, off = Decimal(0), Decimal(0)               # f(mu) = mu
        else:
            origin, off = _root(poles, weights, 0 if j == 0 else len(poles))
        mu = origin + off
        for p in idle:
            if (j == 0 and p <= mu) or (j == mm and p >= mu):
                raise WeightlessPole(f'pole {p} of weight zero is the selected eigenvalue (root {mu})')
        y = [Decimal(0) if where[i] < 0 else b[i] / ((origin - D[i]) + off) for i in range(mm)]
        eta = 1 / (1 + sum(v * v for v in y)).sqrt()
        scale = a if eta >= CLAMP else eta * a / CLAMP
        return np.array([float(v * scale) for v in y])


def dsda_formula_ref(lam, ghat, j, alpha):
    """The reference implementation's `dsda` FORMULA (stepper.py:139-156) for eigenpair j of one block, evaluated at 60
    digits — not the derivative of the step (see the module docstring), and without the formula's 1e-12 clamps: for
    problems where no pole and no other eigenvalue comes that close to the root.  sum_{j != o} v_j (v_j . c) /
    (L_j - L_o) is the pseudo-inverse of A - mu applied to c on the complement of v, whatever basis a cluster gets.
    The float64 oracle evaluates the same formula through a dense `eigh`, whose absolute eigenvector error swamps
    small components (a gradient of 1e-12); this stands in where the oracle cannot deliver the tolerance."""
    mm = len(lam)
    with localcontext() as ctx:
        ctx.prec = PREC
        a = _dec(alpha)
        D, b, poles, weights, where, idle = _merged(lam, ghat, alpha)
        if 0 < j < mm:
            if idle or len(poles) != mm:
                raise ValueError('dsda_formula_ref: interior roots need distinct poles with nonzero weights')
            origin, off = _root(poles, weights, j)
        elif not poles:
            raise ValueError('dsda_formula_ref: no weight at all')
        else:
            origin, off = _root(poles, weights, 0 if j == 0 else len(poles))
        for p in idle:
            if (j == 0 and p <= origin + off) or (j == mm and p >= origin + off):
                raise WeightlessPole('the selected eigenvalue is a pole of weight zero')
        y = [b[i] / ((origin - D[i]) + off) for i in range(mm)]
        eta = 1 / (1 + sum(t * t for t in y)).sqrt()
        v = [t * eta for t in y] + [eta]
        lamd = [_dec(x) for x in lam]
        gd = [_dec(x) for x in ghat]
        c = [2 * a * lamd[i] * v[i] + gd[i] * eta for i in range(mm)] + [sum(gd[i] * v[i] for i in range(mm))]
        vc = sum(p * q for p, q in zip(v, c))
        c = [q - vc * p for p, q in zip(v, c)]
        # x = pinv(A - mu) c on the complement of v: a particular solution with last component 0, v projected out
        x = [c[i] / ((D[i] - origin) - off) for i in range(mm)] + [Decimal(0)]
        vx = sum(p * q for p, q in zip(v, x))
        x = [q - vx * p for p, q in zip(v, x)]
        return np.array([float(v[i] / eta + (a / eta) * x[i] - (v[i] * a / (eta * eta)) * x[mm]) for i in range(mm)])


def rfo_block_ref(lam, ghat, order_in_block, alpha):
    """shat of an EXTERIOR root: order_in_block = 0 (lowest root) or len(lam) (highest)."""
    if order_in_block not in (0, len(lam)):
        raise ValueError('rfo_block_ref: exterior roots only (see rfo_interior_ref)')
    return _block(lam, ghat, order_in_block, alpha)


def rfo_interior_ref(lam, ghat, order, alpha):
    """shat of interior root `order` (0 < order < len(lam)); distinct poles with nonzero weights only."""
    if not 0 < order < len(lam):
        raise ValueError('rfo_interior_ref: interior roots only')
    return _block(lam, ghat, order, alpha)


def rfo_ref(lam, ghat, order, alpha):
    return _block(lam, ghat, order, alpha)


def prfo_ref(lam, ghat, order, alpha):
    """Top root of the max block (the `order` lowest modes) and lowest root of the min block (stepper.py:163-185)."""
    return np.concatenate((rfo_block_ref(lam[:order], ghat[:order], order, alpha),
                           rfo_block_ref(lam[order:], ghat[order:], 0, alpha)))


def qn_ref(lam, ghat, order, alpha):
    """stepper.py:82-96:  -ghat_i / (sgn_i (|lam_i| + alpha)),  sgn = -1 on the `order` lowest modes."""
    with localcontext() as ctx:
        ctx.prec = PREC
        a = _dec(alpha)
        return np.array([float(-_dec(g) / ((-1 if i < order else 1) * (abs(_dec(x)) + a)))
                         for i, (x, g) in enumerate(zip(lam, ghat))])


def qn_irc_ref(lam, ghat, d1hat, alpha):
    """stepper.py:99-111:  -(ghat_i + alpha d1hat_i) / (|lam_i| + alpha)."""
    with localcontext() as ctx:
        ctx.prec = PREC
        a = _dec(alpha)
        return np.array([float(-(_dec(g) + a * _dec(d)) / (abs(_dec(x)) + a)) for x, g, d in zip(lam, ghat, d1hat)])


def shat_ref(kind, lam, ghat, order, alpha, d1hat=None):
    lam = [float(x) for x in lam]
    ghat = [float(x) for x in ghat]
    if kind == 'qn':
        return qn_ref(lam, ghat, order, alpha)
    if kind == 'qn_irc':
        return qn_irc_ref(lam, ghat, d1hat, alpha)
    if kind == 'rfo':
        return rfo_ref(lam, ghat, order, alpha)
    if kind == 'prfo':
        return prfo_ref(lam, ghat, order, alpha)
    raise ValueError(kind)


def step_ref(kind, V, lam, g, order, alpha, d1hat=None):
    """V @ shat with ghat = V^T g in float64 (the two products are the only float64 arithmetic)."""
    V = np.asarray(V, dtype=float)
    return V @ shat_ref(kind, lam, V.T @ np.asarray(g, dtype=float), order, alpha, d1hat)


def exterior_eigenvalue(D, z, alpha, top):
    """Lowest (top=False) or highest eigenvalue of the arrowhead [[diag(D), z], [z^T, alpha]] as a float: the exterior
    root of the shifted secular equation, or a weightless pole / alpha itself where that lies outside it."""
    with localcontext() as ctx:
        ctx.prec = PREC
        a = _dec(alpha)
        Dd = [_dec(x) - a for x in D]
        poles, weights, idle = [], [], []
        for i in sorted(range(len(Dd)), key=lambda i: Dd[i]):
            w = _dec(z[i]) * _dec(z[i])
            if w == 0:
                idle.append(Dd[i])
            elif poles and poles[-1] == Dd[i]:
                weights[-1] += w
            else:
                poles.append(Dd[i])
                weights.append(w)
        if poles:
            origin, off = _root(poles, weights, len(poles) if top else 0)
            mu = origin + off
        else:
            mu = Decimal(0)
        cand = idle + [mu]
        return float((max(cand) if top else min(cand)) + a)
