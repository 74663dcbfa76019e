// tric.hip — TRIC fragment rotations: value, gradient, Hessian-vector product and Hessian blocks of the
// exponential-map rotation coordinate of each fragment, batched over the fragments of one structure.
//
// Replaces the NumPy closed forms of sella/internal.py:507-1010 (`_build_F_matrix_np`, `_stabilize_quaternion`,
// `_asinc_np`, `_rotation_3axis_jacobian_np`, `_rotation_hessian_np`) behind `Rotation.calc` / `calc_gradient` /
// `calc_hessian` (:1030-1078).  For a fragment with atoms i, current positions p_i and centred reference positions
// ref_i:
//     R = sum_i p_i (x) ref_i                     (the centroid term vanishes because sum_i ref_i = 0)
//     F(R) = [[tr R, y^T], [y, R + R^T - tr R I]],  y = (R_12 - R_21, R_20 - R_02, R_01 - R_10)
//     c = top eigenvector of F (the quaternion that best aligns ref with p), on the branch of q_prev
//     v_k = 2 c_{k+1} asinc(c_0),  asinc(x) = acos(x) / sqrt(1 - x^2),   k = 0, 1, 2.
// F is linear in the positions, so with F_a = dF/dx_a (a = (atom, xyz)), lam = c^T F c, lam_a = c^T F_a c and
// P = (F - lam)^+ (directions whose eigenvalue gap is <= 1e-14 dropped: degenerate top eigenspaces of diatomic
// and linear fragments):
//     c_a  = -P F_a c
//     c_ab = -P [(F_a - lam_a) c_b + (F_b - lam_b) c_a] - c (c_a . c_b)
// and the chain rule through asinc gives the gradient and Hessian of v_k.  H t uses the same formula with b
// replaced by the tangent direction: F_t = F(sum_i t_i (x) ref_i), c_t = -P F_t c.
//
// Shape: one wave64 per fragment, four fragments per 256-thread workgroup.  The 18 sums of R and R_t are reduced
// with a fixed xor butterfly (every lane ends with the same bits: each step adds the same two numbers), every lane
// then solves the 4x4 eigenproblem redundantly in registers by cyclic Jacobi — no LDS, no barrier — and the lanes
// stride over the 3m degrees of freedom, each of which needs only per-fragment quantities.  The Hessian blocks are
// a second launch, one thread per (a, b) pair writing all three axes, from a per-fragment state (c, P, asinc and
// its derivatives) the first launch leaves behind.
//
// Periodic images (`sella_internals_tric_eval_shifted`): a fragment that crosses a cell boundary is evaluated at its
// unwrapped geometry without moving any atom.  Each CSR slot p may carry a Cartesian shift s_p (in practice n_p @ cell
// for an integer image n_p), added to that slot's position wherever a position is read — the anchor and the sums of R
// in launch 1; the Hessian launch reads no position.  The shift comes first, (pos + s) - anchor, the operation order of
// a host that unwraps the positions and calls the unshifted entry, so the two agree bit for bit.  The tangent takes no
// shift: a lattice vector is constant, derivatives do not see it.
#include "internal.h"

namespace sella {
namespace {

constexpr int TRIC_WAVES = 4;                 // fragments per workgroup
constexpr int TRIC_STATE = 24;                // per-fragment state: c[4] | P[16] | s, s', s'' | pad
constexpr double TRIC_TOP_TOL = 1e-10;        // eigenvalues within this of the largest span the top eigenspace
constexpr double TRIC_GAP_TOL = 1e-14;        // pseudo-inverse: gaps at or below this are dropped

// F(R) v for a 3x3 R (row-major)
__device__ __forceinline__ void applyF(const double* R, const double* v, double* out) {
    const double tr = R[0] + R[4] + R[8];
    const double y0 = R[5] - R[7], y1 = R[6] - R[2], y2 = R[1] - R[3];
    out[0] = tr * v[0] + y0 * v[1] + y1 * v[2] + y2 * v[3];
    out[1] = y0 * v[0] + (2.0 * R[0] - tr) * v[1] + (R[1] + R[3]) * v[2] + (R[2] + R[6]) * v[3];
    out[2] = y1 * v[0] + (R[1] + R[3]) * v[1] + (2.0 * R[4] - tr) * v[2] + (R[5] + R[7]) * v[3];
    out[3] = y2 * v[0] + (R[2] + R[6]) * v[1] + (R[5] + R[7]) * v[2] + (2.0 * R[8] - tr) * v[3];
}

// F_a v for a = (atom with reference position r, Cartesian direction d): R_a = e_d (x) r
__device__ __forceinline__ void applyFa(int d, const double* r, const double* v, double* out) {
    double R[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = 0.0;
    R[3 * d + 0] = r[0];
    R[3 * d + 1] = r[1];
    R[3 * d + 2] = r[2];
    applyF(R, v, out);
}

__device__ __forceinline__ void matvec4(const double* P, const double* v, double* out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = P[4 * i] * v[0] + P[4 * i + 1] * v[1] + P[4 * i + 2] * v[2] + P[4 * i + 3] * v[3];
}

__device__ __forceinline__ double dot4(const double* u, const double* v) {
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2] + u[3] * v[3];
}

// asinc(x) = acos(x) / sqrt(1 - x^2) and its first two derivatives; the Taylor series in y = x - 1 for x >= 0.97
// (sella/internal.py:584-598), differentiated term by term there
__device__ __forceinline__ void asinc3(double x, double* s, double* s1, double* s2) {
    if (x < 0.97) {
        const double om = 1.0 - x * x;
        s[0] = ::acos(x) / ::sqrt(om);
        s1[0] = (x * s[0] - 1.0) / om;
        s2[0] = (s[0] + 3.0 * x * s1[0]) / om;
        return;
    }
    const double a[10] = {1.0, -1.0 / 3, 2.0 / 15, -2.0 / 35, 8.0 / 315, -8.0 / 693, 16.0 / 3003, -16.0 / 6435,
                          128.0 / 109395, -128.0 / 230945};
    const double y = x - 1.0;
    double v = a[9], d1 = 9.0 * a[9], d2 = 72.0 * a[9];
    for (int n = 8; n >= 0; --n) v = v * y + a[n];
    for (int n = 8; n >= 1; --n) d1 = d1 * y + n * a[n];
    for (int n = 8; n >= 2; --n) d2 = d2 * y + n * (n - 1) * a[n];
    s[0] = v;
    s1[0] = d1;
    s2[0] = d2;
}

// Symmetric 4x4 eigenproblem by cyclic Jacobi: A is destroyed, w eigenvalues (unsorted), V columns eigenvectors
// (V[4 * row + col]).
__device__ __forceinline__ void jacobi4(double* A, double* w, double* V) {
#pragma unroll
    for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    double fro = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) fro += A[i] * A[i];
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) off += A[4 * p + q] * A[4 * p + q];
        if (off <= 1e-36 * fro) break;
        for (int p = 0; p < 3; ++p) {
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[4 * p + q];
                if (apq == 0.0) continue;
                const double theta = (A[4 * q + q] - A[4 * p + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (::fabs(theta) + ::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / ::sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 4; ++k) {                  // A <- A J (columns p, q)
                    const double akp = A[4 * k + p], akq = A[4 * k + q];
                    A[4 * k + p] = cs * akp - sn * akq;
                    A[4 * k + q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < 4; ++k) {                  // A <- J^T A (rows p, q)
                    const double apk = A[4 * p + k], aqk = A[4 * q + k];
                    A[4 * p + k] = cs * apk - sn * aqk;
                    A[4 * q + k] = sn * apk + cs * aqk;
                }
                A[4 * p + q] = A[4 * q + p] = 0.0;
                for (int k = 0; k < 4; ++k) {                  // V <- V J
                    const double vkp = V[4 * k + p], vkq = V[4 * k + q];
                    V[4 * k + p] = cs * vkp - sn * vkq;
                    V[4 * k + q] = sn * vkp + cs * vkq;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = A[5 * i];
}

// Per-fragment quantities from R: the branch-stable quaternion c (projection of qp onto the top eigenspace when
// `branch`, else qp itself), the pseudo-inverse P = (F - lam)^+ and asinc(c_0) with two derivatives.
__device__ __forceinline__ void tric_setup(const double* R, const double* qp, bool branch, double* c, double* P,
                                           double* s) {
    double A[16], w[4], V[16];
    const double tr = R[0] + R[4] + R[8];
    const double y[3] = {R[5] - R[7], R[6] - R[2], R[1] - R[3]};
    A[0] = tr;
    for (int i = 0; i < 3; ++i) A[i + 1] = A[4 * (i + 1)] = y[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[4 * (i + 1) + j + 1] = R[3 * i + j] + R[3 * j + i] - (i == j ? tr : 0.0);
    jacobi4(A, w, V);
    int top = 0;
    for (int k = 1; k < 4; ++k)
        if (w[k] > w[top]) top = k;
    const double lam = w[top];
    if (branch) {
        double q[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < 4; ++k) {
            if (lam - w[k] < TRIC_TOP_TOL) {
                const double co = V[k] * qp[0] + V[4 + k] * qp[1] + V[8 + k] * qp[2] + V[12 + k] * qp[3];
                for (int i = 0; i < 4; ++i) q[i] += co * V[4 * i + k];
            }
        }
        const double nrm = ::sqrt(dot4(q, q));
        if (nrm < 1e-14) {
            for (int i = 0; i < 4; ++i) q[i] = V[4 * i + top];
        } else {
            for (int i = 0; i < 4; ++i) q[i] /= nrm;
        }
        const double sg = q[0] < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < 4; ++i) c[i] = sg * q[i];
    } else {
        for (int i = 0; i < 4; ++i) c[i] = qp[i];
    }
    for (int i = 0; i < 16; ++i) P[i] = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double gap = w[k] - lam;
        if (::fabs(gap) <= TRIC_GAP_TOL) continue;
        const double ig = 1.0 / gap;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) P[4 * i + j] += V[4 * i + k] * V[4 * j + k] * ig;
    }
    asinc3(c[0], s, s + 1, s + 2);
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Launch 1: one wave per fragment.  flags bit 0: value evaluation (take the branch of q_prev, store the new c).
__global__ __launch_bounds__(256) void tric_kernel(int nf, const int* __restrict__ fptr, const int* __restrict__ fatoms,
                                                   const double* __restrict__ pos, const double* __restrict__ shift,
                                                   const double* __restrict__ ref, double* __restrict__ qprev,
                                                   const double* __restrict__ tangent,
                                                   int flags, double* __restrict__ state, double* __restrict__ val,
                                                   double* __restrict__ grad, double* __restrict__ hvp) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * TRIC_WAVES + (threadIdx.x >> 6);
    if (f >= nf) return;                                 // whole waves only: no barrier below
    const int p0 = fptr[f], m = fptr[f + 1] - p0;
    double qp[4];
    for (int i = 0; i < 4; ++i) qp[i] = qprev[4 * f + i];     // read by every lane before lane 0 may store
    // R = sum_i (p_i - p_anchor) (x) ref_i: the anchor (first atom) drops out as the centroid does, and keeps the
    // products free of the absolute position of the fragment.  Shifts (periodic images) are added first.
    const int a0 = fatoms[p0];
    double anc[3] = {pos[3 * a0], pos[3 * a0 + 1], pos[3 * a0 + 2]};
    if (shift)
        for (int d = 0; d < 3; ++d) anc[d] += shift[3 * (size_t)p0 + d];
    double R[9], Rt[9];
    for (int e = 0; e < 9; ++e) R[e] = Rt[e] = 0.0;
    for (int i = lane; i < m; i += 64) {
        const int at = fatoms[p0 + i];
        const double* r = ref + 3 * (size_t)(p0 + i);
        for (int d = 0; d < 3; ++d) {
            double x = pos[3 * (size_t)at + d];
            if (shift) x += shift[3 * (size_t)(p0 + i) + d];
            x -= anc[d];
            for (int e = 0; e < 3; ++e) R[3 * d + e] += x * r[e];
        }
        if (tangent) {
            for (int d = 0; d < 3; ++d) {
                const double t = tangent[3 * (size_t)at + d];
                for (int e = 0; e < 3; ++e) Rt[3 * d + e] += t * r[e];
            }
        }
    }
    for (int e = 0; e < 9; ++e) R[e] = wave_sum(R[e]);
    if (tangent)
        for (int e = 0; e < 9; ++e) Rt[e] = wave_sum(Rt[e]);
    double c[4], P[16], s[3];
    tric_setup(R, qp, flags & 1, c, P, s);
    if (lane == 0) {
        if (flags & 1)
            for (int i = 0; i < 4; ++i) qprev[4 * f + i] = c[i];
        for (int k = 0; k < 3; ++k) val[3 * f + k] = 2.0 * c[k + 1] * s[0];
        if (state) {
            double* st = state + (size_t)TRIC_STATE * f;
            for (int i = 0; i < 4; ++i) st[i] = c[i];
            for (int i = 0; i < 16; ++i) st[4 + i] = P[i];
            for (int i = 0; i < 3; ++i) st[20 + i] = s[i];
            st[23] = 0.0;
        }
    }
    // tangent direction: F_t c, c_t = -P F_t c, lam_t = c . F_t c
    double Ftc[4], ct[4], lamt = 0.0;
    if (tangent) {
        applyF(Rt, c, Ftc);
        matvec4(P, Ftc, ct);
        for (int i = 0; i < 4; ++i) ct[i] = -ct[i];
        lamt = dot4(c, Ftc);
    }
    const int nv = 3 * m;
    double* g = grad + 9 * (size_t)p0;                   // (3 axes, m atoms, 3)
    double* hv = hvp ? hvp + 9 * (size_t)p0 : nullptr;
    for (int a = lane; a < nv; a += 64) {
        const double* r = ref + 3 * (size_t)(p0 + a / 3);
        const int d = a % 3;
        double Fac[4], ca[4];
        applyFa(d, r, c, Fac);
        matvec4(P, Fac, ca);
        for (int i = 0; i < 4; ++i) ca[i] = -ca[i];
        for (int k = 0; k < 3; ++k) g[(size_t)k * nv + a] = 2.0 * (ca[k + 1] * s[0] + c[k + 1] * s[1] * ca[0]);
        if (hv) {
            const double lama = dot4(c, Fac);
            double Fact[4], Ftca[4], u[4], cat[4];
            applyFa(d, r, ct, Fact);
            applyF(Rt, ca, Ftca);
            for (int i = 0; i < 4; ++i) u[i] = (Fact[i] - lama * ct[i]) + (Ftca[i] - lamt * ca[i]);
            matvec4(P, u, cat);
            const double cc = dot4(ca, ct);
            for (int i = 0; i < 4; ++i) cat[i] = -cat[i] - c[i] * cc;
            for (int k = 0; k < 3; ++k)
                hv[(size_t)k * nv + a] = 2.0 * (cat[k + 1] * s[0] + (ca[k + 1] * s[1] * ct[0] + ct[k + 1] * s[1] * ca[0]) +
                                                c[k + 1] * (s[2] * ca[0] * ct[0] + s[1] * cat[0]));
        }
    }
}

// Launch 2: Hessian blocks (3 axes, 3m, 3m) per fragment at hoff[f]; one thread per (a, b), grid-stride over the
// pairs (x) and the fragments (y).  The (a, b) and (b, a) entries are computed with the same operations in the
// same order, so the blocks are symmetric bit for bit.
__global__ __launch_bounds__(256) void tric_hess_kernel(int nf, const int* __restrict__ fptr,
                                                        const double* __restrict__ ref, const double* __restrict__ state,
                                                        const long* __restrict__ hoff, double* __restrict__ hess) {
    for (int f = blockIdx.y; f < nf; f += gridDim.y) {
        const int p0 = fptr[f], m = fptr[f + 1] - p0;
        const long nv = 3 * (long)m, nn = nv * nv;
        const double* st = state + (size_t)TRIC_STATE * f;
        const double* c = st;
        const double* P = st + 4;
        const double* s = st + 20;
        double* H = hess + hoff[f];
        for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nn; e += (long)gridDim.x * blockDim.x) {
            const int a = (int)(e / nv), b = (int)(e % nv);
            double Fac[4], Fbc[4], ca[4], cb[4], Facb[4], Fbca[4], u[4], cab[4];
            applyFa(a % 3, ref + 3 * (size_t)(p0 + a / 3), c, Fac);
            applyFa(b % 3, ref + 3 * (size_t)(p0 + b / 3), c, Fbc);
            matvec4(P, Fac, ca);
            matvec4(P, Fbc, cb);
            for (int i = 0; i < 4; ++i) {
                ca[i] = -ca[i];
                cb[i] = -cb[i];
            }
            const double lama = dot4(c, Fac), lamb = dot4(c, Fbc);
            applyFa(a % 3, ref + 3 * (size_t)(p0 + a / 3), cb, Facb);
            applyFa(b % 3, ref + 3 * (size_t)(p0 + b / 3), ca, Fbca);
            for (int i = 0; i < 4; ++i) u[i] = (Facb[i] - lama * cb[i]) + (Fbca[i] - lamb * ca[i]);
            matvec4(P, u, cab);
            const double cc = dot4(ca, cb);
            for (int i = 0; i < 4; ++i) cab[i] = -cab[i] - c[i] * cc;
            for (int k = 0; k < 3; ++k)
                H[k * nn + e] = 2.0 * (cab[k + 1] * s[0] + (ca[k + 1] * s[1] * cb[0] + cb[k + 1] * s[1] * ca[0]) +
                                       c[k + 1] * (s[2] * ca[0] * cb[0] + s[1] * cab[0]));
        }
    }
}

}  // namespace
}  // namespace sella

using namespace sella;

extern "C" int sella_internals_tric_eval_shifted(sella_ctx* c, int natoms, int nf, const int* frag_ptr,
                                                 const int* frag_atoms, const double* pos, const double* shift,
                                                 const double* refpos, double* q_prev, const double* tangent, int flags,
                                                 double* val, double* grad, double* hvp, double* hess) {
    if (!c || natoms < 0 || nf < 0 || (nf && (!frag_ptr || !frag_atoms || !pos || !refpos || !q_prev || !val || !grad)) ||
        (tangent && !hvp) || (flags & ~1)) {
        set_error("internals_tric_eval: invalid arguments");
        return SELLA_E_INVALID;
    }
    if (nf == 0) return SELLA_OK;
    // every index the kernels follow is checked here, on the host, before anything reaches the device
    if (frag_ptr[0] != 0) {
        set_error("internals_tric_eval: frag_ptr[0] must be 0");
        return SELLA_E_INVALID;
    }
    long maxnn = 0, hwords = 0;
    for (int f = 0; f < nf; ++f) {
        const long m = (long)frag_ptr[f + 1] - frag_ptr[f];
        if (m < 1) {
            set_error("internals_tric_eval: fragment %d has no atoms", f);
            return SELLA_E_INVALID;
        }
        maxnn = m * 9 * m > maxnn ? m * 9 * m : maxnn;
        hwords += 27 * m * m;
    }
    const long nslot = frag_ptr[nf];
    for (long p = 0; p < nslot; ++p) {
        if (frag_atoms[p] < 0 || frag_atoms[p] >= natoms) {
            set_error("internals_tric_eval: atom index %d out of range [0, %d)", frag_atoms[p], natoms);
            return SELLA_E_INVALID;
        }
    }
    const size_t n3 = 3 * (size_t)natoms;
    // one scratch block: pos | shift | refpos | tangent | q | val | grad | hvp | state | hoff | frag_ptr | frag_atoms |
    // hess
    const size_t iwords = ((size_t)nf + 1 + nslot + 1) / 2 + 1;
    const size_t words = n3 + (shift ? 3 * nslot : 0) + 3 * nslot + (tangent ? n3 : 0) + 4 * (size_t)nf +
                         3 * (size_t)nf + 9 * nslot + (tangent ? 9 * nslot : 0) +
                         (hess ? (size_t)TRIC_STATE * nf + nf : 0) + iwords + (hess ? (size_t)hwords : 0) + 64;
    double* buf;
    SCHK(scratch_get(c, SCR_MISC0, words * sizeof(double), &buf));
    double* dpos = buf;
    double* dshift = dpos + n3;
    double* dref = dshift + (shift ? 3 * nslot : 0);
    double* dtan = dref + 3 * nslot;
    double* dq = dtan + (tangent ? n3 : 0);
    double* dval = dq + 4 * (size_t)nf;
    double* dgrad = dval + 3 * (size_t)nf;
    double* dhvp = dgrad + 9 * nslot;
    double* dstate = dhvp + (tangent ? 9 * nslot : 0);
    long* dhoff = (long*)(dstate + (hess ? (size_t)TRIC_STATE * nf : 0));
    int* dptr = (int*)(dhoff + (hess ? nf : 0));
    int* datoms = dptr + nf + 1;
    double* dhess = (double*)dptr + iwords;
    SCHK(h2d_async(c, dpos, pos, n3 * sizeof(double)));
    if (shift) SCHK(h2d_async(c, dshift, shift, 3 * nslot * sizeof(double)));
    SCHK(h2d_async(c, dref, refpos, 3 * nslot * sizeof(double)));
    if (tangent) SCHK(h2d_async(c, dtan, tangent, n3 * sizeof(double)));
    SCHK(h2d_async(c, dq, q_prev, 4 * (size_t)nf * sizeof(double)));
    SCHK(h2d_async(c, dptr, frag_ptr, ((size_t)nf + 1) * sizeof(int)));
    SCHK(h2d_async(c, datoms, frag_atoms, nslot * sizeof(int)));
    std::vector<long> hoff;
    if (hess) {
        hoff.resize(nf);
        long off = 0;
        for (int f = 0; f < nf; ++f) {
            const long m = (long)frag_ptr[f + 1] - frag_ptr[f];
            hoff[f] = off;
            off += 27 * m * m;
        }
        SCHK(h2d_async(c, dhoff, hoff.data(), (size_t)nf * sizeof(long)));
    }
    // algorithmic bytes: positions (+ shifts) and reference positions in, value + gradient (+ H t) out
    const double bytes = 8.0 * (6.0 * nslot + (shift ? 3.0 * nslot : 0.0) + (tangent ? 3.0 * nslot : 0.0) + 11.0 * nf +
                                9.0 * nslot * (tangent ? 2 : 1));
    prof_begin(c, PROF_OTHER, bytes, 0.0);
    SELLA_LAUNCH(c, tric_kernel, dim3((unsigned)((nf + TRIC_WAVES - 1) / TRIC_WAVES)), dim3(64 * TRIC_WAVES), 0, nf,
                 dptr, datoms, dpos, shift ? dshift : nullptr, dref, dq, tangent ? dtan : nullptr, flags,
                 hess ? dstate : nullptr, dval, dgrad, tangent ? dhvp : nullptr);
    prof_end(c);
    HIPCHK(hipGetLastError());
    if (hess) {
        const long bx = (maxnn + 255) / 256;
        const unsigned gx = (unsigned)(bx < 1024 ? bx : 1024);
        const unsigned gy = (unsigned)(nf < 65535 ? nf : 65535);
        hipLaunchKernelGGL(tric_hess_kernel, dim3(gx, gy), dim3(256), 0, c->stream, nf, dptr, dref, dstate, dhoff,
                           dhess);
        HIPCHK(hipGetLastError());
    }
    SCHK(d2h_async(c, q_prev, dq, 4 * (size_t)nf * sizeof(double)));
    SCHK(d2h_async(c, val, dval, 3 * (size_t)nf * sizeof(double)));
    SCHK(d2h_async(c, grad, dgrad, 9 * nslot * sizeof(double)));
    if (tangent) SCHK(d2h_async(c, hvp, dhvp, 9 * nslot * sizeof(double)));
    if (hess) SCHK(d2h_async(c, hess, dhess, (size_t)hwords * sizeof(double)));
    SCHK(stream_wait(c));
    return SELLA_OK;
}

extern "C" int sella_internals_tric_eval(sella_ctx* c, int natoms, int nf, const int* frag_ptr, const int* frag_atoms,
                                         const double* pos, const double* refpos, double* q_prev, const double* tangent,
                                         int flags, double* val, double* grad, double* hvp, double* hess) {
    return sella_internals_tric_eval_shifted(c, natoms, nf, frag_ptr, frag_atoms, pos, nullptr, refpos, q_prev, tangent,
                                             flags, val, grad, hvp, hess);
}
