// tip3p.hip — TIP3P water on the device (the potential of the reference's tests/integration/test_tip3p_cluster.py, ASE's
// ase/calculators/tip3p.py): rigid three-site molecules in consecutive triples, E = sum over the molecule pairs m < n of
// t(d) U_mn, U_mn = 4 eps ((sigma/d)^12 - (sigma/d)^6) + k_e sum over the nine site pairs of q_a q_b / r_ab, d the O-O distance
// and t the switch 1 -> 0 over [rc - width, rc].  Nothing inside a molecule.  In a periodic direction of the (orthorhombic) box
// ONE shift per molecule pair, S = -L rint(D / L) of the O-O difference D, moves all nine site pairs; r_ab = (x_b - x_a) + S
// is then the exact negative of what the partner sees, so both ends of a pair pick the same pairs and compute the same
// numbers.  A calculator that lives in the library (calc.hip, kind 3).
//
// Inside a kernel the sites of a molecule are taken in the order O, H, H whatever their order in memory (site a of the
// kernel is site (a + o) mod 3 of the triple): the arithmetic of `O H H` and `H H O` input is the same.
//   eval:     one workgroup of 256 per molecule m, the threads stride over the partners n != m (every pair is visited from
//             both ends).  The O-O distance test comes first, the ten radial terms for the pairs inside rc only.  Per
//             molecule 1/2 sum t U and the nine gradient entries t G_a + U t' dd/dx_a, G_a = -sum_b phi'_ab u_ab.
//   hessian:  the workgroup of m writes its nine rows.  A thread owns whole partners and writes their 9 x 9 blocks (zero
//             beyond rc); the 9 x 9 diagonal block — the switch couples the sites of a molecule — is a block reduction of 51
//             sums.  Then (H + H^T) / 2.
//   product:  on the kept visits of the geometry (TipHvpState, tip3p.h): 16 lanes share the visits of a (molecule, vector),
//             lane l takes visits l, l + 16, ..., and the 16 partial sums are added in lane order.  The single-vector kernel
//             packs 16 molecules into a workgroup, the block kernel the 16 vectors of a panel: the same row arithmetic, so a
//             row's result does not depend on its slot, on the other rows, or on which of the two kernels took it.
// Sums are per thread in a fixed order and then reduced in LDS — no atomics, the same bits from call to call.  The terms are
// rounded product by product (no contraction into fused multiply-adds).
#include <algorithm>
#include <vector>

#include "tip3p.h"

namespace sella {
namespace {

struct TipGeo {
    int nmol, o;
    const double* pos;      // 3 nmol x 3
    double bx, by, bz;      // box edges, 0: not periodic
    double qH, sigma, eps4, ke, rc, width;
};

// site a of the kernels' order (O, H, H) in the triple
__device__ __forceinline__ int tip_site(int o, int a) {
    const int s = a + o;
    return s >= 3 ? s - 3 : s;
}
__device__ __forceinline__ void tip_load(const double* __restrict__ p, int o, int m, double (&x)[3][3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double* s = p + (size_t)9 * m + 3 * tip_site(o, a);
        x[a][0] = s[0]; x[a][1] = s[1]; x[a][2] = s[2];
    }
}
// xx, yy, zz, yz, xz, xy
__device__ __forceinline__ int tip_sym(int k, int l) { return k == l ? k : 6 - k - l; }

// The shift S of the molecule pair with oxygens at xm, xn and whether it lies inside rc (then d is the O-O distance)
__device__ __forceinline__ bool tip_near(const TipGeo& g, const double (&xm)[3], const double (&xn)[3], double (&S)[3], double& d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double Dx = xn[0] - xm[0], Dy = xn[1] - xm[1], Dz = xn[2] - xm[2];
    S[0] = g.bx > 0.0 ? -g.bx * rint(Dx / g.bx) : 0.0;
    S[1] = g.by > 0.0 ? -g.by * rint(Dy / g.by) : 0.0;
    S[2] = g.bz > 0.0 ? -g.bz * rint(Dz / g.bz) : 0.0;
    const double ox = Dx + S[0], oy = Dy + S[1], oz = Dz + S[2];
    const double d2 = ox * ox + oy * oy + oz * oz;
    if (!(d2 <= g.rc * g.rc * (1.0 + 1e-12))) return false;
    d = sqrt(d2);
    return d < g.rc;
}

struct TipVisit {
    double u[9][3], c1[9], c2[9];       // site pair p = 3 a + b: unit vector, t phi'/r, t (phi'' - phi'/r)
    double Gm[3][3], Gn[3][3];          // dU/dx at the sites of m and of n (not switched)
    double uo[3];                       // u_OO
    double d, t, t1, t2, U;
};

// the visit m <- n; false: beyond rc.  SECOND: the second-derivative coefficients too.
template <bool SECOND>
__device__ __forceinline__ bool tip_visit(const TipGeo& g, const double (&xm)[3][3], const double (&xn)[3][3], TipVisit& v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double S[3];
    if (!tip_near(g, xm[0], xn[0], S, v.d)) return false;
    const double d = v.d, r0 = g.rc - g.width;
    v.t = 1.0; v.t1 = 0.0; v.t2 = 0.0;
    if (d > r0) {
        const double y = (d - r0) / g.width;
        v.t = 1.0 - (y * y) * (3.0 - 2.0 * y);
        v.t1 = -6.0 * (y * (1.0 - y)) / g.width;
        v.t2 = -6.0 * (1.0 - 2.0 * y) / (g.width * g.width);
    }
    double U = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) v.Gm[a][k] = v.Gn[a][k] = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int p = 3 * a + b;
            const double rx = (xn[b][0] - xm[a][0]) + S[0], ry = (xn[b][1] - xm[a][1]) + S[1], rz = (xn[b][2] - xm[a][2]) + S[2];
            const double rr = sqrt(rx * rx + ry * ry + rz * rz);
            const bool live = rr > 1e-8;                        // a coincident site pair is skipped: every term of it is zero
            const double r = live ? rr : 1.0;
            const double qa = a == 0 ? -2.0 * g.qH : g.qH, qb = b == 0 ? -2.0 * g.qH : g.qH;
            double phi = (live ? g.ke : 0.0) * (qa * qb) / r;
            double d1 = -phi / r;
            double d2 = -2.0 * d1 / r;
            if (a == 0 && b == 0) {
                const double e4 = live ? g.eps4 : 0.0;
                const double s = g.sigma / r, s2 = s * s, s6 = s2 * s2 * s2, s12 = s6 * s6;
                phi += e4 * (s12 - s6);
                d1 += e4 * (6.0 * s6 - 12.0 * s12) / r;
                d2 += e4 * (156.0 * s12 - 42.0 * s6) / (r * r);
            }
            const double ux = live ? rx / r : 0.0, uy = live ? ry / r : 0.0, uz = live ? rz / r : 0.0;
            v.u[p][0] = ux; v.u[p][1] = uy; v.u[p][2] = uz;
            U += phi;
            v.Gm[a][0] -= d1 * ux; v.Gm[a][1] -= d1 * uy; v.Gm[a][2] -= d1 * uz;
            v.Gn[b][0] += d1 * ux; v.Gn[b][1] += d1 * uy; v.Gn[b][2] += d1 * uz;
            if constexpr (SECOND) {
                const double c1 = d1 / r;
                v.c1[p] = v.t * c1;
                v.c2[p] = v.t * (d2 - c1);
            }
        }
    }
    v.U = U;
    v.uo[0] = v.u[0][0]; v.uo[1] = v.u[0][1]; v.uo[2] = v.u[0][2];
    return true;
}

// per-molecule energy 1/2 sum t U to emol[m], the nine gradient entries of m's sites to grad + 9 m
__device__ __forceinline__ void tip3p_eval_vb(const VB vb, TipGeo g, double* __restrict__ emol, double* __restrict__ grad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double part[4][10];
    const int m = vb.x;
    double xm[3][3], xn[3][3];
    tip_load(g.pos, g.o, m, xm);
    double e = 0.0, gr[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) gr[k] = 0.0;
    for (int n = threadIdx.x; n < g.nmol; n += 256) {
        if (n == m) continue;
        tip_load(g.pos, g.o, n, xn);
        TipVisit v;
        if (!tip_visit<false>(g, xm, xn, v)) continue;
        e += 0.5 * (v.t * v.U);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) gr[3 * a + k] += v.t * v.Gm[a][k];
        const double w = v.U * v.t1;                            // dd/dx_O(m) = -u_OO
#pragma unroll
        for (int k = 0; k < 3; ++k) gr[k] -= w * v.uo[k];
    }
    block_put<10>(part, 0, e);
#pragma unroll
    for (int k = 0; k < 9; ++k) block_put<10>(part, 1 + k, gr[k]);
    __syncthreads();
    const int t = threadIdx.x;
    if (t == 0) emol[m] = block_total<10>(part, 0);
    if (t < 9) grad[(size_t)9 * m + 3 * tip_site(g.o, t / 3) + t % 3] = block_total<10>(part, 1 + t);
}
__global__ __launch_bounds__(256) void tip3p_eval_kernel(TipGeo g, double* __restrict__ emol, double* __restrict__ grad) {
    tip3p_eval_vb(vb_hw(), g, emol, grad);
}

// Rows 9 m .. 9 m + 8 of H (9 nmol square, rows ldh apart): every entry is written, so nothing has to be zero on entry.
// With K_ab t = c1 I + c2 u u^T, G' = t' G, s2 = U t'', s3 = U t' / d, u = u_OO, the block of (site a of m, site b of n) is
//   -K_ab t  +  [b = O] G'_a u^T  -  [a = O] u G'_b^T  -  [a = b = O] (s2 u u^T + s3 (I - u u^T))
// and the diagonal block (a, a') sums  [a = a'] sum_b K_ab t  -  [a' = O] G'_a u^T  -  [a = O] u G'_a'^T  +  [a = a' = O] (...).
__device__ __forceinline__ void tip3p_hess_vb(const VB vb, TipGeo g, double* __restrict__ H, int ldh) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double part[4][51];
    const int m = vb.x;
    double xm[3][3], xn[3][3];
    tip_load(g.pos, g.o, m, xm);
    double kd[3][6], P[3][9], Q[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int k = 0; k < 6; ++k) kd[a][k] = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) P[a][k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) Q[k] = 0.0;
    double* Hm = H + (size_t)9 * m * ldh;
    for (int n = threadIdx.x; n < g.nmol; n += 256) {
        if (n == m) continue;
        tip_load(g.pos, g.o, n, xn);
        TipVisit v;
        const bool in = tip_visit<true>(g, xm, xn, v);
        if (!in) {
#pragma unroll
            for (int r = 0; r < 9; ++r)
#pragma unroll
                for (int c = 0; c < 9; ++c) Hm[(size_t)r * ldh + 9 * n + c] = 0.0;
            continue;
        }
        const double s2 = v.U * v.t2, s3 = v.U * v.t1 / v.d;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double* Ha = Hm + (size_t)3 * tip_site(g.o, a) * ldh + 9 * n;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int p = 3 * a + b;
                double* Hb = Ha + 3 * tip_site(g.o, b);
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int l = 0; l < 3; ++l) {
                        const double K = (k == l ? v.c1[p] : 0.0) + v.c2[p] * (v.u[p][k] * v.u[p][l]);
                        double h = -K;
                        if (b == 0) h += (v.t1 * v.Gm[a][k]) * v.uo[l];
                        if (a == 0) h -= v.uo[k] * (v.t1 * v.Gn[b][l]);
                        if (a == 0 && b == 0) h -= s2 * (v.uo[k] * v.uo[l]) + s3 * ((k == l ? 1.0 : 0.0) - v.uo[k] * v.uo[l]);
                        Hb[(size_t)k * ldh + l] = h;
                        if (k <= l) kd[a][tip_sym(k, l)] += K;
                    }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int l = 0; l < 3; ++l) P[a][3 * k + l] += (v.t1 * v.Gm[a][k]) * v.uo[l];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int l = k; l < 3; ++l) Q[tip_sym(k, l)] += s2 * (v.uo[k] * v.uo[l]) + s3 * ((k == l ? 1.0 : 0.0) - v.uo[k] * v.uo[l]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int k = 0; k < 6; ++k) block_put<51>(part, 6 * a + k, kd[a][k]);
#pragma unroll
        for (int k = 0; k < 9; ++k) block_put<51>(part, 18 + 9 * a + k, P[a][k]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) block_put<51>(part, 45 + k, Q[k]);
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= 81) return;
    const int r = t / 9, c = t - 9 * r, a = r / 3, k = r - 3 * a, b = c / 3, l = c - 3 * b;
    double h = 0.0;
    if (a == b) h += block_total<51>(part, 6 * a + tip_sym(k, l));
    if (b == 0) h -= block_total<51>(part, 18 + 9 * a + 3 * k + l);
    if (a == 0) h -= block_total<51>(part, 18 + 9 * b + 3 * l + k);
    if (a == 0 && b == 0) h += block_total<51>(part, 45 + tip_sym(k, l));
    Hm[(size_t)(3 * tip_site(g.o, a) + k) * ldh + 9 * m + 3 * tip_site(g.o, b) + l] = h;
}
__global__ __launch_bounds__(256) void tip3p_hess_kernel(TipGeo g, double* __restrict__ H, int ldh) { tip3p_hess_vb(vb_hw(), g, H, ldh); }

// ---- the visits of a geometry, kept for the operator ----------------------------------------------------------------------
// count: the partners of molecule m inside rc.  fill: the same sweep twice — every thread counts its own visits, an exclusive
// scan over the threads gives each its place behind off[m], and the second sweep writes them there.
__device__ __forceinline__ void tip3p_count_vb(const VB vb, TipGeo g, int* __restrict__ cnt) {
    __shared__ double red[4];
    const int m = vb.x;
    double xm[3][3], xn[3][3], S[3], d;
    tip_load(g.pos, g.o, m, xm);
    int mine = 0;
    for (int n = threadIdx.x; n < g.nmol; n += 256) {
        if (n == m) continue;
        tip_load(g.pos, g.o, n, xn);
        if (tip_near(g, xm[0], xn[0], S, d)) ++mine;
    }
    const double all = block_sum((double)mine, red);
    if (threadIdx.x == 0) cnt[m] = (int)all;
}
__global__ __launch_bounds__(256) void tip3p_count_kernel(TipGeo g, int* __restrict__ cnt) { tip3p_count_vb(vb_hw(), g, cnt); }

struct TipFill {
    const int* off;         // nmol + 1
    int* nbr;
    double* q;              // TIP_Q x nvisit
    int nvisit;
};
__device__ __forceinline__ void tip3p_fill_vb(const VB vb, TipGeo g, TipFill o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ int scan[256];
    const int m = vb.x, tid = threadIdx.x;
    double xm[3][3], xn[3][3], S[3], d;
    tip_load(g.pos, g.o, m, xm);
    int mine = 0;
    for (int n = tid; n < g.nmol; n += 256) {
        if (n == m) continue;
        tip_load(g.pos, g.o, n, xn);
        if (tip_near(g, xm[0], xn[0], S, d)) ++mine;
    }
    scan[tid] = mine;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const int below = tid >= s ? scan[tid - s] : 0;
        __syncthreads();
        scan[tid] += below;
        __syncthreads();
    }
    const size_t M = (size_t)o.nvisit;
    int w = o.off[m] + scan[tid] - mine;
    const int end = o.off[m + 1];
    for (int n = tid; n < g.nmol; n += 256) {
        if (n == m) continue;
        tip_load(g.pos, g.o, n, xn);
        TipVisit v;
        if (!tip_visit<true>(g, xm, xn, v)) continue;
        if (w >= end) continue;                                 // (never: the count was taken on the same positions)
        o.nbr[w] = n;
        double* q = o.q + w;
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            q[(3 * p) * M] = v.u[p][0]; q[(3 * p + 1) * M] = v.u[p][1]; q[(3 * p + 2) * M] = v.u[p][2];
            q[(27 + p) * M] = v.c1[p];
            q[(36 + p) * M] = v.c2[p];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                q[(45 + 3 * a + k) * M] = v.t1 * v.Gm[a][k];
                q[(54 + 3 * a + k) * M] = v.t1 * v.Gn[a][k];
            }
        q[63 * M] = v.uo[0]; q[64 * M] = v.uo[1]; q[65 * M] = v.uo[2];
        q[66 * M] = v.U * v.t2;
        q[67 * M] = v.U * v.t1 / v.d;
        ++w;
    }
}
__global__ __launch_bounds__(256) void tip3p_fill_kernel(TipGeo g, TipFill o) { tip3p_fill_vb(vb_hw(), g, o); }

// ---- products on the kept visits --------------------------------------------------------------------------------------------
struct TipOp {
    const int* off;
    const int* nbr;
    const double* q;
    int nvisit, nmol, o;
};
constexpr int TIP_W = 16;               // vectors of a block, and lanes that share the visits of a (molecule, vector)

// Lane `lane` of the 16 that take molecule m's visits for the vector v: its share of (H v) at the nine coordinates of m, in
// the kernels' site order
__device__ __forceinline__ void tip_row(const TipOp& o, int m, const double* __restrict__ v, int lane, double (&acc)[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t M = (size_t)o.nvisit;
    double vm[3][3], vn[3][3];
    tip_load(v, o.o, m, vm);
    const int hi = o.off[m + 1];
    for (int e = o.off[m] + lane; e < hi; e += TIP_W) {
        const double* q = o.q + e;
        tip_load(v, o.o, o.nbr[e], vn);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int p = 3 * a + b;
                const double ux = q[(3 * p) * M], uy = q[(3 * p + 1) * M], uz = q[(3 * p + 2) * M];
                const double c1 = q[(27 + p) * M], c2 = q[(36 + p) * M];
                const double dx = vm[a][0] - vn[b][0], dy = vm[a][1] - vn[b][1], dz = vm[a][2] - vn[b][2];
                const double s = c2 * (ux * dx + uy * dy + uz * dz);
                acc[3 * a] += c1 * dx + s * ux;
                acc[3 * a + 1] += c1 * dy + s * uy;
                acc[3 * a + 2] += c1 * dz + s * uz;
            }
        const double uo[3] = {q[63 * M], q[64 * M], q[65 * M]};
        const double dv[3] = {vn[0][0] - vm[0][0], vn[0][1] - vm[0][1], vn[0][2] - vm[0][2]};
        const double w = uo[0] * dv[0] + uo[1] * dv[1] + uo[2] * dv[2];
        double dU = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double gm = q[(45 + 3 * a + k) * M];
                dU += gm * vm[a][k];
                acc[3 * a + k] += w * gm;
            }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) dU += q[(54 + 3 * a + k) * M] * vn[a][k];
        const double hO = dU + q[66 * M] * w, s3 = q[67 * M];
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] -= uo[k] * hO + s3 * (dv[k] - uo[k] * w);
    }
}

// the 16 lanes' shares of group `grp` added in lane order; valid for lane < 9 after the barrier inside
__device__ __forceinline__ double tip_combine(double (*part)[TIP_W][9], int grp, int lane, const double (&acc)[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
    for (int k = 0; k < 9; ++k) part[grp][lane][k] = acc[k];
    __syncthreads();
    double s = 0.0;
    if (lane < 9)
        for (int l = 0; l < TIP_W; ++l) s += part[grp][l][lane];
    return s;
}

// One vector of the operator, 16 molecules per workgroup: v and hv are rows of its pair record (full length 9 nmol).  |v|^2
// comes in `nb` partial sums; a vanishing vector (|v| < 1e-12) gives a zero product and flag 0.  The rows of the free
// coordinates also go into the eigensolver's vector y (inv: full coordinate -> its index there, -1 if pinned; null: all free).
struct TipOut1 {
    const double* part; int nb;
    const int* inv;
    double* y;
    int* flag;
};
__device__ __forceinline__ void tip3p_hvp1_vb(const VB vb, TipOp o, const double* __restrict__ v, double* __restrict__ hv,
                                              TipOut1 w) {
    __shared__ double red1[4];
    __shared__ double part[TIP_W][TIP_W][9];
    double s = 0.0;
    for (int b = threadIdx.x; b < w.nb; b += 256) s += w.part[b];
    s = block_sum(s, red1);
    const bool live = !(sqrt(s) < 1e-12);
    if (vb.x == 0 && threadIdx.x == 0) *w.flag = live ? 1 : 0;
    const int grp = threadIdx.x >> 4, lane = threadIdx.x & 15, m = (int)vb.x * TIP_W + grp;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    if (m < o.nmol) tip_row(o, m, v, lane, acc);
    const double sum = tip_combine(part, grp, lane, acc);
    if (m >= o.nmol || lane >= 9) return;
    const double h = live ? sum : 0.0;
    const int p = 9 * m + 3 * tip_site(o.o, lane / 3) + lane % 3, q = w.inv ? w.inv[p] : p;
    hv[p] = h;
    if (q >= 0) w.y[q] = h;
}
__global__ __launch_bounds__(256) void tip3p_hvp1_kernel(TipOp o, const double* __restrict__ v, double* __restrict__ hv,
                                                         TipOut1 w) { tip3p_hvp1_vb(vb_hw(), o, v, hv, w); }

// Up to TIP_W vectors, the rows of a device panel (row h at V + h ldv, full length), one workgroup per molecule: group h of 16
// lanes takes row h with tip_row's arithmetic.  Rows beyond nh are neither read nor stored.
struct TipBlock {
    const double* V; int ldv;
    int nh;
    const int* inv;
    double* Y; int ldy;
};
__device__ __forceinline__ void tip3p_hvpb_vb(const VB vb, TipOp o, TipBlock b) {
    __shared__ double part[TIP_W][TIP_W][9];
    const int m = vb.x, grp = threadIdx.x >> 4, lane = threadIdx.x & 15;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    if (grp < b.nh) tip_row(o, m, b.V + (size_t)grp * b.ldv, lane, acc);
    const double sum = tip_combine(part, grp, lane, acc);
    if (grp >= b.nh || lane >= 9) return;
    const int p = 9 * m + 3 * tip_site(o.o, lane / 3) + lane % 3, r = b.inv ? b.inv[p] : p;
    if (r >= 0) b.Y[(size_t)grp * b.ldy + r] = sum;
}
__global__ __launch_bounds__(256) void tip3p_hvpb_kernel(TipOp o, TipBlock b) { tip3p_hvpb_vb(vb_hw(), o, b); }

// diag(H)[free], 16 molecules per workgroup: site a, coordinate k of m sums c1 + c2 u_k^2 over the visits' pairs (a, b), the
// oxygen also -2 u_k G'_k + s2 u_k^2 + s3 (1 - u_k^2)
__device__ __forceinline__ void tip3p_hdiag_vb(const VB vb, TipOp o, const int* __restrict__ inv, double* __restrict__ y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double part[TIP_W][TIP_W][9];
    const int grp = threadIdx.x >> 4, lane = threadIdx.x & 15, m = (int)vb.x * TIP_W + grp;
    const size_t M = (size_t)o.nvisit;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    if (m < o.nmol) {
        const int hi = o.off[m + 1];
        for (int e = o.off[m] + lane; e < hi; e += TIP_W) {
            const double* q = o.q + e;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const int p = 3 * a + b;
                    const double c1 = q[(27 + p) * M], c2 = q[(36 + p) * M];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double u = q[(3 * p + k) * M];
                        acc[3 * a + k] += c1 + c2 * (u * u);
                    }
                }
            const double s2 = q[66 * M], s3 = q[67 * M];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double u = q[(63 + k) * M], uu = u * u;
                acc[k] += (s2 * uu + s3 * (1.0 - uu)) - 2.0 * (u * q[(45 + k) * M]);
            }
        }
    }
    const double sum = tip_combine(part, grp, lane, acc);
    if (m >= o.nmol || lane >= 9) return;
    const int p = 9 * m + 3 * tip_site(o.o, lane / 3) + lane % 3, r = inv ? inv[p] : p;
    if (r >= 0) y[r] = sum;
}
__global__ __launch_bounds__(256) void tip3p_hdiag_kernel(TipOp o, const int* __restrict__ inv, double* __restrict__ y) {
    tip3p_hdiag_vb(vb_hw(), o, inv, y);
}

}  // namespace
}  // namespace sella

using namespace sella;

static TipGeo tip_geo(const TipPot& p, const double* dpos) {
    TipGeo g;
    g.nmol = p.nmol; g.o = p.o; g.pos = dpos;
    g.bx = p.box[0]; g.by = p.box[1]; g.bz = p.box[2];
    g.qH = p.qH; g.sigma = p.sigma; g.eps4 = p.eps4; g.ke = p.ke; g.rc = p.rc; g.width = p.width;
    return g;
}

int sella::tip3p_queue(sella_ctx* c, const TipPot& pot, const double* pos, double** emol, double** grad) {
    const size_t n = (size_t)pot.nmol;                          // positions | per-molecule energies | gradient
    double* buf;
    SCHK(scratch_get(c, SCR_MISC0, (9 * n + n + 9 * n) * sizeof(double), &buf));
    double *dpos = buf, *dem = buf + 9 * n, *dgr = dem + n;
    SCHK(h2d_async(c, dpos, pos, 9 * n * sizeof(double)));
    SELLA_LAUNCHB(c, tip3p_eval_kernel, tip3p_eval_vb, 256, dim3(pot.nmol), dim3(256), 0, tip_geo(pot, dpos), dem, dgr);
    HIPCHK(hipGetLastError());
    *emol = dem;
    *grad = dgr;
    return SELLA_OK;
}

// one upload, one kernel, one read-back; the per-molecule energies are summed here in index order
int sella::tip3p_eval_resident(sella_ctx* c, const TipPot& pot, const double* pos, double* energy, double* grad) {
    double *dem, *dgr;
    SCHK(tip3p_queue(c, pot, pos, &dem, &dgr));
    const size_t n = (size_t)pot.nmol;
    std::vector<double>& out = c->hbuf_b;
    out.resize(10 * n);
    SCHK(d2h_async(c, out.data(), dem, 10 * n * sizeof(double)));
    SCHK(stream_wait(c));
    double e = 0.0;
    for (size_t m = 0; m < n; ++m) e += out[m];
    *energy = e;
    for (size_t i = 0; i < 9 * n; ++i) grad[i] = out[n + i];
    return SELLA_OK;
}

int sella::tip3p_hessian_resident(sella_ctx* c, const TipPot& pot, const double* pos, sella_mat out) {
    const int dim = 9 * pot.nmol;
    Mat* H = mat_get(c, out);
    if (!H || H->rows != dim || H->cols != dim) {
        set_error("tip3p_hessian: out must be the %d x %d matrix of %d molecules", dim, dim, pot.nmol);
        return SELLA_E_INVALID;
    }
    double* dpos;
    SCHK(scratch_get(c, SCR_MISC0, (size_t)dim * sizeof(double), &dpos));
    SCHK(h2d_async(c, dpos, pos, (size_t)dim * sizeof(double)));
    // (no clearing pass: the kernel writes every entry, and the padding of a device matrix is zero already)
    SELLA_LAUNCHB(c, tip3p_hess_kernel, tip3p_hess_vb, 256, dim3(pot.nmol), dim3(256), 0, tip_geo(pot, dpos), H->d, H->ld);
    HIPCHK(hipGetLastError());
    SCHK(launch_symmetrize(c, H->d, dim, H->ld));
    return stream_wait(c);
}

// ---- the resident state of the Hessian-vector operator (tip3p.h) ---------------------------------------------------------
int sella::tip3p_hvp_state_create(sella_ctx* c, const TipPot& pot, const double* pos, TipHvpState* st) {
    const int n = pot.nmol;
    const size_t wpos = (size_t)9 * n, wcnt = ((size_t)n + 2) / 2, woff = ((size_t)n + 3) / 2;
    st->nmol = n; st->o = pot.o;
    st->geo_bytes = (wpos + wcnt + woff) * sizeof(double);
    if (dev_alloc(c, st->geo_bytes, &st->geo) != SELLA_OK) { st->geo = nullptr; return SELLA_E_NOMEM; }
    double* dpos = st->geo;
    int* dcnt = reinterpret_cast<int*>(dpos + wpos);
    int* doff = reinterpret_cast<int*>(dpos + wpos + wcnt);
    SCHK(h2d_async(c, dpos, pos, wpos * sizeof(double)));
    const TipGeo g = tip_geo(pot, dpos);
    SELLA_LAUNCHB(c, tip3p_count_kernel, tip3p_count_vb, 256, dim3(n), dim3(256), 0, g, dcnt);
    HIPCHK(hipGetLastError());
    std::vector<int> off((size_t)n + 1, 0);
    SCHK(d2h_async(c, off.data() + 1, dcnt, (size_t)n * sizeof(int)));
    SCHK(stream_wait(c));
    long total = 0;
    for (int m = 0; m < n; ++m) {
        total += off[(size_t)m + 1];
        if (total > 0x7fffffffL / TIP_Q) {
            set_error("tip3p hvp state: more than 2^31 / %d visits", TIP_Q);
            return SELLA_E_INVALID;
        }
        off[(size_t)m + 1] = (int)total;
    }
    st->nvisit = (int)total;
    const size_t M = (size_t)std::max<long>(total, 1);
    st->ent_bytes = (TIP_Q * M + (M + 1) / 2) * sizeof(double);
    if (dev_alloc(c, st->ent_bytes, &st->ent) != SELLA_OK) { st->ent = nullptr; return SELLA_E_NOMEM; }
    st->q = st->ent;
    st->nbr = reinterpret_cast<int*>(st->ent + TIP_Q * M);
    st->off = doff;
    SCHK(h2d_async(c, doff, off.data(), ((size_t)n + 1) * sizeof(int)));
    TipFill f;
    f.off = doff; f.nbr = const_cast<int*>(st->nbr); f.q = st->ent; f.nvisit = (int)M;
    SELLA_LAUNCHB(c, tip3p_fill_kernel, tip3p_fill_vb, 256, dim3(n), dim3(256), 0, g, f);
    HIPCHK(hipGetLastError());
    return stream_wait(c);
}

void sella::tip3p_hvp_state_destroy(sella_ctx* c, TipHvpState* st) {
    if (st->geo) dev_free(c, st->geo, st->geo_bytes);
    if (st->ent) dev_free(c, st->ent, st->ent_bytes);
    st->geo = st->ent = nullptr;
}

static TipOp tip_op(const TipHvpState& st) {
    TipOp p;
    p.off = st.off; p.nbr = st.nbr; p.q = st.q; p.nvisit = std::max(st.nvisit, 1); p.nmol = st.nmol; p.o = st.o;
    return p;
}

// hv = H v (rows of 9 nmol on the device) and the free rows into y: one launch on the context's stream, nothing waited for
int sella::tip3p_hvp_state_apply(sella_ctx* c, const TipHvpState& st, const double* v, double* hv, const double* part, int nb,
                                 const int* inv, double* y, int* flag) {
    TipOut1 w;
    w.part = part; w.nb = nb; w.inv = inv; w.y = y; w.flag = flag;
    SELLA_LAUNCHB(c, tip3p_hvp1_kernel, tip3p_hvp1_vb, 256, dim3((st.nmol + TIP_W - 1) / TIP_W), dim3(256), 0, tip_op(st), v, hv, w);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

// Y[h] = (H v_h)[free] for the nh <= TIP_W rows of the panel V: one launch, nothing waited for
int sella::tip3p_hvp_state_apply_block(sella_ctx* c, const TipHvpState& st, const double* V, int ldv, int nh, const int* inv,
                                       double* Y, int ldy) {
    TipBlock b;
    b.V = V; b.ldv = ldv; b.nh = nh; b.inv = inv; b.Y = Y; b.ldy = ldy;
    SELLA_LAUNCHB(c, tip3p_hvpb_kernel, tip3p_hvpb_vb, 256, dim3(st.nmol), dim3(256), 0, tip_op(st), b);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

int sella::tip3p_hvp_state_diag(sella_ctx* c, const TipHvpState& st, const int* inv, double* y) {
    SELLA_LAUNCHB(c, tip3p_hdiag_kernel, tip3p_hdiag_vb, 256, dim3((st.nmol + TIP_W - 1) / TIP_W), dim3(256), 0, tip_op(st), inv, y);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

// the state of this geometry for the length of the call, the vectors through the block kernel in chunks of TIP_W rows
int sella::tip3p_hvp_resident(sella_ctx* c, const TipPot& pot, const double* pos, const double* V, int k, double* HV) {
    struct Held {
        sella_ctx* c;
        TipHvpState st;
        ~Held() { (void)stream_sync_raw(c); tip3p_hvp_state_destroy(c, &st); }
    } held{c, {}};
    SCHK(tip3p_hvp_state_create(c, pot, pos, &held.st));
    const size_t n9 = (size_t)9 * pot.nmol;
    double* buf;
    SCHK(scratch_get(c, SCR_MISC0, 2 * TIP_W * n9 * sizeof(double), &buf));
    double *dV = buf, *dY = buf + TIP_W * n9;
    for (int r0 = 0; r0 < k; r0 += TIP_W) {
        const int nh = std::min(TIP_W, k - r0);
        SCHK(h2d_async(c, dV, V + (size_t)r0 * n9, (size_t)nh * n9 * sizeof(double)));
        SCHK(tip3p_hvp_state_apply_block(c, held.st, dV, (int)n9, nh, nullptr, dY, (int)n9));
        SCHK(d2h_async(c, HV + (size_t)r0 * n9, dY, (size_t)nh * n9 * sizeof(double)));
        SCHK(stream_wait(c));
    }
    return SELLA_OK;
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
static int tip_check(const char* who, sella_ctx* c, int nmol, const double* pos, int o, const double* box, const double* params,
                     TipPot* pot) {
    const char* bad = !c ? "invalid arguments" : tip3p_pot_make(nmol, pos, o, box, params, pot);
    if (!bad) return SELLA_OK;
    set_error("%s: %s", who, bad);
    return SELLA_E_INVALID;
}

extern "C" int sella_tip3p_eval(sella_ctx* c, int n_mol, const double* pos, int o, const double* box, const double* params,
                                double* energy, double* grad) {
    TipPot pot;
    SCHK(tip_check("tip3p_eval", c, n_mol, pos, o, box, params, &pot));
    if (!energy || !grad) {
        set_error("tip3p_eval: invalid arguments");
        return SELLA_E_INVALID;
    }
    return tip3p_eval_resident(c, pot, pos, energy, grad);
}

extern "C" int sella_tip3p_hessian(sella_ctx* c, int n_mol, const double* pos, int o, const double* box, const double* params,
                                   sella_mat out) {
    TipPot pot;
    SCHK(tip_check("tip3p_hessian", c, n_mol, pos, o, box, params, &pot));
    return tip3p_hessian_resident(c, pot, pos, out);
}

extern "C" int sella_tip3p_hvp(sella_ctx* c, int n_mol, const double* pos, int o, const double* box, const double* params,
                               const double* V, int k, double* HV) {
    TipPot pot;
    SCHK(tip_check("tip3p_hvp", c, n_mol, pos, o, box, params, &pot));
    if (!V || k <= 0 || !HV) {
        set_error("tip3p_hvp: invalid arguments");
        return SELLA_E_INVALID;
    }
    return tip3p_hvp_resident(c, pot, pos, V, k, HV);
}
