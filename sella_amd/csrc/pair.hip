// pair.hip — pair potentials on the device: E = 1/2 sum over the ordered visits (i <- j, image s) of phi(r),
// r = |x_j + S_s - x_i|, with phi the Morse or the Lennard-Jones function, plain (no cutoff: clusters) or in shifted-force
// form inside a cutoff (pair_pot.h).  The potential of the reference's integration test (tests/integration/
// test_morse_cluster.py) and of the classic cluster benchmarks, as a calculator that lives in the library (calc.hip, kind 2).
//
// Same all-pairs shape as emt.hip: one workgroup of 256 per atom i, the (neighbour, image) pairs of the atom through EMT's
// sweep (emt_pairs, emt.h: distance test first, the radial function for the pairs inside the cutoff only), every sum per
// thread in the order of the sweep and then reduced with block_sum's arithmetic — no atomics, the same bits from run to run
// and whether or not a thread's list overflowed (emt_hcap).  One radial form per kernel instantiation.
//   eval:     ONE pass (there is no density): per-atom energy 1/2 sum phi, gradient -sum (phi'/r) d over the visits j != i,
//             optionally the virial 1/2 sum (phi'/r) d (x) d.  A visit of an atom to its own image adds 1/2 phi to the energy
//             and its share to the virial (its distance depends on the cell), nothing to the gradient.
//   hessian:  row block i of H: -K on (i, j), sum K on (i, i), K = phi'' u u^T + (phi'/r)(I - u u^T).  Thread t owns the atoms
//             j = t, t + 256, ... through ALL their images, so a block (i, j) has one writer whatever the number of images
//             and no barrier is needed; then (H + H^T) / 2.  No embedding term: no matrix product.
//   product:  (H v)_i = sum over the visits j != i of K (v_i - v_j): a single gather pass (no dots pass: there is no c_i).
//             The operator (calc.hip, sella_hvp) keeps the visits of its geometry with u, phi'/r and phi'' - phi'/r
//             (PairHvpState, pair.h), so a product evaluates no exp, sqrt or division; the products with host vectors
//             (sella_pair_hvp) build that state for the length of the call.
// The pair terms are rounded product by product (no contraction into fused multiply-adds): a kernel with and without the
// virial, and a vector in one row of a block or another, then give the same bits.
#include <algorithm>
#include <vector>

#include "pair.h"

namespace sella {
namespace {

struct PairVisit {
    int j;
    double dx, dy, dz, r;
};
// the visit t = (image << 24 | neighbour) of the atom at (xi, yi, zi); false: outside the cutoff, or the atom itself
__device__ __forceinline__ bool pair_visit(const EmtArgs& g, double xi, double yi, double zi, int t, PairVisit& v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int j = t & 0xffffff, s = t >> 24;
    v.j = j;
    v.dx = g.pos[3 * j] + g.shifts[3 * s] - xi;
    v.dy = g.pos[3 * j + 1] + g.shifts[3 * s + 1] - yi;
    v.dz = g.pos[3 * j + 2] + g.shifts[3 * s + 2] - zi;
    v.r = sqrt(v.dx * v.dx + v.dy * v.dy + v.dz * v.dz);
    return v.r < g.cutoff && v.r > 1e-8;
}

// VIRIAL: the six per-atom virial sums (xx, yy, zz, yz, xz, xy) to grad + 3 n + 6 i, as emt_force_virial does
template <int FORM, bool VIRIAL>
__device__ __forceinline__ void pair_eval_body(const VB vb, PairArgs a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double part[4][10];
    __shared__ int hits[256][EMT_HCAP + 1];
    __shared__ EmtStage stage;
    const int i = vb.x;
    const double xi = a.g.pos[3 * i], yi = a.g.pos[3 * i + 1], zi = a.g.pos[3 * i + 2];
    double e = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    double wxx = 0.0, wyy = 0.0, wzz = 0.0, wyz = 0.0, wxz = 0.0, wxy = 0.0;
    auto heavy = [&](int t) {
        PairVisit v;
        if (!pair_visit(a.g, xi, yi, zi, t, v)) return;
        const PairRadial q = pair_radial<FORM>(a.pot, v.r);
        e += 0.5 * q.phi;
        const double f = q.d1 / v.r;                            // dr/dx_i = -(d / r)
        if (v.j != i) {
            gx -= f * v.dx;
            gy -= f * v.dy;
            gz -= f * v.dz;
        }
        if constexpr (VIRIAL) {
            const double h = 0.5 * f;
            wxx += h * (v.dx * v.dx); wyy += h * (v.dy * v.dy); wzz += h * (v.dz * v.dz);
            wyz += h * (v.dy * v.dz); wxz += h * (v.dx * v.dz); wxy += h * (v.dx * v.dy);
        }
    };
    (void)emt_pairs(a.g, xi, yi, zi, &stage, hits, heavy);
    block_put<10>(part, 0, e);
    block_put<10>(part, 1, gx); block_put<10>(part, 2, gy); block_put<10>(part, 3, gz);
    if constexpr (VIRIAL) {
        block_put<10>(part, 4, wxx); block_put<10>(part, 5, wyy); block_put<10>(part, 6, wzz);
        block_put<10>(part, 7, wyz); block_put<10>(part, 8, wxz); block_put<10>(part, 9, wxy);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    a.g.eatom[i] = block_total<10>(part, 0);
    for (int k = 0; k < 3; ++k) a.g.grad[3 * i + k] = block_total<10>(part, 1 + k);
    if constexpr (VIRIAL) {
        double* w = a.g.grad + 3 * (size_t)a.g.n + 6 * (size_t)i;
        for (int k = 0; k < 6; ++k) w[k] = block_total<10>(part, 4 + k);
    }
}

// K = c1 I + c2 u u^T of a visit in the order xx, yy, zz, yz, xz, xy, added to k
__device__ __forceinline__ void pair_add_K(double c1, double c2, double ux, double uy, double uz, double k[6]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    k[0] += c1 + c2 * (ux * ux); k[1] += c1 + c2 * (uy * uy); k[2] += c1 + c2 * (uz * uz);
    k[3] += c2 * (uy * uz); k[4] += c2 * (ux * uz); k[5] += c2 * (ux * uy);
}

// Row block i of H (3n x 3n, rows ldh apart): every block (i, j) is written, so nothing has to be zero on entry
template <int FORM>
__device__ __forceinline__ void pair_hess_body(const VB vb, PairArgs a, double* __restrict__ H, int ldh) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double part[4][6];
    const int i = vb.x, n = a.g.n;
    const double xi = a.g.pos[3 * i], yi = a.g.pos[3 * i + 1], zi = a.g.pos[3 * i + 2];
    const double cut2 = a.g.cutoff * a.g.cutoff * (1.0 + 1e-12);
    double* H0 = H + (size_t)(3 * i) * ldh;
    double* H1 = H0 + ldh;
    double* H2 = H1 + ldh;
    double kd[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < n; j += 256) {
        if (j == i) continue;
        const double px = a.g.pos[3 * j], py = a.g.pos[3 * j + 1], pz = a.g.pos[3 * j + 2];
        double ks[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < a.g.nshift; ++s) {
            const double dx = px + a.g.shifts[3 * s] - xi, dy = py + a.g.shifts[3 * s + 1] - yi;
            const double dz = pz + a.g.shifts[3 * s + 2] - zi;
            const double d2 = dx * dx + dy * dy + dz * dz;
            if (!(d2 <= cut2)) continue;
            const double r = sqrt(d2);
            if (!(r < a.g.cutoff && r > 1e-8)) continue;
            const PairRadial q = pair_radial<FORM>(a.pot, r);
            const double c1 = q.d1 / r;
            pair_add_K(c1, q.d2 - c1, dx / r, dy / r, dz / r, ks);
        }
        const int c = 3 * j;
        H0[c] = -ks[0]; H0[c + 1] = -ks[5]; H0[c + 2] = -ks[4];
        H1[c] = -ks[5]; H1[c + 1] = -ks[1]; H1[c + 2] = -ks[3];
        H2[c] = -ks[4]; H2[c + 1] = -ks[3]; H2[c + 2] = -ks[2];
#pragma unroll
        for (int k = 0; k < 6; ++k) kd[k] += ks[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) block_put<6>(part, k, kd[k]);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[6];
    for (int k = 0; k < 6; ++k) s[k] = block_total<6>(part, k);
    const int c = 3 * i;
    H0[c] = s[0]; H0[c + 1] = s[5]; H0[c + 2] = s[4];
    H1[c] = s[5]; H1[c + 1] = s[1]; H1[c + 2] = s[3];
    H2[c] = s[4]; H2[c + 1] = s[3]; H2[c + 2] = s[2];
}

// ---- the visits of a geometry, kept for the operator ----------------------------------------------------------------------
// count: the visits j != i of atom i.  fill: the same sweep twice — every thread counts its own visits, an exclusive scan
// over the threads gives each its place behind off[i], and the second sweep writes them there.
__device__ __forceinline__ void pair_count_vb(const VB vb, EmtArgs g, int* __restrict__ cnt) {
    __shared__ double red[4];
    __shared__ int hits[256][EMT_HCAP + 1];
    __shared__ EmtStage stage;
    const int i = vb.x;
    const double xi = g.pos[3 * i], yi = g.pos[3 * i + 1], zi = g.pos[3 * i + 2];
    int mine = 0;
    auto heavy = [&](int t) {
        PairVisit v;
        if (pair_visit(g, xi, yi, zi, t, v) && v.j != i) ++mine;
    };
    (void)emt_pairs(g, xi, yi, zi, &stage, hits, heavy);
    const double all = block_sum((double)mine, red);
    if (threadIdx.x == 0) cnt[i] = (int)all;
}
__global__ __launch_bounds__(256) void pair_count_kernel(EmtArgs g, int* __restrict__ cnt) { pair_count_vb(vb_hw(), g, cnt); }

struct PairFill {
    const int* off;         // n + 1
    int* nbr;
    double* q;              // 5 x nvisit
    int nvisit;
};
template <int FORM>
__device__ __forceinline__ void pair_fill_body(const VB vb, PairArgs a, PairFill o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ int scan[256];
    __shared__ int hits[256][EMT_HCAP + 1];
    __shared__ EmtStage stage;
    const int i = vb.x, tid = threadIdx.x;
    const double xi = a.g.pos[3 * i], yi = a.g.pos[3 * i + 1], zi = a.g.pos[3 * i + 2];
    int mine = 0;
    auto count = [&](int t) {
        PairVisit v;
        if (pair_visit(a.g, xi, yi, zi, t, v) && v.j != i) ++mine;
    };
    (void)emt_pairs(a.g, xi, yi, zi, &stage, hits, count);
    scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int below = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += below;
        __syncthreads();
    }
    const size_t M = (size_t)o.nvisit;
    int w = o.off[i] + scan[tid] - mine;
    const int end = o.off[i + 1];
    auto write = [&](int t) {
        PairVisit v;
        if (!(pair_visit(a.g, xi, yi, zi, t, v) && v.j != i)) return;
        if (w >= end) return;                                   // (never: the count was taken on the same positions)
        const PairRadial q = pair_radial<FORM>(a.pot, v.r);
        const double c1 = q.d1 / v.r;
        o.nbr[w] = v.j;
        o.q[w] = v.dx / v.r; o.q[M + w] = v.dy / v.r; o.q[2 * M + w] = v.dz / v.r;
        o.q[3 * M + w] = c1; o.q[4 * M + w] = q.d2 - c1;
        ++w;
    };
    (void)emt_pairs(a.g, xi, yi, zi, &stage, hits, write);
}

// ---- products on the kept visits --------------------------------------------------------------------------------------------
struct PairOp {
    const int* off;
    const int* nbr;
    const double* q;
    int nvisit;
};
struct PairEntry {
    int j;
    double ux, uy, uz, c1, c2;
};
__device__ __forceinline__ PairEntry pair_entry(const PairOp& o, int e) {
    const size_t M = (size_t)o.nvisit;
    PairEntry p;
    p.j = o.nbr[e];
    p.ux = o.q[e]; p.uy = o.q[M + e]; p.uz = o.q[2 * M + e]; p.c1 = o.q[3 * M + e]; p.c2 = o.q[4 * M + e];
    return p;
}

// One vector of the operator: v and hv are rows of its pair record (full length 3n).  |v|^2 comes in `nb` partial sums; a
// vanishing vector (|v| < 1e-12) gives a zero product and flag 0.  The rows of the free coordinates also go into the
// eigensolver's vector y (inv: full coordinate -> its index there, -1 if pinned; null: all free).
struct PairOut1 {
    const double* part; int nb;
    const int* inv;
    double* y;
    int* flag;
};
__device__ __forceinline__ void pair_hvp1_vb(const VB vb, PairOp o, const double* __restrict__ v, double* __restrict__ hv,
                                             PairOut1 w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double red1[4];
    __shared__ double part[4][3];
    double s = 0.0;
    for (int b = threadIdx.x; b < w.nb; b += 256) s += w.part[b];
    s = block_sum(s, red1);
    const bool live = !(sqrt(s) < 1e-12);
    if (vb.x == 0 && threadIdx.x == 0) *w.flag = live ? 1 : 0;
    const int i = vb.x;
    const double vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    const int hi = o.off[i + 1];
    for (int e = o.off[i] + threadIdx.x; e < hi; e += 256) {
        const PairEntry p = pair_entry(o, e);
        const double dx = vx - v[3 * p.j], dy = vy - v[3 * p.j + 1], dz = vz - v[3 * p.j + 2];
        const double t = p.c2 * (p.ux * dx + p.uy * dy + p.uz * dz);
        y0 += p.c1 * dx + t * p.ux;
        y1 += p.c1 * dy + t * p.uy;
        y2 += p.c1 * dz + t * p.uz;
    }
    block_put<3>(part, 0, y0); block_put<3>(part, 1, y1); block_put<3>(part, 2, y2);
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= 3) return;
    const double h = live ? block_total<3>(part, c) : 0.0;
    const int p = 3 * i + c, q = w.inv ? w.inv[p] : p;
    hv[p] = h;
    if (q >= 0) w.y[q] = h;
}
__global__ __launch_bounds__(256) void pair_hvp1_kernel(PairOp o, const double* __restrict__ v, double* __restrict__ hv,
                                                        PairOut1 w) { pair_hvp1_vb(vb_hw(), o, v, hv, w); }

// Up to PAIR_W vectors, the rows of a device panel (row h at V + h ldv, full length), all in one workgroup per atom: a visit
// is read once for all of them.  Rows beyond nh are never read (the row index is clamped: their slots repeat row nh - 1 and
// are not stored).  Every row's sums are taken in the order of the single-vector kernel with the same arithmetic, so a row's
// result does not depend on which row it is, on what stands in the other rows, or on nh.
constexpr int PAIR_W = 16;
struct PairBlock {
    const double* V; int ldv;
    int nh;
    const int* inv;
    double* Y; int ldy;
};
__device__ __forceinline__ void pair_hvpb_vb(const VB vb, PairOp o, PairBlock b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double part[4][3 * PAIR_W];
    const int i = vb.x;
    double acc[PAIR_W][3];
#pragma unroll
    for (int q = 0; q < PAIR_W; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0.0;
    const int hi = o.off[i + 1];
    for (int e = o.off[i] + threadIdx.x; e < hi; e += 256) {
        const PairEntry p = pair_entry(o, e);
#pragma unroll
        for (int q = 0; q < PAIR_W; ++q) {
            const double* v = b.V + (size_t)(q < b.nh ? q : b.nh - 1) * b.ldv;
            const double dx = v[3 * i] - v[3 * p.j], dy = v[3 * i + 1] - v[3 * p.j + 1], dz = v[3 * i + 2] - v[3 * p.j + 2];
            const double t = p.c2 * (p.ux * dx + p.uy * dy + p.uz * dz);
            acc[q][0] += p.c1 * dx + t * p.ux;
            acc[q][1] += p.c1 * dy + t * p.uy;
            acc[q][2] += p.c1 * dz + t * p.uz;
        }
    }
#pragma unroll
    for (int q = 0; q < PAIR_W; ++q) {
        block_put<3 * PAIR_W>(part, 3 * q, acc[q][0]);
        block_put<3 * PAIR_W>(part, 3 * q + 1, acc[q][1]);
        block_put<3 * PAIR_W>(part, 3 * q + 2, acc[q][2]);
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= 3 * PAIR_W) return;
    const int q = t / 3, c = t - 3 * q;
    const int p = 3 * i + c, r = b.inv ? b.inv[p] : p;
    if (q < b.nh && r >= 0) b.Y[(size_t)q * b.ldy + r] = block_total<3 * PAIR_W>(part, t);
}
__global__ __launch_bounds__(256) void pair_hvpb_kernel(PairOp o, PairBlock b) { pair_hvpb_vb(vb_hw(), o, b); }

// diag(H)[free]: H[(i,a),(i,a)] = sum over the visits of K_aa
__device__ __forceinline__ void pair_hdiag_vb(const VB vb, PairOp o, const int* __restrict__ inv, double* __restrict__ y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double part[4][3];
    const int i = vb.x;
    double k[3] = {0.0, 0.0, 0.0};
    const int hi = o.off[i + 1];
    for (int e = o.off[i] + threadIdx.x; e < hi; e += 256) {
        const PairEntry p = pair_entry(o, e);
        k[0] += p.c1 + p.c2 * (p.ux * p.ux);
        k[1] += p.c1 + p.c2 * (p.uy * p.uy);
        k[2] += p.c1 + p.c2 * (p.uz * p.uz);
    }
    block_put<3>(part, 0, k[0]); block_put<3>(part, 1, k[1]); block_put<3>(part, 2, k[2]);
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= 3) return;
    const int p = 3 * i + c, r = inv ? inv[p] : p;
    if (r >= 0) y[r] = block_total<3>(part, c);
}
__global__ __launch_bounds__(256) void pair_hdiag_kernel(PairOp o, const int* __restrict__ inv, double* __restrict__ y) {
    pair_hdiag_vb(vb_hw(), o, inv, y);
}

// one kernel and one batchable body per radial form (the launch macro takes plain names)
#define PAIR_FORMS(name, use, ...)                                                                                          \
    __device__ __forceinline__ void name##_morse_vb(const VB vb, __VA_ARGS__) { name##_body<PAIR_MORSE> use; }                  \
    __device__ __forceinline__ void name##_lj_vb(const VB vb, __VA_ARGS__) { name##_body<PAIR_LJ> use; }                        \
    __global__ __launch_bounds__(256) void name##_morse_kernel(__VA_ARGS__) { const VB vb = vb_hw(); name##_body<PAIR_MORSE> use; } \
    __global__ __launch_bounds__(256) void name##_lj_kernel(__VA_ARGS__) { const VB vb = vb_hw(); name##_body<PAIR_LJ> use; }
template <int FORM> __device__ __forceinline__ void pair_force_body(const VB vb, PairArgs a) { pair_eval_body<FORM, false>(vb, a); }
template <int FORM> __device__ __forceinline__ void pair_force_virial_body(const VB vb, PairArgs a) { pair_eval_body<FORM, true>(vb, a); }
PAIR_FORMS(pair_force, (vb, a), PairArgs a)
PAIR_FORMS(pair_force_virial, (vb, a), PairArgs a)
PAIR_FORMS(pair_hess, (vb, a, H, ldh), PairArgs a, double* __restrict__ H, int ldh)
PAIR_FORMS(pair_fill, (vb, a, o), PairArgs a, PairFill o)
#undef PAIR_FORMS

}  // namespace
}  // namespace sella

using namespace sella;

// `launch` with the instantiation of kernel family `name` for `form`
#define PAIR_LAUNCH(c, form, name, grid, ...)                                                                    \
    do {                                                                                                         \
        if ((form) == PAIR_MORSE)                                                                                \
            SELLA_LAUNCHB(c, name##_morse_kernel, name##_morse_vb, 256, grid, dim3(256), 0, __VA_ARGS__);        \
        else                                                                                                     \
            SELLA_LAUNCHB(c, name##_lj_kernel, name##_lj_vb, 256, grid, dim3(256), 0, __VA_ARGS__);              \
    } while (0)

static PairArgs pair_args(sella_ctx* c, int n, int nshift, const PairPot& pot, const double* dpos, const double* dsh) {
    PairArgs a;
    memset(&a, 0, sizeof(a));
    a.g.n = n; a.g.nshift = nshift; a.g.pos = dpos; a.g.shifts = dsh;
    a.g.hcap = (int)std::min<long>(std::max<long>(c->opt.emt_hcap, 1), EMT_HCAP);
    a.g.cutoff = pot.cutoff;
    a.pot = pot;
    return a;
}

int sella::pair_queue(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift, const double* shifts,
                      const double* dshifts, double** eatom, double** grad, bool virial) {
    // positions | shifts | per-atom energies | gradient | per-atom virials (always part of the layout)
    const size_t words = (size_t)3 * n + (size_t)3 * nshift + (size_t)n + (size_t)3 * n + (size_t)6 * n;
    double* buf;
    SCHK(scratch_get(c, SCR_MISC0, words * sizeof(double), &buf));
    double* dpos = buf;
    double* dsh = dpos + 3 * (size_t)n;
    double* dea = dsh + 3 * (size_t)nshift;
    SCHK(h2d_async(c, dpos, pos, (size_t)3 * n * sizeof(double)));
    if (dshifts) dsh = const_cast<double*>(dshifts);
    else SCHK(h2d_async(c, dsh, shifts, (size_t)3 * nshift * sizeof(double)));
    PairArgs a = pair_args(c, n, nshift, pot, dpos, dsh);
    a.g.eatom = dea; a.g.grad = dea + n;
    if (virial) PAIR_LAUNCH(c, form, pair_force_virial, dim3(n), a);
    else PAIR_LAUNCH(c, form, pair_force, dim3(n), a);
    HIPCHK(hipGetLastError());
    *eatom = a.g.eatom;
    *grad = a.g.grad;
    return SELLA_OK;
}

// energy, gradient and (virial6 != nullptr) the six virial sums: one upload, one kernel, one read-back; the per-atom numbers
// are summed here in index order
int sella::pair_eval_resident(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift,
                              const double* shifts, const double* dshifts, double* energy, double* grad, double* virial6) {
    double *dea, *dgr;
    SCHK(pair_queue(c, n, pos, form, pot, nshift, shifts, dshifts, &dea, &dgr, virial6 != nullptr));
    const size_t nout = (size_t)(virial6 ? 10 : 4) * n;
    std::vector<double>& out = c->hbuf_b;
    out.resize(nout);
    SCHK(d2h_async(c, out.data(), dea, nout * sizeof(double)));
    SCHK(stream_wait(c));
    double e = 0.0;
    for (int i = 0; i < n; ++i) e += out[i];
    *energy = e;
    for (size_t i = 0; i < (size_t)3 * n; ++i) grad[i] = out[(size_t)n + i];
    if (virial6) {
        const double* w = out.data() + (size_t)4 * n;
        for (int k = 0; k < 6; ++k) {
            double v = 0.0;
            for (int i = 0; i < n; ++i) v += w[6 * (size_t)i + k];
            virial6[k] = v;
        }
    }
    return SELLA_OK;
}

int sella::pair_hessian_resident(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift,
                                 const double* shifts, const double* dshifts, sella_mat out) {
    Mat* H = mat_get(c, out);
    if (!H || H->rows != 3 * n || H->cols != 3 * n) {
        set_error("pair_hessian: out must be the %d x %d matrix of %d atoms", 3 * n, 3 * n, n);
        return SELLA_E_INVALID;
    }
    double* buf;
    SCHK(scratch_get(c, SCR_MISC0, ((size_t)3 * n + (size_t)3 * nshift) * sizeof(double), &buf));
    double* dsh = buf + 3 * (size_t)n;
    SCHK(h2d_async(c, buf, pos, (size_t)3 * n * sizeof(double)));
    if (dshifts) dsh = const_cast<double*>(dshifts);
    else SCHK(h2d_async(c, dsh, shifts, (size_t)3 * nshift * sizeof(double)));
    const PairArgs a = pair_args(c, n, nshift, pot, buf, dsh);
    HIPCHK(s_memset0(c, H->d, (size_t)H->rows * H->ld * sizeof(double)));
    PAIR_LAUNCH(c, form, pair_hess, dim3(n), a, H->d, H->ld);
    HIPCHK(hipGetLastError());
    // the two triangles agree to rounding only (x_j + shift - x_i from either end)
    SCHK(launch_symmetrize(c, H->d, 3 * n, H->ld));
    return stream_wait(c);
}

// ---- the resident state of the Hessian-vector operator (pair.h) ----------------------------------------------------------
int sella::pair_hvp_state_create(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift,
                                 const double* shifts, PairHvpState* st) {
    const size_t wpos = (size_t)3 * n, wsh = (size_t)3 * nshift, wcnt = ((size_t)n + 2) / 2, woff = ((size_t)n + 3) / 2;
    st->n = n;
    st->geo_bytes = (wpos + wsh + wcnt + woff) * sizeof(double);
    if (dev_alloc(c, st->geo_bytes, &st->geo) != SELLA_OK) { st->geo = nullptr; return SELLA_E_NOMEM; }
    double* dpos = st->geo;
    double* dsh = dpos + wpos;
    int* dcnt = reinterpret_cast<int*>(dsh + wsh);
    int* doff = reinterpret_cast<int*>(dsh + wsh + wcnt);
    SCHK(h2d_async(c, dpos, pos, wpos * sizeof(double)));
    SCHK(h2d_async(c, dsh, shifts, wsh * sizeof(double)));
    const PairArgs a = pair_args(c, n, nshift, pot, dpos, dsh);
    SELLA_LAUNCHB(c, pair_count_kernel, pair_count_vb, 256, dim3(n), dim3(256), 0, a.g, dcnt);
    HIPCHK(hipGetLastError());
    std::vector<int> off((size_t)n + 1, 0);
    SCHK(d2h_async(c, off.data() + 1, dcnt, (size_t)n * sizeof(int)));
    SCHK(stream_wait(c));
    long total = 0;
    for (int i = 0; i < n; ++i) {
        total += off[(size_t)i + 1];
        if (total > 0x7fffffffL) {
            set_error("pair hvp state: more than 2^31 visits");
            return SELLA_E_INVALID;
        }
        off[(size_t)i + 1] = (int)total;
    }
    st->nvisit = (int)total;
    const size_t M = (size_t)std::max<long>(total, 1);
    st->ent_bytes = (5 * M + (M + 1) / 2) * sizeof(double);
    if (dev_alloc(c, st->ent_bytes, &st->ent) != SELLA_OK) { st->ent = nullptr; return SELLA_E_NOMEM; }
    st->q = st->ent;
    st->nbr = reinterpret_cast<int*>(st->ent + 5 * M);
    st->off = doff;
    SCHK(h2d_async(c, doff, off.data(), ((size_t)n + 1) * sizeof(int)));
    PairFill f;
    f.off = doff; f.nbr = const_cast<int*>(st->nbr); f.q = st->ent; f.nvisit = (int)M;
    PAIR_LAUNCH(c, form, pair_fill, dim3(n), a, f);
    HIPCHK(hipGetLastError());
    return stream_wait(c);
}

void sella::pair_hvp_state_destroy(sella_ctx* c, PairHvpState* st) {
    if (st->geo) dev_free(c, st->geo, st->geo_bytes);
    if (st->ent) dev_free(c, st->ent, st->ent_bytes);
    st->geo = st->ent = nullptr;
}

static PairOp pair_op(const PairHvpState& st) {
    PairOp o;
    o.off = st.off; o.nbr = st.nbr; o.q = st.q; o.nvisit = std::max(st.nvisit, 1);
    return o;
}

// hv = H v (rows of 3n on the device) and the free rows into y: one launch on the context's stream, nothing waited for
int sella::pair_hvp_state_apply(sella_ctx* c, const PairHvpState& st, const double* v, double* hv, const double* part, int nb,
                                const int* inv, double* y, int* flag) {
    PairOut1 w;
    w.part = part; w.nb = nb; w.inv = inv; w.y = y; w.flag = flag;
    SELLA_LAUNCHB(c, pair_hvp1_kernel, pair_hvp1_vb, 256, dim3(st.n), dim3(256), 0, pair_op(st), v, hv, w);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

// Y[h] = (H v_h)[free] for the nh <= PAIR_W rows of the panel V: one launch, nothing waited for
int sella::pair_hvp_state_apply_block(sella_ctx* c, const PairHvpState& st, const double* V, int ldv, int nh, const int* inv,
                                      double* Y, int ldy) {
    PairBlock b;
    b.V = V; b.ldv = ldv; b.nh = nh; b.inv = inv; b.Y = Y; b.ldy = ldy;
    SELLA_LAUNCHB(c, pair_hvpb_kernel, pair_hvpb_vb, 256, dim3(st.n), dim3(256), 0, pair_op(st), b);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

int sella::pair_hvp_state_diag(sella_ctx* c, const PairHvpState& st, const int* inv, double* y) {
    SELLA_LAUNCHB(c, pair_hdiag_kernel, pair_hdiag_vb, 256, dim3(st.n), dim3(256), 0, pair_op(st), inv, y);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

// the state of this geometry for the length of the call, the vectors through the block kernel in chunks of PAIR_W rows
int sella::pair_hvp_resident(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift,
                             const double* shifts, const double* V, int k, double* HV) {
    struct Held {
        sella_ctx* c;
        PairHvpState st;
        ~Held() { (void)stream_sync_raw(c); pair_hvp_state_destroy(c, &st); }
    } held{c, {}};
    SCHK(pair_hvp_state_create(c, n, pos, form, pot, nshift, shifts, &held.st));
    const size_t n3 = (size_t)3 * n;
    double* buf;
    SCHK(scratch_get(c, SCR_MISC0, 2 * PAIR_W * n3 * sizeof(double), &buf));
    double *dV = buf, *dY = buf + PAIR_W * n3;
    for (int r0 = 0; r0 < k; r0 += PAIR_W) {
        const int nh = std::min(PAIR_W, k - r0);
        SCHK(h2d_async(c, dV, V + (size_t)r0 * n3, (size_t)nh * n3 * sizeof(double)));
        SCHK(pair_hvp_state_apply_block(c, held.st, dV, (int)n3, nh, nullptr, dY, (int)n3));
        SCHK(d2h_async(c, HV + (size_t)r0 * n3, dY, (size_t)nh * n3 * sizeof(double)));
        SCHK(stream_wait(c));
    }
    return SELLA_OK;
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
static int pair_check(const char* who, sella_ctx* c, int n, const double* pos, int form, const double* params, int nshift,
                      const double* shifts, double rcut, PairPot* pot) {
    const char* bad = (!c || !pos) ? "invalid arguments" : pair_pot_make(n, form, params, nshift, shifts, rcut, pot);
    if (!bad) return SELLA_OK;
    set_error("%s: %s", who, bad);
    return SELLA_E_INVALID;
}

extern "C" int sella_pair_eval(sella_ctx* c, int n, const double* pos, int form, const double* params, int nshift,
                               const double* shifts, double rcut, double* energy, double* grad) {
    PairPot pot;
    SCHK(pair_check("pair_eval", c, n, pos, form, params, nshift, shifts, rcut, &pot));
    if (!energy || !grad) {
        set_error("pair_eval: invalid arguments");
        return SELLA_E_INVALID;
    }
    return pair_eval_resident(c, n, pos, form, pot, nshift, shifts, nullptr, energy, grad, nullptr);
}

extern "C" int sella_pair_eval_stress(sella_ctx* c, int n, const double* pos, int form, const double* params, int nshift,
                                      const double* shifts, double rcut, double* energy, double* grad, double* virial6) {
    PairPot pot;
    SCHK(pair_check("pair_eval_stress", c, n, pos, form, params, nshift, shifts, rcut, &pot));
    if (!energy || !grad || !virial6) {
        set_error("pair_eval_stress: invalid arguments");
        return SELLA_E_INVALID;
    }
    return pair_eval_resident(c, n, pos, form, pot, nshift, shifts, nullptr, energy, grad, virial6);
}

extern "C" int sella_pair_hessian(sella_ctx* c, int n, const double* pos, int form, const double* params, int nshift,
                                  const double* shifts, double rcut, sella_mat out) {
    PairPot pot;
    SCHK(pair_check("pair_hessian", c, n, pos, form, params, nshift, shifts, rcut, &pot));
    return pair_hessian_resident(c, n, pos, form, pot, nshift, shifts, nullptr, out);
}

extern "C" int sella_pair_hvp(sella_ctx* c, int n, const double* pos, int form, const double* params, int nshift,
                              const double* shifts, double rcut, const double* V, int k, double* HV) {
    PairPot pot;
    SCHK(pair_check("pair_hvp", c, n, pos, form, params, nshift, shifts, rcut, &pot));
    if (!V || k <= 0 || !HV) {
        set_error("pair_hvp: invalid arguments");
        return SELLA_E_INVALID;
    }
    return pair_hvp_resident(c, n, pos, form, pot, nshift, shifts, V, k, HV);
}
