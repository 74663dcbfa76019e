// emt_hessian.hip — second derivatives of the effective-medium-theory energy of emt.hip: the dense Cartesian Hessian
// (a producer for `hessian_function`, left on the device) and Hessian-vector products without 3N x 3N storage.
//
// The energy is E = sum_i [Phi_i(sigma_i) - sum y], sigma_i = sum w over the ordered pairs (i <- j, image s), with w and
// y functions of the pair distance r alone.  Two differentiations give
//
//     H = sum_i F2_i g_i g_i^T  +  sum_pairs K (x) [(i,i) + (j,j) - (i,j) - (j,i)]
//
// with F2_i = Phi_i'', g_i = grad sigma_i (w' u on atom j, -w' u on atom i, u = d / r), and per ordered pair
// K = e2 u u^T + (e1 / r)(I - u u^T), e1 = F1_i w' - y', e2 = F1_i w'' - y'' (F1_i = Phi_i' = dEdsig of the force pass).
// A pair of an atom with its own image enters sigma_i (and so F1, F2) but its four blocks cancel and it adds nothing to
// g_i: such visits are skipped here.
//
// Same all-pairs structure as the force pass: one workgroup per atom i walks the neighbour lists its threads noted in the
// density pass and takes both ordered pairs (i <- j) and (j <- i) of a visit together (same distance).
//   dense:   emt_f2 (per atom) -> emt_hess_pair (row block i of H: -K off the diagonal, sum K on it; row i of G^T and of
//            diag(F2) G^T) -> H += G diag(F2) G^T on the matrix cores (launch_gemm) -> (H + H^T) / 2
//   product: emt_f2 -> dots (c_i = g_i . v) -> gather ((H v)_i from c_i, c_j and the pair blocks).  The two passes are
//            written once (emt_dots_body, emt_gather_body) over a description of the vectors a workgroup carries; the
//            kernels are its instantiations:
//              emt_hvp_dots, emt_hvp_gather     HVP_KQ rows of host vectors per workgroup
//              emt_hvp1_dots, emt_hvp1_gather   the operator: ONE vector (3 accumulators per thread instead of 24) on a state
//                    that is built once per geometry and owned by the operator (EmtHvpState: positions, sigma1, dEdsig, the
//                    lists, F2), device vector in, device vector out, nothing waited for (calc.hip, sella_hvp_*)
//              emt_hvpb_dots, emt_hvpb_gather   the up to 16 rows of a device panel on the same state, all in one workgroup
//                    per atom, the free rows written straight into the caller's panel — with the diagonal of H (emt_hdiag)
//                    the operator of the block Davidson
//              emt_chvp_dots, emt_chvp_gather   CHVP_KQ rows of positions and cell (below)
// No atomics: an atom can be a neighbour through several images, and those visits belong to different threads unless
// 256 divides N, so everything that lands in a shared place is added image by image with a barrier in between (one
// writer per (i, j) within an image, images in index order); per-thread sums run in the order of the lists and are
// reduced with block_sum's arithmetic, all sums of a kernel behind one barrier (block_put, block_total: emt.h).  The
// result does not depend on whether the lists were complete.
//
// The cell (sella_emt_cell_hessian).  The lattice vectors (rows of C) enter only through the image translations
// S_s = n_s C, n_s whole numbers: for a visit d = x_j + n_s C - x_i, so dd_a / dC_kb = n_k delta_ab, and in the coordinates
// [x; C.ravel()] (positions fixed while C varies) the same pair quantities give, with gamma_i = d sigma_i / dC,
//     gamma_i[(k,b)]   = sum_visits of i  w'_ij u_b n_k
//     A[(i,a),(k,b)]   = d2E / dx_ia dC_kb = - sum_visits of i, j != i  K_ab n_k  +  sum_m F2_m g_m[(i,a)] gamma_m[(k,b)]
//     B[(k,a),(l,b)]   = d2E / dC_ka dC_lb = 1/2 sum_all visits  K_ab n_k n_l   +  sum_m F2_m gamma_m[(k,a)] gamma_m[(l,b)]
// The pair term of B is sum over ORDERED pairs of their own K n_k n_l; a visit's K holds the ordered pairs (i <- j, s) and
// (j <- i, -s), whose n_k n_l agree, and each of the two is met again in the visit from the other end: hence the 1/2.  A
// visit of an atom to its own image s holds (i <- i, s) and (i <- i, -s), both met again in the visit to image -s: the
// same 1/2.  Those visits move no position block (x_i - x_i cancels in d) but d = n_s C does depend on the cell, so the
// cell pass — and only it — takes them (emt_pair<true>), for gamma_i and B.
//   emt_hessian passes into the leading 3n x 3n block -> emt_cell_pair (per atom: the pair term of row block i of A, row i
//   of gamma, atom i's share of B: 36 numbers, K_ab n_k n_l being symmetric in (a,b) and in (k,l)) -> emt_cell_embed (A +=
//   (diag(F2) G^T)^T gamma) -> emt_cell_finish (B from the shares and gamma, summed in a fixed order; A^T into the last rows)
//
// The product with that Hessian (sella_emt_cell_hvp).  A direction [v; W] (W the 3 x 3 variation of C) displaces the pair
// of a visit by dd = v_j - v_i + n_s W (for an own image: n_s W), and [A-part; B-part] applied to it is, with
// c_i = g_i . v + gamma_i . W = sum_all visits of i  w'_ij u . dd,
//     (y_x)_i      = - sum_visits of i, j != i  [ K dd + u (F2_i c_i w'_ij + F2_j c_j w'_ji) ]
//     y_C[(k,b)]   = sum_i s_i[(k,b)],   s_i[(k,b)] = sum_all visits of i  n_k [ 1/2 (K dd)_b + F2_i c_i w'_ij u_b ]
// (the 1/2 of B; the second term of s_i is F2_i c_i gamma_i): the two passes of the product at fixed cell with dd in place
// of v_j - v_i and own images included, nine more sums per vector, and a sum over the atoms in a fixed order.
//   emt_f2 -> emt_chvp_dots (c_i) -> emt_chvp_gather ((y_x)_i and s_i; the table T_q[s] = n_s W_q of every vector comes from
//   the host) -> emt_chvp_finish (y_C), CHVP_KQ vectors per workgroup; nothing of size (3n)^2 is formed
#include <cmath>
#include <type_traits>

#include "emt.h"

namespace sella {
namespace {

constexpr int HVP_KQ = 8;                  // vectors of a product a workgroup carries (3 HVP_KQ accumulators per thread)

// d2 Phi_i / d sigma_i^2 from the density of the density pass
__device__ __forceinline__ void emt_f2_vb(const VB vb, EmtArgs a, double* __restrict__ F2) {
    const int i = vb.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const double sig = a.sigma1[i];
    const double cs = 1.0 / (a.beta * a.p.eta2[i]);                  // ds = -cs log(sigma / 12)
    const double ds = -log(sig / 12.0) * cs;
    const double lam = a.p.lam[i], kap = a.p.kappa[i], E0 = a.p.E0[i];
    const double xl = lam * ds, yl = exp(-xl);
    const double z = 6.0 * a.p.V0[i] * exp(-kap * ds);
    const double d1 = -E0 * lam * xl * yl - kap * z;                 // dPhi / dds
    const double d2 = -E0 * lam * lam * yl * (1.0 - xl) + kap * kap * z;
    const double q = cs / sig;                                       // -dds / dsigma;  d2ds / dsigma2 = q / sigma
    F2[i] = d2 * q * q + d1 * q / sig;
}
__global__ __launch_bounds__(256) void emt_f2_kernel(EmtArgs a, double* __restrict__ F2) { emt_f2_vb(vb_hw(), a, F2); }

struct EmtAtom {                            // what the pair terms need of the workgroup's own atom
    int i;
    double x, y, z, n0, g1, g2, V0, eta2, kap, s0, F1;
};
__device__ __forceinline__ EmtAtom emt_atom(const EmtArgs& a, int i) {
    EmtAtom m;
    m.i = i;
    m.x = a.pos[3 * i]; m.y = a.pos[3 * i + 1]; m.z = a.pos[3 * i + 2];
    m.n0 = a.p.n0[i]; m.g1 = a.p.gamma1[i]; m.g2 = a.p.gamma2[i]; m.V0 = a.p.V0[i];
    m.eta2 = a.p.eta2[i]; m.kap = a.p.kappa[i]; m.s0 = a.p.s0[i]; m.F1 = a.dEdsig[i];
    return m;
}

struct EmtPair {                            // one visit (neighbour j through image s), both ordered pairs
    int j;
    double r, ux, uy, uz;
    double wp_ij, wp_ji;                    // dw/dr of (i <- j) and of (j <- i)
    double e1, e2;                          // first and second radial derivative of the energy of the two pairs
};
// false: not a pair (outside the cutoff, the atom itself, or the atom's own image).  SELF: the atom's own images are
// pairs too (the cell pass: their distance depends on the cell); j = i, and both ordered pairs are (i <- i).
template <bool SELF = false>
__device__ __forceinline__ bool emt_pair(const EmtArgs& a, const EmtAtom& m, int t, EmtPair& p) {
    const int j = t & 0xffffff, s = t >> 24;
    if (!SELF && j == m.i) return false;
    const double dx = a.pos[3 * j] + a.shifts[3 * s] - m.x;
    const double dy = a.pos[3 * j + 1] + a.shifts[3 * s + 1] - m.y;
    const double dz = a.pos[3 * j + 2] + a.shifts[3 * s + 2] - m.z;
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    if (!(r < a.cutoff && r > 1e-8)) return false;
    const double x = exp(a.acut * (r - a.rc));
    const double theta = 1.0 / (1.0 + x);
    const double L = -a.acut * x * theta;                            // theta' / theta
    const double Lp = L * (a.acut + L);                              // its derivative
    const double chi = a.p.n0[j] / m.n0;
    const double eta2j = a.p.eta2[j], kapj = a.p.kappa[j], s0j = a.p.s0[j];
    const double w_ij = exp(-eta2j * (r - a.beta * s0j)) * chi * theta / m.g1;
    const double y_ij = 0.5 * m.V0 * exp(-kapj * (r / a.beta - s0j)) * chi / m.g2 * theta;
    const double w_ji = exp(-m.eta2 * (r - a.beta * m.s0)) / chi * theta / a.p.gamma1[j];
    const double y_ji = 0.5 * a.p.V0[j] * exp(-m.kap * (r / a.beta - m.s0)) / chi / a.p.gamma2[j] * theta;
    const double aw_ij = -eta2j + L, ay_ij = -kapj / a.beta + L;     // logarithmic derivatives
    const double aw_ji = -m.eta2 + L, ay_ji = -m.kap / a.beta + L;
    const double F1j = a.dEdsig[j];
    p.j = j;
    p.r = r;
    p.ux = dx / r; p.uy = dy / r; p.uz = dz / r;
    p.wp_ij = w_ij * aw_ij;
    p.wp_ji = w_ji * aw_ji;
    p.e1 = m.F1 * p.wp_ij - y_ij * ay_ij + F1j * p.wp_ji - y_ji * ay_ji;
    p.e2 = m.F1 * w_ij * (aw_ij * aw_ij + Lp) - y_ij * (ay_ij * ay_ij + Lp)
           + F1j * w_ji * (aw_ji * aw_ji + Lp) - y_ji * (ay_ji * ay_ji + Lp);
    return true;
}

// Every (neighbour, image) candidate of atom i's workgroup through `visit`, image by image: each thread takes its own
// candidates (t = s n + j = tid mod 256, as in the density pass) in increasing t, from the list it noted there, or — if
// any thread's list overflowed — from a sweep over all its candidates (visit() tests the distance itself, so both ways
// see the same pairs in the same order).  SYNC: a barrier after every image, for visits that add into places other
// threads add into through other images.
template <bool SYNC, class Visit>
__device__ __forceinline__ void emt_by_image(const EmtArgs& a, int i, int* incomplete, Visit visit) {
    const int tid = threadIdx.x, n = a.n;
    const int* lst = a.nbr + ((size_t)i * 256 + tid) * (EMT_HCAP + 1);
    const int cnt = lst[0];
    if (tid == 0) *incomplete = 0;
    __syncthreads();
    if (cnt < 0) *incomplete = 1;
    __syncthreads();
    if (*incomplete) {
        for (int s = 0; s < a.nshift; ++s) {
            for (int j = (((tid - s * n) % 256) + 256) % 256; j < n; j += 256) visit(emt_pack(j, s));
            if (SYNC) __syncthreads();
        }
    } else {
        int h = 0;
        for (int s = 0; s < a.nshift; ++s) {
            while (h < cnt && (lst[1 + h] >> 24) == s) visit(lst[1 + h++]);
            if (SYNC) __syncthreads();
        }
    }
}

// symmetric index of (a, b), a, b in 0..2, in the order xx, yy, zz, yz, xz, xy
__host__ __device__ __forceinline__ int sym6(int a, int b) { return a == b ? a : 6 - a - b; }

// K = c1 I + c2 u u^T of a visit, in the order of sym6
__device__ __forceinline__ void emt_pair_K(const EmtPair& p, double K[6]) {
    const double c1 = p.e1 / p.r, c2 = p.e2 - c1;
    K[0] = c1 + c2 * (p.ux * p.ux); K[1] = c1 + c2 * (p.uy * p.uy); K[2] = c1 + c2 * (p.uz * p.uz);
    K[3] = c2 * (p.uy * p.uz); K[4] = c2 * (p.ux * p.uz); K[5] = c2 * (p.ux * p.uy);
}

struct EmtHessOut {
    const double* F2;
    double* H; int ldh;                     // 3n x 3n, zero on entry
    double* Gt; double* Gs; int ldg;        // n x 3n each: row i = g_i (zero on entry) and F2_i g_i
};

// Row block i of the pair term of H, and rows i of G^T and diag(F2) G^T.
__device__ __forceinline__ void emt_hess_pair_vb(const VB vb, EmtArgs a, EmtHessOut o) {
    __shared__ double part[4][9];
    __shared__ int incomplete;
    const int i = vb.x;
    const EmtAtom m = emt_atom(a, i);
    double* H0 = o.H + (size_t)(3 * i) * o.ldh;
    double* H1 = H0 + o.ldh;
    double* H2 = H1 + o.ldh;
    double* G = o.Gt + (size_t)i * o.ldg;
    double kd[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                                // diagonal block: sum of K
    double gx = 0.0, gy = 0.0, gz = 0.0;                                          // g_i on atom i: -sum w' u
    auto visit = [&](int t) {
        EmtPair p;
        if (!emt_pair(a, m, t, p)) return;
        double K[6];
        emt_pair_K(p, K);
        const int q = 3 * p.j;
        H0[q] -= K[0]; H0[q + 1] -= K[5]; H0[q + 2] -= K[4];
        H1[q] -= K[5]; H1[q + 1] -= K[1]; H1[q + 2] -= K[3];
        H2[q] -= K[4]; H2[q + 1] -= K[3]; H2[q + 2] -= K[2];
#pragma unroll
        for (int c = 0; c < 6; ++c) kd[c] += K[c];
        const double wx = p.wp_ij * p.ux, wy = p.wp_ij * p.uy, wz = p.wp_ij * p.uz;
        G[q] += wx; G[q + 1] += wy; G[q + 2] += wz;
        gx -= wx; gy -= wy; gz -= wz;
    };
    emt_by_image<true>(a, i, &incomplete, visit);
#pragma unroll
    for (int c = 0; c < 6; ++c) block_put<9>(part, c, kd[c]);
    block_put<9>(part, 6, gx); block_put<9>(part, 7, gy); block_put<9>(part, 8, gz);
    __syncthreads();
    if (threadIdx.x == 0) {
        double s[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) s[c] = block_total<9>(part, c);
        const int q = 3 * i;
        H0[q] = s[0]; H0[q + 1] = s[5]; H0[q + 2] = s[4];
        H1[q] = s[5]; H1[q + 1] = s[1]; H1[q + 2] = s[3];
        H2[q] = s[4]; H2[q + 1] = s[3]; H2[q + 2] = s[2];
        G[q] = s[6]; G[q + 1] = s[7]; G[q + 2] = s[8];
    }
    __syncthreads();
    const double f2 = o.F2[i];
    double* Gs = o.Gs + (size_t)i * o.ldg;
    for (int q = threadIdx.x; q < 3 * a.n; q += 256) Gs[q] = f2 * G[q];
}
__global__ __launch_bounds__(256) void emt_hess_pair_kernel(EmtArgs a, EmtHessOut o) { emt_hess_pair_vb(vb_hw(), a, o); }

// ---- the two passes of a product ------------------------------------------------------------------------------------------
// One workgroup per atom i carries W vectors through both passes: the pair quantities of a visit are evaluated once for
// all of them.  What a kernel family chooses is a description P of its vectors:
//   P::W                    how many vectors (accumulators per thread: W in the dots pass, 3 W or 12 W in the gather pass)
//   P::CELL                 vectors [v; W] of positions and cell: an atom's own images are visits too, and the pair of a visit
//                           through image s is displaced by shift(q, s) = T_q[s] = n_s W_q more; nimg = the n_s
//   load(q, j, x)           x = row of atom j in vector q
//   c(q, j)                 where the dot c_j of vector q lives
//   P::Terms                the arithmetic of one vector in one visit, contracted or not (below)
// The arithmetic of one vector in a visit, d the displacement of the pair by the vector (row: the position rows; cell: the
// nine cell sums of a CELL description).  It stands twice because `#pragma
// clang fp contract` is lexical and no template can switch it: EmtTerms leaves the contraction into fused multiply-adds to
// the compiler, EmtTermsExact rounds every product on its own (the panel of the block product: see there).
struct EmtTerms {
    static __device__ __forceinline__ double dot(const EmtPair& p, const double d[3]) {                  // w'_ij u . d
        return p.wp_ij * (p.ux * d[0] + p.uy * d[1] + p.uz * d[2]);
    }
    // acc += K d - u (fi w'_ij + fj w'_ji), K = c1 I + c2 u u^T
    static __device__ __forceinline__ void row(const EmtPair& p, double c1, double c2, const double d[3], double fi, double fj,
                                               double acc[3]) {
        const double along = c2 * (p.ux * d[0] + p.uy * d[1] + p.uz * d[2]) - (fi * p.wp_ij + fj * p.wp_ji);
        acc[0] += c1 * d[0] + along * p.ux;
        acc[1] += c1 * d[1] + along * p.uy;
        acc[2] += c1 * d[2] + along * p.uz;
    }
    // CELL: acc9[3 k + b] += n_k [fi w'_ij u_b - 1/2 (K d)_b], the atom's share of the nine cell rows
    static __device__ __forceinline__ void cell(const EmtPair& p, double c1, double c2, const double d[3], double fi,
                                                const double nv[3], double* acc9) {
        const double u[3] = {p.ux, p.uy, p.uz};
        const double along = c2 * (p.ux * d[0] + p.uy * d[1] + p.uz * d[2]), own = fi * p.wp_ij;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double tb = own * u[b] - 0.5 * (c1 * d[b] + along * u[b]);
#pragma unroll
            for (int k = 0; k < 3; ++k) acc9[3 * k + b] += nv[k] * tb;
        }
    }
};
struct EmtTermsExact {
    static __device__ __forceinline__ double dot(const EmtPair& p, const double d[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        return p.wp_ij * (p.ux * d[0] + p.uy * d[1] + p.uz * d[2]);
    }
    static __device__ __forceinline__ void row(const EmtPair& p, double c1, double c2, const double d[3], double fi, double fj,
                                               double acc[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double along = c2 * (p.ux * d[0] + p.uy * d[1] + p.uz * d[2]) - (fi * p.wp_ij + fj * p.wp_ji);
        acc[0] += c1 * d[0] + along * p.ux;
        acc[1] += c1 * d[1] + along * p.uy;
        acc[2] += c1 * d[2] + along * p.uz;
    }
    // CELL: acc9[3 k + b] += n_k [fi w'_ij u_b - 1/2 (K d)_b], the atom's share of the nine cell rows
    static __device__ __forceinline__ void cell(const EmtPair& p, double c1, double c2, const double d[3], double fi,
                                                const double nv[3], double* acc9) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double u[3] = {p.ux, p.uy, p.uz};
        const double along = c2 * (p.ux * d[0] + p.uy * d[1] + p.uz * d[2]), own = fi * p.wp_ij;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double tb = own * u[b] - 0.5 * (c1 * d[b] + along * u[b]);
#pragma unroll
            for (int k = 0; k < 3; ++k) acc9[3 * k + b] += nv[k] * tb;
        }
    }
};

// c_i[q] = sum over the visits of w'_ij u . dd, dd = v_j - v_i (+ T_q[s]): g_i . v_q (+ gamma_i . W_q; for an own image
// dd = T_q[s])
template <class P>
__device__ __forceinline__ void emt_dots_body(const VB vb, const EmtArgs& a, const P& o) {
    __shared__ double part[4][P::W];
    __shared__ int incomplete;
    const int i = vb.x;
    const EmtAtom m = emt_atom(a, i);
    double vi[P::W][3], acc[P::W];
#pragma unroll
    for (int q = 0; q < P::W; ++q) {
        o.load(q, i, vi[q]);
        acc[q] = 0.0;
    }
    auto visit = [&](int t) {
        EmtPair p;
        if (!emt_pair<P::CELL>(a, m, t, p)) return;
#pragma unroll
        for (int q = 0; q < P::W; ++q) {
            double d[3];
            o.load(q, p.j, d);
#pragma unroll
            for (int b = 0; b < 3; ++b) d[b] -= vi[q][b];
            if constexpr (P::CELL) {
                const double* T = o.shift(q, t >> 24);
#pragma unroll
                for (int b = 0; b < 3; ++b) d[b] += T[b];
            }
            acc[q] += P::Terms::dot(p, d);
        }
    };
    emt_by_image<false>(a, i, &incomplete, visit);
#pragma unroll
    for (int q = 0; q < P::W; ++q) block_put<P::W>(part, q, acc[q]);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < P::W) o.c(t, i) = block_total<P::W>(part, t);
}

// (H v)_i = sum over the visits with j != i of  K d - u (F2_i c_i w'_ij + F2_j c_j w'_ji),  d = v_i - v_j (- T_q[s]):
// g_i on atom i is -sum w'_ij u, g_j on atom i is -w'_ji u (atom i seen from j lies along -u).
// CELL: nine more sums per vector, atom i's share of the cell rows: s_i[(k, b)] = sum over ALL visits of
// n_k [F2_i c_i w'_ij u_b - 1/2 (K d)_b] (the 1/2 of the `B` formula; the first term is F2_i c_i gamma_i).
// The NA = 3 or 12 sums of every vector are reduced behind one barrier; thread NA q + c then hands sum c of vector q to
// store(q, c, sum).
template <class P, class Store>
__device__ __forceinline__ void emt_gather_body(const VB vb, const EmtArgs& a, const double* F2, const P& o, Store store) {
    constexpr int NA = P::CELL ? 12 : 3;
    __shared__ double part[4][NA * P::W];
    __shared__ int incomplete;
    const int i = vb.x;
    const EmtAtom m = emt_atom(a, i);
    const double f2i = F2[i];
    double vi[P::W][3], fc[P::W], acc[P::W][NA];
#pragma unroll
    for (int q = 0; q < P::W; ++q) {
        o.load(q, i, vi[q]);
        fc[q] = f2i * o.c(q, i);
#pragma unroll
        for (int c = 0; c < NA; ++c) acc[q][c] = 0.0;
    }
    auto visit = [&](int t) {
        EmtPair p;
        if (!emt_pair<P::CELL>(a, m, t, p)) return;
        const double c1 = p.e1 / p.r, c2 = p.e2 - c1;                             // K = c1 I + c2 u u^T
        const double f2j = F2[p.j];
        double nv[3] = {0.0, 0.0, 0.0};
        if constexpr (P::CELL) {
            const double* ns = o.nimg + 3 * (t >> 24);
            nv[0] = ns[0]; nv[1] = ns[1]; nv[2] = ns[2];
        }
#pragma unroll
        for (int q = 0; q < P::W; ++q) {
            double d[3];
            o.load(q, p.j, d);
#pragma unroll
            for (int b = 0; b < 3; ++b) d[b] = vi[q][b] - d[b];
            if constexpr (P::CELL) {
                const double* T = o.shift(q, t >> 24);
#pragma unroll
                for (int b = 0; b < 3; ++b) d[b] -= T[b];
            }
            if (!P::CELL || p.j != i) P::Terms::row(p, c1, c2, d, fc[q], f2j * o.c(q, p.j), acc[q]);   // an own image moves no position block
            if constexpr (P::CELL) P::Terms::cell(p, c1, c2, d, fc[q], nv, acc[q] + 3);
        }
    };
    emt_by_image<false>(a, i, &incomplete, visit);
#pragma unroll
    for (int q = 0; q < P::W; ++q)
#pragma unroll
        for (int c = 0; c < NA; ++c) block_put<NA * P::W>(part, NA * q + c, acc[q][c]);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < NA * P::W) store(t / NA, t % NA, block_total<NA * P::W>(part, t));
}

// Vectors q0 .. q0 + KQ - 1 of the rows of a host product: every array holds round_up(k, KQ) rows, those of V (and T)
// beyond k zero; the dots vector-major
template <int KQ, bool CELL_>
struct EmtRows {
    using Terms = EmtTerms;
    static constexpr int W = KQ;
    static constexpr bool CELL = CELL_;
    const double* V; size_t ld;             // (k, ld), atom j of a row at 3 j
    double* cdot; int n;                    // (k, n)
    int q0;
    const double* nimg; const double* T; int nshift;          // CELL: n_s (nshift x 3) and T_q[s] = n_s W_q (k, nshift, 3)
    __device__ __forceinline__ void load(int q, int j, double x[3]) const {
        const double* v = V + (size_t)(q0 + q) * ld + 3 * j;
        x[0] = v[0]; x[1] = v[1]; x[2] = v[2];
    }
    __device__ __forceinline__ double& c(int q, int j) const { return cdot[(size_t)(q0 + q) * n + j]; }
    __device__ __forceinline__ const double* shift(int q, int s) const { return T + ((size_t)(q0 + q) * nshift + s) * 3; }
};

struct EmtHvp {                             // k vectors
    const double* F2;
    const double* V;                        // (k, 3n)
    double* cdot;                           // (k, n): c_i = g_i . v
    double* HV;                             // (k, 3n)
};
template <int KQ>
__device__ __forceinline__ EmtRows<KQ, false> emt_rows(const VB vb, const EmtArgs& a, const EmtHvp& o) {
    return {o.V, (size_t)3 * a.n, o.cdot, a.n, (int)vb.y * KQ, nullptr, nullptr, 0};
}

__device__ __forceinline__ void emt_hvp_dots_vb(const VB vb, EmtArgs a, EmtHvp o) { emt_dots_body(vb, a, emt_rows<HVP_KQ>(vb, a, o)); }
__global__ __launch_bounds__(256) void emt_hvp_dots_kernel(EmtArgs a, EmtHvp o) { emt_hvp_dots_vb(vb_hw(), a, o); }
__device__ __forceinline__ void emt_hvp1_dots_vb(const VB vb, EmtArgs a, EmtHvp o) { emt_dots_body(vb, a, emt_rows<1>(vb, a, o)); }
__global__ __launch_bounds__(256) void emt_hvp1_dots_kernel(EmtArgs a, EmtHvp o) { emt_hvp1_dots_vb(vb_hw(), a, o); }

__device__ __forceinline__ void emt_hvp_gather_vb(const VB vb, EmtArgs a, EmtHvp o) {
    const auto rows = emt_rows<HVP_KQ>(vb, a, o);
    emt_gather_body(vb, a, o.F2, rows, [&](int q, int c, double v) { o.HV[(rows.q0 + q) * rows.ld + 3 * vb.x + c] = v; });
}
__global__ __launch_bounds__(256) void emt_hvp_gather_kernel(EmtArgs a, EmtHvp o) { emt_hvp_gather_vb(vb_hw(), a, o); }

// One vector of the operator (calc.hip, sella_hvp): V and HV of `o` are rows of its pair record (full length 3n).  |v|^2
// comes in `nb` partial sums; a vanishing vector (|v| < 1e-12) gives a zero product and flag 0, as sella_fd_matvec does.
// The rows of the free coordinates also go into the eigensolver's vector y (inv: full coordinate -> its index there, -1
// if pinned; null: all free).
struct EmtHvpOut1 {
    const double* part; int nb;
    const int* inv;
    double* y;
    int* flag;
};
__device__ __forceinline__ void emt_hvp1_gather_vb(const VB vb, EmtArgs a, EmtHvp o, EmtHvpOut1 w) {
    __shared__ double red1[4];
    double s = 0.0;
    for (int b = threadIdx.x; b < w.nb; b += 256) s += w.part[b];
    s = block_sum(s, red1);
    const bool live = !(sqrt(s) < 1e-12);
    if (vb.x == 0 && threadIdx.x == 0) *w.flag = live ? 1 : 0;
    emt_gather_body(vb, a, o.F2, emt_rows<1>(vb, a, o), [&](int, int c, double v) {
        const int p = 3 * vb.x + c, q = w.inv ? w.inv[p] : p;
        const double h = live ? v : 0.0;
        o.HV[p] = h;
        if (q >= 0) w.y[q] = h;
    });
}
__global__ __launch_bounds__(256) void emt_hvp1_gather_kernel(EmtArgs a, EmtHvp o, EmtHvpOut1 w) { emt_hvp1_gather_vb(vb_hw(), a, o, w); }

// ---- the block product of the operator (calc.hip, hvp_device_apply_block) -------------------------------------------------
// Up to HVB_W vectors, the rows of a device panel (row h at V + h ldv: the eigensolver's own panel when all 3n coordinates
// are free, else the full-length rows a scatter filled), on the operator's resident state.  One workgroup per atom carries
// all HVB_W vectors (48 accumulators per thread in the gather pass; 8 per workgroup, and a panel staged atom-major, were
// measured and lost: profiles/block_hvp.md).  The dots c_j are kept atom-major.  Rows beyond nh are never read (the row
// index is clamped: their slots repeat row nh - 1 and are not stored).  Every vector's sums are taken in the order of the
// single-vector kernels and every product is rounded on its own (no contraction into fused multiply-adds, which the
// compiler chooses slot by slot in the unrolled loops: measured, the same vector in slot 0 and in slot 11 differed in the
// last bit), so a row's result does not depend on which row it is, on what stands in the other rows, or on nh.
constexpr int HVB_W = 16;

struct EmtHvpB {
    using Terms = EmtTermsExact;
    static constexpr int W = HVB_W;
    static constexpr bool CELL = false;
    const double* F2;
    const double* V; int ldv;               // the panel
    int nh;
    double* cdot;                           // n x HVB_W: c_j of vector q at [HVB_W j + q]
    const int* inv;                         // full coordinate -> column of Y, -1 if pinned; null: all free
    double* Y; int ldy;                     // (nh, m): the free rows of the products
    __device__ __forceinline__ void load(int q, int j, double x[3]) const {
        const double* v = V + (size_t)(q < nh ? q : nh - 1) * ldv + 3 * j;
        x[0] = v[0]; x[1] = v[1]; x[2] = v[2];
    }
    __device__ __forceinline__ double& c(int q, int j) const { return cdot[(size_t)j * HVB_W + q]; }
};

__device__ __forceinline__ void emt_hvpb_dots_vb(const VB vb, EmtArgs a, EmtHvpB o) { emt_dots_body(vb, a, o); }
__global__ __launch_bounds__(256) void emt_hvpb_dots_kernel(EmtArgs a, EmtHvpB o) { emt_hvpb_dots_vb(vb_hw(), a, o); }

__device__ __forceinline__ void emt_hvpb_gather_vb(const VB vb, EmtArgs a, EmtHvpB o) {
    emt_gather_body(vb, a, o.F2, o, [&](int q, int c, double v) {
        const int p = 3 * vb.x + c, r = o.inv ? o.inv[p] : p;
        if (q < o.nh && r >= 0) o.Y[(size_t)q * o.ldy + r] = v;
    });
}
__global__ __launch_bounds__(256) void emt_hvpb_gather_kernel(EmtArgs a, EmtHvpB o) { emt_hvpb_gather_vb(vb_hw(), a, o); }

// The diagonal of H on the same state: H[(i,a),(i,a)] = sum_{visits, j != i} K_aa + F2_i g_i[a]^2 + sum_{j != i} F2_j g_j[(i,a)]^2,
// g_i[a] = -sum_visits w'_ij u_a and g_j[(i,a)] = -sum over the visits TO ATOM j of w'_ji u_a: a neighbour seen through
// several images enters the last term with the square of its summed share, not the sum of squares, so the visits are
// taken neighbour by neighbour here — thread t owns the atoms j = t, t + 256, ... through all their images (the sweep of
// emt_by_image in the other order; emt_pair tests the distance itself) — and no sum crosses threads before block_sum's
// arithmetic.  The free entries go to y (inv as above).
__device__ __forceinline__ void emt_hdiag_vb(const VB vb, EmtArgs a, const double* __restrict__ F2, const int* __restrict__ inv,
                                             double* __restrict__ y) {
    __shared__ double part[4][9];
    const int i = vb.x;
    const EmtAtom m = emt_atom(a, i);
    double k[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0}, e[3] = {0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < a.n; j += 256) {
        double h[3] = {0.0, 0.0, 0.0};
        for (int s = 0; s < a.nshift; ++s) {
            EmtPair p;
            if (!emt_pair(a, m, emt_pack(j, s), p)) continue;
            double K[6];
            emt_pair_K(p, K);
            const double u[3] = {p.ux, p.uy, p.uz};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                k[c] += K[c];
                g[c] -= p.wp_ij * u[c];
                h[c] -= p.wp_ji * u[c];
            }
        }
        const double f2j = F2[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] += f2j * (h[c] * h[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        block_put<9>(part, c, k[c]);
        block_put<9>(part, 3 + c, g[c]);
        block_put<9>(part, 6 + c, e[c]);
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= 3) return;
    const double gi = block_total<9>(part, 3 + t);
    const int p = 3 * i + t, r = inv ? inv[p] : p;
    if (r >= 0) y[r] = block_total<9>(part, t) + F2[i] * (gi * gi) + block_total<9>(part, 6 + t);
}
__global__ __launch_bounds__(256) void emt_hdiag_kernel(EmtArgs a, const double* __restrict__ F2, const int* __restrict__ inv,
                                                        double* __restrict__ y) { emt_hdiag_vb(vb_hw(), a, F2, inv, y); }

// ---- the cell columns ---------------------------------------------------------------------------------------------------
struct EmtCell {
    const double* F2;
    const double* nimg;                     // nshift x 3: n_s = S_s C^-1, whole numbers
    double* H; int ldh;                     // (3n + 9) square
    double* gam; int ldgam;                 // n x 9: row i = gamma_i, column 3 k + b
    double* share;                          // n x 36: atom i's share of the pair term of B, [sym6(k, l)][sym6(a, b)]
};

// Pair term of row block i of A (into columns 3n .. 3n + 8 of rows 3i .. 3i + 2 of H), row i of gamma, atom i's share of B.
__device__ __forceinline__ void emt_cell_pair_vb(const VB vb, EmtArgs a, EmtCell o) {
    __shared__ double part[4][63];
    __shared__ int incomplete;
    const int i = vb.x;
    const EmtAtom m = emt_atom(a, i);
    double kn[3][6], gk[3][3], kk[6][6];    // sum K n_k (j != i); sum w' u_b n_k; sum K n_k n_l
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int q = 0; q < 6; ++q) kn[k][q] = 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) gk[k][b] = 0.0;
    }
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = 0; q < 6; ++q) kk[p][q] = 0.0;
    auto visit = [&](int t) {
        const double* ns = o.nimg + 3 * (t >> 24);
        const double nv[3] = {ns[0], ns[1], ns[2]};
        if (nv[0] == 0.0 && nv[1] == 0.0 && nv[2] == 0.0) return;                 // the home image: no cell in d
        EmtPair p;
        if (!emt_pair<true>(a, m, t, p)) return;
        double K[6];
        emt_pair_K(p, K);
        const double wu[3] = {p.wp_ij * p.ux, p.wp_ij * p.uy, p.wp_ij * p.uz};
        const double nn[6] = {nv[0] * nv[0], nv[1] * nv[1], nv[2] * nv[2], nv[1] * nv[2], nv[0] * nv[2], nv[0] * nv[1]};
        const double other = p.j != i ? 1.0 : 0.0;                                // an own image moves no position block
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double nk = other * nv[k];
#pragma unroll
            for (int q = 0; q < 6; ++q) kn[k][q] += K[q] * nk;
#pragma unroll
            for (int b = 0; b < 3; ++b) gk[k][b] += wu[b] * nv[k];
        }
#pragma unroll
        for (int pq = 0; pq < 6; ++pq)
#pragma unroll
            for (int q = 0; q < 6; ++q) kk[pq][q] += K[q] * nn[pq];
    };
    emt_by_image<false>(a, i, &incomplete, visit);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int q = 0; q < 6; ++q) block_put<63>(part, 6 * k + q, kn[k][q]);
#pragma unroll
        for (int b = 0; b < 3; ++b) block_put<63>(part, 18 + 3 * k + b, gk[k][b]);
    }
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = 0; q < 6; ++q) block_put<63>(part, 27 + 6 * p + q, kk[p][q]);
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= 63) return;
    const double v = block_total<63>(part, t);
    if (t < 18) {                           // - sum K_rb n_k into A[(i, r), (k, b)], both (r, b) of an off-diagonal component
        const int k = t / 6, q = t % 6, n3 = 3 * a.n;
        for (int r = 0; r < 3; ++r)
            for (int b = 0; b < 3; ++b)
                if (sym6(r, b) == q) o.H[(size_t)(3 * i + r) * o.ldh + n3 + 3 * k + b] = -v;
    } else if (t < 27) {
        o.gam[(size_t)i * o.ldgam + (t - 18)] = v;
    } else {
        o.share[(size_t)i * 36 + (t - 27)] = 0.5 * v;
    }
}
__global__ __launch_bounds__(256) void emt_cell_pair_kernel(EmtArgs a, EmtCell o) { emt_cell_pair_vb(vb_hw(), a, o); }

// A += (diag(F2) G^T)^T gamma, 3n x 9 with inner dimension n, too thin for the tiles of launch_gemm: a workgroup takes 16
// rows q of A (columns of Gs, n x 3n) and splits the inner index m over 16 slices (m = slice, slice + 16, ...: a
// wavefront reads four 128-byte pieces of rows of Gs at a time); the slices meet in LDS and are added in index order.
__device__ __forceinline__ void emt_cell_embed_vb(const VB vb, int n, const double* __restrict__ Gs, int ldg, EmtCell o) {
    __shared__ double part[16][16][9];
    const int ql = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int n3 = 3 * n, q = vb.x * 16 + ql;
    double acc[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) acc[c] = 0.0;
    if (q < n3)
        for (int m = sl; m < n; m += 16) {
            const double g = Gs[(size_t)m * ldg + q];
            const double* gm = o.gam + (size_t)m * o.ldgam;
#pragma unroll
            for (int c = 0; c < 9; ++c) acc[c] += g * gm[c];
        }
#pragma unroll
    for (int c = 0; c < 9; ++c) part[sl][ql][c] = acc[c];
    __syncthreads();
    if (threadIdx.x >= 144) return;
    const int qo = vb.x * 16 + threadIdx.x / 9, c = threadIdx.x % 9;
    if (qo >= n3) return;
    double sum = 0.0;
    for (int u = 0; u < 16; ++u) sum += part[u][threadIdx.x / 9][c];
    o.H[(size_t)qo * o.ldh + n3 + c] += sum;
}
__global__ __launch_bounds__(256) void emt_cell_embed_kernel(int n, const double* __restrict__ Gs, int ldg, EmtCell o) {
    emt_cell_embed_vb(vb_hw(), n, Gs, ldg, o);
}

// Workgroups 0 .. 44: entry (P, Q), P <= Q, of B = sum_i share_i + sum_i F2_i gamma_i gamma_i^T and its mirror image — every
// thread adds its atoms (i = tid, tid + 256, ...) in increasing i, block_sum adds the threads: one fixed order.  The
// workgroups behind them copy A (rows of the positions, last nine columns) into the last nine rows.
__device__ __forceinline__ void emt_cell_finish_vb(const VB vb, int n, EmtCell o) {
    __shared__ double red[4];
    const int n3 = 3 * n;
    if (vb.x >= 45) {
        const int r = (vb.x - 45) * 256 + threadIdx.x;
        if (r < n3)
            for (int q = 0; q < 9; ++q) o.H[(size_t)(n3 + q) * o.ldh + r] = o.H[(size_t)r * o.ldh + n3 + q];
        return;
    }
    int P = 0, rest = vb.x;                 // row P of the upper triangle holds 9 - P entries
    while (rest >= 9 - P) { rest -= 9 - P; ++P; }
    const int Q = P + rest;
    const int w = 6 * sym6(P / 3, Q / 3) + sym6(P % 3, Q % 3);
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double* g = o.gam + (size_t)i * o.ldgam;
        acc += o.share[(size_t)i * 36 + w] + o.F2[i] * g[P] * g[Q];
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) {
        o.H[(size_t)(n3 + P) * o.ldh + n3 + Q] = acc;
        o.H[(size_t)(n3 + Q) * o.ldh + n3 + P] = acc;
    }
}
__global__ __launch_bounds__(256) void emt_cell_finish_kernel(int n, EmtCell o) { emt_cell_finish_vb(vb_hw(), n, o); }

// ---- the product in the coordinates of the cell Hessian (sella_emt_cell_hvp) ------------------------------------------------
// y = [A-part, B-part] applied to a direction [v; W] (W the 3 x 3 variation of C) without forming anything: the direction
// displaces the pair of a visit by dd = v_j - v_i + n_s W, and with that in place of v_j - v_i the two passes of the
// product at fixed cell give the position rows; the cell rows are the same pair quantities contracted with n_k (header).
// T_q[s] = n_s W_q comes from the host (nshift x 3 per vector), so a visit costs one more 3-vector load per vector.  Twelve
// accumulators per vector in the gather pass (three position components, nine cell entries) against three at fixed cell:
// CHVP_KQ vectors per workgroup (profiles/cell_hvp.md).
constexpr int CHVP_KQ = 4;

struct EmtCellHvp {                         // k vectors: every array holds round_up(k, CHVP_KQ) rows, those of V and T beyond k zero
    const double* F2;
    const double* nimg;                     // nshift x 3: n_s
    const double* T;                        // (k, nshift, 3): T_q[s] = n_s W_q
    const double* V;                        // (k, ld): [v; W.ravel()]
    double* HV;                             // (k, ld)
    int ld;                                 // 3n + 9
    double* cdot;                           // (k, n): c_i = sum_visits w'_ij u . dd
    double* share;                          // (k, n, 9): atom i's share of the cell rows, column 3 k + b
};
__device__ __forceinline__ EmtRows<CHVP_KQ, true> emt_rows(const VB vb, const EmtArgs& a, const EmtCellHvp& o) {
    return {o.V, (size_t)o.ld, o.cdot, a.n, (int)vb.y * CHVP_KQ, o.nimg, o.T, a.nshift};
}

__device__ __forceinline__ void emt_chvp_dots_vb(const VB vb, EmtArgs a, EmtCellHvp o) { emt_dots_body(vb, a, emt_rows(vb, a, o)); }
__global__ __launch_bounds__(256) void emt_chvp_dots_kernel(EmtArgs a, EmtCellHvp o) { emt_chvp_dots_vb(vb_hw(), a, o); }

// sums 0 .. 2 of a vector: its position rows of atom i; 3 .. 11: the atom's share of its cell rows
__device__ __forceinline__ void emt_chvp_gather_vb(const VB vb, EmtArgs a, EmtCellHvp o) {
    const auto rows = emt_rows(vb, a, o);
    emt_gather_body(vb, a, o.F2, rows, [&](int q, int c, double v) {
        if (c < 3) o.HV[(rows.q0 + q) * rows.ld + 3 * vb.x + c] = v;
        else o.share[((size_t)(rows.q0 + q) * a.n + vb.x) * 9 + (c - 3)] = v;
    });
}
__global__ __launch_bounds__(256) void emt_chvp_gather_kernel(EmtArgs a, EmtCellHvp o) { emt_chvp_gather_vb(vb_hw(), a, o); }

// cell rows of vector vb.x: y_C = sum_i s_i — every thread adds its atoms (i = tid, tid + 256, ...) in increasing i, then
// block_sum's arithmetic over the threads: one fixed order
__device__ __forceinline__ void emt_chvp_finish_vb(const VB vb, int n, EmtCellHvp o) {
    __shared__ double part[4][9];
    const int q = vb.x;
    double acc[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) acc[c] = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double* s = o.share + ((size_t)q * n + i) * 9;
#pragma unroll
        for (int c = 0; c < 9; ++c) acc[c] += s[c];
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) block_put<9>(part, c, acc[c]);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 9) o.HV[(size_t)q * o.ld + 3 * n + t] = block_total<9>(part, t);
}
__global__ __launch_bounds__(256) void emt_chvp_finish_kernel(int n, EmtCellHvp o) { emt_chvp_finish_vb(vb_hw(), n, o); }

// ---- the resident operator of positions and cell (calc.hip, sella_hvp_create_cell) -------------------------------------------
// The product above in the coordinates [x; p] of a cell run (p: mc parameters of the cell, W = J p its variation), on a state
// that stays on the device (EmtCellHvpState) and on device vectors: y_x as above with T[s] = n_s W, y_p = J^T (y_C + P W) + G p.
// Four stages, for ONE vector (it is recorded, |v| < 1e-12 gives zero and flag 0) or for the nh <= HVB_W rows of a panel:
//   emt_chvpo_scatter   row h = vb.y: the free position entries into the full-length row, |v|^2 in partial sums (the cell
//                       entries included); the workgroup behind those of the positions forms W = J v_p and T[s] = n_s W and
//                       puts v_p into the full-length row
//   dots, gather        emt_dots_body / emt_gather_body with CELL: emt_chvpo1_* one vector per workgroup, emt_chvpob_*
//                       CHVP_KQ rows of the panel per workgroup on a grid (n, ceil(nh / CHVP_KQ)), every product rounded on its
//                       own (EmtTermsExact) like the block at fixed cell: a row's result does not depend on its slot, on nh or
//                       on the other rows.  Position rows go to Y (and the record), the nine cell sums to the share array.
//   emt_chvpo_finish    row h = vb.x: y_C = sum_i s_i in the order of emt_chvp_finish, + P W, y_p = J^T y_C + G v_p
// Scatter and finish are the same kernels for one vector and for a panel.
struct EmtCellOp {
    const double* F2;
    const double *nimg, *J, *G, *P;         // n_s (nshift x 3), 9 x mc, mc x mc, 9 x 9
    int mc, nshift;
    double *T, *wv, *share, *cdot;          // (HVB_W, nshift, 3); (HVB_W, 18): W, v_p; (HVB_W, n, 9); n (one vector) or n x HVB_W
    const double* X; int ldx;               // the eigensolver's vectors: mx free position entries, then mc
    double* Y; int ldy;
    const int* inv; int mx;                 // position coordinate -> entry of X, -1 if pinned; null: all free
    double* vfull; int ldv;                 // full-length rows: 3n position entries, then mc
    double* hvfull;                         // one vector: the product in full length (the pair record)
    const double* partc; double* part; int nb;    // one vector: nb + 1 partial sums of |v|^2 (nb = workgroups of the positions)
    int* flag;
    int nh;
};

__device__ __forceinline__ void emt_chvpo_scatter_vb(const VB vb, int n3, EmtCellOp o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double red[4];
    __shared__ double Wl[9];
    const int h = vb.y, t = threadIdx.x;
    const double* x = o.X + (size_t)h * o.ldx;
    double* vf = o.vfull + (size_t)h * o.ldv;
    double v = 0.0;
    if ((int)vb.x < o.nb) {
        const int p = vb.x * 256 + t;
        if (p < n3) {
            const int q = o.inv ? o.inv[p] : p;
            if (q >= 0) v = x[q];
            vf[p] = v;
        }
    } else if (t < o.mc) {
        v = x[o.mx + t];
        vf[n3 + t] = v;
        o.wv[h * 18 + 9 + t] = v;
    }
    if (o.part) {
        const double s = block_sum(v * v, red);
        if (t == 0) o.part[vb.x] = s;
    }
    if ((int)vb.x < o.nb) return;
    if (t < 9) {
        double w = 0.0;
        for (int c = 0; c < o.mc; ++c) w += o.J[t * o.mc + c] * x[o.mx + c];
        Wl[t] = w;
        o.wv[h * 18 + t] = w;
    }
    __syncthreads();
    double* T = o.T + (size_t)h * o.nshift * 3;
    for (int s = t; s < o.nshift; s += 256) {
        const double* ns = o.nimg + 3 * s;
#pragma unroll
        for (int b = 0; b < 3; ++b) T[3 * s + b] = ns[0] * Wl[b] + ns[1] * Wl[3 + b] + ns[2] * Wl[6 + b];
    }
}
__global__ __launch_bounds__(256) void emt_chvpo_scatter_kernel(int n3, EmtCellOp o) { emt_chvpo_scatter_vb(vb_hw(), n3, o); }

__device__ __forceinline__ EmtRows<1, true> emt_rows1(const EmtArgs& a, const EmtCellOp& o) {
    return {o.vfull, 0, o.cdot, a.n, 0, o.nimg, o.T, o.nshift};
}
__device__ __forceinline__ void emt_chvpo1_dots_vb(const VB vb, EmtArgs a, EmtCellOp o) { emt_dots_body(vb, a, emt_rows1(a, o)); }
__global__ __launch_bounds__(256) void emt_chvpo1_dots_kernel(EmtArgs a, EmtCellOp o) { emt_chvpo1_dots_vb(vb_hw(), a, o); }

// whether the vector of a single product counts (|v| >= 1e-12), from the partial sums of the scatter
__device__ __forceinline__ bool emt_chvpo_live(const EmtCellOp& o, double* red) {
    double s = 0.0;
    for (int b = threadIdx.x; b < o.nb + 1; b += 256) s += o.partc[b];
    s = block_sum(s, red);
    return !(sqrt(s) < 1e-12);
}

__device__ __forceinline__ void emt_chvpo1_gather_vb(const VB vb, EmtArgs a, EmtCellOp o) {
    __shared__ double red1[4];
    const bool live = emt_chvpo_live(o, red1);
    emt_gather_body(vb, a, o.F2, emt_rows1(a, o), [&](int, int c, double v) {
        if (c < 3) {
            const int p = 3 * vb.x + c, q = o.inv ? o.inv[p] : p;
            const double h = live ? v : 0.0;
            o.hvfull[p] = h;
            if (q >= 0) o.Y[q] = h;
        } else {
            o.share[(size_t)vb.x * 9 + (c - 3)] = v;
        }
    });
}
__global__ __launch_bounds__(256) void emt_chvpo1_gather_kernel(EmtArgs a, EmtCellOp o) { emt_chvpo1_gather_vb(vb_hw(), a, o); }

// rows q0 .. q0 + CHVP_KQ - 1 of the panel; rows beyond nh are never read (their slots repeat row nh - 1 and are not stored)
struct EmtCellHvpB {
    using Terms = EmtTermsExact;
    static constexpr int W = CHVP_KQ;
    static constexpr bool CELL = true;
    const double* V; int ldv;
    int nh, q0;
    double* cdot;                           // n x HVB_W: c_j of row r at [HVB_W j + r]
    const double* nimg; const double* T; int nshift;
    __device__ __forceinline__ int row(int q) const { return q0 + q < nh ? q0 + q : nh - 1; }
    __device__ __forceinline__ void load(int q, int j, double x[3]) const {
        const double* v = V + (size_t)row(q) * ldv + 3 * j;
        x[0] = v[0]; x[1] = v[1]; x[2] = v[2];
    }
    __device__ __forceinline__ double& c(int q, int j) const { return cdot[(size_t)j * HVB_W + q0 + q]; }
    __device__ __forceinline__ const double* shift(int q, int s) const { return T + ((size_t)row(q) * nshift + s) * 3; }
};
__device__ __forceinline__ EmtCellHvpB emt_rowsb(const VB vb, const EmtCellOp& o) {
    return {o.vfull, o.ldv, o.nh, (int)vb.y * CHVP_KQ, o.cdot, o.nimg, o.T, o.nshift};
}
__device__ __forceinline__ void emt_chvpob_dots_vb(const VB vb, EmtArgs a, EmtCellOp o) { emt_dots_body(vb, a, emt_rowsb(vb, o)); }
__global__ __launch_bounds__(256) void emt_chvpob_dots_kernel(EmtArgs a, EmtCellOp o) { emt_chvpob_dots_vb(vb_hw(), a, o); }

__device__ __forceinline__ void emt_chvpob_gather_vb(const VB vb, EmtArgs a, EmtCellOp o) {
    const auto rows = emt_rowsb(vb, o);
    emt_gather_body(vb, a, o.F2, rows, [&](int q, int c, double v) {
        const int h = rows.q0 + q;
        if (h >= o.nh) return;
        if (c < 3) {
            const int p = 3 * vb.x + c, r = o.inv ? o.inv[p] : p;
            if (r >= 0) o.Y[(size_t)h * o.ldy + r] = v;
        } else {
            o.share[((size_t)h * a.n + vb.x) * 9 + (c - 3)] = v;
        }
    });
}
__global__ __launch_bounds__(256) void emt_chvpob_gather_kernel(EmtArgs a, EmtCellOp o) { emt_chvpob_gather_vb(vb_hw(), a, o); }

__device__ __forceinline__ void emt_chvpo_finish_vb(const VB vb, int n, EmtCellOp o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double part[4][9];
    __shared__ double red1[4];
    __shared__ double yC[9];
    const int h = vb.x, t = threadIdx.x;
    const bool live = o.partc ? emt_chvpo_live(o, red1) : true;
    double acc[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) acc[c] = 0.0;
    for (int i = t; i < n; i += 256) {
        const double* s = o.share + ((size_t)h * n + i) * 9;
#pragma unroll
        for (int c = 0; c < 9; ++c) acc[c] += s[c];
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) block_put<9>(part, c, acc[c]);
    __syncthreads();
    const double* w = o.wv + h * 18;
    if (t < 9) {
        double y = block_total<9>(part, t);
        for (int u = 0; u < 9; ++u) y += o.P[t * 9 + u] * w[u];
        yC[t] = y;
    }
    __syncthreads();
    if (t < o.mc) {
        double y = 0.0;
        for (int r = 0; r < 9; ++r) y += o.J[r * o.mc + t] * yC[r];
        for (int c = 0; c < o.mc; ++c) y += o.G[t * o.mc + c] * w[9 + c];
        if (!live) y = 0.0;
        if (o.hvfull) o.hvfull[3 * n + t] = y;
        o.Y[(size_t)h * o.ldy + o.mx + t] = y;
    }
    if (o.flag && t == 0) *o.flag = live ? 1 : 0;
}
__global__ __launch_bounds__(256) void emt_chvpo_finish_kernel(int n, EmtCellOp o) { emt_chvpo_finish_vb(vb_hw(), n, o); }

struct TempMats {                           // device matrices of one call, back to the pool on every way out (stream-ordered)
    sella_ctx* c;
    sella_mat h[3] = {SELLA_NO_MAT, SELLA_NO_MAT, SELLA_NO_MAT};
    explicit TempMats(sella_ctx* ctx) : c(ctx) {}
    ~TempMats() {
        for (sella_mat m : h)
            if (m != SELLA_NO_MAT) sella_mat_free(c, m);
    }
};

}  // namespace
}  // namespace sella

using namespace sella;

// What every entry does first: the density pass queued (emt_density_queue: dconst and the scratch slot as there) and F2
// behind it.  *F2 holds n numbers; the caller's `extra_words` doubles follow it.
static int emt_f2_queue(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                        const double* dconst, double rc, double acut, double cutoff, double beta, size_t extra_words, EmtArgs* a,
                        double** F2) {
    SCHK(emt_density_queue(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta, (size_t)n + extra_words, a, F2));
    SELLA_LAUNCHB(c, emt_f2_kernel, emt_f2_vb, 256, dim3((n + 255) / 256), dim3(256), 0, *a, *F2);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

// The k rows of `len` numbers of a host array to the device, the rows up to kp (k rounded up to the vectors of a
// workgroup) zero
static int emt_upload_rows(sella_ctx* c, double* dst, const double* src, int k, size_t kp, size_t len) {
    SCHK(h2d_async(c, dst, src, (size_t)k * len * sizeof(double)));
    if (kp > (size_t)k) HIPCHK(s_memset0(c, dst + (size_t)k * len, (kp - k) * len * sizeof(double)));
    return SELLA_OK;
}

// The passes of the dense Hessian into the leading 3n x 3n block of H (rows ldh apart, zero on entry), symmetrised.
// G^T and diag(F2) G^T (n x 3n) stay behind in t.h[0], t.h[1].
static int emt_hessian_block(sella_ctx* c, int n, const EmtArgs& a, double* F2, double* H, int ldh, TempMats& t) {
    SCHK(mat_new(c, n, 3 * n, &t.h[0]));                              // zeroed: the visits add into the rows
    SCHK(mat_new(c, n, 3 * n, &t.h[1]));
    Mat *Gt = mat_get(c, t.h[0]), *Gs = mat_get(c, t.h[1]);
    EmtHessOut o;
    o.F2 = F2; o.H = H; o.ldh = ldh; o.Gt = Gt->d; o.Gs = Gs->d; o.ldg = Gt->ld;
    SELLA_LAUNCHB(c, emt_hess_pair_kernel, emt_hess_pair_vb, 256, dim3(n), dim3(256), 0, a, o);
    HIPCHK(hipGetLastError());
    // H += G diag(F2) G^T, G^T = Gt (n x 3n)
    SCHK(launch_gemm(c, 1, 0, 3 * n, 3 * n, n, 1.0, Gt->d, Gt->ld, Gs->d, Gs->ld, 1.0, H, ldh));
    // the two triangles agree to rounding only (x_j + shift - x_i from either end, the tiles of the product)
    return launch_symmetrize(c, H, 3 * n, ldh);
}

// dconst as in emt_eval_resident.  `out` (3n x 3n) is overwritten and stays on the device.
int sella::emt_hessian_resident(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                                const double* dconst, double rc, double acut, double cutoff, double beta, sella_mat out) {
    Mat* H = mat_get(c, out);
    if (!H || H->rows != 3 * n || H->cols != 3 * n) {
        set_error("emt_hessian: out must be the %d x %d matrix of %d atoms", 3 * n, 3 * n, n);
        return SELLA_E_INVALID;
    }
    EmtArgs a;
    double* F2;
    SCHK(emt_f2_queue(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta, 0, &a, &F2));
    TempMats t(c);
    HIPCHK(s_memset0(c, H->d, (size_t)H->rows * H->ld * sizeof(double)));
    SCHK(emt_hessian_block(c, n, a, F2, H->d, H->ld, t));
    return stream_wait(c);
}

// Image indices n_s = S_s C^-1 of the shifts in the cell (lattice vectors in the rows of C): whole numbers, or the
// shifts are no lattice translations of this cell.
static int emt_image_indices(const double* cell, int nshift, const double* shifts, std::vector<double>& nimg) {
    // (emt_density_queue's limit, here before `shifts` is read)
    if (nshift > 127) { set_error("emt: at most 2^24 atoms and 127 periodic images"); return SELLA_E_INVALID; }
    const double* C = cell;
    const double cof[9] = {C[4] * C[8] - C[5] * C[7], C[2] * C[7] - C[1] * C[8], C[1] * C[5] - C[2] * C[4],
                           C[5] * C[6] - C[3] * C[8], C[0] * C[8] - C[2] * C[6], C[2] * C[3] - C[0] * C[5],
                           C[3] * C[7] - C[4] * C[6], C[1] * C[6] - C[0] * C[7], C[0] * C[4] - C[1] * C[3]};   // adj(C)
    const double det = C[0] * cof[0] + C[1] * cof[3] + C[2] * cof[6];
    double scale = 1.0;
    for (int k = 0; k < 3; ++k) scale *= std::sqrt(C[3 * k] * C[3 * k] + C[3 * k + 1] * C[3 * k + 1] + C[3 * k + 2] * C[3 * k + 2]);
    if (!std::isfinite(det) || !(std::fabs(det) > 1e-12 * scale)) {
        set_error("emt_cell_hessian: the cell is singular (determinant %g)", det);
        return SELLA_E_INVALID;
    }
    nimg.resize((size_t)3 * nshift);
    for (int s = 0; s < nshift; ++s)
        for (int k = 0; k < 3; ++k) {
            const double* S = shifts + 3 * s;
            const double v = (S[0] * cof[k] + S[1] * cof[3 + k] + S[2] * cof[6 + k]) / det;
            const double w = std::nearbyint(v);
            if (!(std::fabs(v - w) <= 1e-6)) {
                set_error("emt_cell_hessian: shift %d is no lattice translation of the cell (index %g along vector %d)", s, v, k);
                return SELLA_E_INVALID;
            }
            nimg[(size_t)3 * s + k] = w;
        }
    return SELLA_OK;
}

extern "C" int sella_emt_cell_hessian(sella_ctx* c, int n, const double* pos, const double* par /* 9 x n */, int nshift,
                                      const double* shifts, const double* cell, double rc, double acut, double cutoff,
                                      double beta, sella_mat out) {
    if (!c || n <= 0 || !pos || !par || nshift <= 0 || !shifts || !cell) {
        set_error("emt_cell_hessian: invalid arguments");
        return SELLA_E_INVALID;
    }
    const int n3 = 3 * n, dim = n3 + 9;
    Mat* H = mat_get(c, out);
    if (!H || H->rows != dim || H->cols != dim) {
        set_error("emt_cell_hessian: out must be the %d x %d matrix of %d atoms and the cell", dim, dim, n);
        return SELLA_E_INVALID;
    }
    std::vector<double> nimg;
    SCHK(emt_image_indices(cell, nshift, shifts, nimg));
    EmtArgs a;
    double* ex;                                                       // F2 (n), image indices (3 nshift), shares of B (36 n)
    SCHK(emt_f2_queue(c, n, pos, par, nshift, shifts, nullptr, rc, acut, cutoff, beta, (size_t)3 * nshift + (size_t)36 * n, &a,
                      &ex));
    double* dn = ex + n;
    SCHK(h2d_async(c, dn, nimg.data(), nimg.size() * sizeof(double)));
    TempMats t(c);
    H = mat_get(c, out);
    HIPCHK(s_memset0(c, H->d, (size_t)H->rows * H->ld * sizeof(double)));
    // the 3n x 3n block: the passes of sella_emt_hessian, only the row stride differs
    SCHK(emt_hessian_block(c, n, a, ex, H->d, H->ld, t));
    SCHK(mat_new(c, n, 9, &t.h[2]));
    H = mat_get(c, out);
    Mat *Gs = mat_get(c, t.h[1]), *gam = mat_get(c, t.h[2]);
    EmtCell o;
    o.F2 = ex; o.nimg = dn; o.H = H->d; o.ldh = H->ld; o.gam = gam->d; o.ldgam = gam->ld; o.share = dn + (size_t)3 * nshift;
    SELLA_LAUNCHB(c, emt_cell_pair_kernel, emt_cell_pair_vb, 256, dim3(n), dim3(256), 0, a, o);
    HIPCHK(hipGetLastError());
    // A += G diag(F2) gamma: (diag(F2) G^T)^T (3n x n) times gamma (n x 9)
    SELLA_LAUNCHB(c, emt_cell_embed_kernel, emt_cell_embed_vb, 256, dim3((n3 + 15) / 16), dim3(256), 0, n,
                  (const double*)Gs->d, Gs->ld, o);
    SELLA_LAUNCHB(c, emt_cell_finish_kernel, emt_cell_finish_vb, 256, dim3(45 + (n3 + 255) / 256), dim3(256), 0, n, o);
    HIPCHK(hipGetLastError());
    return stream_wait(c);
}

// V, HV: (k, 3n + 9) host arrays, one vector [v; W.ravel()] per row, in the coordinates of sella_emt_cell_hessian
extern "C" int sella_emt_cell_hvp(sella_ctx* c, int n, const double* pos, const double* par /* 9 x n */, int nshift,
                                  const double* shifts, const double* cell, double rc, double acut, double cutoff, double beta,
                                  const double* V, int k, double* HV) {
    if (!c || n <= 0 || !pos || !par || nshift <= 0 || !shifts || !cell || !V || k <= 0 || !HV) {
        set_error("emt_cell_hvp: invalid arguments");
        return SELLA_E_INVALID;
    }
    std::vector<double> nimg;
    SCHK(emt_image_indices(cell, nshift, shifts, nimg));
    const size_t dim = (size_t)3 * n + 9, kp = (size_t)round_up(k, CHVP_KQ), nT = (size_t)3 * nshift;
    std::vector<double> T(kp * nT, 0.0);                              // T_q[s] = n_s W_q; zero for the rows beyond k
    for (int q = 0; q < k; ++q) {
        const double* W = V + (size_t)q * dim + (size_t)3 * n;
        for (int s = 0; s < nshift; ++s)
            for (int b = 0; b < 3; ++b)
                T[(size_t)q * nT + 3 * s + b] = nimg[3 * s] * W[b] + nimg[3 * s + 1] * W[3 + b] + nimg[3 * s + 2] * W[6 + b];
    }
    EmtArgs a;
    double* ex;                     // F2 (n), image indices (3 nshift), T (kp 3 nshift), V and HV (kp dim each), dots (kp n), shares (kp 9 n)
    SCHK(emt_f2_queue(c, n, pos, par, nshift, shifts, nullptr, rc, acut, cutoff, beta, nT + kp * (nT + 2 * dim + (size_t)10 * n),
                      &a, &ex));
    double* dn = ex + n;
    double* dT = dn + nT;
    double* dV = dT + kp * nT;
    EmtCellHvp o;
    o.F2 = ex; o.nimg = dn; o.T = dT; o.V = dV; o.HV = dV + kp * dim; o.ld = (int)dim;
    o.cdot = o.HV + kp * dim; o.share = o.cdot + kp * n;
    SCHK(h2d_async(c, dn, nimg.data(), nT * sizeof(double)));
    SCHK(h2d_async(c, dT, T.data(), kp * nT * sizeof(double)));
    SCHK(emt_upload_rows(c, dV, V, k, kp, dim));
    const dim3 grid(n, (unsigned)(kp / CHVP_KQ));
    SELLA_LAUNCHB(c, emt_chvp_dots_kernel, emt_chvp_dots_vb, 256, grid, dim3(256), 0, a, o);
    SELLA_LAUNCHB(c, emt_chvp_gather_kernel, emt_chvp_gather_vb, 256, grid, dim3(256), 0, a, o);
    SELLA_LAUNCHB(c, emt_chvp_finish_kernel, emt_chvp_finish_vb, 256, dim3(k), dim3(256), 0, n, o);
    HIPCHK(hipGetLastError());
    SCHK(d2h_async(c, HV, o.HV, (size_t)k * dim * sizeof(double)));
    return stream_wait(c);
}

// V, HV: (k, 3n) host arrays, one vector per row
int sella::emt_hvp_resident(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                            const double* dconst, double rc, double acut, double cutoff, double beta, const double* V, int k,
                            double* HV) {
    const size_t n3 = (size_t)3 * n, kp = (size_t)round_up(k, HVP_KQ);
    EmtArgs a;
    double* ex;
    SCHK(emt_f2_queue(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta, kp * (2 * n3 + n), &a, &ex));
    EmtHvp o;
    double* dV = ex + n;
    o.F2 = ex; o.V = dV; o.cdot = dV + kp * n3; o.HV = o.cdot + kp * n;
    SCHK(emt_upload_rows(c, dV, V, k, kp, n3));
    const dim3 grid(n, (unsigned)(kp / HVP_KQ));
    SELLA_LAUNCHB(c, emt_hvp_dots_kernel, emt_hvp_dots_vb, 256, grid, dim3(256), 0, a, o);
    SELLA_LAUNCHB(c, emt_hvp_gather_kernel, emt_hvp_gather_vb, 256, grid, dim3(256), 0, a, o);
    HIPCHK(hipGetLastError());
    SCHK(d2h_async(c, HV, o.HV, (size_t)k * n3 * sizeof(double)));
    return stream_wait(c);
}

// ---- the resident state of the Hessian-vector operator (emt.h) ---------------------------------------------------------
// One density pass and one emt_f2 at `pos`; what they leave in scratch slot SCR_MISC0 (positions, sigma1, dEdsig, the
// lists, F2 — and the parameter table and shifts unless `dconst` holds them) is copied into an allocation of the state's
// own, because the next force call reuses the slot.
// `room` more doubles of the state's own behind them at *behind (contents undefined).
static int emt_hvp_state_create_room(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                                     const double* dconst, double rc, double acut, double cutoff, double beta, size_t room,
                                     EmtHvpState* st, double** behind) {
    EmtArgs a;
    double* ex;                                                       // F2 (n), c_i = g_i . v (n; HVB_W n for a block product)
    const size_t dots = (size_t)HVB_W * n;
    SCHK(emt_f2_queue(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta, dots, &a, &ex));
    const char* lo = reinterpret_cast<const char*>(a.pos);            // (the positions lead the slot)
    const char* hi = reinterpret_cast<const char*>(ex + n + dots);
    st->own_bytes = (size_t)(hi - lo) + room * sizeof(double);
    SCHK(dev_alloc(c, st->own_bytes, &st->own));
    HIPCHK(s_memcpy(c, st->own, lo, (size_t)(hi - lo), hipMemcpyDeviceToDevice));
    char* base = reinterpret_cast<char*>(st->own);
    auto moved = [&](auto*& p) {                                      // pointers into the slot follow the copy
        const char* q = reinterpret_cast<const char*>(p);
        if (q >= lo && q < hi) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + (q - lo));
    };
    moved(a.pos); moved(a.shifts); moved(a.sigma1); moved(a.epair); moved(a.dEdsig); moved(a.eatom); moved(a.grad); moved(a.nbr);
    moved(a.p.E0); moved(a.p.s0); moved(a.p.V0); moved(a.p.eta2); moved(a.p.kappa); moved(a.p.lam); moved(a.p.n0);
    moved(a.p.gamma1); moved(a.p.gamma2);
    moved(ex);
    st->a = a;
    st->F2 = ex;
    st->cdot = ex + n;
    if (behind) *behind = ex + n + dots;
    return stream_wait(c);
}

int sella::emt_hvp_state_create(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                                const double* dconst, double rc, double acut, double cutoff, double beta, EmtHvpState* st) {
    return emt_hvp_state_create_room(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta, 0, st, nullptr);
}

void sella::emt_hvp_state_destroy(sella_ctx* c, EmtHvpState* st) {
    if (st->own) dev_free(c, st->own, st->own_bytes);
    st->own = nullptr;
}

// hv = H v (rows of 3n on the device) and the free rows into y: two launches on the context's stream, nothing waited for
int sella::emt_hvp_state_apply(sella_ctx* c, const EmtHvpState& st, const double* v, double* hv, const double* part, int nb,
                               const int* inv, double* y, int* flag) {
    EmtHvp o;
    o.F2 = st.F2; o.V = v; o.cdot = st.cdot; o.HV = hv;
    EmtHvpOut1 w;
    w.part = part; w.nb = nb; w.inv = inv; w.y = y; w.flag = flag;
    const dim3 grid(st.a.n);
    SELLA_LAUNCHB(c, emt_hvp1_dots_kernel, emt_hvp1_dots_vb, 256, grid, dim3(256), 0, st.a, o);
    SELLA_LAUNCHB(c, emt_hvp1_gather_kernel, emt_hvp1_gather_vb, 256, grid, dim3(256), 0, st.a, o, w);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

// Y[h] = (H v_h)[free] for the nh <= HVB_W rows of the panel V (row h at V + h ldv, full length): two launches on the
// context's stream, nothing waited for.
int sella::emt_hvp_state_apply_block(sella_ctx* c, const EmtHvpState& st, const double* V, int ldv, int nh, const int* inv,
                                     double* Y, int ldy) {
    EmtHvpB o;
    o.F2 = st.F2; o.V = V; o.ldv = ldv; o.nh = nh; o.cdot = st.cdot; o.inv = inv; o.Y = Y; o.ldy = ldy;
    const dim3 grid(st.a.n);
    SELLA_LAUNCHB(c, emt_hvpb_dots_kernel, emt_hvpb_dots_vb, 256, grid, dim3(256), 0, st.a, o);
    SELLA_LAUNCHB(c, emt_hvpb_gather_kernel, emt_hvpb_gather_vb, 256, grid, dim3(256), 0, st.a, o);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

// y = diag(H)[free] on the device: one launch, nothing waited for
int sella::emt_hvp_state_diag(sella_ctx* c, const EmtHvpState& st, const int* inv, double* y) {
    SELLA_LAUNCHB(c, emt_hdiag_kernel, emt_hdiag_vb, 256, dim3(st.a.n), dim3(256), 0, st.a, (const double*)st.F2, inv, y);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

// ---- the resident state of the operator of positions and cell (emt.h) ---------------------------------------------------
// SELLA_E_INVALID before anything is queued: a singular cell, shifts that are no lattice translations of it.
int sella::emt_chvp_state_create(sella_ctx* c, int n, const double* pos, const double* cell, const double* par, int nshift,
                                 const double* shifts, const double* dconst, double rc, double acut, double cutoff, double beta,
                                 int mc, const double* J, const double* G, const double* P, EmtCellHvpState* st) {
    std::vector<double> fix;                                          // n_s, J, G, P as they lie on the device
    SCHK(emt_image_indices(cell, nshift, shifts, fix));
    const size_t nT = (size_t)3 * nshift, nfix = nT + (size_t)9 * mc + (size_t)mc * mc + 81;
    fix.insert(fix.end(), J, J + 9 * mc);
    fix.insert(fix.end(), G, G + mc * mc);
    if (P) fix.insert(fix.end(), P, P + 81);
    else fix.insert(fix.end(), 81, 0.0);
    double* room;
    SCHK(emt_hvp_state_create_room(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta,
                                   nfix + (size_t)HVB_W * (nT + 18 + (size_t)9 * n), &st->s, &room));
    st->mc = mc;
    st->nimg = room; st->J = st->nimg + nT; st->G = st->J + 9 * mc; st->P = st->G + mc * mc;
    st->T = room + nfix; st->wv = st->T + HVB_W * nT; st->share = st->wv + HVB_W * 18;
    SCHK(h2d_async(c, room, fix.data(), nfix * sizeof(double)));
    return stream_wait(c);
}

static EmtCellOp emt_cell_op(const EmtCellHvpState& st, const EmtCellHvpIO& io, int nh) {
    EmtCellOp o;
    o.F2 = st.s.F2; o.nimg = st.nimg; o.J = st.J; o.G = st.G; o.P = st.P; o.mc = st.mc; o.nshift = st.s.a.nshift;
    o.T = st.T; o.wv = st.wv; o.share = st.share; o.cdot = st.s.cdot;
    o.X = io.X; o.ldx = io.ldx; o.Y = io.Y; o.ldy = io.ldy; o.inv = io.inv; o.mx = io.mx;
    o.vfull = io.vfull; o.ldv = io.ldv; o.hvfull = io.hvfull; o.partc = io.part; o.part = io.part;
    o.nb = (3 * st.s.a.n + 255) / 256; o.flag = io.flag; o.nh = nh;
    return o;
}

// one vector: four launches on the context's stream, nothing copied, nothing waited for
int sella::emt_chvp_state_apply(sella_ctx* c, const EmtCellHvpState& st, const EmtCellHvpIO& io) {
    const EmtCellOp o = emt_cell_op(st, io, 1);
    const int n = st.s.a.n;
    SELLA_LAUNCHB(c, emt_chvpo_scatter_kernel, emt_chvpo_scatter_vb, 256, dim3(o.nb + 1, 1), dim3(256), 0, 3 * n, o);
    SELLA_LAUNCHB(c, emt_chvpo1_dots_kernel, emt_chvpo1_dots_vb, 256, dim3(n), dim3(256), 0, st.s.a, o);
    SELLA_LAUNCHB(c, emt_chvpo1_gather_kernel, emt_chvpo1_gather_vb, 256, dim3(n), dim3(256), 0, st.s.a, o);
    SELLA_LAUNCHB(c, emt_chvpo_finish_kernel, emt_chvpo_finish_vb, 256, dim3(1), dim3(256), 0, n, o);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

// the nh <= HVB_W rows of a panel: the same four stages, CHVP_KQ rows per workgroup in the two pair passes
int sella::emt_chvp_state_apply_block(sella_ctx* c, const EmtCellHvpState& st, const EmtCellHvpIO& io, int nh) {
    const EmtCellOp o = emt_cell_op(st, io, nh);
    const int n = st.s.a.n;
    const dim3 grid(n, (unsigned)((nh + CHVP_KQ - 1) / CHVP_KQ));
    SELLA_LAUNCHB(c, emt_chvpo_scatter_kernel, emt_chvpo_scatter_vb, 256, dim3(o.nb + 1, nh), dim3(256), 0, 3 * n, o);
    SELLA_LAUNCHB(c, emt_chvpob_dots_kernel, emt_chvpob_dots_vb, 256, grid, dim3(256), 0, st.s.a, o);
    SELLA_LAUNCHB(c, emt_chvpob_gather_kernel, emt_chvpob_gather_vb, 256, grid, dim3(256), 0, st.s.a, o);
    SELLA_LAUNCHB(c, emt_chvpo_finish_kernel, emt_chvpo_finish_vb, 256, dim3(nh), dim3(256), 0, n, o);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

extern "C" int sella_emt_hessian(sella_ctx* c, int n, const double* pos, const double* par /* 9 x n */, int nshift,
                                 const double* shifts, double rc, double acut, double cutoff, double beta, sella_mat out) {
    if (!c || n <= 0 || !pos || !par || nshift <= 0 || !shifts) {
        set_error("emt_hessian: invalid arguments");
        return SELLA_E_INVALID;
    }
    return emt_hessian_resident(c, n, pos, par, nshift, shifts, nullptr, rc, acut, cutoff, beta, out);
}

extern "C" int sella_emt_hvp(sella_ctx* c, int n, const double* pos, const double* par /* 9 x n */, int nshift,
                             const double* shifts, double rc, double acut, double cutoff, double beta, const double* V, int k,
                             double* HV) {
    if (!c || n <= 0 || !pos || !par || nshift <= 0 || !shifts || !V || k <= 0 || !HV) {
        set_error("emt_hvp: invalid arguments");
        return SELLA_E_INVALID;
    }
    return emt_hvp_resident(c, n, pos, par, nshift, shifts, nullptr, rc, acut, cutoff, beta, V, k, HV);
}
