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
//   product: emt_f2 -> emt_hvp_dots (c_i = g_i . v) -> emt_hvp_gather ((H v)_i from c_i, c_j and the pair blocks), for up
//            to HVP_KQ vectors per workgroup
// No atomics: an atom can be a neighbour through several images, and those visits belong to different threads unless
// 256 divides N, so everything that lands in a shared place is added image by image with a barrier in between (one
// writer per (i, j) within an image, images in index order); per-thread sums run in the order of the lists and are
// reduced by block_sum.  The result does not depend on whether the lists were complete.
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
// false: not a pair (outside the cutoff, the atom itself, or the atom's own image)
__device__ __forceinline__ bool emt_pair(const EmtArgs& a, const EmtAtom& m, int t, EmtPair& p) {
    const int j = t & 0xffffff, s = t >> 24;
    if (j == m.i) return false;
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

struct EmtHessOut {
    const double* F2;
    double* H; int ldh;                     // 3n x 3n, zero on entry
    double* Gt; double* Gs; int ldg;        // n x 3n each: row i = g_i (zero on entry) and F2_i g_i
};

// Row block i of the pair term of H, and rows i of G^T and diag(F2) G^T.
__device__ __forceinline__ void emt_hess_pair_vb(const VB vb, EmtArgs a, EmtHessOut o) {
    __shared__ double red[4];
    __shared__ int incomplete;
    const int i = vb.x;
    const EmtAtom m = emt_atom(a, i);
    double* H0 = o.H + (size_t)(3 * i) * o.ldh;
    double* H1 = H0 + o.ldh;
    double* H2 = H1 + o.ldh;
    double* G = o.Gt + (size_t)i * o.ldg;
    double kxx = 0.0, kyy = 0.0, kzz = 0.0, kyz = 0.0, kxz = 0.0, kxy = 0.0;       // diagonal block: sum of K
    double gx = 0.0, gy = 0.0, gz = 0.0;                                          // g_i on atom i: -sum w' u
    auto visit = [&](int t) {
        EmtPair p;
        if (!emt_pair(a, m, t, p)) return;
        const double c1 = p.e1 / p.r, c2 = p.e2 - c1;                             // K = c1 I + c2 u u^T
        const double xx = c1 + c2 * (p.ux * p.ux), yy = c1 + c2 * (p.uy * p.uy), zz = c1 + c2 * (p.uz * p.uz);
        const double yz = c2 * (p.uy * p.uz), xz = c2 * (p.ux * p.uz), xy = c2 * (p.ux * p.uy);
        const int q = 3 * p.j;
        H0[q] -= xx; H0[q + 1] -= xy; H0[q + 2] -= xz;
        H1[q] -= xy; H1[q + 1] -= yy; H1[q + 2] -= yz;
        H2[q] -= xz; H2[q + 1] -= yz; H2[q + 2] -= zz;
        kxx += xx; kyy += yy; kzz += zz; kyz += yz; kxz += xz; kxy += xy;
        const double wx = p.wp_ij * p.ux, wy = p.wp_ij * p.uy, wz = p.wp_ij * p.uz;
        G[q] += wx; G[q + 1] += wy; G[q + 2] += wz;
        gx -= wx; gy -= wy; gz -= wz;
    };
    emt_by_image<true>(a, i, &incomplete, visit);
    kxx = block_sum(kxx, red); kyy = block_sum(kyy, red); kzz = block_sum(kzz, red);
    kyz = block_sum(kyz, red); kxz = block_sum(kxz, red); kxy = block_sum(kxy, red);
    gx = block_sum(gx, red); gy = block_sum(gy, red); gz = block_sum(gz, red);
    if (threadIdx.x == 0) {
        const int q = 3 * i;
        H0[q] = kxx; H0[q + 1] = kxy; H0[q + 2] = kxz;
        H1[q] = kxy; H1[q + 1] = kyy; H1[q + 2] = kyz;
        H2[q] = kxz; H2[q + 1] = kyz; H2[q + 2] = kzz;
        G[q] = gx; G[q + 1] = gy; G[q + 2] = gz;
    }
    __syncthreads();
    const double f2 = o.F2[i];
    double* Gs = o.Gs + (size_t)i * o.ldg;
    for (int q = threadIdx.x; q < 3 * a.n; q += 256) Gs[q] = f2 * G[q];
}
__global__ __launch_bounds__(256) void emt_hess_pair_kernel(EmtArgs a, EmtHessOut o) { emt_hess_pair_vb(vb_hw(), a, o); }

struct EmtHvp {                             // k vectors: every array holds round_up(k, HVP_KQ) rows, those of V beyond k zero
    const double* F2;
    const double* V;                        // (k, 3n)
    double* cdot;                           // (k, n): c_i = g_i . v
    double* HV;                             // (k, 3n)
};

// c_i[q] = g_i . v_q = sum over the pairs of w' u . (v_j - v_i), vectors HVP_KQ vb.y .. of the product
__device__ __forceinline__ void emt_hvp_dots_vb(const VB vb, EmtArgs a, EmtHvp o) {
    __shared__ double red[4];
    __shared__ int incomplete;
    const int i = vb.x, q0 = vb.y * HVP_KQ;
    const size_t n3 = (size_t)3 * a.n;
    const EmtAtom m = emt_atom(a, i);
    double vi[HVP_KQ][3], acc[HVP_KQ];
#pragma unroll
    for (int q = 0; q < HVP_KQ; ++q) {
        const double* v = o.V + (size_t)(q0 + q) * n3 + 3 * i;
        vi[q][0] = v[0]; vi[q][1] = v[1]; vi[q][2] = v[2];
        acc[q] = 0.0;
    }
    auto visit = [&](int t) {
        EmtPair p;
        if (!emt_pair(a, m, t, p)) return;
#pragma unroll
        for (int q = 0; q < HVP_KQ; ++q) {
            const double* v = o.V + (size_t)(q0 + q) * n3 + 3 * p.j;
            acc[q] += p.wp_ij * (p.ux * (v[0] - vi[q][0]) + p.uy * (v[1] - vi[q][1]) + p.uz * (v[2] - vi[q][2]));
        }
    };
    emt_by_image<false>(a, i, &incomplete, visit);
#pragma unroll
    for (int q = 0; q < HVP_KQ; ++q) {
        const double s = block_sum(acc[q], red);
        if (threadIdx.x == 0) o.cdot[(size_t)(q0 + q) * a.n + i] = s;
    }
}
__global__ __launch_bounds__(256) void emt_hvp_dots_kernel(EmtArgs a, EmtHvp o) { emt_hvp_dots_vb(vb_hw(), a, o); }

// (H v)_i = sum over the pairs of  -u (F2_i c_i w'_ij + F2_j c_j w'_ji)  +  K (v_i - v_j):
// g_i on atom i is -sum w'_ij u, g_j on atom i is -w'_ji u (atom i seen from j lies along -u)
__device__ __forceinline__ void emt_hvp_gather_vb(const VB vb, EmtArgs a, EmtHvp o) {
    __shared__ double red[4];
    __shared__ int incomplete;
    const int i = vb.x, q0 = vb.y * HVP_KQ;
    const size_t n3 = (size_t)3 * a.n;
    const EmtAtom m = emt_atom(a, i);
    const double f2i = o.F2[i];
    double vi[HVP_KQ][3], fc[HVP_KQ], acc[HVP_KQ][3];
#pragma unroll
    for (int q = 0; q < HVP_KQ; ++q) {
        const double* v = o.V + (size_t)(q0 + q) * n3 + 3 * i;
        vi[q][0] = v[0]; vi[q][1] = v[1]; vi[q][2] = v[2];
        fc[q] = f2i * o.cdot[(size_t)(q0 + q) * a.n + i];
        acc[q][0] = acc[q][1] = acc[q][2] = 0.0;
    }
    auto visit = [&](int t) {
        EmtPair p;
        if (!emt_pair(a, m, t, p)) return;
        const double c1 = p.e1 / p.r, c2 = p.e2 - c1;
        const double f2j = o.F2[p.j];
#pragma unroll
        for (int q = 0; q < HVP_KQ; ++q) {
            const double* v = o.V + (size_t)(q0 + q) * n3 + 3 * p.j;
            const double dx = vi[q][0] - v[0], dy = vi[q][1] - v[1], dz = vi[q][2] - v[2];
            const double along = c2 * (p.ux * dx + p.uy * dy + p.uz * dz)
                                 - (fc[q] * p.wp_ij + f2j * o.cdot[(size_t)(q0 + q) * a.n + p.j] * p.wp_ji);
            acc[q][0] += c1 * dx + along * p.ux;
            acc[q][1] += c1 * dy + along * p.uy;
            acc[q][2] += c1 * dz + along * p.uz;
        }
    };
    emt_by_image<false>(a, i, &incomplete, visit);
#pragma unroll
    for (int q = 0; q < HVP_KQ; ++q) {
        const double sx = block_sum(acc[q][0], red), sy = block_sum(acc[q][1], red), sz = block_sum(acc[q][2], red);
        if (threadIdx.x == 0) {
            double* out = o.HV + (size_t)(q0 + q) * n3 + 3 * i;
            out[0] = sx; out[1] = sy; out[2] = sz;
        }
    }
}
__global__ __launch_bounds__(256) void emt_hvp_gather_kernel(EmtArgs a, EmtHvp o) { emt_hvp_gather_vb(vb_hw(), a, o); }

struct TempMats {                           // device matrices of one call, back to the pool on every way out (stream-ordered)
    sella_ctx* c;
    sella_mat h[2] = {SELLA_NO_MAT, SELLA_NO_MAT};
    explicit TempMats(sella_ctx* ctx) : c(ctx) {}
    ~TempMats() {
        for (sella_mat m : h)
            if (m != SELLA_NO_MAT) sella_mat_free(c, m);
    }
};

}  // namespace
}  // namespace sella

using namespace sella;

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
    SCHK(emt_density_queue(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta, (size_t)n, &a, &F2));
    TempMats t(c);
    SCHK(mat_new(c, n, 3 * n, &t.h[0]));                              // zeroed: the visits add into the rows
    SCHK(mat_new(c, n, 3 * n, &t.h[1]));
    H = mat_get(c, out);
    Mat *Gt = mat_get(c, t.h[0]), *Gs = mat_get(c, t.h[1]);
    HIPCHK(s_memset0(c, H->d, (size_t)H->rows * H->ld * sizeof(double)));
    SELLA_LAUNCHB(c, emt_f2_kernel, emt_f2_vb, 256, dim3((n + 255) / 256), dim3(256), 0, a, F2);
    EmtHessOut o;
    o.F2 = F2; o.H = H->d; o.ldh = H->ld; o.Gt = Gt->d; o.Gs = Gs->d; o.ldg = Gt->ld;
    SELLA_LAUNCHB(c, emt_hess_pair_kernel, emt_hess_pair_vb, 256, dim3(n), dim3(256), 0, a, o);
    HIPCHK(hipGetLastError());
    // H += G diag(F2) G^T, G^T = Gt (n x 3n)
    SCHK(launch_gemm(c, 1, 0, 3 * n, 3 * n, n, 1.0, Gt->d, Gt->ld, Gs->d, Gs->ld, 1.0, H->d, H->ld));
    // the two triangles agree to rounding only (x_j + shift - x_i from either end, the tiles of the product)
    SCHK(launch_symmetrize(c, H->d, 3 * n, H->ld));
    return stream_wait(c);
}

// V, HV: (k, 3n) host arrays, one vector per row
int sella::emt_hvp_resident(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                            const double* dconst, double rc, double acut, double cutoff, double beta, const double* V, int k,
                            double* HV) {
    const size_t n3 = (size_t)3 * n, kp = (size_t)round_up(k, HVP_KQ);
    EmtArgs a;
    double* ex;
    SCHK(emt_density_queue(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta, (size_t)n + kp * (2 * n3 + n), &a,
                           &ex));
    EmtHvp o;
    double* dV = ex + n;
    o.F2 = ex; o.V = dV; o.cdot = dV + kp * n3; o.HV = o.cdot + kp * n;
    SCHK(h2d_async(c, dV, V, (size_t)k * n3 * sizeof(double)));
    if (kp > (size_t)k) HIPCHK(s_memset0(c, dV + (size_t)k * n3, (kp - k) * n3 * sizeof(double)));
    SELLA_LAUNCHB(c, emt_f2_kernel, emt_f2_vb, 256, dim3((n + 255) / 256), dim3(256), 0, a, ex);
    const dim3 grid(n, (unsigned)(kp / HVP_KQ));
    SELLA_LAUNCHB(c, emt_hvp_dots_kernel, emt_hvp_dots_vb, 256, grid, dim3(256), 0, a, o);
    SELLA_LAUNCHB(c, emt_hvp_gather_kernel, emt_hvp_gather_vb, 256, grid, dim3(256), 0, a, o);
    HIPCHK(hipGetLastError());
    SCHK(d2h_async(c, HV, o.HV, (size_t)k * n3 * sizeof(double)));
    return stream_wait(c);
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
