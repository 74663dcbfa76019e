// The far side of the calculator boundary, for calculators that live in this library (sella/peswrapper.py:413-418 calls
// `atoms.get_potential_energy()` / `get_forces()`; any ASE calculator stays a host-language callback), and the
// finite-difference Hessian operator of sella/linalg.py:14-101 on top of one — so that an iterative diagonalisation
// (peswrapper.py:508-556) through such a calculator is ONE library call: sella_davidson with sella_fd_matvec as its
// operator, no host-language frame between the force calls.
//
//   sella_calc_model_*   f(x) = 1/2 x^T A x + c/3 sum_j (u_j . x)^3, A resident (the model PES of SURVEY.md section 8d)
//   sella_calc_emt_*     effective-medium theory (emt.hip, sella_emt_eval)
//   sella_calc_pair_*    a Morse or Lennard-Jones pair potential (pair.hip, sella_pair_eval)
//   sella_calc_tip3p_*   TIP3P water (tip3p.hip, sella_tip3p_eval)
//   sella_fd_*           H v ~ (g(x0 + eta v^) - g0) / eta (or the central form), seen through a selection of free
//                        coordinates; every product is remembered as a secant pair for the Hessian update afterwards
//   sella_hvp_*          H v in closed form (EMT: emt_hessian.hip; pair: pair.hip; TIP3P: tip3p.hip; model: A v + sum_j 2 c (u_j . x0)(u_j . v) u_j) through the
//                        same selection, on a state built once at x0 and owned by the operator: device vector in, device
//                        vector out, no host wait per product (the third operator kind of sella_davidson, davidson.hip);
//                        the pairs are recorded on the device.  Not force calls.  The same for the rows of a device panel
//                        (hvp_device_apply_block: the operator of sella_davidson_block_hvp; not recorded), and diag(H).
//                        A second kind (sella_hvp_create_cell, EMT only): the Hessian of positions and cell in the
//                        coordinates [x; p] of a cell run, through the same entries
#include "emt.h"
#include "pair.h"
#include "tip3p.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace sella;

struct sella_calc {
    sella_ctx* c = nullptr;
    int kind = 0;                     // 0 model, 1 EMT, 2 pair potential, 3 TIP3P water
    int n = 0;
    long ncalls = 0;
    // model
    sella_mat A = SELLA_NO_MAT;
    std::vector<double> U;
    int nu = 0;
    double cc = 0.0;
    // EMT
    int natoms = 0, nshift = 0;
    std::vector<double> par, shifts;
    double rc = 0, acut = 0, cutoff = 0, beta = 0;
    std::vector<double> work;
    // pair potential (natoms, nshift, shifts as for EMT)
    int form = 0;
    PairPot pot = {};
    double* dconst = nullptr;         // EMT: parameter table + shift vectors, resident; model: the rows u_j (nu x ld);
                                      // pair: the parameters as given (3 doubles) + shift vectors
    size_t dconst_bytes = 0;
    // TIP3P (natoms = 3 molecules' sites; nothing resident: the parameters travel in the kernel arguments)
    TipPot tip = {};
};

namespace {
// g_i = (A x)_i + sum_j c p_j^2 u_j[i],  p = U x: the gradient of the cubic terms, the rows u_j taken in order
__device__ __forceinline__ void model_grad_vb(const VB vb, int n, int nu, int ld, double cc, const double* __restrict__ Ax,
                                                         const double* __restrict__ p, const double* __restrict__ U,
                                                         double* __restrict__ g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int i = vb.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = Ax[i];
    for (int j = 0; j < nu; ++j) {
        const double w = cc * p[j] * p[j];
        v += w * U[(size_t)j * ld + i];
    }
    g[i] = v;
}
__global__ __launch_bounds__(256) void model_grad_kernel(int n, int nu, int ld, double cc, const double* __restrict__ Ax,
                                                         const double* __restrict__ p, const double* __restrict__ U,
                                                         double* __restrict__ g) { model_grad_vb(vb_hw(), n, nu, ld, cc, Ax, p, U, g); }

// The eigensolver's vector x (its entry inv[p] belongs to full coordinate p; -1: pinned, zero; inv null: all free) as a
// full-length row of the pair record, and |v|^2 of this workgroup's 256 entries into part[workgroup]
__device__ __forceinline__ void hvp_scatter_vb(const VB vb, int n, const double* __restrict__ x, const int* __restrict__ inv,
                                               double* __restrict__ vfull, double* __restrict__ part) {
    __shared__ double red[4];
    const int p = vb.x * 256 + threadIdx.x;
    double v = 0.0;
    if (p < n) {
        const int q = inv ? inv[p] : p;
        if (q >= 0) v = x[q];
        vfull[p] = v;
    }
    const double s = block_sum(v * v, red);
    if (threadIdx.x == 0) part[vb.x] = s;
}
__global__ __launch_bounds__(256) void hvp_scatter_kernel(int n, const double* __restrict__ x, const int* __restrict__ inv,
                                                          double* __restrict__ vfull, double* __restrict__ part) { hvp_scatter_vb(vb_hw(), n, x, inv, vfull, part); }

// Model kind: hv = A v (there already) + sum_j t_j S_j, S_j = 2 c (u_j . x0) u_j, t = U v, the rows taken in order; a
// vanishing vector (|v| < 1e-12 from the partial sums) gives zero and flag 0; the free rows also go into y
__device__ __forceinline__ void hvp_model_finish_vb(const VB vb, int n, int nu, int ld, const double* __restrict__ S,
                                                    const double* __restrict__ t, const double* __restrict__ part, int nb,
                                                    const int* __restrict__ inv, double* __restrict__ hv, double* __restrict__ y,
                                                    int* __restrict__ flag) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double red[4];
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s += part[b];
    s = block_sum(s, red);
    const bool live = !(sqrt(s) < 1e-12);
    if (vb.x == 0 && threadIdx.x == 0) *flag = live ? 1 : 0;
    const int p = vb.x * 256 + threadIdx.x;
    if (p >= n) return;
    double h = hv[p];
    for (int j = 0; j < nu; ++j) h += t[j] * S[(size_t)j * ld + p];
    if (!live) h = 0.0;
    hv[p] = h;
    const int q = inv ? inv[p] : p;
    if (q >= 0) y[q] = h;
}
__global__ __launch_bounds__(256) void hvp_model_finish_kernel(int n, int nu, int ld, const double* __restrict__ S,
                                                               const double* __restrict__ t, const double* __restrict__ part, int nb,
                                                               const int* __restrict__ inv, double* __restrict__ hv, double* __restrict__ y,
                                                               int* __restrict__ flag) { hvp_model_finish_vb(vb_hw(), n, nu, ld, S, t, part, nb, inv, hv, y, flag); }

// The block form of hvp_scatter: the nh <= 16 rows of the eigensolver's panel X (row h at X + h ldx) as full-length rows,
// zero on the pinned coordinates and in the rows from nh on, row h at out + h ldo.  No |v|^2: a block product has no
// vanishing-vector rule.
__device__ __forceinline__ void hvp_scatter_block_vb(const VB vb, int n, int nh, const double* __restrict__ X, int ldx,
                                                     const int* __restrict__ inv, double* __restrict__ out, int ldo) {
    const int p = vb.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int q = inv ? inv[p] : p;
#pragma unroll
    for (int h = 0; h < 16; ++h) {
        const double v = (h < nh && q >= 0) ? X[(size_t)h * ldx + q] : 0.0;
        out[(size_t)h * ldo + p] = v;
    }
}
__global__ __launch_bounds__(256) void hvp_scatter_block_kernel(int n, int nh, const double* __restrict__ X, int ldx,
                                                                const int* __restrict__ inv, double* __restrict__ out, int ldo) { hvp_scatter_block_vb(vb_hw(), n, nh, X, ldx, inv, out, ldo); }

// Model kind, row vb.y of a block: hvp_model_finish's arithmetic (hv = A v + sum_j t_j S_j, the rows taken in order) on the
// panels A V (HV) and U V (T), the free entries into row vb.y of Y
__device__ __forceinline__ void hvp_model_finish_block_vb(const VB vb, int n, int nu, int ld, const double* __restrict__ S,
                                                          const double* __restrict__ T, int ldt, const double* __restrict__ HV,
                                                          int ldh, const int* __restrict__ inv, double* __restrict__ Y, int ldy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int p = vb.x * 256 + threadIdx.x, h = vb.y;
    if (p >= n) return;
    double v = HV[(size_t)h * ldh + p];
    for (int j = 0; j < nu; ++j) v += T[(size_t)h * ldt + j] * S[(size_t)j * ld + p];
    const int q = inv ? inv[p] : p;
    if (q >= 0) Y[(size_t)h * ldy + q] = v;
}
__global__ __launch_bounds__(256) void hvp_model_finish_block_kernel(int n, int nu, int ld, const double* __restrict__ S,
                                                                     const double* __restrict__ T, int ldt, const double* __restrict__ HV,
                                                                     int ldh, const int* __restrict__ inv, double* __restrict__ Y, int ldy) { hvp_model_finish_block_vb(vb_hw(), n, nu, ld, S, T, ldt, HV, ldh, inv, Y, ldy); }

// Model kind: diag(H)[free] = A_pp + sum_j S_j[p] u_j[p], the rows taken in order
__device__ __forceinline__ void hvp_model_diag_vb(const VB vb, int n, int nu, int ld, const double* __restrict__ A, int lda,
                                                  const double* __restrict__ S, const double* __restrict__ U,
                                                  const int* __restrict__ inv, double* __restrict__ y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int p = vb.x * 256 + threadIdx.x;
    if (p >= n) return;
    double d = A[(size_t)p * lda + p];
    for (int j = 0; j < nu; ++j) d += S[(size_t)j * ld + p] * U[(size_t)j * ld + p];
    const int q = inv ? inv[p] : p;
    if (q >= 0) y[q] = d;
}
__global__ __launch_bounds__(256) void hvp_model_diag_kernel(int n, int nu, int ld, const double* __restrict__ A, int lda,
                                                             const double* __restrict__ S, const double* __restrict__ U,
                                                             const int* __restrict__ inv, double* __restrict__ y) { hvp_model_diag_vb(vb_hw(), n, nu, ld, A, lda, S, U, inv, y); }
}  // namespace

extern "C" int sella_calc_model_create(sella_ctx* c, sella_mat A, const double* U, int nu, int n, double cc, sella_calc** out) {
    Mat* a = mat_get(c, A);
    if (!c || !out || !a || a->rows != n || a->cols != n || nu < 0 || (nu > 0 && !U)) {
        set_error("calc_model: invalid arguments");
        return SELLA_E_INVALID;
    }
    sella_calc* k = new sella_calc();
    k->c = c; k->kind = 0; k->n = n; k->A = A; k->nu = nu; k->cc = cc;
    k->U.assign(U, U + (size_t)nu * n);
    k->work.resize((size_t)n);
    if (nu > 0) {
        const int ld = round_up(n, 8);
        k->dconst_bytes = ((size_t)nu + 2) * ld * sizeof(double);
        int st = dev_alloc(c, k->dconst_bytes, &k->dconst);
        if (st == SELLA_OK) st = s_memset0(c, k->dconst, k->dconst_bytes) == hipSuccess ? SELLA_OK : SELLA_E_HIP;
        for (int j = 0; j < nu && st == SELLA_OK; ++j)
            st = h2d_async(c, k->dconst + (size_t)j * ld, U + (size_t)j * n, (size_t)n * sizeof(double));
        if (st == SELLA_OK) st = stream_wait(c);
        if (st != SELLA_OK) { delete k; return st; }
    }
    *out = k;
    return SELLA_OK;
}

int sella::calc_queue(sella_calc* k, const double* x, double** g_dev, double** aux_dev, int* naux) {
    sella_ctx* c = k->c;
    ++k->ncalls;
    if (k->kind == 1) {
        double *dea, *dgr;
        SCHK(emt_queue(c, k->natoms, x, k->par.data(), k->nshift, k->shifts.data(), k->dconst, k->rc, k->acut, k->cutoff, k->beta,
                       &dea, &dgr));
        *g_dev = dgr;
        *aux_dev = dea;
        *naux = k->natoms;
        return SELLA_OK;
    }
    if (k->kind == 2) {
        double *dea, *dgr;
        SCHK(pair_queue(c, k->natoms, x, k->form, k->pot, k->nshift, k->shifts.data(), k->dconst ? k->dconst + 3 : nullptr, &dea,
                        &dgr, false));
        *g_dev = dgr;
        *aux_dev = dea;
        *naux = k->natoms;
        return SELLA_OK;
    }
    if (k->kind == 3) {
        double *dem, *dgr;
        SCHK(tip3p_queue(c, k->tip, x, &dem, &dgr));
        *g_dev = dgr;
        *aux_dev = dem;
        *naux = k->tip.nmol;
        return SELLA_OK;
    }
    const int n = k->n, ld = round_up(n, 8), nu = k->nu;
    Mat* A = mat_get(c, k->A);
    if (!A) return SELLA_E_INVALID;
    double* buf;                                       // x | A x | p (8-padded) | g
    const int ldp = round_up(nu > 0 ? nu : 1, 8);
    SCHK(scratch_get(c, SCR_MISC0, ((size_t)3 * ld + ldp) * sizeof(double), &buf));
    double *dx = buf, *dAx = buf + ld, *dp = buf + 2 * (size_t)ld, *dg = dp + ldp;
    SCHK(h2d_async(c, dx, x, (size_t)n * sizeof(double)));
    SCHK(launch_gemv_rows(c, A->d, n, n, A->ld, dx, ld, 1, dAx, ld, GemvEpi()));
    if (nu > 0) SCHK(launch_gemv_rows(c, k->dconst, nu, n, ld, dx, ld, 1, dp, ldp, GemvEpi()));
    SELLA_LAUNCHB(c, model_grad_kernel, model_grad_vb, 256, dim3((n + 255) / 256), dim3(256), 0, n, nu, ld, k->cc, dAx, dp, k->dconst, dg);
    HIPCHK(hipGetLastError());
    *g_dev = dg;
    *aux_dev = dAx;                                    // A x (ld entries) then p: one read-back
    *naux = ld + ldp;
    return SELLA_OK;
}

double sella::calc_finish(sella_calc* k, const double* x, const double* aux) {
    if (k->kind == 1 || k->kind == 2 || k->kind == 3) {
        const int ne = k->kind == 3 ? k->tip.nmol : k->natoms;      // per-atom or per-molecule energies, in index order
        double e = 0.0;
        for (int i = 0; i < ne; ++i) e += aux[i];
        return e;
    }
    const int n = k->n, ld = round_up(n, 8);
    double e = 0.0;
    for (int i = 0; i < n; ++i) e += x[i] * aux[i];
    e *= 0.5;
    double cub = 0.0;
    for (int j = 0; j < k->nu; ++j) { const double p = aux[ld + j]; cub += p * p * p; }
    return e + k->cc / 3.0 * cub;
}

extern "C" int sella_calc_emt_create(sella_ctx* c, int natoms, const double* par, int nshift, const double* shifts, double rc,
                                     double acut, double cutoff, double beta, sella_calc** out) {
    if (!c || !out || natoms <= 0 || !par || nshift <= 0 || !shifts) {
        set_error("calc_emt: invalid arguments");
        return SELLA_E_INVALID;
    }
    sella_calc* k = new sella_calc();
    k->c = c; k->kind = 1; k->n = 3 * natoms; k->natoms = natoms; k->nshift = nshift;
    k->par.assign(par, par + (size_t)9 * natoms);
    k->shifts.assign(shifts, shifts + (size_t)3 * nshift);
    k->rc = rc; k->acut = acut; k->cutoff = cutoff; k->beta = beta;
    k->dconst_bytes = ((size_t)9 * natoms + (size_t)3 * nshift) * sizeof(double);
    if (dev_alloc(c, k->dconst_bytes, &k->dconst) == SELLA_OK) {
        int st = h2d_async(c, k->dconst, par, (size_t)9 * natoms * sizeof(double));
        if (st == SELLA_OK) st = h2d_async(c, k->dconst + (size_t)9 * natoms, shifts, (size_t)3 * nshift * sizeof(double));
        if (st == SELLA_OK) st = stream_wait(c);
        if (st != SELLA_OK) { dev_free(c, k->dconst, k->dconst_bytes); k->dconst = nullptr; }
    } else {
        k->dconst = nullptr;
    }
    *out = k;
    return SELLA_OK;
}

// A pair potential (pair.hip): form 0 Morse (params D, a, r0), 1 Lennard-Jones (params eps, sigma); rcut <= 0: no cutoff, for a
// system without periodic images only.  The parameters as given and the shifts stay resident.
extern "C" int sella_calc_pair_create(sella_ctx* c, int natoms, int form, const double* params, int nshift, const double* shifts,
                                      double rcut, sella_calc** out) {
    PairPot pot;
    const char* bad = (!c || !out) ? "invalid arguments" : pair_pot_make(natoms, form, params, nshift, shifts, rcut, &pot);
    if (bad) {
        set_error("calc_pair: %s", bad);
        return SELLA_E_INVALID;
    }
    sella_calc* k = new sella_calc();
    k->c = c; k->kind = 2; k->n = 3 * natoms; k->natoms = natoms; k->nshift = nshift;
    k->form = form; k->pot = pot;
    k->shifts.assign(shifts, shifts + (size_t)3 * nshift);
    const double par3[3] = {params[0], params[1], form == PAIR_MORSE ? params[2] : 0.0};
    k->dconst_bytes = ((size_t)3 + (size_t)3 * nshift) * sizeof(double);
    if (dev_alloc(c, k->dconst_bytes, &k->dconst) == SELLA_OK) {
        int st = h2d_async(c, k->dconst, par3, sizeof(par3));
        if (st == SELLA_OK) st = h2d_async(c, k->dconst + 3, shifts, (size_t)3 * nshift * sizeof(double));
        if (st == SELLA_OK) st = stream_wait(c);
        if (st != SELLA_OK) { dev_free(c, k->dconst, k->dconst_bytes); k->dconst = nullptr; }
    } else {
        k->dconst = nullptr;
    }
    *out = k;
    return SELLA_OK;
}

// TIP3P water (tip3p.hip): n_mol molecules as consecutive triples with the oxygen at site o, box edges (<= 0: not periodic),
// params q_H, sigma, epsilon, k_e, rc, width.  Everything travels in the kernel arguments: nothing is resident.
extern "C" int sella_calc_tip3p_create(sella_ctx* c, int n_mol, int o, const double* box, const double* params, sella_calc** out) {
    TipPot pot;
    const double origin[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // (the positions come with every call: one molecule's worth of zeros stands in for them in the check)
    const char* bad = (!c || !out || n_mol <= 0) ? "invalid arguments" : tip3p_pot_make(1, origin, o, box, params, &pot);
    if (!bad && (long)3 * n_mol >= (1L << 24)) bad = "at most 2^24 sites";
    if (bad) {
        set_error("calc_tip3p: %s", bad);
        return SELLA_E_INVALID;
    }
    pot.nmol = n_mol;
    sella_calc* k = new sella_calc();
    k->c = c; k->kind = 3; k->n = 9 * n_mol; k->natoms = 3 * n_mol; k->tip = pot;
    *out = k;
    return SELLA_OK;
}

// energy and gradient dE/dx at x (n entries)
extern "C" int sella_calc_eval(sella_calc* k, const double* x, double* f, double* g) {
    if (!k || !x || !f || !g) return SELLA_E_INVALID;
    double *dg, *daux;
    int naux = 0;
    SCHK(calc_queue(k, x, &dg, &daux, &naux));
    std::vector<double>& aux = k->work;
    aux.resize((size_t)naux);
    SCHK(d2h_async(k->c, aux.data(), daux, (size_t)naux * sizeof(double)));
    SCHK(d2h_async(k->c, g, dg, (size_t)k->n * sizeof(double)));
    SCHK(stream_wait(k->c));
    *f = calc_finish(k, x, aux.data());
    return SELLA_OK;
}

// Second derivatives at x: `out` (n x n, the caller's) stays on the device.  EMT: emt_hessian.hip on the resident
// constants; model: A + 2 c sum_j (u_j . x) u_j u_j^T, the rows u_j scaled on the host and one rank-nu product.
// Not force calls: ncalls is unchanged.
extern "C" int sella_calc_hessian(sella_calc* k, const double* x, sella_mat out) {
    if (!k || !x) {
        set_error("calc_hessian: invalid arguments");
        return SELLA_E_INVALID;
    }
    sella_ctx* c = k->c;
    if (k->kind == 1)
        return emt_hessian_resident(c, k->natoms, x, k->par.data(), k->nshift, k->shifts.data(), k->dconst, k->rc, k->acut,
                                    k->cutoff, k->beta, out);
    if (k->kind == 2)
        return pair_hessian_resident(c, k->natoms, x, k->form, k->pot, k->nshift, k->shifts.data(),
                                     k->dconst ? k->dconst + 3 : nullptr, out);
    if (k->kind == 3) return tip3p_hessian_resident(c, k->tip, x, out);
    const int n = k->n, nu = k->nu, ld = round_up(n, 8);
    Mat *A = mat_get(c, k->A), *H = mat_get(c, out);
    if (!A) {
        set_error("calc_hessian: the model calculator's matrix A is gone");
        return SELLA_E_INVALID;
    }
    if (!H || H->rows != n || H->cols != n) {
        set_error("calc_hessian: out must be %d x %d", n, n);
        return SELLA_E_INVALID;
    }
    SCHK(launch_axpby2d(c, n, n, 1.0, A->d, A->ld, 0.0, nullptr, 0, H->d, H->ld));
    if (nu > 0) {
        std::vector<double>& S = c->hbuf_b;                            // rows 2 c (u_j . x) u_j, padded like the resident rows
        S.assign((size_t)nu * ld, 0.0);
        for (int j = 0; j < nu; ++j) {
            const double* u = k->U.data() + (size_t)j * n;
            double p = 0.0;
            for (int i = 0; i < n; ++i) p += u[i] * x[i];
            for (int i = 0; i < n; ++i) S[(size_t)j * ld + i] = 2.0 * k->cc * p * u[i];
        }
        double* dS;
        SCHK(scratch_get(c, SCR_MISC0, (size_t)nu * ld * sizeof(double), &dS));
        SCHK(h2d_async(c, dS, S.data(), (size_t)nu * ld * sizeof(double)));
        SCHK(launch_gemm(c, 1, 0, n, n, nu, 1.0, dS, ld, k->dconst, ld, 1.0, H->d, H->ld));
    }
    return stream_wait(c);
}

// H V^T for k vectors (V, HV: (k, n) host arrays, one vector per row), without the matrix for the EMT kind
extern "C" int sella_calc_hvp(sella_calc* k, const double* x, const double* V, int nv, double* HV) {
    if (!k || !x || !V || nv <= 0 || !HV) {
        set_error("calc_hvp: invalid arguments");
        return SELLA_E_INVALID;
    }
    sella_ctx* c = k->c;
    if (k->kind == 1)
        return emt_hvp_resident(c, k->natoms, x, k->par.data(), k->nshift, k->shifts.data(), k->dconst, k->rc, k->acut,
                                k->cutoff, k->beta, V, nv, HV);
    if (k->kind == 2)
        return pair_hvp_resident(c, k->natoms, x, k->form, k->pot, k->nshift, k->shifts.data(), V, nv, HV);
    if (k->kind == 3) return tip3p_hvp_resident(c, k->tip, x, V, nv, HV);
    const int n = k->n, nu = k->nu, ld = round_up(n, 8);
    Mat* A = mat_get(c, k->A);
    if (!A) {
        set_error("calc_hvp: the model calculator's matrix A is gone");
        return SELLA_E_INVALID;
    }
    double* buf;                                                       // V | A V (rows of ld)
    SCHK(scratch_get(c, SCR_MISC0, (size_t)2 * nv * ld * sizeof(double), &buf));
    double *dV = buf, *dAV = buf + (size_t)nv * ld;
    HIPCHK(s_memset0(c, dV, (size_t)nv * ld * sizeof(double)));
    for (int q = 0; q < nv; ++q) SCHK(h2d_async(c, dV + (size_t)q * ld, V + (size_t)q * n, (size_t)n * sizeof(double)));
    SCHK(launch_gemm(c, 0, 1, nv, n, n, 1.0, dV, ld, A->d, A->ld, 0.0, dAV, ld));     // row q: (A v_q)^T
    SCHK(d2h_async_2d(c, HV, dAV, (size_t)ld * sizeof(double), (size_t)n * sizeof(double), (size_t)nv));
    SCHK(stream_wait(c));
    for (int j = 0; j < nu; ++j) {                                     // + 2 c (u_j . x) (u_j . v_q) u_j
        const double* u = k->U.data() + (size_t)j * n;
        double p = 0.0;
        for (int i = 0; i < n; ++i) p += u[i] * x[i];
        for (int q = 0; q < nv; ++q) {
            double t = 0.0;
            for (int i = 0; i < n; ++i) t += u[i] * V[(size_t)q * n + i];
            const double f = 2.0 * k->cc * p * t;
            for (int i = 0; i < n; ++i) HV[(size_t)q * n + i] += f * u[i];
        }
    }
    return SELLA_OK;
}

extern "C" long sella_calc_ncalls(sella_calc* k) { return k ? k->ncalls : 0; }
extern "C" int sella_calc_dim(sella_calc* k) { return k ? k->n : 0; }
extern "C" int sella_calc_destroy(sella_calc* k) {
    if (k && k->dconst) dev_free(k->c, k->dconst, k->dconst_bytes);
    delete k;
    return SELLA_OK;
}

// ---- finite-difference Hessian operator (sella/linalg.py:14-101) ---------------------------------------------------------
struct sella_fd {
    sella_calc* calc = nullptr;
    int n = 0, m = 0;                 // full dimension, dimension the eigensolver sees
    double eta = 0.0;
    int threepoint = 0;
    std::vector<double> x0, g0, vfull, xd, ahead, behind;
    std::vector<int> idx;             // free coordinates (empty: all)
    std::vector<double> Vs, AVs;      // recorded pairs, k x n each (pair-major)
    int npairs = 0;
    long calls = 0;
};

extern "C" int sella_fd_create(sella_calc* calc, int n, const double* x0, const double* g0, double eta, int threepoint,
                               const int* idx, int m, sella_fd** out) {
    if (!calc || !out || !x0 || !g0 || n <= 0 || calc->n != n || !(eta > 0.0) || (idx && (m <= 0 || m > n))) {
        set_error("fd operator: invalid arguments");
        return SELLA_E_INVALID;
    }
    sella_fd* o = new sella_fd();
    o->calc = calc; o->n = n; o->eta = eta; o->threepoint = threepoint;
    o->x0.assign(x0, x0 + n);
    o->g0.assign(g0, g0 + n);
    if (idx) o->idx.assign(idx, idx + m);
    o->m = idx ? m : n;
    o->vfull.resize(n); o->xd.resize(n); o->ahead.resize(n); o->behind.resize(n);
    *out = o;
    return SELLA_OK;
}

// sella_matvec_fn: Av = U^T H U v through finite differences of the calculator's gradient
extern "C" int sella_fd_matvec(void* user, const double* v, double* Av, int m) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    sella_fd* o = static_cast<sella_fd*>(user);
    if (!o || !v || !Av || m != o->m) return SELLA_E_INVALID;
    const int n = o->n;
    ++o->calls;
    double* vf = o->vfull.data();
    if (o->idx.empty()) {
        for (int i = 0; i < n; ++i) vf[i] = v[i];
    } else {
        for (int i = 0; i < n; ++i) vf[i] = 0.0;
        for (int q = 0; q < m; ++q) vf[o->idx[q]] = v[q];
    }
    double len2 = 0.0;
    for (int i = 0; i < n; ++i) len2 += vf[i] * vf[i];
    const double length = std::sqrt(len2);
    if (length < 1e-12) {
        for (int q = 0; q < m; ++q) Av[q] = 0.0;
        return SELLA_OK;
    }
    // which of +-v is displaced along (linalg.py:45-73): downhill if v has a gradient component, else towards the origin,
    // else so that the first significant component is positive
    double sign = 0.0;
    const double* refs[2] = {o->g0.data(), o->x0.data()};
    for (int t = 0; t < 2 && sign == 0.0; ++t) {
        double proj = 0.0;
        for (int i = 0; i < n; ++i) proj += vf[i] * refs[t][i];
        if (std::fabs(proj) > 1e-4) sign = proj > 0.0 ? -1.0 : 1.0;
    }
    if (sign == 0.0) {
        sign = 1.0;
        for (int i = 0; i < n; ++i)
            if (std::fabs(vf[i]) > 1e-4) { sign = vf[i] < 0.0 ? -1.0 : 1.0; break; }
    }
    const double scale = sign * length;
    double f;
    for (int i = 0; i < n; ++i) o->xd[i] = o->x0[i] + (o->eta * vf[i]) / scale;
    SCHK(sella_calc_eval(o->calc, o->xd.data(), &f, o->ahead.data()));
    o->Vs.insert(o->Vs.end(), vf, vf + n);
    const size_t at = o->AVs.size();
    o->AVs.resize(at + n);
    double* out = o->AVs.data() + at;
    if (o->threepoint) {
        for (int i = 0; i < n; ++i) o->xd[i] = o->x0[i] - (o->eta * vf[i]) / scale;
        SCHK(sella_calc_eval(o->calc, o->xd.data(), &f, o->behind.data()));
        for (int i = 0; i < n; ++i) out[i] = (scale * (o->ahead[i] - o->behind[i])) / (2 * o->eta);
    } else {
        for (int i = 0; i < n; ++i) out[i] = (scale * (o->ahead[i] - o->g0[i])) / o->eta;
    }
    ++o->npairs;
    if (o->idx.empty()) for (int i = 0; i < n; ++i) Av[i] = out[i];
    else for (int q = 0; q < m; ++q) Av[q] = out[o->idx[q]];
    return SELLA_OK;
}

extern "C" int sella_fd_npairs(sella_fd* o) { return o ? o->npairs : 0; }
extern "C" long sella_fd_calls(sella_fd* o) { return o ? o->calls : 0; }

// recorded pairs as (n x k) row-major matrices (columns = products in call order)
extern "C" int sella_fd_pairs(sella_fd* o, double* Vs, double* AVs) {
    if (!o || !Vs || !AVs) return SELLA_E_INVALID;
    const int n = o->n, k = o->npairs;
    for (int p = 0; p < k; ++p)
        for (int i = 0; i < n; ++i) {
            Vs[(size_t)i * k + p] = o->Vs[(size_t)p * n + i];
            AVs[(size_t)i * k + p] = o->AVs[(size_t)p * n + i];
        }
    return SELLA_OK;
}

extern "C" int sella_fd_destroy(sella_fd* o) {
    delete o;
    return SELLA_OK;
}

// ---- analytic Hessian-vector operator ---------------------------------------------------------------------------------------
// The pair record lives on the device in chunks of HVP_CHUNK products that are added as products arrive (never sized by
// the eigensolver's iteration limit): rows [0, HVP_CHUNK) the full-space vectors, rows [HVP_CHUNK, 2 HVP_CHUNK) their
// products, ld apart and zero beyond n, then one int per product: 1 recorded, 0 a vanishing vector.  Single product number
// k (from zero, vanishing ones included; the rows of block products do not count here) owns row k mod HVP_CHUNK of chunk
// k / HVP_CHUNK, so the kernels write where the record wants the result and the host learns which rows count when it asks
// for the pairs.
constexpr int HVP_CHUNK = 16;
constexpr int HVP_BLOCK = 16;             // rows of a block product (the panel of sella_davidson_block)

struct sella_hvp {
    sella_calc* calc = nullptr;
    int n = 0, m = 0, ld = 0, nb = 0;     // full dimension, the eigensolver's, row stride, workgroups of the scatter
    bool select = false;
    EmtHvpState emt;                      // EMT kind
    PairHvpState pair;                    // pair kind
    TipHvpState tip;                      // TIP3P kind
    // the kind of positions and cell (sella_hvp_create_cell): n = nx + mc and m = mx + mc, the mc cell parameters behind the
    // nx position coordinates (mx of them free: inv covers the positions); nb counts the workgroups of the positions
    bool cell = false;
    int nx = 0, mx = 0, mc = 0;
    EmtCellHvpState cemt;
    double* aux = nullptr;                // part (nb) | x, y of the host entry (ld each) | model: S (nu x ld), t | inv (n ints)
    size_t aux_bytes = 0, chunk_bytes = 0;
    double *part = nullptr, *dx = nullptr, *dy = nullptr, *S = nullptr, *t = nullptr;
    int* inv = nullptr;
    std::vector<double*> chunks;
    std::vector<int> flags;               // host copy, valid for the first `nflags` products
    long calls = 0, nrec = 0;             // products taken (rows of block products included); single products = slots of the record
    // block products (hvp_device_apply_block), allocated with the first one: x, y of the host entry (HVP_BLOCK rows of ldm),
    // the full-length rows of a panel with pinned coordinates (HVP_BLOCK x ld), model: A V
    // (HVP_BLOCK x ld) and U V (HVP_BLOCK x ldt)
    double* blk = nullptr;
    size_t blk_bytes = 0;
    double *bx = nullptr, *by = nullptr, *bstage = nullptr, *bhv = nullptr, *bt = nullptr;
    int ldm = 0, ldt = 0;
};

static void hvp_release(sella_hvp* o) {
    sella_ctx* c = o->calc->c;
    (void)stream_sync_raw(c);
    if (o->cell) emt_hvp_state_destroy(c, &o->cemt.s);
    else if (o->calc->kind == 1) emt_hvp_state_destroy(c, &o->emt);
    else if (o->calc->kind == 2) pair_hvp_state_destroy(c, &o->pair);
    else if (o->calc->kind == 3) tip3p_hvp_state_destroy(c, &o->tip);
    for (double* p : o->chunks) dev_free(c, p, o->chunk_bytes);
    if (o->aux) dev_free(c, o->aux, o->aux_bytes);
    if (o->blk) dev_free(c, o->blk, o->blk_bytes);
    delete o;
}

// The operator's own device arrays (o->aux; o->n, o->ld set): `nparts` partial sums of |v|^2, the vectors of the host entry,
// the model kind's rows, and inv over the `ninv` coordinates the m indices idx select (idx null: no inv)
static int hvp_aux(sella_hvp* o, const int* idx, int m, int ninv, int nparts, int nu) {
    sella_ctx* c = o->calc->c;
    const size_t ld = (size_t)o->ld, ldp = (size_t)round_up(nu > 0 ? nu : 1, 8), nbp = (size_t)round_up(nparts, 8);
    const size_t words = nbp + 2 * ld + (size_t)nu * ld + ldp + (ld + 1) / 2;
    o->aux_bytes = words * sizeof(double);
    o->chunk_bytes = ((size_t)2 * HVP_CHUNK * ld + HVP_CHUNK) * sizeof(double);
    const int st = dev_alloc(c, o->aux_bytes, &o->aux);
    if (st != SELLA_OK) { o->aux = nullptr; return st; }
    HIPCHK(s_memset0(c, o->aux, o->aux_bytes));
    o->part = o->aux; o->dx = o->part + nbp; o->dy = o->dx + ld; o->S = o->dy + ld; o->t = o->S + (size_t)nu * ld;
    if (idx) {
        std::vector<int> inv((size_t)ninv, -1);
        for (int q = 0; q < m; ++q) inv[idx[q]] = q;
        o->inv = reinterpret_cast<int*>(o->t + ldp);
        SCHK(h2d_async(c, o->inv, inv.data(), (size_t)ninv * sizeof(int)));
    }
    return SELLA_OK;
}

static bool hvp_ascending(const int* idx, int m, int n) {
    for (int q = 0; q < m; ++q)
        if (idx[q] < 0 || idx[q] >= n || (q > 0 && idx[q] <= idx[q - 1])) return false;
    return true;
}

extern "C" int sella_hvp_create(sella_calc* calc, int n, const double* x0, const int* idx, int m, sella_hvp** out) {
    if (!calc || !out || !x0 || n <= 0 || calc->n != n || (idx && (m <= 0 || m > n))) {
        set_error("hvp operator: invalid arguments");
        return SELLA_E_INVALID;
    }
    if (idx && !hvp_ascending(idx, m, n)) {
        set_error("hvp operator: the free coordinates must be ascending indices below %d", n);
        return SELLA_E_INVALID;
    }
    sella_ctx* c = calc->c;
    const int nu = calc->kind == 0 ? calc->nu : 0;
    if (calc->kind == 0 && !mat_get(c, calc->A)) {
        set_error("hvp operator: the model calculator's matrix A is gone");
        return SELLA_E_INVALID;
    }
    sella_hvp* o = new sella_hvp();
    o->calc = calc; o->n = n; o->m = idx ? m : n; o->select = idx != nullptr;
    o->ld = round_up(n, 8);
    o->nb = (n + 255) / 256;
    auto fail = [&](int st) { hvp_release(o); return st; };
    int st = hvp_aux(o, idx, m, n, o->nb, nu);
    if (st != SELLA_OK) return fail(st);
    const size_t ld = (size_t)o->ld;
    if (calc->kind == 1) {
        st = emt_hvp_state_create(c, calc->natoms, x0, calc->par.data(), calc->nshift, calc->shifts.data(), calc->dconst, calc->rc,
                                  calc->acut, calc->cutoff, calc->beta, &o->emt);
    } else if (calc->kind == 2) {
        st = pair_hvp_state_create(c, calc->natoms, x0, calc->form, calc->pot, calc->nshift, calc->shifts.data(), &o->pair);
    } else if (calc->kind == 3) {
        st = tip3p_hvp_state_create(c, calc->tip, x0, &o->tip);
    } else {
        if (nu > 0) {
            std::vector<double> S((size_t)nu * ld, 0.0);               // rows 2 c (u_j . x0) u_j, as sella_calc_hessian builds them
            for (int j = 0; j < nu; ++j) {
                const double* u = calc->U.data() + (size_t)j * n;
                double p = 0.0;
                for (int i = 0; i < n; ++i) p += u[i] * x0[i];
                for (int i = 0; i < n; ++i) S[(size_t)j * ld + i] = 2.0 * calc->cc * p * u[i];
            }
            st = h2d_async(c, o->S, S.data(), S.size() * sizeof(double));
        }
        if (st == SELLA_OK) st = stream_wait(c);
    }
    if (st != SELLA_OK) return fail(st);
    *out = o;
    return SELLA_OK;
}

// The Hessian of positions and cell in the coordinates [x; p] of a cell run (emt_hessian.hip, the resident operator of
// positions and cell): n position coordinates at x0 in `cell` (lattice vectors in its rows), mc cell parameters with
// dC/dp = J (9 x mc), the curvature G (mc x mc, symmetric) of the parametrisation and P (9 x 9) of a pressure (NULL: none).
// idx: the mx free POSITION coordinates; the cell parameters are always free and stand behind them.
extern "C" int sella_hvp_create_cell(sella_calc* calc, int n, const double* x0, const double* cell, const int* idx, int mx, int mc,
                                     const double* J, const double* G, const double* P, sella_hvp** out) {
    if (!calc || !out || !x0 || !cell || !J || !G || n <= 0 || calc->n != n || (idx && (mx < 0 || mx > n))) {
        set_error("hvp cell operator: invalid arguments");
        return SELLA_E_INVALID;
    }
    if (calc->kind != 1) {
        static const char* const names[] = {"model", "EMT", "pair-potential", "TIP3P"};
        set_error("hvp cell operator: only the EMT calculator has second derivatives with respect to the cell, not the %s "
                  "calculator (kind %d)", names[calc->kind], calc->kind);
        return SELLA_E_INVALID;
    }
    if (mc < 1 || mc > 9) {
        set_error("hvp cell operator: 1 to 9 cell parameters, not %d", mc);
        return SELLA_E_INVALID;
    }
    if (idx && !hvp_ascending(idx, mx, n)) {
        set_error("hvp cell operator: the free coordinates must be ascending indices below %d", n);
        return SELLA_E_INVALID;
    }
    sella_ctx* c = calc->c;
    sella_hvp* o = new sella_hvp();
    o->calc = calc; o->cell = true; o->select = idx != nullptr;
    o->nx = n; o->mx = idx ? mx : n; o->mc = mc;
    o->n = n + mc; o->m = o->mx + mc;
    o->ld = round_up(o->n, 8);
    o->nb = (n + 255) / 256;
    int st = emt_chvp_state_create(c, calc->natoms, x0, cell, calc->par.data(), calc->nshift, calc->shifts.data(), calc->dconst,
                                   calc->rc, calc->acut, calc->cutoff, calc->beta, mc, J, G, P, &o->cemt);
    if (st == SELLA_OK) st = hvp_aux(o, idx, mx, n, o->nb + 1, 0);
    if (st != SELLA_OK) { hvp_release(o); return st; }
    *out = o;
    return SELLA_OK;
}

// y (m entries) = (H vfull)[free], x (m entries) the free entries of vfull, both on the device: queued on the context's
// stream, nothing waited for, nothing copied.  The product is a call whatever |x| is.
int sella::hvp_device_apply(sella_hvp* o, const double* x, double* y) {
    sella_calc* k = o->calc;
    sella_ctx* c = k->c;
    const long slot = o->nrec;
    const size_t ci = (size_t)(slot / HVP_CHUNK), r = (size_t)(slot % HVP_CHUNK), ld = (size_t)o->ld;
    if (ci == o->chunks.size()) {
        double* p;
        SCHK(dev_alloc(c, o->chunk_bytes, &p));
        o->chunks.push_back(p);
        HIPCHK(s_memset0(c, p, o->chunk_bytes));
    }
    double* base = o->chunks[ci];
    double *v = base + r * ld, *hv = base + (HVP_CHUNK + r) * ld;
    int* flag = reinterpret_cast<int*>(base + (size_t)2 * HVP_CHUNK * ld) + r;
    ++o->calls;
    ++o->nrec;
    if (o->cell) {
        const EmtCellHvpIO io = {x, 0, y, 0, o->inv, o->mx, v, 0, hv, o->part, flag};
        return emt_chvp_state_apply(c, o->cemt, io);
    }
    const int n = o->n;
    SELLA_LAUNCHB(c, hvp_scatter_kernel, hvp_scatter_vb, 256, dim3(o->nb), dim3(256), 0, n, x, (const int*)o->inv, v, o->part);
    if (k->kind == 1) return emt_hvp_state_apply(c, o->emt, v, hv, o->part, o->nb, o->inv, y, flag);
    if (k->kind == 2) return pair_hvp_state_apply(c, o->pair, v, hv, o->part, o->nb, o->inv, y, flag);
    if (k->kind == 3) return tip3p_hvp_state_apply(c, o->tip, v, hv, o->part, o->nb, o->inv, y, flag);
    Mat* A = mat_get(c, k->A);
    if (!A) {
        set_error("hvp operator: the model calculator's matrix A is gone");
        return SELLA_E_INVALID;
    }
    SCHK(launch_gemv_rows(c, A->d, n, n, A->ld, v, o->ld, 1, hv, o->ld, GemvEpi()));
    if (k->nu > 0) SCHK(launch_gemv_rows(c, k->dconst, k->nu, n, o->ld, v, o->ld, 1, o->t, round_up(k->nu, 8), GemvEpi()));
    SELLA_LAUNCHB(c, hvp_model_finish_kernel, hvp_model_finish_vb, 256, dim3(o->nb), dim3(256), 0, n, k->nu, o->ld,
                  (const double*)o->S, (const double*)o->t, (const double*)o->part, o->nb, (const int*)o->inv, hv, y, flag);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

static int hvp_block_buffers(sella_hvp* o) {
    if (o->blk) return SELLA_OK;
    sella_calc* k = o->calc;
    sella_ctx* c = k->c;
    const bool model = k->kind == 0;
    o->ldm = round_up(o->m, 8);
    o->ldt = round_up(model && k->nu > 0 ? k->nu : 1, 8);
    const size_t panel = (size_t)HVP_BLOCK * o->ld;
    const size_t words = (size_t)2 * HVP_BLOCK * o->ldm + panel + (model ? panel + (size_t)HVP_BLOCK * o->ldt : 0);
    double* p;
    SCHK(dev_alloc(c, words * sizeof(double), &p));
    if (s_memset0(c, p, words * sizeof(double)) != hipSuccess) {          // (the padding of the rows stays zero: panel operands)
        dev_free(c, p, words * sizeof(double));
        return SELLA_E_HIP;
    }
    o->blk = p;
    o->blk_bytes = words * sizeof(double);
    o->bx = p; o->by = o->bx + (size_t)HVP_BLOCK * o->ldm; o->bstage = o->by + (size_t)HVP_BLOCK * o->ldm;
    o->bhv = o->bstage + panel; o->bt = o->bhv + panel;
    return SELLA_OK;
}

// the kind of positions and cell: the rows are spread into the staging panel (the kernels need T = n_s W of every row anyway)
static int hvp_cell_block(sella_hvp* o, const double* X, int ldx, int nh, double* Y, int ldy) {
    const EmtCellHvpIO io = {X, ldx, Y, ldy, o->inv, o->mx, o->bstage, o->ld, nullptr, nullptr, nullptr};
    return emt_chvp_state_apply_block(o->calc->c, o->cemt, io, nh);
}

// Y[h] = (H vfull_h)[free] for the nh <= 16 rows of the device panel X (m entries each, rows ldx / ldy apart), vfull_h zero on
// the pinned coordinates: queued on the context's stream, nothing waited for, nothing copied.  nh calls; not entered in the
// pair record (that belongs to the secant update of PES.diag), and no vanishing-vector rule: a zero row gives a zero row.
// EMT: the block kernels of emt_hessian.hip on the resident state, reading X where it stands unless coordinates are pinned
// (a scatter into full-length rows).  Model: A V and U V on the matrix cores
// (launch_panel16, whose operand rows are as long as A's: X itself only if ldx is A's leading dimension and all are free).
int sella::hvp_device_apply_block(sella_hvp* o, const double* X, int ldx, int nh, double* Y, int ldy) {
    sella_calc* k = o->calc;
    sella_ctx* c = k->c;
    if (!X || !Y || nh < 1 || nh > HVP_BLOCK || ldx < o->m || ldy < o->m) {
        set_error("hvp operator: a block product takes 1 to %d rows of at least %d entries", HVP_BLOCK, o->m);
        return SELLA_E_INVALID;
    }
    SCHK(hvp_block_buffers(o));
    const int n = o->n;
    Mat* A = nullptr;
    if (k->kind == 0) {
        A = mat_get(c, k->A);
        if (!A || A->ld != o->ld) {
            set_error("hvp operator: the model calculator's matrix A is gone");
            return SELLA_E_INVALID;
        }
    }
    o->calls += nh;
    if (o->cell) return hvp_cell_block(o, X, ldx, nh, Y, ldy);
    const double* V = X;
    int ldv = ldx;
    if (o->inv || (k->kind == 0 && ldx != o->ld)) {
        ldv = o->ld;
        SELLA_LAUNCHB(c, hvp_scatter_block_kernel, hvp_scatter_block_vb, 256, dim3(o->nb), dim3(256), 0, n, nh, X, ldx,
                      (const int*)o->inv, o->bstage, ldv);
        V = o->bstage;
    }
    if (k->kind == 1) return emt_hvp_state_apply_block(c, o->emt, V, ldv, nh, o->inv, Y, ldy);
    if (k->kind == 2) return pair_hvp_state_apply_block(c, o->pair, V, ldv, nh, o->inv, Y, ldy);
    if (k->kind == 3) return tip3p_hvp_state_apply_block(c, o->tip, V, ldv, nh, o->inv, Y, ldy);
    SCHK(launch_panel16(c, A->d, n, n, A->ld, V, nh, o->bhv, o->ld));
    if (k->nu > 0) SCHK(launch_panel16(c, k->dconst, k->nu, n, o->ld, V, nh, o->bt, o->ldt));
    SELLA_LAUNCHB(c, hvp_model_finish_block_kernel, hvp_model_finish_block_vb, 256, dim3(o->nb, nh), dim3(256), 0, n, k->nu, o->ld,
                  (const double*)o->S, (const double*)o->bt, o->ldt, (const double*)o->bhv, o->ld, (const int*)o->inv, Y, ldy);
    HIPCHK(hipGetLastError());
    return SELLA_OK;
}

int sella::hvp_dim(const sella_hvp* o) { return o->m; }
long sella::hvp_calls(const sella_hvp* o) { return o->calls; }
sella_ctx* sella::hvp_ctx(const sella_hvp* o) { return o->calc->c; }

// host panels: V, HV (k, m), any k >= 1, through the device block path in chunks of 16 rows
extern "C" int sella_hvp_apply_block(sella_hvp* o, const double* V, int k, double* HV) {
    if (!o || !V || !HV || k <= 0) {
        set_error("hvp operator: invalid arguments");
        return SELLA_E_INVALID;
    }
    sella_ctx* c = o->calc->c;
    SCHK(hvp_block_buffers(o));
    const size_t m = (size_t)o->m, ldm = (size_t)o->ldm;
    for (int r0 = 0; r0 < k; r0 += HVP_BLOCK) {
        const int nh = std::min(HVP_BLOCK, k - r0);
        for (int h = 0; h < nh; ++h) SCHK(h2d_async(c, o->bx + h * ldm, V + (r0 + h) * m, m * sizeof(double)));
        if (nh < HVP_BLOCK) HIPCHK(s_memset0(c, o->bx + nh * ldm, (HVP_BLOCK - nh) * ldm * sizeof(double)));
        SCHK(hvp_device_apply_block(o, o->bx, o->ldm, nh, o->by, o->ldm));
        SCHK(d2h_async_2d(c, HV + r0 * m, o->by, ldm * sizeof(double), m * sizeof(double), (size_t)nh));
        SCHK(stream_wait(c));
    }
    return SELLA_OK;
}

// diag(H)[free] at the operator's geometry (m entries, host).  Not a force call and not a product.
extern "C" int sella_hvp_diag(sella_hvp* o, double* diag) {
    if (!o || !diag) {
        set_error("hvp operator: invalid arguments");
        return SELLA_E_INVALID;
    }
    sella_calc* k = o->calc;
    sella_ctx* c = k->c;
    if (o->cell) {
        // the positions from emt_hdiag; the cell entries from one block product of the mc unit rows (not counted): one upload
        // of the rows, one read-back of the mc x mc block behind the positions
        SCHK(emt_hvp_state_diag(c, o->cemt.s, o->inv, o->dy));
        SCHK(hvp_block_buffers(o));
        const size_t ldm = (size_t)o->ldm, mx = (size_t)o->mx, mc = (size_t)o->mc;
        std::vector<double> rows(mc * ldm, 0.0);
        for (size_t h = 0; h < mc; ++h) rows[h * ldm + mx + h] = 1.0;
        SCHK(h2d_async(c, o->bx, rows.data(), rows.size() * sizeof(double)));
        SCHK(hvp_cell_block(o, o->bx, o->ldm, o->mc, o->by, o->ldm));
        double pp[81];
        SCHK(d2h_async(c, diag, o->dy, mx * sizeof(double)));
        SCHK(d2h_async_2d(c, pp, o->by + mx, ldm * sizeof(double), mc * sizeof(double), mc));
        SCHK(stream_wait(c));
        for (size_t h = 0; h < mc; ++h) diag[mx + h] = pp[h * mc + h];
        return SELLA_OK;
    }
    if (k->kind == 1) {
        SCHK(emt_hvp_state_diag(c, o->emt, o->inv, o->dy));
    } else if (k->kind == 2) {
        SCHK(pair_hvp_state_diag(c, o->pair, o->inv, o->dy));
    } else if (k->kind == 3) {
        SCHK(tip3p_hvp_state_diag(c, o->tip, o->inv, o->dy));
    } else {
        Mat* A = mat_get(c, k->A);
        if (!A) {
            set_error("hvp operator: the model calculator's matrix A is gone");
            return SELLA_E_INVALID;
        }
        SELLA_LAUNCHB(c, hvp_model_diag_kernel, hvp_model_diag_vb, 256, dim3(o->nb), dim3(256), 0, o->n, k->nu, o->ld,
                      (const double*)A->d, A->ld, (const double*)o->S, (const double*)k->dconst, (const int*)o->inv, o->dy);
        HIPCHK(hipGetLastError());
    }
    SCHK(d2h_async(c, diag, o->dy, (size_t)o->m * sizeof(double)));
    return stream_wait(c);
}

// sella_matvec_fn: host vectors — upload, the device product, download, wait
extern "C" int sella_hvp_matvec(void* user, const double* v, double* Av, int m) {
    sella_hvp* o = static_cast<sella_hvp*>(user);
    if (!o || !v || !Av || m != o->m) {
        set_error("hvp operator: invalid arguments");
        return SELLA_E_INVALID;
    }
    sella_ctx* c = o->calc->c;
    SCHK(h2d_async(c, o->dx, v, (size_t)m * sizeof(double)));
    SCHK(hvp_device_apply(o, o->dx, o->dy));
    SCHK(d2h_async(c, Av, o->dy, (size_t)m * sizeof(double)));
    return stream_wait(c);
}

// which products are recorded: the flags of the products since the last look, one wait
static int hvp_sync_flags(sella_hvp* o) {
    sella_ctx* c = o->calc->c;
    const size_t have = o->flags.size(), want = (size_t)o->nrec;
    if (have == want) return SELLA_OK;
    o->flags.resize(want);
    for (size_t ci = have / HVP_CHUNK; ci * HVP_CHUNK < want; ++ci) {
        const size_t lo = std::max(have, ci * HVP_CHUNK), hi = std::min(want, (ci + 1) * HVP_CHUNK);
        const int* f = reinterpret_cast<const int*>(o->chunks[ci] + (size_t)2 * HVP_CHUNK * o->ld);
        SCHK(d2h_async(c, o->flags.data() + lo, f + (lo - ci * HVP_CHUNK), (hi - lo) * sizeof(int)));
    }
    return stream_wait(c);
}

extern "C" int sella_hvp_npairs(sella_hvp* o) {
    if (!o || hvp_sync_flags(o) != SELLA_OK) return 0;
    int k = 0;
    for (int f : o->flags) k += f != 0;
    return k;
}
extern "C" long sella_hvp_calls(sella_hvp* o) { return o ? o->calls : 0; }

// recorded pairs as (n x k) row-major matrices (columns = recorded products in call order), as sella_fd_pairs
extern "C" int sella_hvp_pairs(sella_hvp* o, double* Vs, double* AVs) {
    if (!o || !Vs || !AVs) return SELLA_E_INVALID;
    SCHK(hvp_sync_flags(o));
    sella_ctx* c = o->calc->c;
    const int n = o->n;
    const size_t ld = (size_t)o->ld;
    int k = 0;
    for (int f : o->flags) k += f != 0;
    if (k == 0) return SELLA_OK;
    std::vector<double> rows((size_t)2 * k * n);                       // recorded vectors, then their products, one per row
    int p = 0;
    for (size_t s = 0; s < o->flags.size(); ++s) {
        if (!o->flags[s]) continue;
        const double* base = o->chunks[s / HVP_CHUNK];
        const size_t r = s % HVP_CHUNK;
        SCHK(d2h_async(c, rows.data() + (size_t)p * n, base + r * ld, (size_t)n * sizeof(double)));
        SCHK(d2h_async(c, rows.data() + (size_t)(k + p) * n, base + (HVP_CHUNK + r) * ld, (size_t)n * sizeof(double)));
        ++p;
    }
    SCHK(stream_wait(c));
    for (int q = 0; q < k; ++q)
        for (int i = 0; i < n; ++i) {
            Vs[(size_t)i * k + q] = rows[(size_t)q * n + i];
            AVs[(size_t)i * k + q] = rows[(size_t)(k + q) * n + i];
        }
    return SELLA_OK;
}

extern "C" int sella_hvp_destroy(sella_hvp* o) {
    if (o) hvp_release(o);
    return SELLA_OK;
}
