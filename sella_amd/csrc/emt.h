// emt.h — what the effective-medium-theory kernels share (emt.hip: energy, forces, virial; emt_hessian.hip: second
// derivatives): the argument block, the in-block reduction, and the format of the per-thread neighbour lists the density
// pass hands on.  The sweep over the (neighbour, image) pairs of an atom (emt_pairs) stands here too: the pair-potential
// kernels (pair.hip) walk the same pairs in the same order.
#pragma once
#include "internal.h"

namespace sella {

struct EmtPar {             // per-atom parameters, already converted to eV / Angstrom
    const double *E0, *s0, *V0, *eta2, *kappa, *lam, *n0, *gamma1, *gamma2;
};

struct EmtArgs {
    int n, nshift;
    int hcap;               // slots of a thread's neighbour list in use (<= EMT_HCAP; option emt_hcap, tests lower it)
    const double* pos;      // n x 3
    const double* shifts;   // nshift x 3 lattice translations (including 0)
    EmtPar p;
    double rc, acut, cutoff, beta;
    double* sigma1; double* epair; double* dEdsig; double* eatom; double* grad;
    int* nbr;               // n x 256 x (1 + EMT_HCAP): neighbour lists of the density kernel's threads, for the force kernel
};

namespace {

__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// block_sum's arithmetic for NS sums behind ONE barrier: every thread puts its share of each sum, the wavefronts' sums lie
// side by side in LDS (part[4][NS]), and after a __syncthreads() any thread reads sum `slot` with block_total
template <int NS>
__device__ __forceinline__ void block_put(double (*part)[NS], int slot, double v) {
    v = wave_sum64(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][slot] = v;
}
template <int NS>
__device__ __forceinline__ double block_total(const double (*part)[NS], int slot) {
    return (part[0][slot] + part[1][slot]) + (part[2][slot] + part[3][slot]);
}

constexpr int EMT_HCAP = 8;               // slots of a thread's neighbour list

// a noted pair: atom index in the low 24 bits, image above (no division when it is taken up again)
__device__ __forceinline__ int emt_pack(int j, int s) { return (s << 24) | j; }

// The sweep over all (neighbour, image) pairs is split in two per thread: first the distance test alone over the thread's
// pairs (t = tid, tid + 256, ...: no division, squared distance against a slightly widened cutoff), the few pairs inside
// the cutoff noted in LDS; then the exponentials for those only.  Under 1 % of the pairs are neighbours, but with the
// expensive branch inside the sweep every second wavefront iteration took it for some lane; deferred, a wavefront
// pays for the largest number of neighbours any of its lanes found (2-3).  The terms are added per thread in the same
// order as before — sums are bit-identical to the one-loop form.
constexpr int EMT_LDS_ATOMS = 1024;       // up to this many atoms the positions are staged in LDS (structure of arrays)

struct EmtStage {
    double x[EMT_LDS_ATOMS], y[EMT_LDS_ATOMS], z[EMT_LDS_ATOMS];
};

// All pairs of this thread (t = s n + j = tid mod 256, in increasing t) through `heavy`, in two steps: the distance test alone
// — image by image (s uniform: its shift sits in scalar registers), neighbours noted in hits[tid][..] — then the noted pairs.
// A thread whose list fills up (never at EMT's cutoff and 256 threads) works it off and takes its remaining pairs
// directly, in the same order; the count returned is then negative: the stored list is incomplete.
template <bool STAGED, class Heavy>
__device__ __forceinline__ int emt_pairs_impl(const EmtArgs& a, double xi, double yi, double zi, const EmtStage* st,
                                              int (*hits)[EMT_HCAP + 1], Heavy heavy) {
    const int tid = threadIdx.x, n = a.n;
    const double cut2 = a.cutoff * a.cutoff * (1.0 + 1e-12);
    const bool aligned = (n & 255) == 0;
    auto first_j = [&](int s) { return aligned ? tid : (((tid - s * n) % 256) + 256) % 256; };
    // (pos + shift) - x_i as in the terms themselves: the same rounding decides which pairs are neighbours
    auto near = [&](int j, double shx, double shy, double shz) {
        const double px = STAGED ? st->x[j] : a.pos[3 * j], py = STAGED ? st->y[j] : a.pos[3 * j + 1];
        const double pz = STAGED ? st->z[j] : a.pos[3 * j + 2];
        const double dx = px + shx - xi, dy = py + shy - yi, dz = pz + shz - zi;
        return dx * dx + dy * dy + dz * dz <= cut2;
    };
    int nh = 0, rs = -1, rj = 0;
    for (int s = 0; s < a.nshift; ++s) {
        const double shx = a.shifts[3 * s], shy = a.shifts[3 * s + 1], shz = a.shifts[3 * s + 2];
        if (rs >= 0) continue;                                     // (this thread's list is full: see below)
        for (int j = first_j(s); j < n; j += 1024) {
            bool in[4];                                            // four tests at a time: their loads are in flight together
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ju = j + 256 * u;
                in[u] = near(ju < n ? ju : j, shx, shy, shz) && ju < n;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (in[u] && rs < 0) {
                    if (nh == a.hcap) { rs = s; rj = j + 256 * u; }
                    else hits[tid][nh++] = emt_pack(j + 256 * u, s);
                }
            }
            if (rs >= 0) break;
        }
    }
    for (int h = 0; h < nh; ++h) heavy(hits[tid][h]);
    if (rs < 0) return nh;
    for (int s = rs; s < a.nshift; ++s) {
        const double shx = a.shifts[3 * s], shy = a.shifts[3 * s + 1], shz = a.shifts[3 * s + 2];
        for (int j = (s == rs) ? rj : first_j(s); j < n; j += 256)
            if (near(j, shx, shy, shz)) heavy(emt_pack(j, s));
    }
    return -1;
}

template <class Heavy>
__device__ __forceinline__ int emt_pairs(const EmtArgs& a, double xi, double yi, double zi, EmtStage* st, int (*hits)[EMT_HCAP + 1],
                                         Heavy heavy) {
    if (a.n <= EMT_LDS_ATOMS) {
        for (int j = threadIdx.x; j < a.n; j += 256) { st->x[j] = a.pos[3 * j]; st->y[j] = a.pos[3 * j + 1]; st->z[j] = a.pos[3 * j + 2]; }
        __syncthreads();
        return emt_pairs_impl<true>(a, xi, yi, zi, st, hits, heavy);
    }
    return emt_pairs_impl<false>(a, xi, yi, zi, st, hits, heavy);
}

}  // namespace

// emt.hip: positions uploaded (parameter table and shifts too unless `dconst` holds them, see emt_eval_resident), the
// argument block filled in and the density pass queued: sigma1, dEdsig and the neighbour lists of this geometry are then
// on the device, in scratch slot SCR_MISC0, with `extra_words` more doubles behind them at *extra for the caller's own
// intermediates.  Nothing is waited for.
int emt_density_queue(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                      const double* dconst, double rc, double acut, double cutoff, double beta, size_t extra_words,
                      EmtArgs* args, double** extra);

// emt_hessian.hip: what the Hessian-vector operator (calc.hip, sella_hvp) keeps of a geometry — the argument block of the
// density pass with its arrays, F2 and room for the dots of a product (n of one vector in front, 16 n of a block of
// vectors), in ONE allocation of the state's own.
struct EmtHvpState {
    EmtArgs a;
    double* F2 = nullptr;
    double* cdot = nullptr;
    double* own = nullptr;
    size_t own_bytes = 0;
};
int emt_hvp_state_create(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                         const double* dconst, double rc, double acut, double cutoff, double beta, EmtHvpState* st);
void emt_hvp_state_destroy(sella_ctx* c, EmtHvpState* st);
int emt_hvp_state_apply(sella_ctx* c, const EmtHvpState& st, const double* v, double* hv, const double* part, int nb,
                        const int* inv, double* y, int* flag);
// the same for the nh <= 16 rows of a device panel (row h at V + h ldv, full length), the free rows written into Y (row h at
// Y + h ldy), and diag(H)[free] into y
int emt_hvp_state_apply_block(sella_ctx* c, const EmtHvpState& st, const double* V, int ldv, int nh, const int* inv, double* Y,
                              int ldy);
int emt_hvp_state_diag(sella_ctx* c, const EmtHvpState& st, const int* inv, double* y);

// The same state for the operator of positions and cell (calc.hip, sella_hvp_create_cell): the product in the coordinates
// [x; p], p the mc cell parameters, W = J v_p the variation of the cell.  Behind what EmtHvpState keeps, in the same
// allocation: the image indices n_s, J (9 x mc), G (mc x mc), P (9 x 9, zero without a pressure), and per vector of a
// block of 16 (a single product uses slot 0) the table T[s] = n_s W, [W; v_p] and the per-atom shares of the nine cell rows.
struct EmtCellHvpState {
    EmtHvpState s;
    int mc = 0;
    double *nimg = nullptr, *J = nullptr, *G = nullptr, *P = nullptr;
    double *T = nullptr, *wv = nullptr, *share = nullptr;    // (16, nshift, 3); (16, 18): W then v_p; (16, n, 9)
};
// what a product reads and writes besides the state: the eigensolver's vectors X (row h at X + h ldx: mx free position
// entries, then mc cell entries; inv as above, over the 3n position coordinates) and products Y, and the full-length rows
// (3n position entries, then mc) the vectors are spread into (vfull) and, for a single product, the product is recorded in
// (hvfull; null for a block).  part: 3n / 256 (rounded up) + 1 partial sums of |v|^2 and flag, for a single product only.
struct EmtCellHvpIO {
    const double* X; int ldx;
    double* Y; int ldy;
    const int* inv; int mx;
    double* vfull; int ldv;
    double* hvfull;
    double* part; int* flag;
};
int emt_chvp_state_create(sella_ctx* c, int n, const double* pos, const double* cell, const double* par, int nshift,
                          const double* shifts, const double* dconst, double rc, double acut, double cutoff, double beta, int mc,
                          const double* J, const double* G, const double* P, EmtCellHvpState* st);
int emt_chvp_state_apply(sella_ctx* c, const EmtCellHvpState& st, const EmtCellHvpIO& io);
int emt_chvp_state_apply_block(sella_ctx* c, const EmtCellHvpState& st, const EmtCellHvpIO& io, int nh);

}  // namespace sella
