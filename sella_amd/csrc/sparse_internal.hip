// sparse_internal.hip — the per-coordinate Jacobian and Hessian blocks of internal coordinates, resident on the device,
// and their contractions: SparseInternalJacobian / SparseInternalHessian(s) / SparseInternalHessiansSkeleton of
// sella/linalg.py:362-646.
//
// One object holds one topology (the skeleton, linalg.py:470-537): per coordinate its atom list (any length, an atom may
// repeat — a periodic image of itself), the grouping by list length in order of first appearance, and two inverted
// indices built once on the host and kept on the device:
//   * per atom pair (A, B): the (coordinate, a, b) with atoms[a] == A, atoms[b] == B, ordered by size group (order of
//     first appearance), coordinate, a, b — the order in which the reference's bincount (linalg.py:601-618) adds them;
//   * per atom B: the (coordinate, a) with atoms[a] == B in coordinate order — SparseInternalJacobian._rmatvec's add.at
//     order (linalg.py:394-401).
// Value buffers: gradient blocks (m, 3) and Hessian blocks (m, 3, m, 3) per coordinate, concatenated in coordinate
// order.  Every dense output is written by plain stores, one thread per destination element, each gathering what
// lands there (no atomics); every element of the row, padding included, is stored.
#include <algorithm>
#include <numeric>

#include "internal.h"

namespace sella {
struct SpContrib {
    long base;   // offset of H_c[a, 0, b, 0] in the Hessian buffer
    int c;       // coordinate
    int m3;      // 3 m: row stride of the block (and the size group: groups differ in m)
};
struct SpJEnt {
    long g;      // offset of grad_c[a, 0] in the gradient buffer
    long c;      // coordinate
};
}  // namespace sella

struct sella_sparse_int {
    sella_ctx* c = nullptr;
    int natoms = 0, nc = 0;
    std::vector<long> aoff, hoff;          // (nc + 1): first atom entry / first Hessian value of every coordinate
    std::vector<int> atoms;
    // device: topology
    long* d_aoff = nullptr;
    long* d_hoff = nullptr;
    int* d_atoms = nullptr;
    // device: values
    double* d_grad = nullptr;
    double* d_hess = nullptr;
    // device: inverted indices (built on first use)
    long* d_pptr = nullptr;                // (natoms + 1): atom pairs of row atom A
    int* d_pcol = nullptr;                 // column atom B of every pair, ascending within a row atom
    long* d_cptr = nullptr;                // (npairs + 1): contributions of every pair
    sella::SpContrib* d_ctb = nullptr;
    long* d_jptr = nullptr;                // (natoms + 1): gradient entries of atom B
    sella::SpJEnt* d_jent = nullptr;
    std::vector<std::pair<double*, size_t>> blocks;   // every device allocation of the object
};

namespace sella {
namespace {

using Contrib = SpContrib;
using JEnt = SpJEnt;

template <class T>
int obj_alloc(sella_sparse_int* s, size_t count, T** p) {
    const size_t bytes = (count > 0 ? count : 1) * sizeof(T);
    double* d = nullptr;
    SCHK(dev_alloc(s->c, bytes, &d));
    s->blocks.push_back({d, bytes});
    *p = reinterpret_cast<T*>(d);
    return SELLA_OK;
}

template <class T>
int obj_upload(sella_sparse_int* s, const std::vector<T>& host, T** p) {
    SCHK(obj_alloc(s, host.size(), p));
    return h2d_async(s->c, *p, host.data(), host.size() * sizeof(T));
}

// ---- kernels ---------------------------------------------------------------------------------------------------------
constexpr int LDOT_LCAP = 2048;    // pair lists of up to this many column atoms are searched in LDS

// ldot: out[3A+i, 3B+j] = sum over size groups g (first appearance) of (sum over the contributions of g to (A, B), in
// coordinate, a, b order, of H_c[a,i,b,j] * v_c) — every product rounded, each group's sum from 0.0 (linalg.py:613-618).
// ACC: the same sum, then out = beta * out + alpha * sum, once per element (out is not read when beta == 0); ACC = false
// is the plain store of the reference contraction.
template <bool ACC>
__device__ __forceinline__ void sparse_ldot_body(int ndof, int ld, const long* __restrict__ pptr,
                                                 const int* __restrict__ pcol, const long* __restrict__ cptr,
                                                 const Contrib* __restrict__ ctb, const double* __restrict__ v,
                                                 const double* __restrict__ hess, double* __restrict__ out, double alpha,
                                                 double beta) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ int scol[LDOT_LCAP];
    const int r = blockIdx.x;
    const int A = r / 3, i = r - 3 * A;
    const long p0 = pptr[A];
    const long np = pptr[A + 1] - p0;
    const int* cols = pcol + p0;
    if (np <= LDOT_LCAP) {
        for (int t = threadIdx.x; t < np; t += 256) scol[t] = cols[t];
        __syncthreads();
        cols = scol;
    }
    double* row = out + (size_t)r * ld;
    for (int s = threadIdx.x; s < ld; s += 256) {
        double tot = 0.0;
        if (s < ndof && np > 0) {
            const int B = s / 3, j = s - 3 * B;
            long lo = 0, hi = np;
            while (lo < hi) {
                const long mid = (lo + hi) >> 1;
                if (cols[mid] < B) lo = mid + 1;
                else hi = mid;
            }
            if (lo < np && cols[lo] == B) {
                const long k0 = cptr[p0 + lo], k1 = cptr[p0 + lo + 1];
                int m3 = ctb[k0].m3;
                double part = 0.0;
                for (long k = k0; k < k1; ++k) {
                    const Contrib e = ctb[k];
                    if (e.m3 != m3) {
                        tot += part;
                        part = 0.0;
                        m3 = e.m3;
                    }
                    part += hess[e.base + (long)i * e.m3 + j] * v[e.c];
                }
                tot += part;
            }
        }
        if constexpr (ACC) row[s] = beta == 0.0 ? alpha * tot : beta * row[s] + alpha * tot;
        else row[s] = tot;
    }
}
__global__ __launch_bounds__(256) void sparse_ldot_kernel(int ndof, int ld, const long* __restrict__ pptr,
                                                          const int* __restrict__ pcol, const long* __restrict__ cptr,
                                                          const Contrib* __restrict__ ctb, const double* __restrict__ v,
                                                          const double* __restrict__ hess, double* __restrict__ out) {
    sparse_ldot_body<false>(ndof, ld, pptr, pcol, cptr, ctb, v, hess, out, 1.0, 0.0);
}
__global__ __launch_bounds__(256) void sparse_ldot_acc_kernel(int ndof, int ld, const long* __restrict__ pptr,
                                                              const int* __restrict__ pcol, const long* __restrict__ cptr,
                                                              const Contrib* __restrict__ ctb, const double* __restrict__ v,
                                                              const double* __restrict__ hess, double* __restrict__ out,
                                                              double alpha, double beta) {
    sparse_ldot_body<true>(ndof, ld, pptr, pcol, cptr, ctb, v, hess, out, alpha, beta);
}

// rdot: out[c, 3B+j] = sum over a with atoms_c[a] == B of sum_{b, j'} H_c[a,j,b,j'] x[3 atoms_c[b] + j'] (linalg.py:620-640)
__global__ __launch_bounds__(256) void sparse_rdot_kernel(int ndof, int ld, const long* __restrict__ aoff,
                                                          const long* __restrict__ hoff, const int* __restrict__ atoms,
                                                          const double* __restrict__ x, const double* __restrict__ hess,
                                                          double* __restrict__ out) {
    const int c = blockIdx.x;
    const long a0 = aoff[c];
    const int m = (int)(aoff[c + 1] - a0);
    const int* at = atoms + a0;
    const double* H = hess + hoff[c];
    double* row = out + (size_t)c * ld;
    for (int s = threadIdx.x; s < ld; s += 256) {
        double val = 0.0;
        if (s < ndof) {
            const int B = s / 3, j = s - 3 * B;
            for (int a = 0; a < m; ++a) {
                if (at[a] != B) continue;
                const double* h = H + (long)(3 * a + j) * 3 * m;
                double sa = 0.0;
                for (int b = 0; b < m; ++b) {
                    const double* xb = x + 3 * (long)at[b];
                    sa += h[3 * b] * xb[0] + h[3 * b + 1] * xb[1] + h[3 * b + 2] * xb[2];
                }
                val += sa;
            }
        }
        row[s] = val;
    }
}

// ddot: w_c = u_c^T H_c x_c over the coordinate's degrees of freedom (linalg.py:642-646), one thread per coordinate
__global__ __launch_bounds__(256) void sparse_ddot_kernel(int nc, const long* __restrict__ aoff, const long* __restrict__ hoff,
                                                          const int* __restrict__ atoms, const double* __restrict__ u,
                                                          const double* __restrict__ x, const double* __restrict__ hess,
                                                          double* __restrict__ w) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const long a0 = aoff[c];
    const int m = (int)(aoff[c + 1] - a0), m3 = 3 * m;
    const int* at = atoms + a0;
    const double* H = hess + hoff[c];
    double acc = 0.0;
    for (int k = 0; k < m3; ++k) {
        const double* h = H + (long)k * m3;
        double t = 0.0;
        for (int l = 0; l < m3; ++l) t += h[l] * x[3 * (long)at[l / 3] + l % 3];
        acc += u[3 * (long)at[k / 3] + k % 3] * t;
    }
    w[c] = acc;
}

// the dense Hessian of coordinates first .. first+count as (count ndof) x ndof rows (SparseInternalHessian.asarray,
// linalg.py:420-442): out[(c - first) ndof + 3A+i, 3B+j] = sum over (a, b) with atoms_c[a] == A, atoms_c[b] == B
__global__ __launch_bounds__(256) void sparse_hess_dense_kernel(int ndof, int ld, int first, const long* __restrict__ aoff,
                                                                const long* __restrict__ hoff, const int* __restrict__ atoms,
                                                                const double* __restrict__ hess, double* __restrict__ out) {
    const long R = blockIdx.x;
    const int c = first + (int)(R / ndof);
    const int r = (int)(R % ndof);
    const int A = r / 3, i = r - 3 * A;
    const long a0 = aoff[c];
    const int m = (int)(aoff[c + 1] - a0), m3 = 3 * m;
    const int* at = atoms + a0;
    const double* H = hess + hoff[c];
    double* row = out + (size_t)R * ld;
    for (int s = threadIdx.x; s < ld; s += 256) {
        double val = 0.0;
        if (s < ndof) {
            const int B = s / 3, j = s - 3 * B;
            for (int a = 0; a < m; ++a) {
                if (at[a] != A) continue;
                for (int b = 0; b < m; ++b)
                    if (at[b] == B) val += H[(long)(3 * a + i) * m3 + 3 * b + j];
            }
        }
        row[s] = val;
    }
}

// the dense Jacobian rows of coordinates first .. first+count (SparseInternalJacobian.asarray, linalg.py:377-384)
__global__ __launch_bounds__(256) void sparse_jac_dense_kernel(int ndof, int ld, int first, const long* __restrict__ aoff,
                                                               const int* __restrict__ atoms, const double* __restrict__ grad,
                                                               double* __restrict__ out) {
    const int c = first + blockIdx.x;
    const long a0 = aoff[c];
    const int m = (int)(aoff[c + 1] - a0);
    const int* at = atoms + a0;
    const double* G = grad + 3 * a0;
    double* row = out + (size_t)blockIdx.x * ld;
    for (int s = threadIdx.x; s < ld; s += 256) {
        double val = 0.0;
        if (s < ndof) {
            const int B = s / 3, j = s - 3 * B;
            for (int a = 0; a < m; ++a)
                if (at[a] == B) val += G[3 * a + j];
        }
        row[s] = val;
    }
}

// J x (linalg.py:386-392), one thread per coordinate
__global__ __launch_bounds__(256) void sparse_jac_matvec_kernel(int nc, const long* __restrict__ aoff,
                                                                const int* __restrict__ atoms, const double* __restrict__ grad,
                                                                const double* __restrict__ x, double* __restrict__ w) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const long a0 = aoff[c];
    const int m = (int)(aoff[c + 1] - a0);
    const double* G = grad + 3 * a0;
    double acc = 0.0;
    for (int a = 0; a < m; ++a) {
        const double* xa = x + 3 * (long)atoms[a0 + a];
        acc += G[3 * a] * xa[0] + G[3 * a + 1] * xa[1] + G[3 * a + 2] * xa[2];
    }
    w[c] = acc;
}

// J^T y through the per-atom index: out[3B+j] = sum, in coordinate order, of y_c grad_c[a, j] (every product rounded,
// from 0.0: the add.at of linalg.py:394-401)
__global__ __launch_bounds__(256) void sparse_jac_rmatvec_kernel(int ndof, const long* __restrict__ jptr,
                                                                 const JEnt* __restrict__ jent, const double* __restrict__ y,
                                                                 const double* __restrict__ grad, double* __restrict__ out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ndof) return;
    const int B = s / 3, j = s - 3 * B;
    double tot = 0.0;
    for (long k = jptr[B]; k < jptr[B + 1]; ++k) {
        const JEnt e = jent[k];
        tot += y[e.c] * grad[e.g + j];
    }
    out[s] = tot;
}

// ---- host side -------------------------------------------------------------------------------------------------------
int ensure_hess(sella_sparse_int* s) {
    if (!s->d_hess) SCHK(obj_alloc(s, (size_t)s->hoff[s->nc], &s->d_hess));
    return SELLA_OK;
}

// atom-pair index of ldot: contributions emitted in (size group, coordinate, a, b) order, stably bucketed by (A, B)
int ensure_ldot_index(sella_sparse_int* s) {
    if (s->d_pptr) return SELLA_OK;
    const int nc = s->nc, natoms = s->natoms;
    std::vector<int> group_sizes;
    for (int c = 0; c < nc; ++c) {
        const int m = (int)(s->aoff[c + 1] - s->aoff[c]);
        if (std::find(group_sizes.begin(), group_sizes.end(), m) == group_sizes.end()) group_sizes.push_back(m);
    }
    std::vector<long> key;
    std::vector<Contrib> ent;
    for (int m : group_sizes)
        for (int c = 0; c < nc; ++c) {
            if (s->aoff[c + 1] - s->aoff[c] != m) continue;
            const int* at = s->atoms.data() + s->aoff[c];
            for (int a = 0; a < m; ++a)
                for (int b = 0; b < m; ++b) {
                    key.push_back((long)at[a] * natoms + at[b]);
                    ent.push_back(Contrib{s->hoff[c] + (long)a * 9 * m + 3 * b, c, 3 * m});
                }
        }
    std::vector<long> perm(key.size());
    std::iota(perm.begin(), perm.end(), 0L);
    std::stable_sort(perm.begin(), perm.end(), [&](long p, long q) { return key[p] < key[q]; });
    std::vector<long> pptr(natoms + 1, 0), cptr(1, 0);
    std::vector<int> pcol;
    std::vector<Contrib> ctb(ent.size());
    for (size_t k = 0; k < perm.size(); ++k) {
        const long kk = key[perm[k]];
        if (k == 0 || kk != key[perm[k - 1]]) {
            if (k) cptr.push_back((long)k);
            pcol.push_back((int)(kk % natoms));
            ++pptr[kk / natoms + 1];
        }
        ctb[k] = ent[perm[k]];
    }
    cptr.push_back((long)perm.size());
    for (int A = 0; A < natoms; ++A) pptr[A + 1] += pptr[A];
    SCHK(obj_upload(s, pptr, &s->d_pptr));
    SCHK(obj_upload(s, pcol, &s->d_pcol));
    SCHK(obj_upload(s, cptr, &s->d_cptr));
    SCHK(obj_upload(s, ctb, &s->d_ctb));
    return stream_wait(s->c);               // the host vectors go out of scope
}

// atom index of J^T y: (coordinate, a) in coordinate order, counting-sorted by atom
int ensure_jac_index(sella_sparse_int* s) {
    if (s->d_jptr) return SELLA_OK;
    std::vector<long> jptr(s->natoms + 1, 0);
    for (int at : s->atoms) ++jptr[at + 1];
    for (int A = 0; A < s->natoms; ++A) jptr[A + 1] += jptr[A];
    std::vector<long> fill(jptr.begin(), jptr.end() - 1);
    std::vector<JEnt> jent(s->atoms.size());
    for (int c = 0; c < s->nc; ++c)
        for (long k = s->aoff[c]; k < s->aoff[c + 1]; ++k) jent[fill[s->atoms[k]]++] = JEnt{3 * k, c};
    SCHK(obj_upload(s, jptr, &s->d_jptr));
    SCHK(obj_upload(s, jent, &s->d_jent));
    return stream_wait(s->c);
}

// a host vector of n doubles on the device (scratch slot, stream-ordered reuse)
int stage_vec(sella_ctx* c, int slot, const double* v, size_t n, double** d) {
    SCHK(scratch_get(c, slot, (n > 0 ? n : 1) * sizeof(double), d));
    return h2d_async(c, *d, v, n * sizeof(double));
}

Mat* out_mat(sella_sparse_int* s, sella_mat h, long rows, const char* what) {
    Mat* m = mat_get(s->c, h);
    if (!m || m->rows != rows || m->cols != 3 * s->natoms) {
        set_error("%s: output must be a %ld x %d matrix", what, rows, 3 * s->natoms);
        return nullptr;
    }
    return m;
}

}  // namespace
}  // namespace sella

using namespace sella;

extern "C" int sella_sparse_int_create(sella_ctx* c, int natoms, int ncoords, const int* sizes, const int* atoms,
                                       sella_sparse_int** out) {
    if (!c || !out || natoms < 1 || ncoords < 0 || (ncoords > 0 && !sizes) || 3L * natoms > (1L << 30)) {
        set_error("sparse_int_create: invalid arguments");
        return SELLA_E_INVALID;
    }
    sella_sparse_int* s = new sella_sparse_int();
    s->c = c;
    s->natoms = natoms;
    s->nc = ncoords;
    s->aoff.assign(ncoords + 1, 0);
    s->hoff.assign(ncoords + 1, 0);
    for (int k = 0; k < ncoords; ++k) {
        if (sizes[k] < 0 || sizes[k] > natoms) {
            set_error("sparse_int_create: coordinate %d has %d atoms (natoms %d)", k, sizes[k], natoms);
            delete s;
            return SELLA_E_INVALID;
        }
        s->aoff[k + 1] = s->aoff[k] + sizes[k];
        s->hoff[k + 1] = s->hoff[k] + 9L * sizes[k] * sizes[k];
    }
    const long nat = s->aoff[ncoords];
    if (nat > 0 && !atoms) {
        set_error("sparse_int_create: atom lists missing");
        delete s;
        return SELLA_E_INVALID;
    }
    s->atoms.assign(atoms, atoms + nat);
    for (long k = 0; k < nat; ++k)
        if (s->atoms[k] < 0 || s->atoms[k] >= natoms) {
            set_error("sparse_int_create: atom index %d out of range (natoms %d)", s->atoms[k], natoms);
            delete s;
            return SELLA_E_INVALID;
        }
    int st = obj_upload(s, s->aoff, &s->d_aoff);
    if (st == SELLA_OK) st = obj_upload(s, s->hoff, &s->d_hoff);
    if (st == SELLA_OK) st = obj_upload(s, s->atoms, &s->d_atoms);
    if (st == SELLA_OK) st = obj_alloc(s, (size_t)(3 * nat), &s->d_grad);
    if (st == SELLA_OK) st = stream_wait(c);
    if (st != SELLA_OK) {
        sella_sparse_int_destroy(s);
        return st;
    }
    *out = s;
    return SELLA_OK;
}

extern "C" int sella_sparse_int_destroy(sella_sparse_int* s) {
    if (!s) return SELLA_OK;
    for (auto& b : s->blocks) dev_free(s->c, b.first, b.second);
    delete s;
    return SELLA_OK;
}

extern "C" int sella_sparse_int_set_values(sella_sparse_int* s, const double* grad, const double* hess) {
    if (!s) return SELLA_E_INVALID;
    if (grad) SCHK(h2d_async(s->c, s->d_grad, grad, (size_t)(3 * s->aoff[s->nc]) * sizeof(double)));
    if (hess) {
        SCHK(ensure_hess(s));
        SCHK(h2d_async(s->c, s->d_hess, hess, (size_t)s->hoff[s->nc] * sizeof(double)));
    }
    return stream_wait(s->c);
}

extern "C" int sella_sparse_int_get_values(sella_sparse_int* s, double* grad, double* hess) {
    if (!s || (hess && !s->d_hess)) {
        set_error("sparse_int_get_values: invalid arguments (no Hessian values set)");
        return SELLA_E_INVALID;
    }
    if (grad && s->aoff[s->nc]) SCHK(d2h_async(s->c, grad, s->d_grad, (size_t)(3 * s->aoff[s->nc]) * sizeof(double)));
    if (hess && s->hoff[s->nc]) SCHK(d2h_async(s->c, hess, s->d_hess, (size_t)s->hoff[s->nc] * sizeof(double)));
    return stream_wait(s->c);
}

extern "C" int sella_sparse_int_eval(sella_sparse_int* s, int first, int count, int natoms_per_coord, const double* pos,
                                     const double* tvec, int hessian) {
    if (!s || first < 0 || count < 0 || first + (long)count > s->nc || natoms_per_coord < 2 || natoms_per_coord > 4
        || (count > 0 && !pos)) {
        set_error("sparse_int_eval: invalid arguments");
        return SELLA_E_INVALID;
    }
    for (int k = first; k < first + count; ++k)
        if (s->aoff[k + 1] - s->aoff[k] != natoms_per_coord) {
            set_error("sparse_int_eval: coordinate %d does not have %d atoms", k, natoms_per_coord);
            return SELLA_E_INVALID;
        }
    if (count == 0) return SELLA_OK;
    sella_ctx* c = s->c;
    if (hessian) SCHK(ensure_hess(s));
    const size_t nv = 3 * (size_t)natoms_per_coord, ntv = nv - 3;
    double* buf;
    SCHK(scratch_get(c, SCR_MISC0, (size_t)count * (nv + ntv + 1) * sizeof(double) + 64, &buf));
    double* dpos = buf;
    double* dtv = dpos + (size_t)count * nv;
    double* dq = dtv + (size_t)count * ntv;
    SCHK(h2d_async(c, dpos, pos, (size_t)count * nv * sizeof(double)));
    if (tvec) SCHK(h2d_async(c, dtv, tvec, (size_t)count * ntv * sizeof(double)));
    SCHK(internals_queue(c, natoms_per_coord, count, dpos, tvec ? dtv : nullptr, dq, s->d_grad + 3 * s->aoff[first],
                         hessian ? s->d_hess + s->hoff[first] : nullptr));
    return stream_wait(c);
}

namespace sella {
namespace {
// ldot into `out` (3 natoms x 3 natoms): the reference store (acc == false) or out = beta out + alpha sum (acc == true)
int ldot_launch(sella_sparse_int* s, const double* v, sella_mat out, bool acc, double alpha, double beta) {
    if (!s || (s->nc > 0 && !v)) return SELLA_E_INVALID;
    Mat* m = out_mat(s, out, 3L * s->natoms, acc ? "sparse_int_ldot_acc" : "sparse_int_ldot");
    if (!m) return SELLA_E_INVALID;
    sella_ctx* c = s->c;
    SCHK(ensure_hess(s));
    SCHK(ensure_ldot_index(s));
    m = mat_get(c, out);
    double* dv;
    SCHK(stage_vec(c, SCR_MISC1, v, (size_t)s->nc, &dv));
    const int ndof = 3 * s->natoms;
    // algorithmic bytes: the dense matrix written (and read when accumulating), every Hessian value read once
    prof_begin(c, PROF_OTHER, 8.0 * ((acc && beta != 0.0 ? 2.0 : 1.0) * ndof * m->ld + s->hoff[s->nc] + s->nc),
               2.0 * s->hoff[s->nc]);
    if (acc)
        SELLA_LAUNCH(c, sparse_ldot_acc_kernel, dim3((unsigned)ndof), dim3(256), 0, ndof, m->ld, s->d_pptr, s->d_pcol,
                     s->d_cptr, s->d_ctb, dv, s->d_hess, m->d, alpha, beta);
    else
        SELLA_LAUNCH(c, sparse_ldot_kernel, dim3((unsigned)ndof), dim3(256), 0, ndof, m->ld, s->d_pptr, s->d_pcol,
                     s->d_cptr, s->d_ctb, dv, s->d_hess, m->d);
    prof_end(c);
    HIPCHK(hipGetLastError());
    return stream_wait(c);
}
}  // namespace

int sparse_int_ncoords(const sella_sparse_int* s) { return s ? s->nc : -1; }
int sparse_int_natoms(const sella_sparse_int* s) { return s ? s->natoms : -1; }
}  // namespace sella

extern "C" int sella_sparse_int_ldot(sella_sparse_int* s, const double* v, sella_mat out) {
    return ldot_launch(s, v, out, false, 1.0, 0.0);
}

extern "C" int sella_sparse_int_ldot_acc(sella_sparse_int* s, const double* v, double alpha, double beta, sella_mat out) {
    return ldot_launch(s, v, out, true, alpha, beta);
}

extern "C" int sella_sparse_int_rdot(sella_sparse_int* s, const double* x, sella_mat out) {
    if (!s || !x) return SELLA_E_INVALID;
    Mat* m = out_mat(s, out, s->nc, "sparse_int_rdot");
    if (!m) return SELLA_E_INVALID;
    sella_ctx* c = s->c;
    SCHK(ensure_hess(s));
    m = mat_get(c, out);
    if (s->nc == 0) return SELLA_OK;
    const int ndof = 3 * s->natoms;
    double* dx;
    SCHK(stage_vec(c, SCR_MISC1, x, (size_t)ndof, &dx));
    prof_begin(c, PROF_OTHER, 8.0 * ((double)s->nc * m->ld + s->hoff[s->nc]), 2.0 * s->hoff[s->nc]);
    SELLA_LAUNCH(c, sparse_rdot_kernel, dim3((unsigned)s->nc), dim3(256), 0, ndof, m->ld, s->d_aoff, s->d_hoff, s->d_atoms,
                 dx, s->d_hess, m->d);
    prof_end(c);
    HIPCHK(hipGetLastError());
    return stream_wait(c);
}

extern "C" int sella_sparse_int_ddot(sella_sparse_int* s, const double* u, const double* x, double* out) {
    if (!s || !u || !x || (s->nc > 0 && !out)) return SELLA_E_INVALID;
    sella_ctx* c = s->c;
    SCHK(ensure_hess(s));
    if (s->nc == 0) return SELLA_OK;
    const int ndof = 3 * s->natoms;
    double *du, *dx, *dw;
    SCHK(scratch_get(c, SCR_MISC1, (2 * (size_t)ndof + s->nc) * sizeof(double), &du));
    dx = du + ndof;
    dw = dx + ndof;
    SCHK(h2d_async(c, du, u, (size_t)ndof * sizeof(double)));
    SCHK(h2d_async(c, dx, x, (size_t)ndof * sizeof(double)));
    hipLaunchKernelGGL(sparse_ddot_kernel, dim3((unsigned)((s->nc + 255) / 256)), dim3(256), 0, c->stream, s->nc, s->d_aoff,
                       s->d_hoff, s->d_atoms, du, dx, s->d_hess, dw);
    HIPCHK(hipGetLastError());
    SCHK(d2h_async(c, out, dw, (size_t)s->nc * sizeof(double)));
    return stream_wait(c);
}

extern "C" int sella_sparse_int_hess_dense(sella_sparse_int* s, int first, int count, sella_mat out) {
    if (!s || first < 0 || count < 0 || first + (long)count > s->nc) return SELLA_E_INVALID;
    const int ndof = 3 * s->natoms;
    Mat* m = out_mat(s, out, (long)count * ndof, "sparse_int_hess_dense");
    if (!m) return SELLA_E_INVALID;
    sella_ctx* c = s->c;
    SCHK(ensure_hess(s));
    m = mat_get(c, out);
    if (count == 0) return SELLA_OK;
    hipLaunchKernelGGL(sparse_hess_dense_kernel, dim3((unsigned)((long)count * ndof)), dim3(256), 0, c->stream, ndof, m->ld,
                       first, s->d_aoff, s->d_hoff, s->d_atoms, s->d_hess, m->d);
    HIPCHK(hipGetLastError());
    return stream_wait(c);
}

extern "C" int sella_sparse_int_jac_dense(sella_sparse_int* s, int first, int count, sella_mat out) {
    if (!s || first < 0 || count < 0 || first + (long)count > s->nc) return SELLA_E_INVALID;
    Mat* m = out_mat(s, out, count, "sparse_int_jac_dense");
    if (!m) return SELLA_E_INVALID;
    if (count == 0) return SELLA_OK;
    sella_ctx* c = s->c;
    hipLaunchKernelGGL(sparse_jac_dense_kernel, dim3((unsigned)count), dim3(256), 0, c->stream, 3 * s->natoms, m->ld, first,
                       s->d_aoff, s->d_atoms, s->d_grad, m->d);
    HIPCHK(hipGetLastError());
    return stream_wait(c);
}

extern "C" int sella_sparse_int_jac_matvec(sella_sparse_int* s, const double* x, double* out) {
    if (!s || !x || (s->nc > 0 && !out)) return SELLA_E_INVALID;
    if (s->nc == 0) return SELLA_OK;
    sella_ctx* c = s->c;
    const int ndof = 3 * s->natoms;
    double *dx, *dw;
    SCHK(scratch_get(c, SCR_MISC1, ((size_t)ndof + s->nc) * sizeof(double), &dx));
    dw = dx + ndof;
    SCHK(h2d_async(c, dx, x, (size_t)ndof * sizeof(double)));
    hipLaunchKernelGGL(sparse_jac_matvec_kernel, dim3((unsigned)((s->nc + 255) / 256)), dim3(256), 0, c->stream, s->nc,
                       s->d_aoff, s->d_atoms, s->d_grad, dx, dw);
    HIPCHK(hipGetLastError());
    SCHK(d2h_async(c, out, dw, (size_t)s->nc * sizeof(double)));
    return stream_wait(c);
}

extern "C" int sella_sparse_int_jac_rmatvec(sella_sparse_int* s, const double* y, double* out) {
    if (!s || !out || (s->nc > 0 && !y)) return SELLA_E_INVALID;
    sella_ctx* c = s->c;
    SCHK(ensure_jac_index(s));
    const int ndof = 3 * s->natoms;
    double *dy, *dw;
    SCHK(scratch_get(c, SCR_MISC1, ((size_t)s->nc + ndof) * sizeof(double), &dy));
    dw = dy + s->nc;
    SCHK(h2d_async(c, dy, y, (size_t)s->nc * sizeof(double)));
    hipLaunchKernelGGL(sparse_jac_rmatvec_kernel, dim3((unsigned)((ndof + 255) / 256)), dim3(256), 0, c->stream, ndof,
                       s->d_jptr, s->d_jent, dy, s->d_grad, dw);
    HIPCHK(hipGetLastError());
    SCHK(d2h_async(c, out, dw, (size_t)ndof * sizeof(double)));
    return stream_wait(c);
}
