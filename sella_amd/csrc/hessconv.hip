// hessconv.hip — the Cartesian Hessian of a calculator (`hessian_function`) carried into redundant internal coordinates
// and back: InternalPES._convert_cartesian_hessian_to_internal / _convert_internal_hessian_to_cartesian
// (sella/peswrapper.py:1247-1282).
//
// The reference takes a full SVD of B[:, :3N] (an nint x nint U) and forms the two halves of the internal Hessian
// separately: U_r Hnred U_r^T + lambda_bar U_red U_red^T.  Here the caller hands over the thin factors X = V_r S_r^-1 and
// Q = U_r (the PES's spectral factor of B), and the complement enters as lambda_bar (I - Q Q^T), i.e.
// out = Q (Hnred - lambda_bar I) Q^T + lambda_bar I: four GEMMs, one accumulating ldot, one r x r eigenvalue solve.
// Everything stays on the device except the r eigenvalues that lambda_bar is formed from.
#include <cmath>
#include <vector>

#include "internal.h"

namespace sella {
namespace {

// the device matrices of one call, returned to the pool on every way out (stream-ordered: safe behind queued work)
struct CallMats {
    sella_ctx* c;
    std::vector<sella_mat> h;
    explicit CallMats(sella_ctx* ctx) : c(ctx) {}
    ~CallMats() {
        for (sella_mat m : h) sella_mat_free(c, m);
    }
    int make(int rows, int cols, sella_mat* out) {
        SCHK(mat_new(c, rows, cols, out));
        h.push_back(*out);
        return SELLA_OK;
    }
};

bool shape_is(sella_ctx* c, sella_mat h, int rows, int cols) {
    Mat* m = mat_get(c, h);
    return m && m->rows == rows && m->cols == cols;
}

}  // namespace
}  // namespace sella

using namespace sella;

extern "C" int sella_hessian_cart_to_int(sella_ctx* c, sella_sparse_int* s, const double* g, sella_mat Hcart, sella_mat X,
                                         sella_mat Q, sella_mat out, double* lambda_bar) {
    Mat* mx = mat_get(c, X);
    if (!c || !s || !g || !lambda_bar || !mx) {
        set_error("hessian_cart_to_int: invalid arguments");
        return SELLA_E_INVALID;
    }
    const int nint = sparse_int_ncoords(s), n = 3 * sparse_int_natoms(s), r = mx->cols;
    if (!shape_is(c, Hcart, n, n) || !shape_is(c, X, n, r) || !shape_is(c, Q, nint, r) || !shape_is(c, out, nint, nint)) {
        set_error("hessian_cart_to_int: expected Hcart %d x %d, X %d x r, Q %d x r, out %d x %d", n, n, n, nint, nint, nint);
        return SELLA_E_INVALID;
    }
    if (r == 0) {
        set_error("hessian_cart_to_int: B has no singular value above the threshold (r = 0)");
        return SELLA_E_INVALID;
    }
    // Hcorr = Hcart - sum_i g_i d2q_i/dx2, in the caller's matrix (peswrapper.py:1266-1267)
    SCHK(sella_sparse_int_ldot_acc(s, g, -1.0, 1.0, Hcart));
    CallMats t(c);
    sella_mat T, Hn, Hs, Z;
    SCHK(t.make(n, r, &T));
    SCHK(t.make(r, r, &Hn));
    SCHK(sella_gemm(c, 0, 0, 1.0, Hcart, X, 0.0, T));            // Hcorr X
    SCHK(sella_gemm(c, 1, 0, 1.0, X, T, 0.0, Hn));               // Hnred = X^T Hcorr X   (:1268)
    // lambda_bar from the eigenvalues of the symmetric part (:1271-1275; np.linalg.eigh reads one triangle of a matrix it
    // takes to be symmetric — the two agree for a symmetric Hcart)
    SCHK(t.make(r, r, &Hs));
    Mat *mh = mat_get(c, Hn), *ms = mat_get(c, Hs);
    SCHK(launch_axpby2d(c, r, r, 1.0, mh->d, mh->ld, 0.0, nullptr, 0, ms->d, ms->ld));
    SCHK(launch_symmetrize(c, ms->d, r, ms->ld));
    std::vector<double> w(r);
    SCHK(sella_eigh(c, Hs, w.data(), nullptr, nullptr));
    double sum_log = 0.0;
    for (double x : w) sum_log += std::log(std::fabs(x));
    const double lam = std::exp(sum_log / r);
    // out = Q (Hnred - lambda_bar I) Q^T + lambda_bar I = Q Hnred Q^T + lambda_bar (I - Q Q^T)   (:1278)
    SCHK(sella_mat_add_diag(c, Hn, -lam));
    SCHK(t.make(nint, r, &Z));
    SCHK(sella_gemm(c, 0, 0, 1.0, Q, Hn, 0.0, Z));
    SCHK(sella_gemm(c, 0, 1, 1.0, Z, Q, 0.0, out));
    SCHK(sella_mat_add_diag(c, out, lam));
    *lambda_bar = lam;
    return stream_wait(c);
}

extern "C" int sella_hessian_int_to_cart(sella_ctx* c, sella_sparse_int* s, const double* g, sella_mat Hint, sella_mat out) {
    if (!c || !s || !g) {
        set_error("hessian_int_to_cart: invalid arguments");
        return SELLA_E_INVALID;
    }
    const int nint = sparse_int_ncoords(s), n = 3 * sparse_int_natoms(s);
    if (!shape_is(c, Hint, nint, nint) || !shape_is(c, out, n, n)) {
        set_error("hessian_int_to_cart: expected Hint %d x %d and out %d x %d", nint, nint, n, n);
        return SELLA_E_INVALID;
    }
    // out = B^T Hint B + sum_i g_i d2q_i/dx2 (:1277-1282)
    CallMats t(c);
    sella_mat B, T;
    SCHK(t.make(nint, n, &B));
    SCHK(sella_sparse_int_jac_dense(s, 0, nint, B));
    SCHK(t.make(nint, n, &T));
    SCHK(sella_gemm(c, 0, 0, 1.0, Hint, B, 0.0, T));
    SCHK(sella_gemm(c, 1, 0, 1.0, B, T, 0.0, out));
    SCHK(sella_sparse_int_ldot_acc(s, g, 1.0, 1.0, out));
    return stream_wait(c);
}
