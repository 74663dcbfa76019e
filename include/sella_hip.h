/*
 * sella_hip.h — C ABI of libsella_hip.so, the MI355X (gfx950) implementation of the
 * inner saddle-point linear-algebra loop of Sella.
 *
 * This is the drop-in boundary.  The reference has no FFI; the seam it
 * offers for exactly this path is sella/_gpu.py (numpy-in / numpy-out helpers backed by
 * torch.cuda) plus the function-level seams one level up.  Each entry point below names
 * the reference interface it replaces (path:line under /root/reference).  INTEGRATION.md
 * shows the ctypes stub a Sella maintainer would add.
 *
 * Conventions
 *   - all matrices are fp64, C-contiguous row-major; host pointers are borrowed for the
 *     duration of the call only and are never written unless documented as outputs;
 *   - device memory is owned by the context and addressed through integer handles;
 *   - every function returns 0 on success or a negative SELLA_E_* code, the message is
 *     available from sella_last_error(); no exceptions cross the boundary;
 *   - one host thread per context, one HIP stream per context; calls are synchronous at
 *     the boundary (outputs are valid on return);
 *   - there is NO CPU fallback: without a usable HIP device sella_ctx_create fails.
 */
#ifndef SELLA_HIP_H
#define SELLA_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sella_ctx sella_ctx;
typedef int sella_mat;            /* handle of a device-resident row-major matrix */
#define SELLA_NO_MAT (-1)

enum {
    SELLA_OK = 0,
    SELLA_E_INVALID = -1,         /* bad argument / shape mismatch                       */
    SELLA_E_HIP = -2,             /* HIP runtime error (message has the HIP string)      */
    SELLA_E_NOMEM = -3,           /* device allocation failed (cf. _gpu.py:44-52 OOM)    */
    SELLA_E_NOCONV = -4,          /* iteration limit hit (MGS sweeps, secular solver..)  */
    SELLA_E_CALLBACK = -5,        /* host matvec callback reported failure               */
    SELLA_E_NODEVICE = -6,        /* no HIP device visible                               */
    SELLA_E_UNSUPPORTED = -7
};

const char* sella_last_error(void);
const char* sella_version(void);

/* ---- device / context ------------------------------------------------------------ */
/* replaces the implicit torch.cuda device + availability probe, sella/_gpu.py:17-41    */
int sella_device_count(int* count);
int sella_ctx_create(int device, sella_ctx** ctx);
int sella_ctx_destroy(sella_ctx* ctx);
int sella_ctx_sync(sella_ctx* ctx);
int sella_ctx_device_name(sella_ctx* ctx, char* buf, int buflen);
/* Integer tuning options of a context (kernel variant selection for benchmarking and tests).  The list — name, default,
 * accepted values, the measurements behind each default — is sella_amd/csrc/options.h and only that file.  set_option
 * applies the option's rule to the value (booleans normalised to 0 / 1, sizes clamped or rejected) and stores it,
 * get_option reads it back, sella_option_name enumerates the names (index 0, 1, ...; NULL past the end; no context
 * needed).  An unknown key or a rejected value returns SELLA_E_INVALID with the reason in sella_last_error() and changes
 * nothing.  Nothing but set_option changes an option, so a value read with get_option and set again later restores it.
 * What callers rely on: eigh_gemv_flat and eigh_dc_pipeline choose between forms that give the same results bit for
 * bit; rs_fast finds the same root as the reference's Newton / bisection schedule; emt_hcap is meaningful from 1 to 8. */
int sella_ctx_set_option(sella_ctx* ctx, const char* key, long value);
int sella_ctx_get_option(sella_ctx* ctx, const char* key, long* value);
const char* sella_option_name(int index);

/* ---- device matrices --------------------------------------------------------------- */
/* to_gpu(A): sella/_gpu.py:55-67 (upload, cached by ApproximateHessian linalg.py:197-207) */
int sella_mat_upload(sella_ctx* ctx, const double* A, int rows, int cols, sella_mat* h);
int sella_mat_alloc(sella_ctx* ctx, int rows, int cols, sella_mat* h);
int sella_mat_set(sella_ctx* ctx, sella_mat h, const double* A);        /* overwrite    */
int sella_mat_download(sella_ctx* ctx, sella_mat h, double* out);       /* .cpu().numpy() */
int sella_mat_shape(sella_ctx* ctx, sella_mat h, int* rows, int* cols);
int sella_mat_copy(sella_ctx* ctx, sella_mat src, sella_mat* dst);
int sella_mat_transpose(sella_ctx* ctx, sella_mat src, sella_mat* dst);
/* new matrix holding rows [row0, row0 + nrows) of src (the explicit eigenvectors of a structured eigendecomposition
 * are the leading rows of a larger buffer)                                                                        */
int sella_mat_rows(sella_ctx* ctx, sella_mat src, int row0, int nrows, sella_mat* dst);
/* dst rows [0, nrows) <- src rows [0, nrows) (equal column counts): growing such a buffer                          */
int sella_mat_copy_into(sella_ctx* ctx, sella_mat src, sella_mat dst, int nrows);
/* dst[drow + i][dcol + j] <- src[srow + i][scol + j] for a rows x cols block (src and dst different matrices; a block
 * that leaves either matrix: SELLA_E_INVALID): a principal block of one matrix into a frame of another size           */
int sella_mat_copy_block(sella_ctx* ctx, sella_mat src, int srow, int scol, int rows, int cols, sella_mat dst, int drow,
                         int dcol);
/* A[i][i] += alpha: B = lam0 * I of the first-update rule (sella/linalg.py:274-289) is a zero matrix plus this      */
int sella_mat_add_diag(sella_ctx* ctx, sella_mat h, double alpha);
int sella_mat_free(sella_ctx* ctx, sella_mat h);
/* C = alpha * A + beta * B (same shapes; B may be SELLA_NO_MAT with beta ignored)       */
int sella_mat_axpby(sella_ctx* ctx, double alpha, sella_mat A, double beta, sella_mat B,
                    sella_mat* C);

/* ---- dense products ------------------------------------------------------------------ */
/* Y = A X, A (n x n) resident, X and Y host (n x k row-major).
 * ApproximateHessian._matvec/_matmat  sella/linalg.py:324-335; dense A.dot(t) in
 * sella/eigensolvers.py:52,112; B@S in sella/hessian_update.py:119,160-176.             */
int sella_symm_mm(sella_ctx* ctx, sella_mat A, const double* X, int k, double* Y);
/* Y = A^T X for a general resident A (rows x cols), X host (rows x k), Y (cols x k)     */
int sella_gemm_tn_host(sella_ctx* ctx, sella_mat A, const double* X, int k, double* Y);
/* out (m x m) = U^T H U, H (n x n) resident, U host (n x m).
 * gpu_project  sella/_gpu.py:114-132 (peswrapper.py:374,382; linalg.py:306-317)         */
int sella_project(sella_ctx* ctx, sella_mat H, const double* U, int m, double* out);
/* same, result stays on the device as a new handle (and optionally on the host)        */
int sella_project_dev(sella_ctx* ctx, sella_mat H, sella_mat U, sella_mat* out);
/* general C = op(A) op(B) on resident matrices (test / building block)                 */
int sella_gemm(sella_ctx* ctx, int transA, int transB, double alpha, sella_mat A,
               sella_mat B, double beta, sella_mat C);

/* ---- symmetric eigensolver ------------------------------------------------------------ */
/* gpu_eigh / gpu_eigh_t  sella/_gpu.py:70-97 (torch.linalg.eigh).  w (n) ascending.
 * V: new handle holding the eigenvectors as COLUMNS (V[i][j] = component i of vector j),
 * Vt: new handle with the eigenvectors as ROWS.  Either pointer may be NULL.             */
int sella_eigh(sella_ctx* ctx, sella_mat A, double* w, sella_mat* V, sella_mat* Vt);

/* Building block of the eigensolver's divide-and-conquer stage, exposed for testing and reuse:
 * eigendecomposition of diag(D) + rho w w^T (D strictly ascending, w_i != 0, rho > 0).
 * lam (K) ascending; Ut (K x K row-major, may be NULL) has the eigenvectors as rows.          */
int sella_rank1_eig(sella_ctx* ctx, int K, const double* D, const double* w, double rho,
                    double* lam, double* Ut);

/* ---- thin QR ---------------------------------------------------------------------------- */
/* gpu_qr(A) economy mode  sella/_gpu.py:100-111 (peswrapper.py:691).  A host (m x n),
 * m >= n; Q (m x n), R (n x n) host outputs.                                             */
int sella_qr_thin(sella_ctx* ctx, const double* A, int m, int n, double* Q, double* R);

/* ---- Gram-Schmidt --------------------------------------------------------------------- */
/* modified_gram_schmidt(X, Y)  sella/utilities/math.pyx:143-159 (mgs :74-140).
 * X host (n x nx), Y host (n x ny) or NULL; out host (n x nx); *kept = columns kept.
 * Returns SELLA_E_NOCONV where the reference raises RuntimeError("MGS failed.").         */
int sella_mgs(sella_ctx* ctx, const double* X, int n, int nx, const double* Y, int ny,
              double eps1, double eps2, int maxiter, double* out, int* kept);

/* ---- Davidson / Rayleigh-Ritz ----------------------------------------------------------- */
/* rayleigh_ritz(A, gamma, P, B=None, v0, vref, vreftol, method, maxiter)
 *   sella/eigensolvers.py:31-112, expand :115-153.
 * A: resident dense matrix, or SELLA_NO_MAT with a callback (the finite-difference
 *    operator NumericalHessian, sella/linalg.py:39-95, lives behind the calculator boundary:
 *    a host-language callback for an ASE calculator, sella_fd_matvec for one of the library's own).
 *    A third kind, the analytic Hessian-vector operator of a calculator of the library, stays on the device:
 *    sella_davidson_hvp, declared with sella_hvp_* below.
 * P: given by its eigendecomposition P = Q diag(pevals) Q^T with Q resident both as columns
 *    (Pvecs) and as rows (PvecsT) — exactly what sella_eigh returns — or Pvecs = SELLA_NO_MAT
 *    for P = pscale * I.
 * v0: host (n x nv0) start block (nv0 >= 1).  vref may be NULL.
 * Outputs (host): lams (kmax), V and AV (n x k row-major, Ritz vectors as columns), *k.
 * STRUCTURED P: Pvecs (n x r) and PvecsT (r x n) with r < n hold r explicit eigenpairs (pevals, r entries) and the
 *    remaining n - r eigenvalues all equal pscale, their eigenspace being the orthogonal complement of the r vectors:
 *    P = pscale (I - W^T W) + W^T diag(pevals) W — what an approximate Hessian that started as a scaled identity
 *    (sella/linalg.py:274-289) is after any number of quasi-Newton updates.  (P - theta)^-1 then costs O(n r).
 * RE-ENTRANCY CONTRACT of the callbacks (sella_matvec_fn, sella_allgather_fn).  A callback runs on the thread that
 *    called the solver and MAY CALL ANY ENTRY POINT OF THIS LIBRARY ON THE SAME CONTEXT: create, upload, free and
 *    factorise matrices, run sella_eigh / sella_qr_thin / another sella_davidson, synchronise.  (NumericalHessian._matvec,
 *    sella/linalg.py:39-95, evaluates a calculator, and InternalPES transforms the vector through device-resident
 *    Jacobians on the way.)  The library guarantees: (1) matrix handles the solver was given stay valid and keep their
 *    device address while they are live — the handle table never moves an entry; (2) every scratch slot, scalar exchange
 *    buffer and staging buffer of the interrupted call is parked for the duration of the callback, the nested calls work
 *    on a set of their own per call depth; (3) device work queued by the callback is ordered behind the solver's on the
 *    context's single stream.  The callback must NOT free or overwrite the matrices passed to the interrupted solver
 *    (A, Pvecs, PvecsT), must not destroy the context, and must not call the library on this context from another
 *    thread.  v and Av (send / recv) are only valid until it returns.  A non-zero return aborts the solver with
 *    SELLA_E_CALLBACK.                                                                                              */
typedef int (*sella_matvec_fn)(void* user, const double* v, double* Av, int n);
enum { SELLA_DAV_LANCZOS = 0, SELLA_DAV_GD = 1, SELLA_DAV_JD0 = 2, SELLA_DAV_JD0_ALT = 3,
       SELLA_DAV_MJD0 = 4, SELLA_DAV_MJD0_ALT = 5 };
int sella_davidson(sella_ctx* ctx, sella_mat A, sella_matvec_fn matvec, void* user,
                   sella_mat Pvecs, sella_mat PvecsT, const double* pevals, double pscale,
                   int n, const double* v0, int nv0, double gamma, int method, int maxiter,
                   const double* vref, double vreftol,
                   double* lams, double* V, double* AV, int* k, int* nmatvec);

/* Block Davidson for the lowest `nev` eigenpairs of a large dense symmetric operator, `block` (<= 16) new
 * vectors per iteration with the operator streamed once per block on the matrix cores (BASELINE.json
 * configs[4]; the reference adds one vector per iteration, sella/eigensolvers.py:111-112, so there is no
 * trajectory to match: the converged pairs equal those of exact(), sella/eigensolvers.py:9-28).
 * A: resident (n x n), or — with `gather` — this rank's row panel A[row0 : row0 + rows, :] of a matrix whose rows
 *    are split evenly (ceil(n / world) per rank) over `world` ranks; `gather` must all-gather `bytes` bytes from
 *    every rank's device buffer `send` into `recv` (rank-major) on the given HIP stream (ncclAllGather).
 * Preconditioner: the eigendecomposition of an approximate operator P (Pvecs / PvecsT / pevals as for
 *    sella_davidson: t = Q (d - theta)^-1 Q^T r, the 'gd' correction of sella/eigensolvers.py:119-121), else
 *    diag (n, host: t_i = r_i / (diag_i - theta)), else none.
 * V0 (n x nv0, host, nv0 <= 16) start block or NULL.  tol: a pair counts as converged when
 *    |r| <= tol |theta| (the reference's gamma test, sella/eigensolvers.py:80-89).  maxvec: basis limit before a thick
 *    restart, 0 = nev + 3 block (room for two blocks between restarts; at least nev + 2 block).
 * Outputs (host): lams (nev), V (n x nev row-major), res (nev residual norms, may be NULL), *niter,
 *    *nmatvec (operator columns applied), *nconv (pairs converged; nev on success).
 * The gather callback is stream-ordered (no synchronisation around it); the re-entrancy contract above applies.     */
typedef int (*sella_allgather_fn)(void* user, const void* send, void* recv, size_t bytes, void* hip_stream);
int sella_davidson_block(sella_ctx* ctx, sella_mat A, int n, int row0, int world,
                         sella_allgather_fn gather, void* user, sella_mat Pvecs, sella_mat PvecsT,
                         const double* pevals, const double* diag, const double* V0, int nv0, int nev,
                         int block, int maxvec, double tol, int maxiter, double* lams, double* V,
                         double* res, int* niter, int* nmatvec, int* nconv);

/* Raw copy between buffers handed to a callback (kind 0: device -> device, 1: device -> host, 2: host -> device),
 * ordered on the context's stream and complete on return.  Lets a host-side all-gather (the gloo shim of the CPU
 * tests) stage the device buffers of sella_davidson_block; RCCL takes the device pointers directly.              */
int sella_dev_copy(sella_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
/* The context's HIP stream (hipStream_t) and the device address / leading dimension of a resident matrix: the
 * handles a collective library bound from the host language (librccl through ctypes: ncclAllGather(send, recv,
 * count, ncclDouble, comm, stream)) needs to run on the library's own buffers in stream order, without PyTorch.
 * The reference has no collective anywhere; this is new surface for configs[3] / [4].     */
int sella_ctx_stream(sella_ctx* ctx, void** hip_stream);
int sella_mat_ptr(sella_ctx* ctx, sella_mat h, void** device_ptr, int* ld);

/* ---- quasi-Newton update ------------------------------------------------------------------ */
/* update_H(B, S, Y, method, symm, lams, vecs, B_gpu, evals_gpu, evecs_gpu)
 *   sella/hessian_update.py:40-111, formulas :114-157, torch variant :160-203.
 * B resident (n x n) is updated IN PLACE and symmetrised in the same pass.
 * evecs/evals: eigendecomposition of B (columns), needed by TS-BFGS / BFGS_auto only.
 * S, Y host (n x k).  symm in {-1 (None), 0, 1, 2}.                                          */
enum { SELLA_UPD_TS_BFGS = 0, SELLA_UPD_BFGS = 1, SELLA_UPD_PSB = 2, SELLA_UPD_DFP = 3,
       SELLA_UPD_SR1 = 4, SELLA_UPD_GREENSTADT = 5, SELLA_UPD_BFGS_AUTO = 6 };
int sella_update_h(sella_ctx* ctx, sella_mat B, sella_mat evecs, sella_mat evecsT,
                   const double* evals, const double* S, const double* Y, int n, int k,
                   int method, int symm);
/* sella_update_h that also carries the eigendecomposition of B over to the updated matrix: the
 * update B+ - B has rank 2k..4k, so its eigenpairs follow from those of B by that many rank-one
 * modifications (secular equation + one GEMM each, eigh.hip) instead of a new factorisation —
 * what the reference pays torch.linalg.eigh for after every step (linalg.py:174-231).
 * evals (n, in/out), evecs / evecsT updated in place.  If the update has rank > max_rank (or no
 * eigenvectors are given) only B is updated and *nrank1 = -1: the caller then recomputes the
 * eigendecomposition with sella_eigh.  Otherwise *nrank1 = rank-one modifications applied.          */
int sella_update_h_eig(sella_ctx* ctx, sella_mat B, sella_mat evecs, sella_mat evecsT, double* evals,
                       const double* S, const double* Y, int n, int k, int method, int symm,
                       int max_rank, int* nrank1);
/* The same, keeping a principal submatrix of B in step with it: Bsub = B[idx][idx] (idx ascending, m
 * entries) is what `get_HL_projected` (sella/peswrapper.py:363-386) yields when the constraints pin single
 * Cartesian coordinates — U^T B U with U columns of the identity — and the reference re-diagonalises it at
 * every step.  Bsub receives the update restricted to idx; if evecs_sub / evecsT_sub / evals_sub are given
 * (handles != SELLA_NO_MAT) its eigendecomposition is carried the same way, *nrank1_sub as above.          */
int sella_update_h_eig_view(sella_ctx* ctx, sella_mat B, sella_mat evecs, sella_mat evecsT, double* evals,
                            const double* S, const double* Y, int n, int k, int method, int symm,
                            int max_rank, int* nrank1, sella_mat Bsub, sella_mat evecs_sub,
                            sella_mat evecsT_sub, double* evals_sub, const int* idx, int m,
                            int* nrank1_sub);
/* STRUCTURED eigendecomposition.  An approximate Hessian initialised by the first-update rule (sella/linalg.py:274-289:
 * B = lam0 I + update) stays lam0 I + (rank r) for ever: r explicit eigenpairs — mu (host, ascending) and the leading r
 * rows of Wt (capacity rows x n, resident) — plus the eigenvalue lam0 on the orthogonal complement of their span.  The
 * reference re-diagonalises the dense matrix after every update (linalg.py:174-231, torch.linalg.eigh); sella_update_h_eig
 * carries n explicit eigenvectors by rank-one merges with O(n^2) passes; here a rank-one term costs O(n r): the component
 * of its vector outside span(W) joins W as a row with eigenvalue lam0 and the merge runs on r + 1 rows.
 *   B (n x n resident) receives the update as in sella_update_h; *r and mu are updated (r grows by at most 4k per call:
 *   the caller provides capacity); *nrank1 = rank-one merges applied.
 *   Optional principal-submatrix view Bsub = B[idx][idx] with a structured eigendecomposition of its own
 *   (Wt_sub capacity x m, *r_sub, mu_sub; lam0 the same) kept in step; pass Bsub = SELLA_NO_MAT for none, or
 *   Wt_sub = SELLA_NO_MAT to update the view's matrix only.                                                          */
int sella_update_h_lr(sella_ctx* ctx, sella_mat B, sella_mat Wt, int* r, double* mu, double lam0, const double* S,
                      const double* Y, int n, int k, int method, int symm, int* nrank1, sella_mat Bsub,
                      sella_mat Wt_sub, int* r_sub, double* mu_sub, const int* idx, int m, int* nrank1_sub);
/* Structured eigendecomposition of the principal submatrix B[idx][idx] (idx ascending, m entries) from that of B:
 * U^T B U for U = columns of the identity, sella/peswrapper.py:363-386, without an m x m eigh.
 * Wt_sub: capacity (>= min(r, m)) x m; outputs *r_sub, mu_sub (capacity entries).                                    */
int sella_lr_restrict(sella_ctx* ctx, sella_mat Wt, int r, const double* mu, double lam0, const int* idx, int m,
                      sella_mat Wt_sub, int* r_sub, double* mu_sub);
/* symmetrize_Y(S, Y, symm)  sella/hessian_update.py:12-37; out host (n x k)                   */
int sella_symmetrize_y(sella_ctx* ctx, const double* S, const double* Y, int n, int k,
                       int symm, double* out);

/* ---- step solve -------------------------------------------------------------------------- */
/* One evaluation of Stepper.get_s(alpha)  sella/optimize/stepper.py:82-96 (QN), :128-157
 * (RFO), :179-185 (P-RFO) in the eigenbasis of the (projected) Hessian:
 *   evecs (m x m resident, columns) / evecsT (rows), evals (m), g (m) host.
 * kind: 0 = qn, 1 = rfo, 2 = prfo.  Outputs s, dsda (m) host.                               */
enum { SELLA_STEP_QN = 0, SELLA_STEP_RFO = 1, SELLA_STEP_PRFO = 2, SELLA_STEP_QN_IRC = 3 };
typedef struct sella_stepper sella_stepper;
int sella_stepper_create(sella_ctx* ctx, int kind, sella_mat evecs, sella_mat evecsT,
                         const double* evals, const double* g, int m, int order,
                         sella_stepper** st);
/* The same families on a STRUCTURED eigendecomposition (see sella_update_h_lr): r explicit eigenpairs (mu ascending,
 * leading rows of Wt) + eigenvalue lam0 on the complement.  A mode without a gradient component gets a zero step in
 * every family, so the n - r cluster modes are represented by ONE — the normalised component of g outside span(W) —
 * plus min(order, n - r - 1) weightless copies that keep "the `order` lowest modes" and the RFO root index counting the
 * cluster's multiplicity.  The stepper then behaves exactly like one created from the dense eigendecomposition.      */
int sella_stepper_create_lr(sella_ctx* ctx, int kind, sella_mat Wt, int r, const double* mu, double lam0,
                            const double* g, int n, int order, sella_stepper** st);
int sella_stepper_get_s(sella_stepper* st, double alpha, double* s, double* dsda);
int sella_stepper_destroy(sella_stepper* st);
/* QuasiNewtonIRC (sella/optimize/stepper.py:99-111): kind SELLA_STEP_QN_IRC evaluates
 * s(alpha) = -V (V^T g + alpha V^T d1) / (|lam| + alpha); d1hat = V^T d1 (m entries: the accumulated IRC
 * displacement in the eigenbasis of the projected Hessian).  Must be set before the first evaluation.            */
int sella_stepper_set_d1hat(sella_stepper* st, const double* d1hat, int m);

/* The whole restricted-step root find, BaseRestrictedStep.get_s of sella/optimize/restricted_step.py:64-120, in ONE
 * call: the 1-D search over the step-length parameter alpha of the family `st` until the constraint measure of the
 * total step s(alpha) + scons equals the radius delta — same start value, bracket updates, Newton / bisection
 * schedule (bisection only once niter > 4 unless newton_safe), nextafter bracket test and tolerances as the
 * reference, so the sequence of trial alphas is the reference's.
 *   cons: 0 trust region |s| (TrustRegion.cons :136-142); 1 largest per-atom displacement (RestrictedAtomicStep.cons
 *         :172-183: consecutive triples; when nout is not a multiple of 3 — masked cell coordinates behind the atoms — the
 *         trailing partial group counts as padded with zeros); 2 largest weighted component |w_i s_i| (MaxInternalStep.cons :206-216);
 *         3 weighted sphere |(s + d1) * w| (IRCTrustRegion.cons :152-158).
 *   scons (nout) or NULL: the constraint-correction step added to every trial step (:35-37, :73-76);
 *   w (nout) for cons 2 / 3, d1 (nout) for cons 3;
 *   alpha0, alphamin, alphamax, slope, newton_safe: the family's class attributes (stepper.py:20-41);
 *   orthonormal != 0: the columns of the stepper's eigenvector matrix are orthonormal in the OUTPUT space, so for
 *         cons 0 the norm is evaluated in the eigenbasis (|s|^2 = |shat|^2 + 2 shat.V^T scons + |scons|^2) and no
 *         device work at all happens per trial alpha.
 *   sel (m ints) / nfull: the family lives in the subspace of the free coordinates sel[0..m) of an nfull-dimensional
 *         space (projection basis = columns of the identity, constraints that pin single coordinates); scons, w, d1,
 *         the measure and the returned step are then nfull-dimensional.  NULL / 0 otherwise.
 * Per trial alpha otherwise: O(m) host arithmetic, one 2-right-hand-side device matvec and one single-workgroup
 * reduction; only two scalars come back.  Once the schedule is pure bisection (sixth trial on for the families that are
 * not newton_safe, restricted_step.py:100-110) the next four levels of midpoints — 15 trial alphas, the reference's own —
 * are evaluated per round trip (option rs_batch): secular roots per candidate on the device, ONE pass over the
 * eigenvector matrix for all of them on the matrix cores, one measure per workgroup.  Outputs: s (nout) = total step at the final alpha, *val = the measure
 * reported by the reference (the value itself inside the radius, delta on the boundary), alphas[0 .. *nalpha) the
 * trial sequence (capacity maxiter + 1; may be NULL).  Returns SELLA_E_NOCONV where the reference raises
 * RuntimeError("Restricted step failed to converge!").                                                          */
int sella_restricted_step(sella_stepper* st, int cons, double delta, const double* scons, const double* w,
                          const double* d1, double alpha0, double alphamin, double alphamax, double slope,
                          int newton_safe, int orthonormal, double tol, int maxiter, const int* sel, int nfull,
                          double* s, double* val, double* alphas, int* nalpha);

/* ---- one optimizer step per call ------------------------------------------------------------- */
/* Sella.step (sella/optimize/optimize.py:359-440) between two force calls, in ONE call: PES.kick's model prediction,
 * ratio and quasi-Newton update (peswrapper.py:578-602, linalg.py:274-304), the trust-radius rule (optimize.py:413-434)
 * and the restricted step at the new point (restricted_step.py:28-120, stepper.py) — for the Cartesian PES whose
 * approximate Hessian carries a STRUCTURED eigendecomposition (sella_update_h_lr), unconstrained or with constraints
 * that pin single coordinates (idx / m: the free coordinates; the view Bsub = B[idx][idx] with its own structured
 * decomposition as in sella_update_h_lr), constraints satisfied (no correction step).  The calculator boundary
 * (peswrapper.py:413-418) stays with the caller: it moves the atoms by the step returned, evaluates f and g, calls again.
 * Every phase runs the routines of the one-phase entry points, so results are theirs bit for bit.
 *   flags: SELLA_OPT_LEARN  uses dx (step taken, n), g_old, g_new, f_old, f_new, smag (measure of the step taken as
 *                           reported by the restricted step), delta / rho (in-out), the five radius parameters;
 *                           outputs df_pred, ratio + ratio_valid (|df_pred| >= 1e-14), nrank1, nrank1_sub, *r, mu, ...
 *          SELLA_OPT_PROPOSE uses g_new, delta, stepper_kind (SELLA_STEP_*), order, cons (0 tr, 1 ras), tol, maxiter;
 *                           outputs s_out (n), smag_out, nalpha.
 * The re-diagonalisation schedule (optimize.py:363-378) stays with the caller: it asks for LEARN only, runs the
 * iterative diagonalisation, then asks for PROPOSE.                                                                  */
enum { SELLA_OPT_LEARN = 1, SELLA_OPT_PROPOSE = 2 };
typedef struct sella_opt_step_t {
    int flags, n;
    /* approximate Hessian and its structured eigendecomposition (sella_update_h_lr) */
    sella_mat B, Wt;
    int* r;
    double* mu;
    double lam0;
    int update_method, symm;
    int B_stale, Bsub_stale;   /* in-out: the dense mirrors lag behind (W, mu, lam0); rebuilt by sella_lr_materialize when needed */
    /* principal-submatrix view of pinned-coordinate constraints (idx == NULL: none) */
    sella_mat Bsub, Wt_sub;
    int* r_sub;
    double* mu_sub;
    const int* idx;
    int m;
    /* learn */
    const double *dx, *g_old, *g_new;
    double f_old, f_new, smag;
    double delta, rho;                                      /* in-out */
    double delta_min, sigma_inc, sigma_dec, rho_inc, rho_dec;
    double df_pred, ratio;                                  /* out */
    int ratio_valid, updated, nrank1, nrank1_sub;           /* out; updated = 0: step shorter than 1e-8, B left alone */
    /* propose */
    int stepper_kind, order, cons, maxiter;
    double tol;
    double* s_out;                                          /* n */
    double smag_out;                                        /* out */
    int nalpha;                                             /* out */
    double alpha_hint;         /* in-out: alpha at which the previous root search of THIS search ended (0: none): the first
                                * round of the batched search looks around it; same root, fewer rounds                    */
} sella_opt_step_t;
int sella_opt_step(sella_ctx* ctx, sella_opt_step_t* io);
/* Dense mirror of a structured decomposition: B <- lam0 I + W^T diag(mu - lam0) W (B n x n resident, overwritten).  The
 * fast form of sella_opt_step updates (W, mu) only and marks B stale; whoever needs the matrix itself — `H.B`, a matvec, a
 * projection, the general update route — rebuilds it first.                                                             */
int sella_lr_materialize(sella_ctx* ctx, sella_mat B, sella_mat Wt, int r, const double* mu, double lam0);

/* ---- internal-coordinate primitives ----------------------------------------------------------- */
/* Batched value / gradient / Hessian-vector product / Hessian of bonds (natoms = 2), angles (3) and
 * dihedrals (4): the vmapped JAX functions of sella/internal.py:58-135
 *   _bond_value/_angle_value/_dihedral_value (:58-80), *_grad_batched (:85-87),
 *   *_hess_batched (:95-97), *_hvp_batched (:106-135).
 * pos (nc, natoms, 3) gathered atom positions; tvec (nc, natoms-1, 3) periodic shift vectors or NULL;
 * tangent (nc, natoms, 3) or NULL.  Outputs (host): q (nc), grad (nc, natoms, 3),
 * hvp (nc, natoms, 3) when tangent is given, hess (nc, 3 natoms, 3 natoms) when not NULL.            */
int sella_internals_eval(sella_ctx* ctx, int natoms, int nc, const double* pos, const double* tvec,
                         const double* tangent, double* q, double* grad, double* hvp, double* hess);

/* TRIC fragment rotations (sella/internal.py:1030-1078 `Rotation.calc` / `calc_gradient` / `calc_hessian`, closed forms
 * :507-1010): the exponential map v_k = 2 c_{k+1} asinc(c_0), k = 0, 1, 2, of the quaternion c that best aligns each
 * fragment's reference positions with its current ones (top eigenvector of the 4x4 matrix F(R), R = sum_i p_i (x) ref_i).
 * Fragment f holds the atoms frag_atoms[frag_ptr[f] .. frag_ptr[f+1]) (at least one; indices in [0, natoms)).
 *   pos (natoms, 3) positions; refpos (frag_ptr[nf], 3) reference positions, one row per CSR slot, centred per fragment;
 *   q_prev (nf, 4) quaternion state, read and written: with flags bit 0 set (a value evaluation) c is q_prev projected
 *     onto the top eigenspace of F (eigenvalues within 1e-10 of the largest), normalised, sign fixed so that c_0 >= 0
 *     (the top eigenvector if the projection vanishes), and stored back; with the bit clear c = q_prev as given;
 *   tangent (natoms, 3) or NULL.
 * Outputs (host): val (nf, 3); grad (frag_ptr[nf] * 9): per fragment a (3 axes, m, 3) block at offset 9 frag_ptr[f];
 * hvp the same layout (when tangent is given); hess, when not NULL, per fragment (3 axes, 3m, 3m) blocks one after the
 * other (offset sum over earlier fragments of 27 m^2).  Derivatives use the pseudo-inverse of F - lam that drops gaps
 * <= 1e-14, so diatomic and linear fragments give finite numbers.                                                      */
int sella_internals_tric_eval(sella_ctx* ctx, int natoms, int nf, const int* frag_ptr, const int* frag_atoms,
                              const double* pos, const double* refpos, double* q_prev, const double* tangent, int flags,
                              double* val, double* grad, double* hvp, double* hess);
/* The same with periodic images (the reference unwraps each fragment across the cell, internal.py:3334-3362, moving the
 * atoms; here the atoms stay where they are): shift (frag_ptr[nf], 3) holds one Cartesian shift per CSR slot — n @ cell
 * for the slot's integer image n — added to that slot's position wherever a position is read, before anything else:
 * (pos + shift) - anchor, so the results equal, bit for bit, those of sella_internals_tric_eval on positions the host
 * unwrapped itself.  The tangent takes no shift.  shift NULL: exactly sella_internals_tric_eval, which is this entry
 * point called with NULL.                                                                                             */
int sella_internals_tric_eval_shifted(sella_ctx* ctx, int natoms, int nf, const int* frag_ptr, const int* frag_atoms,
                                      const double* pos, const double* shift, const double* refpos, double* q_prev,
                                      const double* tangent, int flags, double* val, double* grad, double* hvp,
                                      double* hess);

/* ---- sparse internal-coordinate Jacobian / Hessians ------------------------------------------------- */
/* SparseInternalJacobian, SparseInternalHessian(s) and SparseInternalHessiansSkeleton of sella/linalg.py:362-646.
 * One object holds one topology — the skeleton of linalg.py:470-537: coordinate k touches the sizes[k] atoms
 * atoms[sum_{k'<k} sizes[k'] ..] (0 <= sizes[k] <= natoms; an atom may repeat, a periodic image of itself, and its
 * entries then accumulate) — plus device-resident values: gradient blocks (sizes[k], 3) and Hessian blocks
 * (sizes[k], 3, sizes[k], 3), concatenated in coordinate order.
 *   set_values / get_values: host <-> device copies of those buffers (NULL: that buffer is left alone);
 *   eval: coordinates first .. first+count (all of natoms_per_coord = 2 / 3 / 4 atoms: bonds / angles / dihedrals)
 *     filled from positions pos (count, natoms_per_coord, 3) and shift vectors tvec (count, natoms_per_coord-1, 3) or
 *     NULL by the kernels of sella_internals_eval (gradient; Hessian too when `hessian`), without a trip to the host;
 *   ldot(v): sum_k v_k H_k, (3 natoms x 3 natoms), linalg.py:601-618, summed in the reference's order (size groups in
 *     order of first appearance, each group's sum from zero, coordinates and (a, b, i, j) in order inside it);
 *   rdot(x): rows H_k x, (ncoords x 3 natoms), linalg.py:620-640;  ddot(u, x): u . H_k x (ncoords), :642-646;
 *   hess_dense: the dense H_k of coordinates first .. first+count as (count 3 natoms x 3 natoms) rows, :420-442, 595-596;
 *   jac_dense (count x 3 natoms) / jac_matvec (ncoords) / jac_rmatvec (3 natoms, add.at order): :377-401.
 *   ldot_acc(v, alpha, beta): out = beta out + alpha ldot(v), the sum formed exactly as by ldot and added once per
 *     element (out is not read when beta == 0: (1, 0) stores what ldot stores, bit for bit).
 * `out` matrices are allocated by the caller with exactly the shapes above; every element, padding included, is
 * stored.  Invalid shapes: SELLA_E_INVALID; a failed allocation: SELLA_E_NOMEM.                                    */
typedef struct sella_sparse_int sella_sparse_int;
int sella_sparse_int_create(sella_ctx* ctx, int natoms, int ncoords, const int* sizes, const int* atoms,
                            sella_sparse_int** out);
int sella_sparse_int_destroy(sella_sparse_int* s);
int sella_sparse_int_set_values(sella_sparse_int* s, const double* grad_vals, const double* hess_vals);
int sella_sparse_int_get_values(sella_sparse_int* s, double* grad_vals, double* hess_vals);
int sella_sparse_int_eval(sella_sparse_int* s, int first, int count, int natoms_per_coord, const double* pos,
                          const double* tvec, int hessian);
int sella_sparse_int_ldot(sella_sparse_int* s, const double* v, sella_mat out);
int sella_sparse_int_ldot_acc(sella_sparse_int* s, const double* v, double alpha, double beta, sella_mat out);
int sella_sparse_int_rdot(sella_sparse_int* s, const double* x, sella_mat out);
int sella_sparse_int_ddot(sella_sparse_int* s, const double* u, const double* x, double* out);
int sella_sparse_int_hess_dense(sella_sparse_int* s, int first, int count, sella_mat out);
int sella_sparse_int_jac_dense(sella_sparse_int* s, int first, int count, sella_mat out);
int sella_sparse_int_jac_matvec(sella_sparse_int* s, const double* x, double* out);
int sella_sparse_int_jac_rmatvec(sella_sparse_int* s, const double* y, double* out);

/* ---- exact Hessians in internal coordinates ------------------------------------------------------ */
/* The Cartesian Hessian of a calculator in the redundant internal coordinates of a topology `s` whose gradient and
 * Hessian blocks hold B = dq/dx and the d2q_i/dx2 of the current geometry, and back
 * (InternalPES._convert_cartesian_hessian_to_internal / _convert_internal_hessian_to_cartesian,
 * sella/peswrapper.py:1247-1282).  n = 3 natoms of `s` (real atoms and dummies), nint = ncoords of `s`, g (nint, host)
 * the internal gradient.
 *   cart_to_int: Hcart (n x n) is overwritten with Hcorr = Hcart - sum_i g_i d2q_i/dx2 (one accumulating ldot);
 *     X (n x r) = V_r S_r^-1 and Q (nint x r) = U_r from the singular value decomposition of B restricted to the real
 *     atoms' columns (rows of X of dummy degrees of freedom zero, like the rows and columns of Hcart);
 *     Hnred = X^T Hcorr X (r x r), lambda_bar = exp(mean log |eig((Hnred + Hnred^T) / 2)|) (the r eigenvalues are the
 *     only read-back), out (nint x nint) = Q (Hnred - lambda_bar I) Q^T + lambda_bar I, left on the device.
 *     r = 0: SELLA_E_INVALID.
 *   int_to_cart: out (n x n) = B^T Hint B + sum_i g_i d2q_i/dx2, Hint (nint x nint).
 * All matrices are allocated by the caller with exactly these shapes; invalid shapes: SELLA_E_INVALID.              */
int sella_hessian_cart_to_int(sella_ctx* ctx, sella_sparse_int* s, const double* g, sella_mat Hcart, sella_mat X,
                              sella_mat Q, sella_mat out, double* lambda_bar);
int sella_hessian_int_to_cart(sella_ctx* ctx, sella_sparse_int* s, const double* g, sella_mat Hint, sella_mat out);

/* ---- EMT calculator (far side of the calculator boundary, sella/peswrapper.py:413-418) -------------- */
/* Energy and gradient of the effective-medium potential (functional form of ase/calculators/emt.py).
 * pos (n x 3); par (9 x n): per-atom E0, s0, V0, eta2, kappa, lambda, n0, gamma1, gamma2 in eV / Angstrom;
 * shifts (nshift x 3): lattice translations of the periodic images to include (with the zero vector);
 * rc, acut, cutoff, beta: cutoff function parameters.  Outputs: *energy, grad (n x 3) = dE/dx.
 * Limits (also of sella_calc_emt_create): n < 2^24 atoms and nshift <= 127 images (SELLA_E_INVALID beyond: the density pass
 * hands each thread's neighbours to the force pass as packed (atom, image) words); the hand-over area is 256 x 9 ints =
 * 9.2 KB of scratch per atom, written and read by every force call (9.4 MB at 1024 atoms).                            */
int sella_emt_eval(sella_ctx* ctx, int n, const double* pos, const double* par, int nshift,
                   const double* shifts, double rc, double acut, double cutoff, double beta,
                   double* energy, double* grad);
/* The same evaluation plus the virial, in the same force pass (one device evaluation, one read-back).
 * virial6 (6): W_ab = dE/d eps_ab, the derivative of the energy under the homogeneous strain x -> (I + eps) x of the
 * positions AND the lattice translations (shifts), summed over the pairs as sum 1/2 (dE/dr / r) d_a d_b, in Voigt order
 * (xx, yy, zz, yz, xz, xy), eV.  ASE's stress is virial6 / V (eV / Angstrom^3; a compressed crystal has negative diagonal
 * stress).  *energy and grad are bit-for-bit those of sella_emt_eval.                                               */
int sella_emt_eval_stress(sella_ctx* ctx, int n, const double* pos, const double* par, int nshift,
                          const double* shifts, double rc, double acut, double cutoff, double beta,
                          double* energy, double* grad, double* virial6);
/* The analytic Hessian d2E/dx2 of the same potential (csrc/emt_hessian.hip), arguments and limits as for sella_emt_eval.
 *   hessian: out (3n x 3n, allocated by the caller) is overwritten and stays on the device; exactly symmetric, and the
 *     same bit for bit whether or not the neighbour lists of the density pass overflowed (emt_hcap).  Besides `out` it
 *     needs two n x 3n device matrices for the length of the call (SELLA_E_NOMEM if they cannot be had).
 *   hvp: HV[q] = H V[q] for k vectors, V and HV (k x 3n) host arrays with one vector per row; no 3n x 3n storage.
 * A wrong shape of `out`, k <= 0 or a null pointer: SELLA_E_INVALID.                                                */
int sella_emt_hessian(sella_ctx* ctx, int n, const double* pos, const double* par, int nshift,
                      const double* shifts, double rc, double acut, double cutoff, double beta, sella_mat out);
int sella_emt_hvp(sella_ctx* ctx, int n, const double* pos, const double* par, int nshift,
                  const double* shifts, double rc, double acut, double cutoff, double beta,
                  const double* V, int k, double* HV);
/* The analytic Hessian of positions AND cell, in the coordinates [x (3n Cartesian positions); C.ravel() (the nine cell
 * entries, row-major, lattice vectors in the rows of C)], the positions held fixed while C varies (the convention of
 * set_cell(scale_atoms=False)).  cell (9): C; shifts must be whole-number combinations n_s C of its rows — the image
 * indices n_s = S_s C^-1 are worked out here, and the cell enters the energy through them alone, so a lattice vector no
 * shift uses (a non-periodic direction) gives zero rows and columns.  out ((3n + 9) square, allocated by the caller) is
 * overwritten and stays on the device: exactly symmetric, the same bit for bit whether or not the neighbour lists
 * overflowed, and its leading 3n x 3n block is bit for bit sella_emt_hessian's (the same passes, written with the wider
 * row stride).  Other arguments, limits and temporary storage as for sella_emt_hessian, plus one n x 9 device matrix.
 * A wrong shape of `out`, a null pointer, a singular cell, or a shift whose image index is not whole to 1e-6:
 * SELLA_E_INVALID.                                                                                                  */
int sella_emt_cell_hessian(sella_ctx* ctx, int n, const double* pos, const double* par, int nshift,
                           const double* shifts, const double* cell, double rc, double acut, double cutoff, double beta,
                           sella_mat out);
/* Products with that Hessian without forming it: HV[q] = H V[q] for k vectors, V and HV (k x (3n + 9)) host arrays with
 * one vector [v (3n); W.ravel() (9, W the variation of C)] per row, in the coordinates of sella_emt_cell_hessian.  A
 * direction displaces the pair of a visit by v_j - v_i + n_s W; the two passes of sella_emt_hvp with that displacement
 * give the position rows, the same pair quantities contracted with the image indices the nine cell rows, summed over the
 * atoms in a fixed order.  No storage of size (3n)^2 or (3n + 9)^2, no atomics, the same bit for bit from call to call
 * and whether or not the neighbour lists overflowed; any k >= 1 (four vectors per workgroup, all groups in one launch
 * of each pass).  A null pointer, n, k or nshift <= 0, nshift > 127, a singular cell, or a shift whose image index is
 * not whole to 1e-6: SELLA_E_INVALID.                                                                                */
int sella_emt_cell_hvp(sella_ctx* ctx, int n, const double* pos, const double* par, int nshift,
                       const double* shifts, const double* cell, double rc, double acut, double cutoff, double beta,
                       const double* V, int k, double* HV);

/* ---- pair potentials (Morse, Lennard-Jones): the potential of tests/integration/test_morse_cluster.py ------------- */
/* Energy and gradient of E = 1/2 sum over the ordered visits (i <- j, image s) of phi(r), r = |x_j + S_s - x_i|
 * (csrc/pair.hip: one pass, one workgroup per atom, sums reduced in-block — the same bits from call to call).
 * pos (n x 3); form and params: 0 Morse, phi = D (1 - e^{-a (r - r0)})^2 - D, params D, a, r0;
 *                               1 Lennard-Jones, phi = 4 eps ((sigma / r)^12 - (sigma / r)^6), params eps, sigma;
 * shifts (nshift x 3): lattice translations of the periodic images to include (with the zero vector), cells narrower than
 * 2 rcut included; rcut > 0: the shifted-force form phi(r) - phi(rcut) - phi'(rcut)(r - rcut) inside rcut and zero beyond
 * (energy and force continuous there, phi'' not); rcut <= 0: no cutoff — plain phi over all pairs, allowed for nshift = 1
 * only.  A visit of an atom to its own image adds 1/2 phi to the energy and to the virial, nothing to forces or Hessian.
 * Outputs: *energy, grad (n x 3) = dE/dx.  Limits (also of sella_calc_pair_create): n < 2^24 atoms and nshift <= 127
 * images.  SELLA_E_INVALID beyond them, for a null pointer, n or nshift <= 0, another form, parameters, shifts or rcut
 * that are not finite, sigma <= 0, or no cutoff with nshift > 1.                                                      */
int sella_pair_eval(sella_ctx* ctx, int n, const double* pos, int form, const double* params, int nshift,
                    const double* shifts, double rcut, double* energy, double* grad);
/* The same evaluation plus the virial in the same pass.  virial6 (6): the convention of sella_emt_eval_stress, W_ab =
 * dE/d eps_ab = 1/2 sum over the visits of (phi'/r) d_a d_b, Voigt order (xx, yy, zz, yz, xz, xy), eV; stress =
 * virial6 / V.  *energy and grad are bit-for-bit those of sella_pair_eval.                                          */
int sella_pair_eval_stress(sella_ctx* ctx, int n, const double* pos, int form, const double* params, int nshift,
                           const double* shifts, double rcut, double* energy, double* grad, double* virial6);
/* The analytic Hessian d2E/dx2 of the same potential, arguments and limits as for sella_pair_eval.
 *   hessian: out (3n x 3n, allocated by the caller) is overwritten and stays on the device; exactly symmetric.  Row block
 *     i holds -K on (i, j) and sum K on (i, i), K = phi'' u u^T + (phi'/r)(I - u u^T) summed over the images of j; no
 *     temporary storage.
 *   hvp: HV[q] = H V[q] for k vectors, V and HV (k x 3n) host arrays with one vector per row; no 3n x 3n storage.  The
 *     visits of the geometry (neighbour, direction, phi'/r, phi'' - phi'/r: 44 bytes each) are built once per call and the
 *     vectors taken through them 16 at a time.
 * A wrong shape of `out`, k <= 0 or a null pointer: SELLA_E_INVALID.                                                */
int sella_pair_hessian(sella_ctx* ctx, int n, const double* pos, int form, const double* params, int nshift,
                       const double* shifts, double rcut, sella_mat out);
int sella_pair_hvp(sella_ctx* ctx, int n, const double* pos, int form, const double* params, int nshift,
                   const double* shifts, double rcut, const double* V, int k, double* HV);

/* ---- TIP3P water: the potential of tests/integration/test_tip3p_cluster.py (ase/calculators/tip3p.py) ------------- */
/* Energy and gradient of rigid three-site water (csrc/tip3p.hip: one workgroup per molecule, every molecule pair visited
 * from both ends, sums reduced in-block — the same bits from call to call).  E = sum over the molecule pairs m < n of
 * t(d) U_mn, U_mn = 4 epsilon ((sigma/d)^12 - (sigma/d)^6) + k_e sum over the nine site pairs of q_a q_b / r_ab, d the O-O
 * distance, t = 1 up to rc - width, 1 - y^2 (3 - 2 y) with y = (d - rc + width) / width up to rc, 0 beyond; nothing inside a
 * molecule.  pos (3 n_mol x 3): consecutive triples, one molecule each, the oxygen at site o: 0 (O H H) or 2 (H H O).
 * box (3): the edges of an orthorhombic cell, <= 0 for a direction that is not periodic; one shift per molecule pair,
 * -L rint(D / L) of the O-O difference D, moves all nine site pairs.  params (6): q_H (q_O = -2 q_H), sigma, epsilon, k_e,
 * rc, width.  A site pair closer than 1e-8 is skipped.  Outputs: *energy, grad (3 n_mol x 3) = dE/dx.  A single molecule is
 * valid (all zero).  SELLA_E_INVALID (also from sella_calc_tip3p_create) for a null pointer, n_mol <= 0, another o,
 * positions, box or parameters that are not finite, sigma <= 0, width <= 0 or width > rc, a periodic edge below 2 rc, or
 * 3 n_mol >= 2^24.                                                                                                    */
int sella_tip3p_eval(sella_ctx* ctx, int n_mol, const double* pos, int o, const double* box, const double* params,
                     double* energy, double* grad);
/* The analytic Hessian d2E/dx2 of the same potential, arguments and limits as for sella_tip3p_eval.
 *   hessian: out (9 n_mol square, allocated by the caller) is overwritten and stays on the device; exactly symmetric.  The
 *     switch acts on whole molecule pairs, so the blocks are 9 x 9 per pair of molecules (the diagonal ones included), not
 *     3 x 3 per pair of atoms; no temporary storage.
 *   hvp: HV[q] = H V[q] for k vectors, V and HV (k x 9 n_mol) host arrays with one vector per row; no 9 n_mol square
 *     storage.  The visits of the geometry (a partner inside rc with its nine site pairs' directions and coefficients, the
 *     switched gradients at the six sites, u_OO and two switch scalars: 548 bytes each) are built once per call and the
 *     vectors taken through them 16 at a time.
 * A wrong shape of `out`, k <= 0 or a null pointer: SELLA_E_INVALID.                                                */
int sella_tip3p_hessian(sella_ctx* ctx, int n_mol, const double* pos, int o, const double* box, const double* params,
                        sella_mat out);
int sella_tip3p_hvp(sella_ctx* ctx, int n_mol, const double* pos, int o, const double* box, const double* params,
                    const double* V, int k, double* HV);

/* ---- calculators that live in the library, and the finite-difference Hessian on top of one ----------------- */
/* sella/peswrapper.py:413-418 evaluates energy and forces through `atoms.calc`; for a calculator implemented HERE that
 * boundary can be crossed without the host language: sella_calc_eval(calc, x, &f, g) -> energy and gradient dE/dx.
 *   model: f(x) = 1/2 x^T A x + c/3 sum_j (u_j . x)^3, A (n x n resident), U (nu x n host, copied);
 *   emt:   the arguments of sella_emt_eval, fixed at creation (n = 3 natoms);
 *   pair:  the arguments of sella_pair_eval, fixed at creation (n = 3 natoms; parameters and shifts resident);
 *   tip3p: the arguments of sella_tip3p_eval but the positions, fixed at creation (n = 9 n_mol).                     */
typedef struct sella_calc sella_calc;
int sella_calc_model_create(sella_ctx* ctx, sella_mat A, const double* U, int nu, int n, double c, sella_calc** calc);
int sella_calc_emt_create(sella_ctx* ctx, int natoms, const double* par, int nshift, const double* shifts, double rc,
                          double acut, double cutoff, double beta, sella_calc** calc);
int sella_calc_pair_create(sella_ctx* ctx, int natoms, int form, const double* params, int nshift, const double* shifts,
                           double rcut, sella_calc** calc);
int sella_calc_tip3p_create(sella_ctx* ctx, int n_mol, int o, const double* box, const double* params, sella_calc** calc);
int sella_calc_eval(sella_calc* calc, const double* x, double* energy, double* grad);
/* Second derivatives at x: the Hessian into out (n x n, allocated by the caller, stays on the device), and its products
 * HV[q] = H V[q] with k host vectors (V, HV: k x n, one vector per row).  emt: sella_emt_hessian / sella_emt_hvp on the
 * calculator's resident constants, bit for bit; pair: sella_pair_hessian / sella_pair_hvp, bit for bit; tip3p:
 * sella_tip3p_hessian / sella_tip3p_hvp, bit for bit; model:
 * A + 2 c sum_j (u_j . x) u_j u_j^T.  Neither counts as a force
 * call (sella_calc_ncalls is unchanged).  Wrong shapes: SELLA_E_INVALID.                                              */
int sella_calc_hessian(sella_calc* calc, const double* x, sella_mat out);
int sella_calc_hvp(sella_calc* calc, const double* x, const double* V, int k, double* HV);
long sella_calc_ncalls(sella_calc* calc);
int sella_calc_dim(sella_calc* calc);
int sella_calc_destroy(sella_calc* calc);
/* NumericalHessian (sella/linalg.py:14-101): H v ~ scale (g(x0 + eta v / scale) - g0) / eta (threepoint: the central
 * form), scale = +-|v| by the reference's orientation rule (:45-73), seen through the free coordinates idx[0..m) of a
 * pinned-coordinate constraint set (NULL: all n).  sella_fd_matvec has the sella_matvec_fn signature with the operator
 * as `user`, so sella_davidson(ctx, SELLA_NO_MAT, sella_fd_matvec, fd, ...) is the iterative diagonalisation of
 * peswrapper.py:508-556 with no host-language frame between its force calls.  Every product is remembered:
 * sella_fd_pairs returns the displaced directions and difference quotients, (n x k) row-major each, k = sella_fd_npairs,
 * which PES.diag turns into secant pairs for the Hessian update (peswrapper.py:545-553).                              */
typedef struct sella_fd sella_fd;
int sella_fd_create(sella_calc* calc, int n, const double* x0, const double* g0, double eta, int threepoint,
                    const int* idx, int m, sella_fd** fd);
int sella_fd_matvec(void* fd, const double* v, double* Av, int m);
int sella_fd_npairs(sella_fd* fd);
long sella_fd_calls(sella_fd* fd);
int sella_fd_pairs(sella_fd* fd, double* Vs, double* AVs);
int sella_fd_destroy(sella_fd* fd);
/* The same operator in closed form, for a calculator that has its second derivatives (sella_calc_hvp): H v exactly, no
 * displacement, no force call (sella_calc_ncalls is unchanged).  What depends on the geometry x0 is built ONCE at creation
 * and stays resident in an allocation of the operator's own — emt: one density pass and the second derivatives of the
 * embedding functions (positions, densities, neighbour lists); pair: the visits of every atom in the order of the sweep, with
 * the neighbour, the unit vector, phi'/r and phi'' - phi'/r of each (one counting and one filling pass; a product then
 * evaluates no exp, sqrt or division); model: the rows 2 c (u_j . x0) u_j — so a product is two
 * launches on one device vector (emt; pair: one; model: two row-panel matvecs) plus one that spreads the m free entries idx[0..m)
 * (ascending; NULL: all n) over the full space.  The product is (H vfull)[idx] with vfull zero on the pinned coordinates.
 *   sella_hvp_matvec     the sella_matvec_fn form with HOST vectors (upload, the device product, download, wait): the
 *                        operator also serves the unchanged sella_davidson as its callback.
 *   sella_davidson_hvp   sella_davidson with this operator as a third operator kind next to the resident matrix and the
 *                        host callback: the iteration hands the operator the device addresses of its vector and of the
 *                        product; no copy, no wait and no callback frame per product.  Arguments from Pvecs on as
 *                        sella_davidson's (n: the operator's m); same synchronous iteration, same results as
 *                        sella_davidson over sella_hvp_matvec.
 * Every product of a non-vanishing vector is remembered, vfull and H vfull in full length (pinned rows included), on the
 * device in chunks that are added as products arrive; sella_hvp_pairs returns them like sella_fd_pairs, (n x k) row-major,
 * k = sella_hvp_npairs.  |v| < 1e-12 gives a zero product, counts as a call (sella_hvp_calls) and is not recorded.
 * Block products — up to 16 vectors, the rows of a panel, through the batched kernels on the same resident state (emt: the
 * pair geometry of a visit is evaluated once for all rows; model: A and the rows u_j streamed once on the matrix cores):
 *   sella_hvp_apply_block      HV (k x m, host) = the products of the rows of V (k x m, host), any k >= 1, in chunks of 16.
 *   sella_davidson_block_hvp   sella_davidson_block (above: the block method, its preconditioners, start block, stopping
 *                        rule |r| <= tol |theta|, thick restarts and outputs; no counterpart in the reference, whose
 *                        rayleigh_ritz adds one vector per iteration, sella/eigensolvers.py:111-112; converged pairs equal
 *                        those of exact(), sella/eigensolvers.py:9-28) with this operator in place of the resident matrix:
 *                        the lowest eigenpairs without n x n storage.  Arguments from Pvecs on as sella_davidson_block's,
 *                        n is the operator's m, one rank (no gather); the panels are round_up(m, 8) apart.  *nmatvec counts
 *                        every row the operator was applied to (= the growth of sella_hvp_calls).  SELLA_E_INVALID: a null
 *                        or foreign op, nev <= 0, nev > m, block < 1 or > 16, nv0 > 16, Pvecs / PvecsT not m x m.  The
 *                        operator must outlive the call; the re-entrancy contract above applies.
 *   sella_hvp_diag       diag(H)[idx] (m, host) at the operator's geometry — the diagonal preconditioner of the block method.
 *                        Neither a force call nor a product (sella_hvp_calls unchanged).
 * A block product is nh calls, is NOT entered in the pair record (the record feeds the secant update of PES.diag) and has no
 * vanishing-vector rule: a zero row gives a zero row.
 * The operator must be destroyed before its calculator and context.  SELLA_E_INVALID: a null pointer, n != sella_calc_dim,
 * m <= 0 or m > n with idx given, idx not ascending, an m (sella_hvp_matvec) / n (sella_davidson_hvp) that is not the
 * operator's.
 * A second kind of the same operator, for the EMT calculator in a cell run (sella_hvp_create_cell): the analytic Hessian of
 * positions and cell in the coordinates [x; p], x the n Cartesian coordinates and p the mc parameters of the cell (the masked
 * log-deformation of CellCartesianPES), resident at the geometry (x0, cell; lattice vectors in the rows of cell).  What the
 * parametrisation contributes depends on the geometry only and is handed over at creation: J = dC.ravel()/dp (9 x mc,
 * row-major), G (mc x mc, symmetric: the first derivative dE/dC contracted with the second derivative of C(p)) and, with a
 * scalar pressure, P = p d2|det C|/dC2 (9 x 9; NULL: none).  For a vector [v_x; v_p]: W = J v_p is the variation of the cell,
 * [y_x; y_C] the product of the Hessian in [x; C.ravel()] with [v_x; W] (the pair passes of sella_emt_cell_hvp on the
 * resident state: nothing uploaded, no density pass per product), and y_p = J^T (y_C + P W) + G v_p.  idx selects the mx free
 * POSITION coordinates (ascending; NULL: all n); the cell parameters are always free and stand behind them, so the
 * eigensolver's dimension is m = (idx ? mx : n) + mc, and the full dimension (the rows of sella_hvp_pairs) is n + mc:
 * [vfull_x; v_p] and its product.  Every entry above means on this kind what it means on the first: single products are
 * recorded, |[v_x; v_p]| < 1e-12 gives a zero product that is counted and not recorded, block products (four rows per
 * workgroup, a row's result independent of its slot, of the number of rows and of the other rows) are counted and not
 * recorded, sella_hvp_diag returns diag(H_xx)[idx] followed by the mc diagonal entries of J^T (H_CC + P) J + G (from one
 * block product of unit rows that is not counted), and both Davidson drivers take it unchanged.  SELLA_E_INVALID: a null
 * pointer (P excepted), a calculator that is not the EMT kind (the message names the kind), n != sella_calc_dim, mc < 1 or mc > 9, idx not ascending or
 * out of range, a singular cell, a shift of the calculator that is no lattice translation of `cell`.                       */
typedef struct sella_hvp sella_hvp;
int sella_hvp_create(sella_calc* calc, int n, const double* x0, const int* idx, int m, sella_hvp** op);
int sella_hvp_create_cell(sella_calc* calc, int n, const double* x0, const double* cell /* 9 */, const int* idx, int mx,
                          int mc, const double* J /* 9 x mc */, const double* G /* mc x mc */, const double* P /* 9 x 9 or NULL */,
                          sella_hvp** op);
int sella_hvp_matvec(void* op, const double* v, double* Av, int m);
int sella_hvp_npairs(sella_hvp* op);
long sella_hvp_calls(sella_hvp* op);
int sella_hvp_pairs(sella_hvp* op, double* Vs, double* AVs);
int sella_hvp_destroy(sella_hvp* op);
int sella_davidson_hvp(sella_ctx* ctx, sella_hvp* op,
                       sella_mat Pvecs, sella_mat PvecsT, const double* pevals, double pscale,
                       int n, const double* v0, int nv0, double gamma, int method, int maxiter,
                       const double* vref, double vreftol,
                       double* lams, double* V, double* AV, int* k, int* nmatvec);
int sella_hvp_apply_block(sella_hvp* op, const double* V, int k, double* HV);
int sella_hvp_diag(sella_hvp* op, double* diag);
int sella_davidson_block_hvp(sella_ctx* ctx, sella_hvp* op, sella_mat Pvecs, sella_mat PvecsT,
                             const double* pevals, const double* diag, const double* V0, int nv0, int nev,
                             int block, int maxvec, double tol, int maxiter, double* lams, double* V,
                             double* res, int* niter, int* nmatvec, int* nconv);

/* ---- a whole search in the library --------------------------------------------------------------------------- */
/* `Sella(atoms, ...).run(fmax, steps)` (sella/optimize/optimize.py:42-440 under ASE's Optimizer.irun) for the
 * configuration an ensemble of independent searches consists of (BASELINE configs[3]): Cartesian PES, no constraints or
 * pinned coordinates (idx / m: the free ones), a calculator of the library (sella_calc_*), TS-BFGS, structured
 * approximate Hessian, built-in step family and measure, eig = True.  The loop is the reference's — first-use
 * diagonalisation (:318-326), restricted step, kick, re-diagonalisation rule (:363-378), trust-radius rule (:413-434),
 * convergence on the largest per-atom projected force (peswrapper.py:438-441) — made of the entry points above
 * (sella_davidson over sella_fd_matvec, sella_update_h_lr, sella_lr_restrict, sella_opt_step); the host language is not
 * entered between creation and return, so one host thread per replica can drive one GPU.  SELLA_E_UNSUPPORTED: the
 * search left the covered configuration (explicit rank beyond 0.4 n, ...): the caller continues with the general driver.
 *   cons: 0 trust region (delta0 = per-coordinate radius x free coordinates, optimize.py:183-186), 1 per-atom measure.  */
typedef struct sella_search sella_search;
typedef struct sella_search_params_t {
    int order, eig, threepoint, dav_method, stepper_kind, cons, update_method, symm, nsteps_per_diag;
    long diag_every_n;                         /* < 0: never */
    double eta, gamma, delta0, delta_min, sigma_inc, sigma_dec, rho_inc, rho_dec;
} sella_search_params_t;
int sella_search_create(sella_ctx* ctx, sella_calc* calc, int n, const double* x0, const int* idx, int m,
                        const sella_search_params_t* params, sella_search** search);
/* energy and gradient (dE/dx, n) at the starting point, if the caller evaluated them already (counts as a force call) */
int sella_search_seed(sella_search* search, double energy, const double* grad);
int sella_search_run(sella_search* search, double fmax, long steps, int* converged);
/* After SELLA_E_UNSUPPORTED: the block of secant pairs of a diagonalisation that no longer fitted the structured form (its
 * force calls are spent and counted; when an optimizer step scheduled the diagonalisation, that step has moved the geometry
 * and is counted): *k pairs (0: none pending), Sm and Ym (n x k row-major; NULL: only the count).  The caller applies them
 * as one block update of the approximate Hessian it takes over (sella/linalg.py:274-304) and is then exactly where the
 * reference is after PES.diag (sella/peswrapper.py:545-553).  Two hand-overs leave the geometry where it was and count
 * no step: k = 0 (the capacity check in front of a step), and the FIRST-USE diagonalisation of a search (k > 0 with
 * counters[0] == 0: optimize.py:318-326 runs it before the first step is taken).                                       */
int sella_search_pending_pairs(sella_search* search, int* k, double* Sm, double* Ym);
/* x, g (n each, may be NULL); scalars[5] = f, fmax, delta, rho, lowest eigenvalue of the approximate Hessian;
 * counters[6] = optimizer steps, force calls, one-call steps, explicit rank, explicit rank of the view (-1: none),
 * first-use diagonalisation done (0 / 1)                                                                              */
int sella_search_state(sella_search* search, double* x, double* g, double* scalars, long* counters);
/* Hand the approximate Hessian over to the caller, who continues with the general driver: the matrix handles change owner
 * (the search cannot be run again).  mats[4] = B, Wt, Bsub, Wt_sub (SELLA_NO_MAT where absent); ints[8] = r (-1: no
 * Hessian yet), r_sub (-1: no view), rows of Wt, rows of Wt_sub, B_stale, Bsub_stale (the dense matrices lag behind the
 * decompositions: sella_lr_materialize), steps since the last diagonalisation, first_diag; mu / mu_sub: `rows` entries.  */
int sella_search_release_hessian(sella_search* search, sella_mat* mats, long* ints, double* mu, double* mu_sub,
                                 double* lam0);
int sella_search_destroy(sella_search* search);
sella_ctx* sella_search_ctx(sella_search* search);        /* the context the search lives on */

/* ---- cohorts: the replica dimension of the ensemble (BASELINE configs[3]) ------------------------- */
/* The reference's ensemble members are independent `Sella` objects (sella/optimize/optimize.py:42-81, 359-440).  A cohort
 * advances up to 16 of them on ONE GPU in lockstep from ONE host thread: every member keeps its own context (memory,
 * rings, scratch), but while the cohort runs the members share one stream, every kernel of the step is launched ONCE for
 * all members that have reached it (the member is the grid's z index, its arguments a by-value descriptor array), and
 * every wait is one stream synchronisation for all of them.  Members whose control flow differs (a further round of the
 * root search, a re-diagonalisation) form launches of their own and rejoin at the next step boundary.  A member's results
 * are bit-identical to sella_search_run on its own.
 *   sella_cohort_create: `members` = n distinct contexts of one device (1 <= n <= 16), each in no other cohort; they stay
 *     usable on their own between runs.  Destroy the cohort before its contexts.
 *   sella_cohort_run_searches: searches[i] lives on member context i (NULL: empty slot); converged[i] / status[i] are what
 *     sella_search_run(searches[i], fmax, steps, ...) would have returned (SELLA_E_UNSUPPORTED: that member left the
 *     covered configuration, see sella_search_pending_pairs); sella_cohort_error(cohort, i) is its message.
 *   sella_cohort_stats: counters[8] = scheduler rounds, launches asked for by the members, launches issued (merged),
 *     waits asked for, stream synchronisations, barrier arrivals, microseconds spent inside the members' host code,
 *     microseconds spent issuing the merged launches — accumulated since creation.                                     */
typedef struct sella_cohort sella_cohort;
int sella_cohort_create(sella_ctx* const* members, int n, sella_cohort** cohort);
int sella_cohort_size(sella_cohort* cohort);
int sella_cohort_run_searches(sella_cohort* cohort, sella_search* const* searches, int n, double fmax, long steps,
                              int* converged, int* status);
/* on != 0: the members' host code between their launches runs on a worker thread each instead of on fibers of the calling
 * thread (parallel host code; the launches are still merged and issued by the caller of sella_cohort_run_searches); width + 1
 * cores spin per cohort while it runs.  Results do not depend on the mode.                                            */
int sella_cohort_member_threads(sella_cohort* cohort, int on);
int sella_cohort_stats(sella_cohort* cohort, long* counters);
const char* sella_cohort_error(sella_cohort* cohort, int member);
int sella_cohort_destroy(sella_cohort* cohort);

/* ---- profiling hooks (bench.py roofline leg) ---------------------------------------------- */
/* When enabled, every launch of the big streaming kernels is bracketed by hipEvents on the
 * context stream.  kind: 0 = row-panel matvec (n x n streams), 1 = gemm, 2 = update, 3 = other,
 * 4 = small matvecs (panel dots), 5 = trailing-matrix matvec of the tridiagonalisation (eigh).     */
int sella_prof_enable(sella_ctx* ctx, int on);
int sella_prof_reset(sella_ctx* ctx);
int sella_prof_get(sella_ctx* ctx, int kind, long* launches, double* total_ms,
                   double* total_bytes, double* total_flops);

#ifdef __cplusplus
}
#endif
#endif /* SELLA_HIP_H */
