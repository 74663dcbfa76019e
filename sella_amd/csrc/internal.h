// internal.h — shared declarations of libsella_hip (context, device matrices, kernel launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <deque>
#include <map>
#include <string>
#include <vector>

#include "../../include/sella_hip.h"

#define SELLA_HD __host__ __device__
#include "small_linalg.h"
#include "cohort.h"

// "this value is in a register from here on": an empty statement the compiler cannot look through.  Placed behind a batch
// of loads it keeps them unconditional and in flight together — otherwise a load whose only use sits behind a condition is
// sunk behind that condition (and the wait for it with everything issued before it).
// SELLA_ARG(x): the same for a kernel argument (uniform): all arguments named at the top of a kernel are fetched by one
// batch of scalar loads instead of one dependent fetch per branch that first needs them.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(SELLA_NO_ARG_BATCH)
#define SELLA_PIN(x) asm volatile("" : "+v"(x))
#define SELLA_ARG(x) asm volatile("" : : "s"(x))
#elif defined(__HIP_DEVICE_COMPILE__)
#define SELLA_PIN(x) asm volatile("" : "+v"(x))
#define SELLA_ARG(x) ((void)0)
#else
#define SELLA_PIN(x) ((void)0)
#define SELLA_ARG(x) ((void)0)
#endif

namespace sella {

// ---- wave64 sum, every lane gets the result -------------------------------------------------------
// Four DPP steps (two quad permutes, half-row mirror, row mirror: VALU-rate cross-lane moves inside
// rows of 16 lanes) and four v_readlane for the rows.  `__shfl_xor` on a double lowers to a pair of
// ds_bpermute_b32 per step, six dependent LDS round trips — the reductions were a visible part of the
// 4.5 us floor of the latency-bound kernels.  All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ double wave_dpp_add(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_readlane(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                            __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double wave_sum64(double v) {
    v = wave_dpp_add<0xB1>(v);          // quad_perm [1,0,3,2]
    v = wave_dpp_add<0x4E>(v);          // quad_perm [2,3,0,1]
    v = wave_dpp_add<0x141>(v);         // row_half_mirror
    v = wave_dpp_add<0x140>(v);         // row_mirror
    return (wave_readlane(v, 0) + wave_readlane(v, 16)) + (wave_readlane(v, 32) + wave_readlane(v, 48));
}

void set_error(const char* fmt, ...);

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            sella::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),        \
                             __FILE__, __LINE__);                                          \
            return SELLA_E_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define SCHK(expr)                                                                         \
    do {                                                                                   \
        int s_ = (expr);                                                                   \
        if (s_ != SELLA_OK) return s_;                                                     \
    } while (0)

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
static inline long round_up_l(long x, long m) { return (x + m - 1) / m * m; }

// Device matrix, row-major, leading dimension padded to a multiple of 8 doubles (64 B) with
// the padding kept at zero, so 16-byte vector loads never straddle a row and never see NaNs.
struct Mat {
    double* d = nullptr;
    int rows = 0, cols = 0, ld = 0;
    bool live = false;
};

enum ProfKind { PROF_GEMV = 0, PROF_GEMM = 1, PROF_UPDATE = 2, PROF_OTHER = 3, PROF_GEMV_SMALL = 4, PROF_TRD_GEMV = 5,
                PROF_NKIND = 6 };

struct ProfPending {
    hipEvent_t a, b;
    int kind;
    double bytes, flops;
};

struct ProfSlot {
    long launches = 0;
    double ms = 0, bytes = 0, flops = 0;
};

// the tuning options of a context, written by sella_ctx_set_option only: options.h is the list
struct Options {
#define SELLA_OPTION(name, dflt, rule) long name = dflt;
#include "options.h"
#undef SELLA_OPTION
};

}  // namespace sella

struct sella_cohort;
struct sella_search;
extern "C" sella_ctx* sella_search_ctx(sella_search* search);

struct sella_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // member of a cohort (cohort.h): while the cohort is being advanced, `stream` is the cohort's stream, batchable
    // launches are parked and merged across the members, and every wait is one synchronisation for all of them
    sella_cohort* cohort = nullptr;
    unsigned long long cohort_phase = 0;       // (optimizer step << 8 | stage) of the member, the high part of its barrier keys
    // Handle table.  A deque: push_back never moves existing elements, so a `Mat*` obtained from mat_get stays valid
    // while the handle is live, even when a host callback (sella_matvec_fn / sella_allgather_fn) re-enters the library
    // and creates matrices.  (It was a std::vector until round 3: a reallocation inside the Davidson callback left
    // the solver reading a freed Mat.)
    std::deque<sella::Mat> mats;
    // small exchange buffers: device scalars + pinned host mirror
    double* dscal = nullptr;
    double* hscal = nullptr;
    int nscal = 0;
    int hscal_hold = 0;             // running calls that need host-visible scalars for their own length (host_scalars())
    // Device allocator: blocks are carved out of a few large arenas and recycled through per-size free
    // lists.  A single hipMalloc was measured at 40-80 ms on this stack whenever the driver has to map new
    // memory, and hipFree synchronises the device; an optimizer loop (or every new member of an ensemble)
    // allocates the same few sizes over and over.  One stream per context, so a recycled block is always
    // used after its last reader.  Arenas are only returned when the context is destroyed.
    struct Arena {
        char* base;
        size_t size, used;
    };
    std::vector<Arena> arenas;
    std::map<size_t, std::vector<void*>> pool;
    // pooled scratch (grown on demand, never shrunk)
    std::vector<std::pair<double*, size_t>> scratch;   // slot -> (ptr, bytes)
    sella::Options opt;
    bool prof = false;
    hipEvent_t prof_a = nullptr, prof_b = nullptr;   // events of the launch being profiled
    std::vector<sella::ProfPending> pending;
    sella::ProfSlot slots[sella::PROF_NKIND];
    char name[256] = {0};
    int num_cu = 256;
    // pinned host staging for bursts of small transfers (divide & conquer levels): pageable copies are
    // synchronous staged copies, ~20 us each with the queue empty
    void* hstage = nullptr;
    size_t hstage_bytes = 0;
    char* hring = nullptr;          // pinned ring behind h2d_async
    size_t hring_bytes = 0, hring_pos = 0;
    // pinned ring behind d2h_async: device -> CALLER memory without a pageable (runtime-staged, process-serialising)
    // copy; the payload lands in the ring and is handed to its destination by stream_wait()
    char* dring = nullptr;
    size_t dring_bytes = 0, dring_pos = 0;
    struct PendingD2H { void* dst; const char* slot; size_t bytes; size_t dpitch, width, rows; };
    std::vector<PendingD2H> d2h_pending;
    std::vector<double> hbuf_a, hbuf_b;             // host work vectors of sella_opt_step (optstep.hip)
    // Re-entrancy: the working state a library call may leave LIVE across a host callback (scalar exchange buffers,
    // pooled scratch slots, pinned staging, host work vectors) exists once per call depth.  callback_enter parks the
    // caller's set and installs the set of the next depth (created on first use); callback_leave restores it.  So a
    // callback may call ANY entry point of the library on the same context without touching what the interrupted
    // call still needs.
    struct Frame {
        double* dscal = nullptr;
        double* hscal = nullptr;
        std::vector<std::pair<double*, size_t>> scratch;
        void* hstage = nullptr;
        size_t hstage_bytes = 0;
        std::vector<double> hbuf_a, hbuf_b;
    };
    // second stream for work that is independent of the main chain for a while (the view job of the one-call optimizer
    // step, lrstep.hip): forked and joined with events, so every wait on `stream` still covers it
    hipStream_t stream2 = nullptr;
    hipStream_t stream_main = nullptr;         // == stream except while a job is being queued on stream2
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    unsigned long long* poll_word = nullptr;   // pinned sequence word of polled waits (davidson.hip, dav_poll) and its last value
    unsigned long long poll_seq = 0;
    unsigned* poll_count = nullptr;            // device counter of poll_arm (zero between uses)
    bool stream2_detached = false;             // stream2 runs work no wait of the main chain has to cover (eigh.hip, WY factors)
    std::deque<Frame> frames;      // frames[d] = parked state of depth d (d != depth)
    int depth = 0;
};

namespace sella {

// ---- context helpers (context.hip) ------------------------------------------------------
int mat_new(sella_ctx* c, int rows, int cols, sella_mat* h);       // zero-initialised
// Bracket EVERY invocation of a host callback with these (see sella_ctx::Frame); CallbackScope does it by scope.
int callback_enter(sella_ctx* c);
void callback_leave(sella_ctx* c);
struct CallbackScope {
    sella_ctx* c;
    int status;
    explicit CallbackScope(sella_ctx* ctx) : c(ctx), status(callback_enter(ctx)) {}
    ~CallbackScope() { if (status == SELLA_OK) callback_leave(c); }
    CallbackScope(const CallbackScope&) = delete;
    CallbackScope& operator=(const CallbackScope&) = delete;
};
Mat* mat_get(sella_ctx* c, sella_mat h);
int scratch_get(sella_ctx* c, int slot, size_t bytes, double** p); // persistent scratch slot
int host_stage(sella_ctx* c, size_t bytes, void** p);               // pinned host staging buffer (grown on demand)
int dev_alloc(sella_ctx* c, size_t bytes, double** p);             // caching allocator (contents undefined)
void dev_free(sella_ctx* c, double* p, size_t bytes);
int upload_panel(sella_ctx* c, const double* X, int n, int k, double* dpanel, int ldp);   // (n x k) host -> k rows
int download_panel(sella_ctx* c, const double* dpanel, int ldp, int n, int k, double* X); // k rows -> (n x k) host
int h2d_async(sella_ctx* c, void* dst, const void* src, size_t bytes);   // caller memory -> device, no wait (pinned ring)
int h2d_pinned(sella_ctx* c, void* dst, const void* pinned_src, size_t bytes);   // pinned source of the caller: by kernel from 16 KB on (h2d_kernel_min)
int h2d_begin(sella_ctx* c, size_t bytes, void** slot);                   // pinned slot (zeroed) for the caller to compose in ...
int h2d_end(sella_ctx* c, void* dst, const void* slot, size_t bytes);     // ... and its transfer queued
// device -> caller memory through the pinned ring: `dst` is valid after the next stream_wait(c).  The 2-D form copies
// `rows` rows of `width` bytes from a device pitch `spitch` into a dense destination.
int d2h_async(sella_ctx* c, void* dst, const void* src_dev, size_t bytes);
int d2h_async_2d(sella_ctx* c, void* dst, const void* src_dev, size_t spitch, size_t width, size_t rows);
// THE wait of the library: stream synchronisation, then the queued device-to-host payloads are delivered and both
// pinned rings rewound.  Every host-side wait goes through here (never hipStreamSynchronize directly).
// Stream-ordered copies and zero-fills of the library.  Outside a cohort they ARE the runtime's hipMemcpyAsync /
// hipMemsetAsync on the context's stream; on a member fiber of a cohort they are batchable kernels like every other launch
// of the step (one launch for all members instead of one runtime blit per member) whenever both sides are visible to the
// device — `host_pinned` says that the host side of an H2D / D2H copy is pinned (hipHostMalloc) memory.
hipError_t s_memcpy(sella_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, bool host_pinned = false);
hipError_t s_memcpy2d(sella_ctx* c, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows,
                      hipMemcpyKind kind, bool host_pinned = false);
hipError_t s_memset0(sella_ctx* c, void* dst, size_t bytes, const char* file = __builtin_FILE(), int line = __builtin_LINE());
int stream_wait(sella_ctx* c);
int stream_sync_raw(sella_ctx* c);                                  // the synchronisation alone (nothing delivered, rings kept)
int event_wait(sella_ctx* c, hipEvent_t ev);
// Polled wait: poll_mark queues a one-thread kernel that stores the next sequence number into a pinned word behind
// everything queued so far; poll_wait spins on that word (a cohort member parks instead).  What kernels in front of the mark
// stored into pinned host memory is visible when the word is.
int poll_mark(sella_ctx* c);
// the same without the extra kernel: the LAST workgroup of the caller's kernel publishes `seq` to `*word` (pinned) after
// counting itself on `*count` (device, zero between uses); on a member fiber of a cohort all three come back null / 0
int poll_arm(sella_ctx* c, unsigned long long** word, unsigned long long* seq, unsigned** count);
int poll_wait(sella_ctx* c);                        // wait for an event recorded on the context's stream
int read_scalars(sella_ctx* c, int offset, int count);             // dscal -> hscal (sync)
// Where a kernel should put scalars that only the HOST consumes next: with host_scalars(c) — the option,
// or a call that holds it on for its own length (sella_davidson's polled waits) — the pinned,
// device-visible host mirror itself (zero-copy: the readback is then just the stream synchronisation and the
// 4 us copy launch disappears from the critical path); otherwise the device buffer.
inline bool host_scalars(const sella_ctx* c) { return c->opt.host_scalars || c->hscal_hold > 0; }
double* scal_out(sella_ctx* c, int offset);
int sync_scalars(sella_ctx* c, int offset, int count);             // makes hscal[offset, offset+count) valid
// layout of the scalar exchange buffer (doubles)
enum { DS_MISC = 0, DS_CVEC = 16384, DS_STAGE = 32768, DS_GRAM = 65536, DS_TOTAL = 131072 };
// Profiling (bench.py roofline leg): prof_begin creates an event pair, the launch between begin and
// end must go through SELLA_LAUNCH, which attaches the pair to the kernel's own dispatch packet
// (hipExtLaunchKernelGGL) so that the elapsed time is the kernel's execution time — the same
// start/end timestamps rocprofv3 reports — and not the distance between two stream markers.
void prof_begin(sella_ctx* c, int kind, double bytes, double flops);
void prof_end(sella_ctx* c);
int prof_flush(sella_ctx* c);
#define SELLA_LAUNCH(c, kernel, grid, block, shmem, ...)                                             \
    do {                                                                                             \
        if ((c)->prof_a)                                                                             \
            hipExtLaunchKernelGGL((kernel), grid, block, shmem, (c)->stream, (c)->prof_a,            \
                                  (c)->prof_b, 0, __VA_ARGS__);                                                   \
        else                                                                                         \
            hipLaunchKernelGGL((kernel), grid, block, shmem, (c)->stream, __VA_ARGS__);              \
    } while (0)

// the same for a kernel with a batchable body (cohort.h): parked and merged on a member fiber of a cohort
#define SELLA_BODY(...) __VA_ARGS__
#define SELLA_LAUNCHB_PROF(c, kernel, body, LB, grid, block, shmem, ...)                                     \
    do {                                                                                                     \
        if ((c)->cohort && sella::cohort_in_fiber())                                                         \
            sella::cohort_launch<body, LB>((c), #body, dim3(grid), dim3(block), (size_t)(shmem), __VA_ARGS__); \
        else                                                                                                 \
            SELLA_LAUNCH(c, (kernel), grid, block, shmem, __VA_ARGS__);                                      \
    } while (0)

enum ScratchSlot {
    SCR_X = 0, SCR_Y, SCR_PART, SCR_V, SCR_AV, SCR_V2, SCR_AV2, SCR_R, SCR_T, SCR_W, SCR_C,
    SCR_EIG0, SCR_EIG1, SCR_EIG2, SCR_EIG3, SCR_EIG4, SCR_EIG5, SCR_EIG6, SCR_UPD0, SCR_UPD1, SCR_UPD2,
    SCR_UPD3, SCR_UPD4, SCR_QR0, SCR_QR1, SCR_STEP0, SCR_STEP1, SCR_STEP2, SCR_MISC0, SCR_MISC1, SCR_PSMALL, SCR_SYMV, SCR_NSLOTS
};

// ---- kernel launchers (kernels.hip) -------------------------------------------------------
// Epilogue of the row-panel matvec.
struct GemvEpi {
    int mode = 0;            // 0: y = alpha*acc; 1: y = alpha*acc/(dvec[i]-theta); 2: y = alpha*acc + beta*y;
                             // 3: * |dvec[i]|; 4: * dvec[i]; 5: * (1/(dvec[i]-theta) - beta)
    const double* dvec = nullptr;
    double theta = 0, alpha = 1, beta = 0;
};
// right-hand sides of the row-panel matvec as up to 8 independent vectors
struct GemvX {
    const double* p[8];
};
// Y[h*ldy + i] = epi(sum_j A[i*lda + j] * X[h*ldx + j]),  i < rows, j < cols, h < nrhs (<= 8).
// A must be 16-byte aligned with even lda; X rows must be readable up to round_up(cols, 2).
int launch_gemv_rows(sella_ctx* c, const double* A, int rows, int cols, int lda, const double* X,
                     int ldx, int nrhs, double* Y, int ldy, const GemvEpi& epi);
// same with the right-hand sides given as separate pointers (no contiguity requirement)
int launch_gemv_rows_xp(sella_ctx* c, const double* A, int rows, int cols, int lda,
                        const double* const* xs, int nrhs, double* Y, int ldy, const GemvEpi& epi);
// y = A x and y2 = A2 x in ONE launch (two row sources, one right-hand side): the speculative A t and the panel dots
// V t of the Davidson chain share a launch boundary
int launch_gemv_rows2(sella_ctx* c, const double* A, int rows, int lda, const double* A2, int rows2, int lda2, int cols,
                      const double* x, double* y, double* y2);
// Y (nrhs <= 16 rows, vector-major) = A X^T on the matrix cores; Xp: 16-row panel with leading dimension lda,
// rows beyond nrhs and the row padding zero
int launch_panel16(sella_ctx* c, const double* A, int rows, int cols, int lda, const double* Xp, int nrhs,
                   double* Y, int ldy);
int launch_panel16_marked(sella_ctx* c, const double* A, int rows, int cols, int lda, const double* Xp, int nrhs, double* Y,
                          int ldy);                  // ... and publishes the sequence word of a polled wait behind it
// |x|^2 -> out[0]; x <- x/|x|   (one single-workgroup launch)
int launch_normalize(sella_ctx* c, double* x, int n, double* out);
// Y[h*ldy + j] = sum_i A[i*lda + j] * X[h*ldx + i]   (transposed product, deterministic 2-pass)
int launch_gemv_cols(sella_ctx* c, const double* A, int rows, int cols, int lda, const double* X,
                     int ldx, int nrhs, double* Y, int ldy);
// out[cidx*ldo + i] = beta * out[..] + sum_j W1[j*ldw1 + cidx] P1[j*ldp1 + i]
//                                   + sum_j W2[j*ldw2 + cidx] P2[j*ldp2 + i]
// W1/W2 are DEVICE pointers (k1 x nout, k2 x nout); P2 may be null.
int launch_lincomb(sella_ctx* c, int n, int nout, const double* P1, int ldp1, int k1,
                   const double* W1, int ldw1, const double* P2, int ldp2, int k2,
                   const double* W2, int ldw2, double beta, double* out, int ldo);
// out[r] = sum_i P[r*ldp + i]^2
int launch_rows_sumsq(sella_ctx* c, const double* P, int ldp, int nrows, int n, double* out);
// x[i] *= f(scal[0]) : mode 0 -> 1/sqrt(s), 1 -> 1/s, 2 -> s
int launch_scale_by(sella_ctx* c, double* x, int n, const double* scal, int mode);
// t = -x + y * (dots[0]/dots[1])  (|dots[1]| < 1e-12 -> t = x), eigensolvers.py:123-139
int launch_jd_combine(sella_ctx* c, const double* x, const double* y, const double* dots,
                      double* t, int n);
// generic elementwise z = a*x + b*y (y may be null)
int launch_axpby(sella_ctx* c, int n, double a, const double* x, double b, const double* y,
                 double* z);
// 2-D: C[i*ldc + j] = a*A[i*lda + j] + b*B[i*ldb + j]
int launch_axpby2d(sella_ctx* c, int rows, int cols, double a, const double* A, int lda, double b,
                   const double* B, int ldb, double* C, int ldc);
int launch_transpose(sella_ctx* c, const double* A, int rows, int cols, int lda, double* At,
                     int ldat);
// C = alpha * op(A) op(B) + beta * C ; op(X) = X or X^T; M,N,K are the product dimensions.
int launch_gemm(sella_ctx* c, int transA, int transB, int M, int N, int K, double alpha,
                const double* A, int lda, const double* B, int ldb, double beta, double* C,
                int ldc);
// B[i][j] = 0.5*(B[i][j] + B[j][i]) in place (square)
int launch_symmetrize(sella_ctx* c, double* B, int n, int ld);
// gs.hip: orthonormalise t (n) against k orthonormal rows of a vector-major panel
int gs_orthonormalise(sella_ctx* c, const double* basis, int ldb, int k, double* t, int n,
                      double eps1, double eps2, int maxiter, int* kept, double* first_norm);
// two sweeps + normalisation without a host round trip: |t|^2 before / after sweep 1 / after sweep 2 -> scalar slots 8..10
int gs_project_twice(sella_ctx* c, const double* basis, int ldb, int k, double* t, int n);
// B <- (B + B^T)/2 + alpha * sum_a (U_a Z_a^T + Z_a U_a^T), U/Z vector-major panels with kk rows
int launch_sym_rank2k(sella_ctx* c, double* B, int n, int ld, const double* Up, const double* Zp,
                      int ldp, int kk, double alpha = 1.0);
// C <- C + alpha sum_a (U_a Z_a^T + Z_a U_a^T) for an ALREADY symmetric block, as a pure stream (no mirror tile; the two
// triangles agree to roundoff, not bitwise): the trailing update of the tridiagonalisation
int launch_rank2k_stream(sella_ctx* c, double* C, int m, int ld, const double* Up, const double* Zp, int ldp, int kk,
                         double alpha, bool upper_only = false);
// The same update of the full block, carrying the panel seam of the blocked tridiagonalisation: the workgroups that own
// row 0 of the updated block also leave it in u[0 .. m), its leading entry in d[0] and one partial of its sum of squares over
// the columns >= 2 per tile column in partA[0 .. *npart) — what the first row launch of the next panel would have computed.
// Needs the streaming kernels (ld even, C 16-byte aligned: SELLA_E_INVALID otherwise).
struct Rank2kSeam { double* u; double* d; double* partA; };
int launch_rank2k_stream_seam(sella_ctx* c, double* C, int m, int ld, const double* Up, const double* Zp, int ldp, int kk,
                              double alpha, const Rank2kSeam& seam, int* npart);
int launch_mirror_upper(sella_ctx* c, double* C, int m, int ld);      // lower triangle <- transpose of the upper one
// eigh.hip: eigendecomposition (w host ascending, Vt rows / V columns, both updated in place) of
// B + sum_a (U_a Z_a^T + Z_a U_a^T) from that of B; *nrank1 = rank-one modifications applied
int eig_lowrank_update(sella_ctx* c, int n, double* w, Mat* V, Mat* Vt, const double* Up, const double* Zp,
                       int ldp, int kk, int* nrank1);
// the same for a STRUCTURED eigendecomposition: r explicit eigenpairs (mu ascending, rows of Wt) + the eigenvalue lam0
// on the orthogonal complement of their span; *r_io and mu are updated (r grows by at most one per rank-one term)
int lr_lowrank_update(sella_ctx* c, int n, int* r_io, double* mu, double lam0, Mat* Wt, const double* Up, const double* Zp,
                      int ldp, int kk, int* nrank1);
// internals.hip: internals_kernel<natoms> queued over nc coordinates whose inputs are already on the device (dpos
// (nc, natoms, 3), dtv (nc, natoms-1, 3) or null); q (nc) and grad (nc, 3 natoms) written, hess (nc, 3 natoms, 3 natoms)
// too when not null.  No wait (sella_sparse_int_eval writes straight into the buffers of its topology).
int internals_queue(sella_ctx* c, int natoms, int nc, const double* dpos, const double* dtv, double* dq, double* dgrad,
                    double* dhess);
// sparse_internal.hip: the dimensions of a topology (-1 for a null object)
int sparse_int_ncoords(const sella_sparse_int* s);
int sparse_int_natoms(const sella_sparse_int* s);
// emt.hip: sella_emt_eval with the parameter table and shift vectors optionally resident (dconst: 9 n + 3 nshift doubles);
// virial6 != nullptr: the six summed virial components too (sella_emt_eval_stress)
int emt_eval_resident(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                      const double* dconst, double rc, double acut, double cutoff, double beta, double* energy, double* grad,
                      double* virial6 = nullptr);
int emt_queue(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts, const double* dconst,
              double rc, double acut, double cutoff, double beta, double** eatom, double** grad, bool virial = false);
// emt_hessian.hip: the analytic Hessian of the same potential into `out` (3n x 3n, stays on the device) and its products
// with k host vectors (V, HV: (k, 3n)); dconst as above
int emt_hessian_resident(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                         const double* dconst, double rc, double acut, double cutoff, double beta, sella_mat out);
int emt_hvp_resident(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                     const double* dconst, double rc, double acut, double cutoff, double beta, const double* V, int k, double* HV);
// calc.hip: a force call of a library calculator in two halves, so that what consumes the gradient can be queued behind
// it without a wait in between.  calc_queue: x (host) uploaded, kernels queued; *g_dev = gradient on the device (n),
// *aux_dev / *naux = what the energy is assembled from.  calc_finish: energy from the read-back aux values, after the wait.
int calc_queue(sella_calc* k, const double* x, double** g_dev, double** aux_dev, int* naux);
double calc_finish(sella_calc* k, const double* x, const double* aux_host);
// the analytic Hessian-vector operator (calc.hip, sella_hvp_*) as sella_davidson_hvp sees it: y = (H vfull)[free] for device
// vectors of hvp_dim() entries, queued on the stream of hvp_ctx(), nothing waited for
int hvp_device_apply(sella_hvp* op, const double* x, double* y);
// the same for the nh <= 16 rows of a device panel (m entries each, ldx / ldy apart), as sella_davidson_block_hvp sees it:
// nh calls, not entered in the pair record
int hvp_device_apply_block(sella_hvp* op, const double* X, int ldx, int nh, double* Y, int ldy);
long hvp_calls(const sella_hvp* op);
int hvp_dim(const sella_hvp* op);
sella_ctx* hvp_ctx(const sella_hvp* op);
// stepper.hip: step family on m modes = rows idx[0..m) of a device panel (gathered into matrices the stepper owns)
int stepper_from_panel(sella_ctx* c, int kind, const double* src, int ld, const int* idx, int m, int n, const double* ev,
                       const double* gh, int order, sella_stepper** out);
// the same without copies: the family reads the rows where they are (trust-region measure only; stepper.hip)
int stepper_on_panel(sella_ctx* c, int kind, const double* src, int ld, const int* idx, int m, int n, const double* ev,
                     const double* gh, int order, sella_stepper** out);
void stepper_panel_scale(sella_stepper* st, int mode, double factor);      // mode's row is stored unnormalised: row * factor
// the interpolating batched root search of sella_restricted_step instead of the reference's alpha schedule (sella_opt_step)
void stepper_set_fast_search(sella_stepper* st, bool on, bool boundary_hint = false);
// where the previous root search of the same saddle search ended (its first round looks there) / where this one ended
void stepper_set_alpha_hint(sella_stepper* st, double hint);
double stepper_alpha_found(const sella_stepper* st);
// lrstep.hip: the learn / adapt / propose step on structured decompositions with every decision on the device
// `pipe` (optional): the force call at the new geometry has NOT been made yet — the step queues it on the stream in front
// of the update that consumes its gradient and waits once for both (csrc/search.hip: no host round trip between force call
// and update).  g_out (n) and f receive gradient and energy; a->g_new must point at g_out, a->f_new is set here.
// done == false on return: the step did not qualify before anything was queued, the caller makes the force call itself.
struct CalcPipe {
    sella_calc* calc = nullptr;
    const double* x = nullptr;
    double* g_out = nullptr;
    double f = 0.0;
    bool done = false;
};
int lr_fused_step(sella_ctx* c, sella_opt_step_t* a, bool* handled, CalcPipe* pipe = nullptr);
// optstep.hip: sella_opt_step with the force call inside (see CalcPipe); *f_new receives the energy
int opt_step_with_calc(sella_ctx* c, sella_opt_step_t* a, sella_calc* calc, const double* x, double* g_new, double* f_new,
                       bool* force_call_made = nullptr);
// batched NN GEMM for the merges of one divide-and-conquer level: batch b multiplies the diagonal blocks
// at offset lo_b:  C[lo.., lo..] (K_b x N_b) = A[lo.., lo..] (K_b x K_b) * B[lo.., lo..] (K_b x N_b), all with
// leading dimension ld.  desc (device): 4 ints per batch {lo, N, K, unused}.
int launch_gemm_merge_batched(sella_ctx* c, int nbatch, const int* desc, int maxN, int maxK, const double* A,
                              const double* B, double* C, int ld);
// gather rows: out[r*ldo + j] = in[idx[r]*ldi + j] (idx device int array)
int launch_gather_rows(sella_ctx* c, const double* in, int ldi, const int* idx, int nrows,
                       int ncols, double* out, int ldo);

}  // namespace sella
