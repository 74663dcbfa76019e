// gemv_l2_lab.hip — where do the bytes of the blocked chain's matvec come from?  (stand-alone, not part of the library)
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/lab/bin/gemv_l2_lab tools/lab/gemv_l2_lab.hip
//   tools/lab/bin/gemv_l2_lab [groups = 128] [repeats = 3]           timing table (device events)
//   rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum -d DIR -o l2 --output-format csv -- tools/lab/bin/gemv_l2_lab 2 1
//   python tools/lab/gemv_l2_pmc.py DIR                               hit rate per launch (variant = kernel name's TAG, m from the grid)
//
// A stream shaped like the chain above 1024 trailing rows: groups of 16 dependent pairs {row-pair matvec over an m x m
// block, 12-workgroup stand-in for the row step}, one read-modify-write pass over the block (the rank-2k update's stand-in)
// in front of every group.  Plain loads and stores only.  The matvec is trd_gemv_kernel<NCH>'s load structure: 256 threads,
// two rows per workgroup, every load issued before the first wait.
//
// Variants (TAG):
//   0       parent: workgroup b takes row pair b, default cache policy
//   1, 2    A: every second pass takes the row pairs in descending groups of eight (b & 7, hence the XCD, preserved);
//           1 = the first pass of a group ascends, 2 = the first pass descends (the update's last tiles are what L2 holds)
//   3       every matrix load non-temporal (does `nt` give up the Infinity Cache too?)
//   4..7    B: row pairs with ((P >> 3) & 15) < k default policy, all others non-temporal; k from C = 16, 20, 24, 28 MB
//   8..11   A + B (first pass descends), same C
//   12      every pass descends (control for A: is it the alternation, or the descending order by itself?)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

typedef double d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

template <int NCH, bool NT>
__device__ __forceinline__ void pair_dots(const d2* r0, const d2* r1, const double* x, int n2, double acc[2]) {
    d2 a0[NCH], a1[NCH], xv[NCH];
    const d2* x2 = reinterpret_cast<const d2*>(x);
    // (identical arms are merged into one plain load block and the hint is lost: this keeps the two copies apart)
    if constexpr (NT) asm volatile("; streamed arm" ::: "memory");
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int jk = threadIdx.x + 256 * k;
        const int jc = (jk < n2) ? jk : n2 - 1;                 // clamped address, masked afterwards
        if constexpr (NT) {
            a0[k] = __builtin_nontemporal_load(r0 + jc);
            a1[k] = __builtin_nontemporal_load(r1 + jc);
        } else {
            a0[k] = r0[jc];
            a1[k] = r1[jc];
        }
        xv[k] = x2[jc];
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        asm volatile("" : "+v"(a0[k].x)); asm volatile("" : "+v"(a0[k].y));
        asm volatile("" : "+v"(a1[k].x)); asm volatile("" : "+v"(a1[k].y));
        asm volatile("" : "+v"(xv[k].x)); asm volatile("" : "+v"(xv[k].y));
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const bool has = (int)threadIdx.x + 256 * k < n2;
        acc[0] += has ? a0[k].x * xv[k].x + a0[k].y * xv[k].y : 0.0;
        acc[1] += has ? a1[k].x * xv[k].x + a1[k].y * xv[k].y : 0.0;
    }
}

struct MvArgs {
    const double* A; int ld, m;
    const double* x; double* y; double* part;
    int nslot;                  // row pairs = logical slots
    int rev;                    // this pass takes the slots in descending groups of eight
    int k;                      // resident classes of sixteen (16: every row default policy, 0: every row non-temporal)
};

template <int NCH, int TAG>
__global__ __launch_bounds__(256) void mv_kernel(MvArgs a) {
    __shared__ double red[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int q = a.rev ? ((int)(gridDim.x >> 3) - 1 - (b >> 3)) * 8 + (b & 7) : b;
    if (q >= a.nslot) return;
    const int row0 = 2 * q;
    const int r1 = (row0 + 1 < a.m) ? row0 + 1 : a.m - 1;
    const d2* p0 = reinterpret_cast<const d2*>(a.A + (size_t)row0 * a.ld);
    const d2* p1 = reinterpret_cast<const d2*>(a.A + (size_t)r1 * a.ld);
    const int n2 = a.m >> 1;
    double acc[2] = {0.0, 0.0};
    if (((q >> 3) & 15) < a.k) pair_dots<NCH, false>(p0, p1, a.x, n2, acc);       // uniform per workgroup
    else pair_dots<NCH, true>(p0, p1, a.x, n2, acc);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const double v = wave_sum(acc[r]);
        if (lane == 0) red[wave][r] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double p = 0.0;
        for (int r = 0; r < 2; ++r) {
            const double res = red[0][r] + red[1][r] + red[2][r] + red[3][r];
            if (row0 + r < a.m) { a.y[row0 + r] = res; p += res * a.x[row0 + r]; }
        }
        a.part[q] = p;
    }
}

// stand-in for the row step: 12 workgroups, the next x from y and the partials (a dependent launch between two matvecs)
__global__ __launch_bounds__(256) void row_kernel(const double* y, const double* part, int nslot, double* x, int m) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nslot; i += 256) s += part[i];
    s = wave_sum(s);
    const double sc = (s == s && s != 0.0) ? 1e-3 : 1e-3 + 1e-300;          // keeps the dependence, keeps x bounded
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) x[i] = sc * (0.5 + 1e-3 * y[i] / (1.0 + fabs(y[i])));
}

// stand-in for the trailing update: one read-modify-write pass over the block, ascending
__global__ __launch_bounds__(256) void rmw_kernel(double* A, int ld, int m, const double* x, double eps) {
    const int row = blockIdx.x;
    d2* p = reinterpret_cast<d2*>(A + (size_t)row * ld);
    const double xr = x[row] * eps;
    for (int j = threadIdx.x; j < (m >> 1); j += 256) {
        d2 v = p[j];
        v.x += xr * x[2 * j]; v.y += xr * x[2 * j + 1];
        p[j] = v;
    }
}

struct Variant { const char* name; int sweep; int first_desc; double C; int all_nt; };
static const Variant variants[13] = {
    {"0 parent", 0, 0, 0, 0},       {"A first asc", 1, 0, 0, 0},    {"A first desc", 1, 1, 0, 0},   {"all nt", 0, 0, 0, 1},
    {"B C=16", 0, 0, 16e6, 0},      {"B C=20", 0, 0, 20e6, 0},      {"B C=24", 0, 0, 24e6, 0},      {"B C=28", 0, 0, 28e6, 0},
    {"A+B C=16", 1, 1, 16e6, 0},    {"A+B C=20", 1, 1, 20e6, 0},    {"A+B C=24", 1, 1, 24e6, 0},    {"A+B C=28", 1, 1, 28e6, 0},
    {"always desc", 2, 1, 0, 0},
};

template <int NCH, int TAG> static void launch_mv(int grid, const MvArgs& a) {
    hipLaunchKernelGGL((mv_kernel<NCH, TAG>), dim3(grid), dim3(256), 0, 0, a);
}
template <int NCH> static void launch_tag(int tag, int grid, const MvArgs& a) {
    switch (tag) {
#define T(X) case X: launch_mv<NCH, X>(grid, a); break;
        T(0) T(1) T(2) T(3) T(4) T(5) T(6) T(7) T(8) T(9) T(10) T(11) T(12)
#undef T
    }
}

int main(int argc, char** argv) {
    const int groups = argc > 1 ? atoi(argv[1]) : 128;
    const int reps = argc > 2 ? atoi(argv[2]) : 3;
    const int ms[7] = {1536, 1792, 2048, 2304, 2560, 2816, 3072};
    const int ld = 3072;
    double *A, *x, *y, *part;
    CK(hipMalloc(&A, (size_t)ld * ld * 8)); CK(hipMalloc(&x, ld * 8)); CK(hipMalloc(&y, ld * 8)); CK(hipMalloc(&part, ld * 8));
    std::vector<double> h((size_t)ld * ld);
    for (auto& v : h) v = (double)rand() / RAND_MAX - 0.5;
    CK(hipMemcpy(A, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(x, h.data(), ld * 8, hipMemcpyHostToDevice));
    CK(hipMemset(y, 0, ld * 8)); CK(hipMemset(part, 0, ld * 8));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    printf("groups of 16 pairs per figure: %d (%d pairs); us per pair = (update pass + 16 matvecs + 16 row steps) / 16\n", groups, 16 * groups);
    printf("%-13s", "variant");
    for (int m : ms) printf(" %8d", m);
    printf("\n");
    for (int rep = 0; rep < reps; ++rep) {
        for (int tag = 0; tag < 13; ++tag) {
            const Variant& v = variants[tag];
            printf("%-13s", v.name);
            for (int m : ms) {
                MvArgs a;
                a.A = A; a.ld = ld; a.m = m; a.x = x; a.y = y; a.part = part;
                a.nslot = m / 2;
                const int grid = (a.nslot + 7) / 8 * 8;
                a.k = v.all_nt ? 0 : 16;
                if (v.C > 0) a.k = std::min(16, std::max(0, (int)(16.0 * v.C / (8.0 * m * (double)m) + 0.5)));
                const int nch = ((m / 2 + 255) / 256 + 1) & ~1;
                auto group = [&]() {
                    hipLaunchKernelGGL(rmw_kernel, dim3(m), dim3(256), 0, 0, A, ld, m, x, 0.0);
                    for (int i = 0; i < 16; ++i) {
                        a.rev = v.sweep == 2 ? 1 : v.sweep ? ((i & 1) ^ v.first_desc) : 0;
                        if (nch <= 4) launch_tag<4>(tag, grid, a); else launch_tag<6>(tag, grid, a);
                        hipLaunchKernelGGL(row_kernel, dim3(12), dim3(256), 0, 0, y, part, a.nslot, x, m);
                    }
                };
                group(); group();
                CK(hipEventRecord(e0));
                for (int g = 0; g < groups; ++g) group();
                CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
                CK(hipGetLastError());
                float t; CK(hipEventElapsedTime(&t, e0, e1));
                printf(" %8.3f", 1e3 * t / (16.0 * groups));
            }
            printf("\n");
            fflush(stdout);
        }
        printf("\n");
    }
    printf("k (resident classes of 16):\n");
    for (int tag = 4; tag < 8; ++tag) {
        printf("%-13s", variants[tag].name);
        for (int m : ms) printf(" %8d", std::min(16, (int)(16.0 * variants[tag].C / (8.0 * m * (double)m) + 0.5)));
        printf("\n");
    }
    double chk;
    CK(hipMemcpy(&chk, y, 8, hipMemcpyDeviceToHost));
    printf("y[0] = %g\n", chk);
    return 0;
}
