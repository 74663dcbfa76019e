// emt.hip — effective-medium-theory energy and forces (the calculator on the far side of PES.eval,
// sella/peswrapper.py:413-418).  Functional form and parameter handling of
// ASE's ase/calculators/emt.py (Jacobsen, Stoltze, Norskov, Surf. Sci. 366, 394 (1996)); ASE is not part of
// /root/reference, so this is a restatement of the published algorithm, checked against the NumPy
// restatement in oracle/ and against finite differences of its own energy.
//
// All-pairs formulation: one workgroup per atom sweeps every (neighbour, periodic image) pair inside the
// cutoff — 1024 atoms x 9 images are 9.4 M pair terms per pass, far below anything a neighbour list would
// pay for itself on this device — and reduces in-block, so energies and forces are deterministic (no atomics).
//   pass 1: sigma1_i = sum_j dsigma(i <- j), pair energy of atom i
//           cohesive function, dE/dsigma1_i                           (own density only: at the end of pass 1)
//   pass 2: F_i by gathering both ordered pairs (i <- j) and (j <- i) of every neighbour
#include "emt.h"

namespace sella {
namespace {

__device__ __forceinline__ void emt_density_vb(const VB vb, EmtArgs a) {
    __shared__ double red[4];
    __shared__ int hits[256][EMT_HCAP + 1];
    __shared__ EmtStage stage;
    const int i = vb.x;
    const double xi = a.pos[3 * i], yi = a.pos[3 * i + 1], zi = a.pos[3 * i + 2];
    const double n0i = a.p.n0[i], g1i = a.p.gamma1[i], g2i = a.p.gamma2[i], V0i = a.p.V0[i];
    double sig = 0.0, ep = 0.0;
    auto heavy = [&](int t) {
        const int j = t & 0xffffff, s = t >> 24;
        const double dx = a.pos[3 * j] + a.shifts[3 * s] - xi;
        const double dy = a.pos[3 * j + 1] + a.shifts[3 * s + 1] - yi;
        const double dz = a.pos[3 * j + 2] + a.shifts[3 * s + 2] - zi;
        const double r = sqrt(dx * dx + dy * dy + dz * dz);
        if (r < a.cutoff && r > 1e-8) {
            const double theta = 1.0 / (1.0 + exp(a.acut * (r - a.rc)));
            const double chi = a.p.n0[j] / n0i;
            sig += exp(-a.p.eta2[j] * (r - a.beta * a.p.s0[j])) * chi * theta / g1i;
            ep += 0.5 * V0i * exp(-a.p.kappa[j] * (r / a.beta - a.p.s0[j])) * chi / g2i * theta;
        }
    };
    const int nh = emt_pairs(a, xi, yi, zi, &stage, hits, heavy);
    // the neighbour lists go on to the force kernel (same atom, same thread, same order): count < 0 = incomplete
    {
        int* out = a.nbr + ((size_t)i * 256 + threadIdx.x) * (EMT_HCAP + 1);
        out[0] = nh;
        for (int h = 0; h < nh; ++h) out[1 + h] = hits[threadIdx.x][h];
    }
    sig = block_sum(sig, red);
    ep = block_sum(ep, red);
    if (threadIdx.x == 0) {
        a.sigma1[i] = sig;
        a.epair[i] = -ep;
        // cohesive function and dE/dsigma1 of this atom (own density only: no pass of its own)
        const double ds = -log(sig / 12.0) / (a.beta * a.p.eta2[i]);
        const double xl = a.p.lam[i] * ds, yl = exp(-xl);
        const double z = 6.0 * a.p.V0[i] * exp(-a.p.kappa[i] * ds);
        a.eatom[i] = a.p.E0[i] * ((1.0 + xl) * yl - 1.0) + z + -ep;
        a.dEdsig[i] = (a.p.E0[i] * xl * yl * a.p.lam[i] + z * a.p.kappa[i]) / (sig * a.beta * a.p.eta2[i]);
    }
}
__global__ __launch_bounds__(256) void emt_density_kernel(EmtArgs a) { emt_density_vb(vb_hw(), a); }

// VIRIAL: every thread also accumulates the symmetric virial of the pairs it visits, 1/2 (dE/dr / r) d (x) d per pair
// (each unordered pair is gathered once from either end), and the block writes the six components (xx, yy, zz, yz, xz,
// xy) of its atom to grad + 3 n + 6 i.  VIRIAL = false is the force pass alone.
template <bool VIRIAL>
__device__ __forceinline__ void emt_force_body(const VB vb, EmtArgs a) {
    __shared__ double red[4];
    __shared__ int hits[256][EMT_HCAP + 1];
    __shared__ EmtStage stage;
    __shared__ int incomplete;
    const int i = vb.x;
    const double xi = a.pos[3 * i], yi = a.pos[3 * i + 1], zi = a.pos[3 * i + 2];
    const double n0i = a.p.n0[i], g1i = a.p.gamma1[i], g2i = a.p.gamma2[i], V0i = a.p.V0[i];
    const double eta2i = a.p.eta2[i], kapi = a.p.kappa[i], s0i = a.p.s0[i], dEi = a.dEdsig[i];
    double gx = 0.0, gy = 0.0, gz = 0.0;
    double wxx = 0.0, wyy = 0.0, wzz = 0.0, wyz = 0.0, wxz = 0.0, wxy = 0.0;
    auto heavy = [&](int t) {
        const int j = t & 0xffffff, s = t >> 24;
        const double dx = a.pos[3 * j] + a.shifts[3 * s] - xi;
        const double dy = a.pos[3 * j + 1] + a.shifts[3 * s + 1] - yi;
        const double dz = a.pos[3 * j + 2] + a.shifts[3 * s + 2] - zi;
        const double r = sqrt(dx * dx + dy * dy + dz * dz);
        if (r < a.cutoff && r > 1e-8) {
            const double x = exp(a.acut * (r - a.rc));
            const double theta = 1.0 / (1.0 + x);
            const double dth = -a.acut * x * theta;             // d(theta)/dr / theta
            const double chi = a.p.n0[j] / n0i;
            // ordered pair (i <- j): neighbour j seen from i
            const double dsig_ij = exp(-a.p.eta2[j] * (r - a.beta * a.p.s0[j])) * chi * theta / g1i;
            const double y_ij = 0.5 * V0i * exp(-a.p.kappa[j] * (r / a.beta - a.p.s0[j])) * chi / g2i * theta;
            // ordered pair (j <- i): this atom seen from j (same distance, opposite direction)
            const double dsig_ji = exp(-eta2i * (r - a.beta * s0i)) / chi * theta / a.p.gamma1[j];
            const double y_ji = 0.5 * a.p.V0[j] * exp(-kapi * (r / a.beta - s0i)) / chi / a.p.gamma2[j] * theta;
            // dE/dr of this pair distance, both ordered pairs:  dE/dsigma1 * dsigma/dr - d(pair energy)/dr
            const double dEdr = dEi * dsig_ij * (-a.p.eta2[j] + dth) - y_ij * (-a.p.kappa[j] / a.beta + dth)
                                + a.dEdsig[j] * dsig_ji * (-eta2i + dth) - y_ji * (-kapi / a.beta + dth);
            const double f = dEdr / r;                          // dr/dx_i = -(d / r)
            gx -= f * dx;
            gy -= f * dy;
            gz -= f * dz;
            if constexpr (VIRIAL) {
                const double h = 0.5 * f;
                wxx += h * (dx * dx); wyy += h * (dy * dy); wzz += h * (dz * dz);
                wyz += h * (dy * dz); wxz += h * (dx * dz); wxy += h * (dx * dy);
            }
        }
    };
    // neighbours from the density kernel's lists; the sweep again only if some thread's list overflowed there
    const int* lst = a.nbr + ((size_t)i * 256 + threadIdx.x) * (EMT_HCAP + 1);
    const int cnt = lst[0];
    if (threadIdx.x == 0) incomplete = 0;
    __syncthreads();
    if (cnt < 0) incomplete = 1;
    __syncthreads();
    if (incomplete) {
        (void)emt_pairs(a, xi, yi, zi, &stage, hits, heavy);
    } else {
        for (int h = 0; h < cnt; ++h) heavy(lst[1 + h]);
    }
    gx = block_sum(gx, red);
    gy = block_sum(gy, red);
    gz = block_sum(gz, red);
    if (threadIdx.x == 0) {
        a.grad[3 * i] = gx;
        a.grad[3 * i + 1] = gy;
        a.grad[3 * i + 2] = gz;
    }
    if constexpr (VIRIAL) {
        wxx = block_sum(wxx, red);
        wyy = block_sum(wyy, red);
        wzz = block_sum(wzz, red);
        wyz = block_sum(wyz, red);
        wxz = block_sum(wxz, red);
        wxy = block_sum(wxy, red);
        if (threadIdx.x == 0) {
            double* w = a.grad + 3 * (size_t)a.n + 6 * (size_t)i;
            w[0] = wxx; w[1] = wyy; w[2] = wzz; w[3] = wyz; w[4] = wxz; w[5] = wxy;
        }
    }
}
__device__ __forceinline__ void emt_force_vb(const VB vb, EmtArgs a) { emt_force_body<false>(vb, a); }
__device__ __forceinline__ void emt_force_virial_vb(const VB vb, EmtArgs a) { emt_force_body<true>(vb, a); }
__global__ __launch_bounds__(256) void emt_force_kernel(EmtArgs a) { emt_force_vb(vb_hw(), a); }
__global__ __launch_bounds__(256) void emt_force_virial_kernel(EmtArgs a) { emt_force_virial_vb(vb_hw(), a); }

}  // namespace
}  // namespace sella

using namespace sella;

// dconst != nullptr: the parameter table and the shift vectors are resident already (9 n + 3 nshift doubles, uploaded by
// the caller once: sella_calc_emt_create) — a force call is then one upload (positions), two kernels, one read-back.
// virial6 != nullptr: the force pass also reduces the per-atom virials (emt_force_virial_kernel), summed here in index
// order like the energies; the read-back is then 10 n doubles instead of 4 n.
int sella::emt_eval_resident(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                             const double* dconst, double rc, double acut, double cutoff, double beta, double* energy,
                             double* grad, double* virial6) {
    double *dea, *dgr;
    SCHK(emt_queue(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta, &dea, &dgr, virial6 != nullptr));
    // per-atom energies, the gradient and (if asked for) the per-atom virials sit back to back: one read-back
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

int sella::emt_density_queue(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                             const double* dconst, double rc, double acut, double cutoff, double beta, size_t extra_words,
                             EmtArgs* args, double** extra) {
    if (n >= (1 << 24) || nshift > 127) { set_error("emt: at most 2^24 atoms and 127 periodic images"); return SELLA_E_INVALID; }
    const size_t nbr_words = ((size_t)n * 256 * (EMT_HCAP + 1) + 1) / 2;
    // (the six virial words per atom are always part of the layout: the lists sit at the same place for every caller)
    const size_t words = (size_t)3 * n + (size_t)9 * n + (size_t)3 * nshift + (size_t)4 * n + (size_t)3 * n + (size_t)6 * n + 64
                         + nbr_words;
    double* buf;
    SCHK(scratch_get(c, SCR_MISC0, (words + extra_words) * sizeof(double), &buf));
    double* dpos = buf;
    double* dpar = dpos + 3 * (size_t)n;
    double* dsh = dpar + 9 * (size_t)n;
    double* dsig = dsh + 3 * (size_t)nshift;
    double* dep = dsig + n;
    double* dde = dep + n;
    double* dea = dde + n;
    double* dgr = dea + n;
    SCHK(h2d_async(c, dpos, pos, (size_t)3 * n * sizeof(double)));
    if (dconst) {
        dpar = const_cast<double*>(dconst);
        dsh = dpar + 9 * (size_t)n;
    } else {
        SCHK(h2d_async(c, dpar, par, (size_t)9 * n * sizeof(double)));
        SCHK(h2d_async(c, dsh, shifts, (size_t)3 * nshift * sizeof(double)));
    }
    EmtArgs a;
    a.n = n; a.nshift = nshift; a.pos = dpos; a.shifts = dsh;
    a.hcap = (int)std::min<long>(std::max<long>(c->opt.emt_hcap, 1), EMT_HCAP);
    a.p.E0 = dpar; a.p.s0 = dpar + n; a.p.V0 = dpar + 2 * (size_t)n; a.p.eta2 = dpar + 3 * (size_t)n;
    a.p.kappa = dpar + 4 * (size_t)n; a.p.lam = dpar + 5 * (size_t)n; a.p.n0 = dpar + 6 * (size_t)n;
    a.p.gamma1 = dpar + 7 * (size_t)n; a.p.gamma2 = dpar + 8 * (size_t)n;
    a.rc = rc; a.acut = acut; a.cutoff = cutoff; a.beta = beta;
    a.sigma1 = dsig; a.epair = dep; a.dEdsig = dde; a.eatom = dea; a.grad = dgr;
    a.nbr = reinterpret_cast<int*>(dgr + 3 * (size_t)n + 6 * (size_t)n + 32);
    SELLA_LAUNCHB(c, emt_density_kernel, emt_density_vb, 256, dim3(n), dim3(256), 0, a);
    HIPCHK(hipGetLastError());
    *args = a;
    if (extra) *extra = buf + words;
    return SELLA_OK;
}

// the same up to the kernels: positions uploaded, two launches queued, nothing waited for.  *eatom (n per-atom
// energies, summed by the caller in index order) and *grad (3 n, directly behind; with `virial`, the n x 6 per-atom
// virials directly behind that) stay valid until scratch slot SCR_MISC0 is used again.
int sella::emt_queue(sella_ctx* c, int n, const double* pos, const double* par, int nshift, const double* shifts,
                     const double* dconst, double rc, double acut, double cutoff, double beta, double** eatom, double** grad,
                     bool virial) {
    EmtArgs a;
    SCHK(emt_density_queue(c, n, pos, par, nshift, shifts, dconst, rc, acut, cutoff, beta, 0, &a, nullptr));
    if (virial)
        SELLA_LAUNCHB(c, emt_force_virial_kernel, emt_force_virial_vb, 256, dim3(n), dim3(256), 0, a);
    else
        SELLA_LAUNCHB(c, emt_force_kernel, emt_force_vb, 256, dim3(n), dim3(256), 0, a);
    HIPCHK(hipGetLastError());
    *eatom = a.eatom;
    *grad = a.grad;
    return SELLA_OK;
}

extern "C" int sella_emt_eval(sella_ctx* c, int n, const double* pos, const double* par /* 9 x n */, int nshift,
                              const double* shifts, double rc, double acut, double cutoff, double beta,
                              double* energy, double* grad) {
    if (!c || n <= 0 || !pos || !par || nshift <= 0 || !shifts || !energy || !grad) {
        set_error("emt_eval: invalid arguments");
        return SELLA_E_INVALID;
    }
    return emt_eval_resident(c, n, pos, par, nshift, shifts, nullptr, rc, acut, cutoff, beta, energy, grad);
}

extern "C" int sella_emt_eval_stress(sella_ctx* c, int n, const double* pos, const double* par /* 9 x n */, int nshift,
                                     const double* shifts, double rc, double acut, double cutoff, double beta,
                                     double* energy, double* grad, double* virial6) {
    if (!c || n <= 0 || !pos || !par || nshift <= 0 || !shifts || !energy || !grad || !virial6) {
        set_error("emt_eval_stress: invalid arguments");
        return SELLA_E_INVALID;
    }
    return emt_eval_resident(c, n, pos, par, nshift, shifts, nullptr, rc, acut, cutoff, beta, energy, grad, virial6);
}
