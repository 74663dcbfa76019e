// tip3p.h — the TIP3P water calculator (tip3p.hip: rigid three-site molecules, Lennard-Jones on the oxygens, Coulomb between
// all sites of different molecules, whole molecule pairs switched off on the O-O distance) as calc.hip sees it: the force call
// in two halves, the dense Hessian, products with host vectors, and the resident state of the Hessian-vector operator.
#pragma once
#include <cmath>

#include "emt.h"

namespace sella {

// The arguments of every TIP3P entry point after the check.  Atoms come as consecutive triples, one molecule each, the
// oxygen at site `o` (0: O H H, 2: H H O); box[k] <= 0: direction k is not periodic.
struct TipPot {
    int nmol, o;
    double box[3];
    double qH, sigma, eps4, ke, rc, width;      // eps4 = 4 epsilon; q_O = -2 q_H
};

// nullptr if the arguments are in order, else what is wrong with them.  params: q_H, sigma, epsilon, k_e, rc, width.
inline const char* tip3p_pot_make(int nmol, const double* pos, int o, const double* box, const double* params, TipPot* pot) {
    if (nmol <= 0 || !pos || !box || !params || !pot) return "invalid arguments";
    if ((long)3 * nmol >= (1L << 24)) return "at most 2^24 sites";
    if (o != 0 && o != 2) return "the oxygen is site 0 (O H H) or site 2 (H H O) of a molecule";
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(params[k])) return "the parameters must be finite";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(box[k])) return "the box edges must be finite";
    if (!(params[1] > 0.0)) return "sigma must be positive";
    if (!(params[5] > 0.0) || !(params[5] <= params[4])) return "0 < width <= rc is required";
    for (int k = 0; k < 3; ++k)
        if (box[k] > 0.0 && box[k] < 2.0 * params[4]) return "a periodic edge must be at least 2 rc";
    for (size_t k = 0; k < (size_t)9 * nmol; ++k)
        if (!std::isfinite(pos[k])) return "the positions must be finite";
    TipPot p;
    p.nmol = nmol; p.o = o;
    for (int k = 0; k < 3; ++k) p.box[k] = box[k] > 0.0 ? box[k] : 0.0;
    p.qH = params[0]; p.sigma = params[1]; p.eps4 = 4.0 * params[2]; p.ke = params[3]; p.rc = params[4]; p.width = params[5];
    *pot = p;
    return nullptr;
}

// positions uploaded, one launch queued, nothing waited for.  *emol (nmol per-molecule energies, summed by the caller in
// index order) and *grad (9 nmol, directly behind) stay valid until scratch slot SCR_MISC0 is used again.
int tip3p_queue(sella_ctx* c, const TipPot& pot, const double* pos, double** emol, double** grad);
int tip3p_eval_resident(sella_ctx* c, const TipPot& pot, const double* pos, double* energy, double* grad);
// `out` (9 nmol square) is overwritten and stays on the device
int tip3p_hessian_resident(sella_ctx* c, const TipPot& pot, const double* pos, sella_mat out);
// V, HV: (k, 9 nmol) host arrays, one vector per row
int tip3p_hvp_resident(sella_ctx* c, const TipPot& pot, const double* pos, const double* V, int k, double* HV);

// What the Hessian-vector operator (calc.hip, sella_hvp) keeps of a geometry: the visits of every molecule m — the partners
// n != m whose oxygen lies inside rc — in the order of the filling sweep (thread by thread, each thread's in its own order),
// molecule after molecule, visit e of molecule m at off[m] + e, as a structure of arrays of TIP_Q doubles per visit:
//    0 .. 26   u_ab, the unit vectors of the nine site pairs (a of m, b of n in the order O, H, H; pair p = 3 a + b at 3 p)
//   27 .. 35   t phi'_ab / r_ab                 (c1: K_ab t = c1 I + c2 u u^T)
//   36 .. 44   t (phi''_ab - phi'_ab / r_ab)    (c2)
//   45 .. 53   t' G at the three sites of m;  54 .. 62   t' G at the three sites of n
//   63 .. 65   u_OO;   66   U t'';   67   U t' / d
// and the partner as an int: 68 x 8 + 4 = 548 bytes per visit, read coalesced.  The G are kept, not rebuilt from the nine
// pairs: a product then evaluates no sqrt and no division.  Inside rc - width the entries from 45 on are zero.
constexpr int TIP_Q = 68;
struct TipHvpState {
    int nmol = 0, o = 0;
    int nvisit = 0;
    const int* off = nullptr;               // nmol + 1
    const int* nbr = nullptr;               // nvisit
    const double* q = nullptr;              // TIP_Q x nvisit
    double* geo = nullptr;                  // positions, counts, offsets
    size_t geo_bytes = 0;
    double* ent = nullptr;                  // q, nbr
    size_t ent_bytes = 0;
};
int tip3p_hvp_state_create(sella_ctx* c, const TipPot& pot, const double* pos, TipHvpState* st);
void tip3p_hvp_state_destroy(sella_ctx* c, TipHvpState* st);
// the three entries of pair.h's operator state, with the same meaning of every argument (n = 9 nmol coordinates)
int tip3p_hvp_state_apply(sella_ctx* c, const TipHvpState& st, const double* v, double* hv, const double* part, int nb,
                          const int* inv, double* y, int* flag);
int tip3p_hvp_state_apply_block(sella_ctx* c, const TipHvpState& st, const double* V, int ldv, int nh, const int* inv, double* Y,
                                int ldy);
int tip3p_hvp_state_diag(sella_ctx* c, const TipHvpState& st, const int* inv, double* y);

}  // namespace sella
