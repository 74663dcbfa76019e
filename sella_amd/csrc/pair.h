// pair.h — the pair-potential calculator (pair.hip: Morse and Lennard-Jones, plain or in shifted-force form, periodic
// directions as an explicit image sum) as calc.hip sees it: the force call in two halves, the dense Hessian, products with
// host vectors, and the resident state of the Hessian-vector operator.
#pragma once
#include "emt.h"
#include "pair_pot.h"

namespace sella {

// The sweep is EMT's (emt_pairs, emt.h) on the geometry fields of an EmtArgs: n, nshift, hcap, pos, shifts, cutoff; eatom
// and grad are the outputs of the eval pass.  Everything else in `g` is unused (null).
struct PairArgs {
    EmtArgs g;
    PairPot pot;
};

// positions uploaded (the shifts too unless `dshifts` holds them on the device), one launch queued, nothing waited for.
// *eatom (n per-atom energies, summed by the caller in index order), *grad (3 n, directly behind) and, with `virial`, the
// n x 6 per-atom virials behind that stay valid until scratch slot SCR_MISC0 is used again.
int pair_queue(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift, const double* shifts,
               const double* dshifts, double** eatom, double** grad, bool virial);
int pair_eval_resident(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift, const double* shifts,
                       const double* dshifts, double* energy, double* grad, double* virial6);
// `out` (3n x 3n) is overwritten and stays on the device
int pair_hessian_resident(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift,
                          const double* shifts, const double* dshifts, sella_mat out);
// V, HV: (k, 3n) host arrays, one vector per row
int pair_hvp_resident(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift, const double* shifts,
                      const double* V, int k, double* HV);

// What the Hessian-vector operator (calc.hip, sella_hvp) keeps of a geometry: the visits of every atom, j != i, in the order
// of the sweep (thread by thread, each thread's in its own order), atom after atom — visit e of atom i at off[i] + e — as a
// structure of arrays: the neighbour j, the unit vector u and the two coefficients of K = c1 I + c2 u u^T (c1 = phi' / r,
// c2 = phi'' - phi' / r).  A product then reads 44 bytes per visit, coalesced, and evaluates no exp, sqrt or division.
struct PairHvpState {
    int n = 0;
    int nvisit = 0;
    const int* off = nullptr;               // n + 1
    const int* nbr = nullptr;               // nvisit
    const double* q = nullptr;              // 5 x nvisit: ux | uy | uz | c1 | c2
    double* geo = nullptr;                  // positions, shifts, counts, offsets
    size_t geo_bytes = 0;
    double* ent = nullptr;                  // q, nbr
    size_t ent_bytes = 0;
};
int pair_hvp_state_create(sella_ctx* c, int n, const double* pos, int form, const PairPot& pot, int nshift,
                          const double* shifts, PairHvpState* st);
void pair_hvp_state_destroy(sella_ctx* c, PairHvpState* st);
// the three entries of emt.h's operator state, with the same meaning of every argument
int pair_hvp_state_apply(sella_ctx* c, const PairHvpState& st, const double* v, double* hv, const double* part, int nb,
                         const int* inv, double* y, int* flag);
int pair_hvp_state_apply_block(sella_ctx* c, const PairHvpState& st, const double* V, int ldv, int nh, const int* inv, double* Y,
                               int ldy);
int pair_hvp_state_diag(sella_ctx* c, const PairHvpState& st, const int* inv, double* y);

}  // namespace sella
