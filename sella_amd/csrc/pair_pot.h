// pair_pot.h — the radial functions of the pair-potential calculator (pair.hip) and the host-side handling of their
// arguments.  Plain C++ (no HIP header): the kernels include it, and tests/pair_args_check.cpp compiles the argument
// handling on its own under the host sanitizers.
//
//   Morse           phi = D (1 - e^{-a (r - r0)})^2 - D              params: D, a, r0
//   Lennard-Jones   phi = 4 eps ((sigma / r)^12 - (sigma / r)^6)     params: eps, sigma
//
// With a cutoff rc the pair function is the shifted-force form phi(r) - phi(rc) - phi'(rc) (r - rc) for r < rc and zero
// beyond: energy and force are continuous at rc, phi'' is that of phi and jumps there.
#pragma once
#include <cmath>

#ifndef SELLA_HD
#define SELLA_HD
#endif

namespace sella {

enum { PAIR_MORSE = 0, PAIR_LJ = 1 };

struct PairPot {
    double p0, p1, p2;      // Morse: D, a, r0;  Lennard-Jones: 4 eps, sigma, unused
    double rc;              // the cutoff the shift refers to (0 without one)
    double phic, dphic;     // phi(rc), phi'(rc) (0 without a cutoff)
    double cutoff;          // the cutoff of the sweep: rc, or PAIR_NO_CUTOFF
};

// "every pair": a distance no geometry reaches whose square is still finite
constexpr double PAIR_NO_CUTOFF = 1e150;

struct PairRadial {
    double phi, d1, d2;     // phi (shifted), phi' (shifted), phi''
};

// No contraction into fused multiply-adds here or in the kernels' pair terms: the instantiations of a kernel (with and
// without the virial, one row of a block or another) then round every term alike.
template <int FORM>
SELLA_HD inline PairRadial pair_plain(const PairPot& p, double r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    PairRadial q;
    if (FORM == PAIR_MORSE) {
        const double x = exp(-p.p1 * (r - p.p2));
        const double da = p.p0 * p.p1;
        q.phi = p.p0 * (x * (x - 2.0));                        // D (1 - x)^2 - D without the cancellation of D against D
        q.d1 = 2.0 * da * ((1.0 - x) * x);
        q.d2 = 2.0 * (da * p.p1) * (x * (2.0 * x - 1.0));
    } else {
        const double s = p.p1 / r, s2 = s * s, s6 = s2 * s2 * s2, s12 = s6 * s6;
        q.phi = p.p0 * (s12 - s6);
        q.d1 = p.p0 * (6.0 * s6 - 12.0 * s12) / r;
        q.d2 = p.p0 * (156.0 * s12 - 42.0 * s6) / (r * r);
    }
    return q;
}

template <int FORM>
SELLA_HD inline PairRadial pair_radial(const PairPot& p, double r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    PairRadial q = pair_plain<FORM>(p, r);
    q.phi = q.phi - p.phic - p.dphic * (r - p.rc);
    q.d1 = q.d1 - p.dphic;
    return q;
}

// The arguments of every pair entry point, checked before anything is queued; nullptr if they are in order, else what is
// wrong with them.  rcut <= 0 means no cutoff, which only a system without periodic images (nshift == 1) may ask for.
inline const char* pair_pot_make(int natoms, int form, const double* params, int nshift, const double* shifts, double rcut,
                                 PairPot* pot) {
    if (natoms <= 0 || !params || nshift <= 0 || !shifts || !pot) return "invalid arguments";
    if (natoms >= (1 << 24) || nshift > 127) return "at most 2^24 atoms and 127 periodic images";
    if (form != PAIR_MORSE && form != PAIR_LJ) return "form must be 0 (Morse) or 1 (Lennard-Jones)";
    const int np = form == PAIR_MORSE ? 3 : 2;
    for (int k = 0; k < np; ++k)
        if (!std::isfinite(params[k])) return "the parameters must be finite";
    for (int k = 0; k < 3 * nshift; ++k)
        if (!std::isfinite(shifts[k])) return "the image translations must be finite";
    if (form == PAIR_LJ && !(params[1] > 0.0)) return "sigma must be positive";
    if (!std::isfinite(rcut) && !(rcut <= 0.0)) return "rcut must be finite, or <= 0 for none";
    const bool cut = rcut > 0.0;
    if (!cut && nshift != 1) return "a periodic system needs a cutoff";
    if (cut && !(rcut < PAIR_NO_CUTOFF)) return "rcut is too large";
    PairPot p;
    p.p0 = form == PAIR_MORSE ? params[0] : 4.0 * params[0];
    p.p1 = params[1];
    p.p2 = form == PAIR_MORSE ? params[2] : 0.0;
    p.rc = 0.0; p.phic = 0.0; p.dphic = 0.0;
    p.cutoff = cut ? rcut : PAIR_NO_CUTOFF;
    if (cut) {
        const PairRadial q = form == PAIR_MORSE ? pair_plain<PAIR_MORSE>(p, rcut) : pair_plain<PAIR_LJ>(p, rcut);
        p.rc = rcut; p.phic = q.phi; p.dphic = q.d1;
    }
    *pot = p;
    return nullptr;
}

}  // namespace sella
