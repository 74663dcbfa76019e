// Stand-alone check of the host-side argument handling of the pair-potential entries (sella_amd/csrc/pair_pot.h:
// pair_pot_make, and the radial functions it evaluates at the cutoff).  Own main, no HIP, nothing loaded into Python:
// tests/test_pair_args_host.py compiles it with the host sanitizers (-fsanitize=address,undefined) and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../sella_amd/csrc/pair_pot.h"

using namespace sella;

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool refused(const char* msg, const char* word) { return msg && std::strstr(msg, word); }

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double morse[3] = {0.3429, 1.3588, 2.866}, lj[2] = {1.0, 1.0};
    // exactly-sized heap arrays: a read past the parameters or the shifts is an AddressSanitizer error
    std::vector<double> m3(morse, morse + 3), l2(lj, lj + 2), one(3, 0.0), s27(81, 0.5), s127(381, 0.0), s128(384, 0.0);
    PairPot p;

    // in order: Morse with a cutoff, the shift constants are phi and phi' at the cutoff
    EXPECT(pair_pot_make(32, PAIR_MORSE, m3.data(), 27, s27.data(), 3.3, &p) == nullptr);
    {
        const double x = std::exp(-morse[1] * (3.3 - morse[2]));
        EXPECT(p.rc == 3.3 && p.cutoff == 3.3);
        EXPECT(std::fabs(p.phic - morse[0] * x * (x - 2.0)) <= 1e-16);
        EXPECT(std::fabs(p.dphic - 2.0 * morse[0] * morse[1] * (x - x * x)) <= 1e-16);
        const PairRadial q = pair_radial<PAIR_MORSE>(p, 3.3);                 // energy and force vanish at the cutoff
        EXPECT(std::fabs(q.phi) <= 1e-16 && std::fabs(q.d1) <= 1e-16);
    }
    // Lennard-Jones reads two parameters only; no cutoff: plain phi, nothing shifted, every pair inside the sweep
    EXPECT(pair_pot_make(13, PAIR_LJ, l2.data(), 1, one.data(), 0.0, &p) == nullptr);
    EXPECT(p.p0 == 4.0 && p.rc == 0.0 && p.phic == 0.0 && p.dphic == 0.0 && p.cutoff == PAIR_NO_CUTOFF);
    EXPECT(std::isfinite(p.cutoff * p.cutoff * (1.0 + 1e-12)));
    {
        const PairRadial q = pair_radial<PAIR_LJ>(p, std::pow(2.0, 1.0 / 6.0));   // the minimum: -eps, no force
        EXPECT(std::fabs(q.phi + 1.0) <= 4e-16 && std::fabs(q.d1) <= 1e-14 && q.d2 > 0.0);
    }
    EXPECT(pair_pot_make(13, PAIR_LJ, l2.data(), 1, one.data(), -inf, &p) == nullptr);
    EXPECT(pair_pot_make(4, PAIR_MORSE, m3.data(), 127, s127.data(), 5.0, &p) == nullptr);   // the last size allowed

    // refusals: nothing is read beyond what is there, *pot is left alone
    PairPot keep;
    std::memset(&keep, 0x5a, sizeof(keep));
    p = keep;
    EXPECT(refused(pair_pot_make(4, PAIR_MORSE, m3.data(), 128, s128.data(), 5.0, &p), "127"));
    EXPECT(refused(pair_pot_make(1 << 24, PAIR_MORSE, m3.data(), 1, one.data(), 5.0, &p), "2^24"));
    EXPECT(refused(pair_pot_make(0, PAIR_MORSE, m3.data(), 1, one.data(), 5.0, &p), "invalid"));
    EXPECT(refused(pair_pot_make(4, PAIR_MORSE, nullptr, 1, one.data(), 5.0, &p), "invalid"));
    EXPECT(refused(pair_pot_make(4, PAIR_MORSE, m3.data(), 1, nullptr, 5.0, &p), "invalid"));
    EXPECT(refused(pair_pot_make(4, PAIR_MORSE, m3.data(), 0, one.data(), 5.0, &p), "invalid"));
    EXPECT(refused(pair_pot_make(4, PAIR_MORSE, m3.data(), 1, one.data(), 5.0, nullptr), "invalid"));
    EXPECT(refused(pair_pot_make(4, 2, m3.data(), 1, one.data(), 5.0, &p), "form"));
    EXPECT(refused(pair_pot_make(4, -1, m3.data(), 1, one.data(), 5.0, &p), "form"));
    EXPECT(refused(pair_pot_make(32, PAIR_MORSE, m3.data(), 27, s27.data(), 0.0, &p), "cutoff"));      // periodic, none
    EXPECT(refused(pair_pot_make(4, PAIR_MORSE, m3.data(), 1, one.data(), nan, &p), "rcut"));
    EXPECT(refused(pair_pot_make(4, PAIR_MORSE, m3.data(), 1, one.data(), inf, &p), "rcut"));
    EXPECT(refused(pair_pot_make(4, PAIR_MORSE, m3.data(), 1, one.data(), 1e200, &p), "rcut"));
    std::vector<double> bad(m3);
    bad[2] = nan;
    EXPECT(refused(pair_pot_make(4, PAIR_MORSE, bad.data(), 1, one.data(), 5.0, &p), "finite"));
    std::vector<double> sig0(l2);
    sig0[1] = 0.0;
    EXPECT(refused(pair_pot_make(4, PAIR_LJ, sig0.data(), 1, one.data(), 2.5, &p), "sigma"));
    std::vector<double> sh(s27);
    sh[80] = inf;
    EXPECT(refused(pair_pot_make(32, PAIR_MORSE, m3.data(), 27, sh.data(), 3.3, &p), "translations"));
    EXPECT(std::memcmp(&p, &keep, sizeof(keep)) == 0);

    std::printf(failures ? "%d checks failed\n" : "pair_args_check ok\n", failures);
    return failures ? 1 : 0;
}
