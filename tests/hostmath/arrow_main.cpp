// Stand-alone driver of sella::hostm::arrow_eig (sella_amd/csrc/host_math.h), the O(k^2) Rayleigh-Ritz update of the
// Davidson loop: TEST INFRASTRUCTURE, built by tests/test_arrow_eig.py with the host sanitizers.
// stdin:  cases "m  D_0 .. D_{m-1}  z_0 .. z_{m-1}  alpha";  stdout per case: rc, lam (m + 1), W ((m + 1)^2, row-major).
#include <cstdio>
#include <vector>

#include "host_math.h"

int main() {
    int m;
    while (scanf("%d", &m) == 1) {
        if (m < 0) return 2;
        std::vector<double> D(m), z(m), lam(m + 1), W((size_t)(m + 1) * (m + 1));
        double alpha;
        for (double& x : D)
            if (scanf("%lf", &x) != 1) return 2;
        for (double& x : z)
            if (scanf("%lf", &x) != 1) return 2;
        if (scanf("%lf", &alpha) != 1) return 2;
        const int rc = sella::hostm::arrow_eig(m, D.data(), z.data(), alpha, lam.data(), W.data());
        printf("%d\n", rc);
        for (double x : lam) printf("%.17g ", x);
        printf("\n");
        for (double x : W) printf("%.17g ", x);
        printf("\n");
    }
    return 0;
}
