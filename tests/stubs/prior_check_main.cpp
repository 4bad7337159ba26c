// Stand-alone host program over the device-free part of the Gaussian prior (mc-alf_amd/csrc/prior_args.h): the checks
// mcalf_set_gauss_prior makes on its arrays and the constants it stores.  tests/test_prior_host.py builds it with
// -fsanitize=address,undefined and reads what it prints:
//   check <label> <rc> <message>      one line per case of gauss_prior_check
//   c <k> <sigma as hex float> <c as hex float>      the stored constants of a run of widths
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "prior_args.h"

using namespace mcalf;

static void run(const char* label, std::vector<double> mu, std::vector<double> sigma, int slot) {
    char msg[256] = "";
    const int rc = gauss_prior_check(mu.data(), sigma.data(), (int)mu.size(), slot, msg, sizeof msg);
    printf("check %s %d %s\n", label, rc, msg);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    run("fine", {0.0, 1.0, 13.0, 2.0}, {0.0, 0.0, 0.5, 3.0}, 1);
    run("all-zero", {nan, inf, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, 1);        // (mu is not looked at where sigma is 0)
    run("sigma-negative", {0.0, 1.0, 13.0, 2.0}, {0.0, 0.0, -0.5, 3.0}, 1);
    run("sigma-nan", {0.0, 1.0, 13.0, 2.0}, {0.0, 0.0, 0.5, nan}, 1);
    run("sigma-inf", {0.0, 1.0, 13.0, 2.0}, {inf, 0.0, 0.5, 1.0}, 1);
    run("mu-nan", {0.0, 1.0, nan, 2.0}, {0.0, 0.0, 0.5, 3.0}, 1);
    run("mu-inf", {0.0, 1.0, 13.0, -inf}, {0.0, 0.0, 0.5, 3.0}, 1);
    run("ncomp-slot", {0.0, 1.0, 13.0, 2.0}, {0.0, 0.25, 0.5, 3.0}, 1);
    run("first-wins", {0.0, 1.0, nan, 2.0}, {-1.0, 0.25, 0.5, 3.0}, 1);
    std::vector<double> sigma;
    for (int k = 0; k < 129; ++k) sigma.push_back(k % 7 == 3 ? 0.0 : std::ldexp(1.0 + 0.37 * (k % 11), (k % 41) - 20));
    sigma.push_back(1e-150);
    sigma.push_back(1e150);
    std::vector<double> c(sigma.size(), -7.0);
    const int n = gauss_prior_constants(sigma.data(), (int)sigma.size(), c.data());
    for (size_t k = 0; k < sigma.size(); ++k) printf("c %zu %a %a\n", k, sigma[k], c[k]);
    printf("ngauss %d\n", n);
    return 0;
}
