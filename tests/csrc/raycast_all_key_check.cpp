// Host property test of the all-hits lists' radix key (mesh_amd/csrc/common.h allhits_t_key): over non-negative doubles
// in ascending order -- zero, the smallest and largest denormals, the smallest normal, runs of adjacent ulps at every
// binade sampled, random values at every scale, the largest finite value and +inf -- the key must be strictly monotone
// (a < b => key(a) < key(b), a == b => equal keys), +inf must get the largest key, and -0.0 must get +0.0's key, since
// the lists compare t by value.  Prints "violations=N" and exits 1 when N > 0.  -DMUTATE_ALLHITS_KEY takes the raw bits
// of t: that build must report the -0.0 violation (tests/test_raycast_all_host.py).
//   hipcc -O2 -std=c++17 -ffp-contract=off -x hip raycast_all_key_check.cpp -I<csrc> -o kc && ./kc
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "common.h"

using namespace msh;

int main() {
    std::vector<double> v;
    const double inf = std::numeric_limits<double>::infinity();
    v.push_back(0.0);
    v.push_back(std::numeric_limits<double>::denorm_min());
    v.push_back(std::numeric_limits<double>::min());
    v.push_back(std::nextafter(std::numeric_limits<double>::min(), 0.0));  // the largest denormal
    v.push_back(std::numeric_limits<double>::max());
    v.push_back(inf);
    for (int e = -1074; e <= 1023; e += 7) {
        double x = std::ldexp(1.0, e);
        double lo = x, hi = x;
        for (int k = 0; k < 4; ++k) {  // adjacent ulps on both sides of a power of two
            lo = std::nextafter(lo, 0.0);
            hi = std::nextafter(hi, inf);
            v.push_back(lo);
            v.push_back(hi);
        }
        v.push_back(x);
    }
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    for (int i = 0; i < 200000; ++i) {
        const double x = std::ldexp(U(rng), (int)(rng() % 2098) - 1074);
        v.push_back(x);
        v.push_back(std::nextafter(x, inf));
    }
    std::sort(v.begin(), v.end());
    long viol = 0, zero_viol = 0, checks = 0;
    for (size_t i = 0; i + 1 < v.size(); ++i) {
        const unsigned long long a = allhits_t_key(v[i]), b = allhits_t_key(v[i + 1]);
        ++checks;
        if (v[i] < v[i + 1] ? !(a < b) : a != b) {
            if (++viol <= 5) std::fprintf(stderr, "order violation: %a -> %llx, %a -> %llx\n", v[i], a, v[i + 1], b);
        }
    }
    if (allhits_t_key(inf) != allhits_t_key(v.back()) || !(allhits_t_key(std::numeric_limits<double>::max()) < allhits_t_key(inf))) {
        ++viol;
        std::fprintf(stderr, "+inf does not order last\n");
    }
    if (allhits_t_key(-0.0) != allhits_t_key(0.0)) {
        ++viol;
        ++zero_viol;
        std::fprintf(stderr, "-0.0 -> %llx, +0.0 -> %llx\n", allhits_t_key(-0.0), allhits_t_key(0.0));
    }
    // the low and high words the radix passes sort on put the key together again
    const unsigned long long k = allhits_t_key(1.0 + 0x1p-30);
    if ((((unsigned long long)(uint32_t)(k >> 32)) << 32 | (uint32_t)k) != k) ++viol;
    std::printf("values=%zu checks=%ld zero_violations=%ld violations=%ld\n", v.size(), checks, zero_viol, viol);
    return viol == 0 && checks > 400000 ? 0 : 1;
}
