// newton_core.h's leaf value without a device: on random integers newton_leaf_value is the expression it was before newton_leaf_quotient was split
// off for the device finalize of refit_codes.hip, and the quotient is refused exactly where a leaf keeps its value.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include "newton_core.h"

int main() {
    std::mt19937_64 rng(7);
    int bad = 0;
    for (int i = 0; i < 200000; ++i) {
        const double scale = std::ldexp(1.0, static_cast<int>(rng() % 41)), l2 = (rng() % 4 == 0) ? 0.0 : static_cast<double>(rng() % 1000) / 256.0;
        const long long Sg = static_cast<long long>(rng() >> (2 + rng() % 40)) * ((rng() & 1) ? 1 : -1), Sh = (rng() % 8 == 0) ? 0 : static_cast<long long>(rng() >> (2 + rng() % 40));
        const long long cnt = static_cast<long long>(rng() % 5) - 1, depth = static_cast<long long>(rng() % 3);
        const float old = static_cast<float>(static_cast<double>(rng() % 2001) / 1000.0 - 1.0);
        const bool keeps = cnt <= 0 || depth <= 0 || !(static_cast<double>(Sh) / scale + l2 > 0.0);
        const float want = keeps ? old : static_cast<float>((static_cast<double>(Sg) / scale) / (static_cast<double>(Sh) / scale + l2));
        const float got = gbrl::kern::newton_leaf_value(Sg, Sh, cnt, static_cast<int>(depth), scale, l2, old);
        double q = 0.0;
        const bool moved = gbrl::kern::newton_leaf_quotient(Sg, Sh, cnt, static_cast<int>(depth), scale, l2, q);
        if (std::memcmp(&got, &want, sizeof(got)) != 0 || moved == keeps || (moved && static_cast<float>(q) != got)) ++bad;
    }
    std::printf("newton_core_check: %d mismatches\n", bad);
    return bad != 0;
}
