// perm_core.h -- the row permutation of permutation_importance_prepared: ONE function of (n, seed, col, repeat, i) that the host
// (gbrl_cpp.permutation_host) and the device (perm_loss.hip) both call, so that "column col shuffled, repeat r" names the same rows wherever it is
// evaluated.  pi = perm(n, seed, col, repeat) is a bijection of [0, n), computed element by element with no state and no table: row i of a variant
// takes its value of column col from row pi(i).
//
// A cycle-walking balanced Feistel network:
//   b     = max(2, bit_length(n - 1)) rounded up to even;  h = b / 2;  mask = 2^h - 1        the domain [0, 2^b) holds [0, n) and is below 4 n (n >= 2)
//   base  = seed ^ 0x7065726D75746174                                                        ("permutat": a stream of its own beside colsampl and gossrest)
//   key_k = base + (4 * uint64(uint32(col)) + k + 1) * 0xD1B54A32D192ED03                    k = 0 .. 3, everything wraps
//   x     = i;  repeat:  L = x >> h, R = x & mask
//                        four rounds k = 0 .. 3:  (L, R) <- (R, L ^ (sample_u24(key_k, repeat, R) & mask))      sample_core.h's hash; h <= 16 <= 24 bits
//                        x = (L << h) | R
//           until x < n                                                                      a bijection of the domain walked along its cycle back into [0, n):
//                                                                                            fewer than four applications are expected
//   pi(i) = x
// Every round is invertible whatever the hash does, so the network is a bijection of the domain; following a cycle of a bijection from a point of
// [0, n) to the next point of [0, n) is a bijection of [0, n).  n = 1: the only point, pi = [0].  n < 2^31: b <= 32, h <= 16.
#pragma once

#include <cstdint>

#include "sample_core.h"

namespace gbrl {
namespace kern {

constexpr uint64_t kPermStream = 0x7065726D75746174ull;
constexpr uint64_t kPermKeyStep = 0xD1B54A32D192ED03ull;
constexpr int kPermRounds = 4;

// what does not depend on the element: the half width and the round keys
struct PermPlan {
    uint32_t n, h, mask;
    int32_t repeat;
    uint64_t key[kPermRounds];
};

GBRL_SAMPLE_HD inline uint32_t perm_half_bits(uint32_t n) {
    uint32_t bits = 0;
    for (uint32_t v = n - 1; v != 0; v >>= 1) ++bits;   // bit_length(n - 1)
    if (bits < 2) bits = 2;
    return (bits + 1) >> 1;                             // (rounded up to even) / 2
}

GBRL_SAMPLE_HD inline PermPlan perm_plan(uint32_t n, uint64_t seed, int32_t col, int32_t repeat) {
    PermPlan p;
    p.n = n;
    p.h = perm_half_bits(n);
    p.mask = (1u << p.h) - 1u;
    p.repeat = repeat;
    const uint64_t base = seed ^ kPermStream;
    for (int k = 0; k < kPermRounds; ++k)
        p.key[k] = base + (4ull * static_cast<uint64_t>(static_cast<uint32_t>(col)) + static_cast<uint64_t>(k) + 1ull) * kPermKeyStep;
    return p;
}

// pi(i), i in [0, n)
GBRL_SAMPLE_HD inline uint32_t perm_at(const PermPlan &p, uint32_t i) {
    uint32_t x = i;
    do {
        uint32_t L = x >> p.h, R = x & p.mask;
        for (int k = 0; k < kPermRounds; ++k) {
            const uint32_t t = L ^ (sample_u24(p.key[k], p.repeat, R) & p.mask);
            L = R;
            R = t;
        }
        x = (L << p.h) | R;
    } while (x >= p.n);
    return x;
}

}  // namespace kern
}  // namespace gbrl
