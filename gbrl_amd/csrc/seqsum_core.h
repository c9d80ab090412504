// seqsum_core.h -- the integer arithmetic of the parallel sequential float32 sum (seqsum.hip): an element as a step of the running sum's
// integer multiple A of u = 2^(e - 23), a run of elements as a function of A's parity, and the test that lets a run be applied in O(1).
// Host and device compile the SAME functions: the kernels of seqsum.hip use them for all of their arithmetic, and the host walk behind
// gbrl_hip_seq_sums_model (seq_sums_model, seqsum.hip) evaluates whole chains with them on the CPU, which is how tests/test_seqsum_host.py
// reaches the edges of a binade without a device.  Nothing wave-specific in here (no shuffles, no loads).
#pragma once

#include "kernels_common.h"

namespace gbrl {
namespace kern {
namespace {

constexpr int kSeqBlock = 256;            // elements per summary (one wave, four per lane)
constexpr int kSeqGroup = 16;             // consecutive blocks under one exponent whose composed summary is tried first
constexpr int kSeqBig = 1 << 28;          // clamp of a summary's fields (anything beyond 2^25 already fails the binade check; two clamped values add without overflow)

struct SeqSumm { int d[2], lo[2], hi[2]; };   // per starting parity: total change, least and greatest partial sum (relative to the start, after >= 1 element)

__host__ __device__ __forceinline__ uint32_t seq_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
__host__ __device__ __forceinline__ float seq_float(uint32_t b) { return __builtin_bit_cast(float, b); }
__host__ __device__ __forceinline__ int seq_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int seq_max(int a, int b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ int seq_clamp(int v) { return seq_max(-kSeqBig, seq_min(kSeqBig, v)); }

// one element under ulp exponent e (u = 2^(e - 23)): f = floor(x / u), h = 0 (fraction below a half) | 1 (above) | 2 (tie); false: not summarisable.
// An element whose exponent reaches the running sum's (k <= 0) always takes the sum out of its binade (same sign: beyond 2^(e+1); opposite: below
// 2^e or through zero), so it is not summarisable by definition -- which keeps every quantity inside 32 bits (|f| < 2^23).
__host__ __device__ __forceinline__ bool seq_element(float x, int e, int &f, int &h) {
    const uint32_t b = seq_bits(x);
    const int ex = static_cast<int>((b >> 23) & 0xffu);
    if (ex == 0xff) return false;                               // inf / nan: the serial loop decides
    const int m = ex ? static_cast<int>((b & 0x7fffffu) | 0x800000u) : static_cast<int>(b & 0x7fffffu);
    const int sm = (b >> 31) ? -m : m;                          // x = sm * 2^(ee - 23)
    const int ee = ex ? ex - 127 : -126;
    const int k = e - ee;
    if (k <= 0) return false;
    if (k >= 25) {                                              // |x| < u / 2: positive rounds away, negative floors to -1 and rounds back up
        f = sm < 0 ? -1 : 0; h = sm < 0 ? 1 : 0;
        return true;
    }
    f = sm >> k;                                                // arithmetic shift = floor
    const int rem = sm - f * (1 << k), half = 1 << (k - 1);   // (f may be negative: no shift of it)
    h = rem < half ? 0 : (rem > half ? 1 : 2);
    return true;
}
__host__ __device__ __forceinline__ SeqSumm seq_one(int f, int h) {
    SeqSumm s;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        int t = f;
        if (h == 1) t += 1;
        else if (h == 2) t += (p + f) & 1;
        s.d[p] = t; s.lo[p] = t; s.hi[p] = t;
    }
    return s;
}
// a, then b
__host__ __device__ __forceinline__ SeqSumm seq_compose(const SeqSumm &a, const SeqSumm &b) {
    SeqSumm r;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int d = a.d[p];
        const int q = (p + d) & 1;
        r.d[p] = seq_clamp(d + b.d[q]);
        r.lo[p] = seq_clamp(seq_min(a.lo[p], d + b.lo[q]));
        r.hi[p] = seq_clamp(seq_max(a.hi[p], d + b.hi[q]));
    }
    return r;
}

// Does the running sum s (normal, exponent e) stay strictly inside its binade through a run summarised by (d, lo, hi)[parity]?  If so apply it.
// Strictly: s = A0 u and every partial sum lie in the OPEN interval (2^23, 2^24) u (mirrored for a negative sum).  The lower end is excluded
// because the parity model rounds to multiples of u, and just below 2^e the float32 spacing is u / 2: from s = 2^e an opposite-sign element of
// (u/4, u/2] steps the plain loop down to 2^e - u/2 where the model stays -- so a run that starts on the power of two, or touches it, is left
// to the serial loop.  (Anything that would end below 2^23 u in the model has touched or crossed it in the plain loop as well, and the upper end
// is a crossing by definition; inside the open interval model and loop round alike.)
__host__ __device__ __forceinline__ bool seq_apply(float &s, int e, int d0, int d1, int lo0, int lo1, int hi0, int hi1) {
    const uint32_t sb = seq_bits(s);
    if (static_cast<int>((sb >> 23) & 0xffu) - 127 != e) return false;
    const int m = static_cast<int>((sb & 0x7fffffu) | 0x800000u);
    const int A0 = (sb >> 31) ? -m : m;
    const bool odd = (A0 & 1) != 0;
    const int d = odd ? d1 : d0, lo = odd ? lo1 : lo0, hi = odd ? hi1 : hi0;
    const bool ok = A0 > 0 ? (A0 > (1 << 23) && A0 + lo > (1 << 23) && A0 + hi < (1 << 24)) : (A0 < -(1 << 23) && A0 + hi < -(1 << 23) && A0 + lo > -(1 << 24));
    if (ok) {                                                   // exact: 2^23 < |A0 + d| < 2^24 is the new mantissa, sign and exponent stay
        const int a = A0 + d;
        s = seq_float((sb & 0xff800000u) | (static_cast<uint32_t>(a < 0 ? -a : a) & 0x7fffffu));
    }
    return ok;
}
__host__ __device__ __forceinline__ bool seq_apply(float &s, int e, const SeqSumm &m) { return seq_apply(s, e, m.d[0], m.d[1], m.lo[0], m.lo[1], m.hi[0], m.hi[1]); }

}  // namespace
}  // namespace kern
}  // namespace gbrl
