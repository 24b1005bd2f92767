// The host's fp32 -> IEEE binary16 rounding (precision "f16": the weight packing, pack.hip).  Pure C++, no HIP
// (tests/test_f16_cpu.py compiles it stand-alone and holds it to torch.float16 bit for bit).  An integer formula: round
// to nearest, ties to even; results below 2^-14 are binary16 subnormals (gradual underflow, nothing is flushed); a
// magnitude of 65520 or more is an infinity (the mode does not saturate); NaN stays NaN.
#pragma once
#include <cstdint>
#include <cstring>

namespace dr {

inline uint16_t f16_rne_bits(uint32_t u) {                   // u = the fp32 bit pattern
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t mag = u & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) return (uint16_t)(sign | 0x7E00u | ((mag >> 13) & 0x3FFu));      // NaN: quiet, payload's top bits kept
    if (mag >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                              // >= 65520 (infinity included)
    if (mag < 0x33000000u) return sign;                                                     // < 2^-25: zero (2^-25 itself ties to even = 0)
    const int e = (int)(mag >> 23);                                                         // biased fp32 exponent, 102 .. 142
    // the 24-bit significand is shifted right until its last kept bit has the weight of the result's ulp: 13 places for a
    // normal result (e >= 113), one more for every binade below 2^-14 (a subnormal result: ulp 2^-24)
    const uint32_t sig = (mag & 0x7FFFFFu) | 0x800000u;
    const int shift = e >= 113 ? 13 : 126 - e;                                              // 13 .. 24
    const uint32_t kept = sig >> shift, rest = sig & ((1u << shift) - 1u), half = 1u << (shift - 1);
    const uint32_t up = (rest > half || (rest == half && (kept & 1u))) ? 1u : 0u;
    // normal: exponent field (e - 112) and the kept significand with its leading 1 at bit 10, which the sum absorbs
    // ((e - 113) << 10) + kept; a carry out of the significand steps the exponent, and subnormal -> smallest normal
    // (kept = 0x400) falls out of the same sum
    const uint32_t base = e >= 113 ? ((uint32_t)(e - 113) << 10) : 0u;
    return (uint16_t)(sign | (base + kept + up));
}

inline uint16_t f16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return f16_rne_bits(u);
}

}  // namespace dr
