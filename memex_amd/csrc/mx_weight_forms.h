// mx_weight_forms.h -- the element conversions of weight_image_kernel (encoder_calibrate.hip), in integer arithmetic so that
// the same text compiles for the host: tests/cpp/test_weight_forms.cpp runs it there against the host routines of encoder.hip
// (upload_weight / upload_weight3 / upload_weight2h), whose images the kernel must reproduce bit for bit.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define MX_WF_HD __host__ __device__
#else
#define MX_WF_HD
#endif

namespace mx {

MX_WF_HD inline uint32_t wf_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
MX_WF_HD inline float wf_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// f32 -> bf16, round to nearest even; NaN keeps its top payload bits and is quieted (encoder.hip's f32_to_bf16)
MX_WF_HD inline uint16_t wf_bf16(uint32_t u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// the lo half of the bf16x3 split, bf16(w - hi).  The subtraction is exact for finite hi; what a host subtraction gives for
// the rest is spelled out, because a GPU's default NaN differs from the host's: NaN - NaN keeps w's payload (lo = hi),
// inf - inf is the host's default NaN (sign set), finite - inf (a carry into infinity) is the opposite infinity.
MX_WF_HD inline uint16_t wf_bf16_lo(uint32_t u, uint16_t hi) {
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return hi;
    if ((hi & 0x7fffu) == 0x7f80u) return a == 0x7f800000u ? (uint16_t)0xffc0u : (uint16_t)(hi ^ 0x8000u);
    return wf_bf16(wf_bits(wf_float(u) - wf_float((uint32_t)hi << 16)));
}

// f32 -> fp16 of the value clamped to +-65504 first, round to nearest even, subnormals kept; NaN quieted with its top payload
// bits (what the host's _Float16 conversion behind upload_weight2h gives)
MX_WF_HD inline uint16_t wf_f16_sat(uint32_t u) {
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x1ffu));
    if (a >= 0x477fe000u) return (uint16_t)(sign | 0x7bffu);  // |w| >= 65504, the infinities included
    const uint32_t e = a >> 23;
    if (e < 102u) return sign;  // below 2^-25: zero
    uint32_t q, rem, half;
    if (e < 113u) {  // below 2^-14: a multiple of 2^-24
        const uint32_t mant = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;  // 14 .. 24
        q = mant >> shift;
        rem = mant & ((1u << shift) - 1u);
        half = 1u << (shift - 1u);
    } else {
        q = ((e - 112u) << 10) | ((a & 0x7fffffu) >> 13);
        rem = a & 0x1fffu;
        half = 0x1000u;
    }
    if (rem > half || (rem == half && (q & 1u))) ++q;  // (a carry runs into the exponent, as it should)
    return (uint16_t)(sign | q);
}

}  // namespace mx
