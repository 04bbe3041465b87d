// mx_exact_dist.h -- the exact DistCosine of a query against a stored row, shared by the translation units that compute it
// (index_kernels.hip, score_kernels.hip).  Both are built with -ffp-contract=off: the arithmetic below must round exactly like the
// reference's scalar code (see the head of index_kernels.hip), and every path that reports a dist reports these bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mx {

__device__ __forceinline__ float score_from_dist(float d) {
    const float t = __fdiv_rn(1.0f, d);  // d == 0 -> +inf
    const float u = __fdiv_rn(1.0f, t);  // +inf -> 0
    return __fsub_rn(1.0f, u);
}
__device__ __forceinline__ float dist_from_sums(double dot, double na, double nb) {
    if (na > 0.0 && nb > 0.0) {
        double d = __dsub_rn(1.0, __ddiv_rn(dot, __dsqrt_rn(__dmul_rn(na, nb))));
        if (d < 0.0) d = 0.0;
        return (float)d;  // round-to-nearest-even, like Rust `as f32`
    }
    return 0.0f;
}

// 4 consecutive dims (4*c4 ..) of a row.  CMP = false: the f32 store.  CMP = true (compressed corpus:
// the bf16 filter copy is the ONLY copy): the 8-byte half of the 16-byte MFMA fragment holding those
// dims (layout: launch_shadow), widened to f32 exactly; a zero-norm row is stored as zeros.
template <bool CMP>
__device__ __forceinline__ float4 row_load4(const float *__restrict__ x, const void *__restrict__ xh, int ds, uint32_t row,
                                            int c4) {
    if (!CMP) return reinterpret_cast<const float4 *>(x + (size_t)row * ds)[c4];
    const uint32_t t = row >> 5, ks = (uint32_t)c4 >> 2, hh = ((uint32_t)c4 >> 1) & 1u, l = (row & 31u) + 32u * hh;
    const uint2 v = reinterpret_cast<const uint2 *>(xh)[(((size_t)t * (uint32_t)(ds >> 4) + ks) * 64 + l) * 2 + (c4 & 1)];
    float4 f;
    f.x = __uint_as_float(v.x << 16);
    f.y = __uint_as_float(v.x & 0xffff0000u);
    f.z = __uint_as_float(v.y << 16);
    f.w = __uint_as_float(v.y & 0xffff0000u);
    f.x = f.x == f.x ? f.x : 0.0f;
    f.y = f.y == f.y ? f.y : 0.0f;
    f.z = f.z == f.z ? f.z : 0.0f;
    f.w = f.w == f.w ? f.w : 0.0f;
    return f;
}

// exact DistCosine of query qv (LDS) against a stored row, read through row_load4
template <bool CMP>
__device__ __forceinline__ float exact_dist_stored(const float *__restrict__ qv, const float *__restrict__ x,
                                                   const void *__restrict__ xh, int ds, uint32_t row, double na) {
    double dot = 0.0, nb = 0.0;
#pragma unroll 8
    for (int i = 0; i < ds / 4; ++i) {
        const float4 c = row_load4<CMP>(x, xh, ds, row, i);
        const float4 a = *reinterpret_cast<const float4 *>(qv + 4 * i);
        dot += (double)__fmul_rn(a.x, c.x); nb += (double)__fmul_rn(c.x, c.x);
        dot += (double)__fmul_rn(a.y, c.y); nb += (double)__fmul_rn(c.y, c.y);
        dot += (double)__fmul_rn(a.z, c.z); nb += (double)__fmul_rn(c.z, c.z);
        dot += (double)__fmul_rn(a.w, c.w); nb += (double)__fmul_rn(c.w, c.w);
    }
    return dist_from_sums(dot, na, nb);
}

}  // namespace mx
