// like_kernels.hip -- the two kernels of the search by examples (mx_index_search_like).  A translation unit
// of their own: the code object of index_kernels.hip, which holds kernels of the headline path, stays what it was.  Exact
// arithmetic: built without FMA contraction, like index_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "index_kernels.h"

namespace mx {

// ---------------------------------------------------------------------------------------------
// search by examples (mx_index_search_like): the weighted blend of a request's stored rows and caller vector
// as one query, and the used examples taken out of the list the pass returns
// ---------------------------------------------------------------------------------------------
// One workgroup per request.  Phase 1: thread t <= m owns term t (0: the caller vector, 1 + i: example i) and walks its dim elements
// for na, in element order.  Phase 2: every thread owns columns 4 * c4 .. 4 * c4 + 3 and runs the f64 chain over the used terms in term
// order.  Rows of the blocks are dim floats apart: 16-byte stores when that keeps them aligned, element stores otherwise.
__global__ __launch_bounds__(256) void like_combine_kernel(LikeCombine p) {
    __shared__ const float *s_v[kLikeMaxExamples + 1];
    __shared__ double s_w[kLikeMaxExamples + 1], s_len[kLikeMaxExamples + 1];  // s_len = sqrt(na); 0: the term is not used
    const int r = blockIdx.x, tid = threadIdx.x, m = p.m, dim = p.dim;
    if (tid <= m) {
        const float *v = nullptr;
        float w = 0.0f;
        if (tid == 0) {
            if (p.q) {
                v = p.q + (size_t)r * dim;
                w = p.wq[r];
            }
        } else {
            const uint32_t src = p.src[(size_t)r * m + (tid - 1)];
            if (src != kLikeNone) {
                v = p.rows + (size_t)src * dim;
                w = p.w[(size_t)r * m + (tid - 1)];
            }
        }
        double na = 0.0;
        if (v && w != 0.0f)
            for (int j = 0; j < dim; ++j) na = __dadd_rn(na, (double)__fmul_rn(v[j], v[j]));
        s_v[tid] = v;
        s_w[tid] = (double)w;
        s_len[tid] = na == 0.0 ? 0.0 : __dsqrt_rn(na);  // (a non-finite caller vector: NaN or inf, and the term is used)
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t mask = 0;
        for (int i = 0; i < m; ++i)
            if (s_len[1 + i] != 0.0) mask |= 1u << i;
        p.used[r] = mask;
        if (p.n_used) p.n_used[r] = __popc(mask);
    }
    float *out = p.out + (size_t)r * dim;
    float *cmb = p.combined ? p.combined + (size_t)r * dim : nullptr;
    const bool wide = (dim & 3) == 0, cmb_wide = cmb && wide && (reinterpret_cast<uintptr_t>(p.combined) & 15) == 0;
    for (int c4 = tid; c4 < (dim + 3) / 4; c4 += 256) {
        const int c = 4 * c4, nc = dim - c < 4 ? dim - c : 4;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int t = 0; t <= m; ++t) {
            const double len = s_len[t];
            if (len == 0.0) continue;  // (block-uniform)
            const float *v = s_v[t];
            const double w = s_w[t];
            for (int e = 0; e < nc; ++e) acc[e] = __dadd_rn(acc[e], __dmul_rn(w, __ddiv_rn((double)v[c + e], len)));
        }
        const float4 f = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);  // (round to nearest even)
        const float fe[4] = {f.x, f.y, f.z, f.w};
        if (wide) {
            reinterpret_cast<float4 *>(out)[c4] = f;
        } else {
            for (int e = 0; e < nc; ++e) out[c + e] = fe[e];
        }
        if (cmb_wide) {
            reinterpret_cast<float4 *>(cmb)[c4] = f;
        } else if (cmb) {
            for (int e = 0; e < nc; ++e) cmb[c + e] = fe[e];
        }
    }
}

hipError_t launch_like_combine(hipStream_t s, const LikeCombine &p) {
    if (p.R <= 0) return hipSuccess;
    if (p.m < 1 || p.m > kLikeMaxExamples || p.dim < 1 || (p.q && !p.wq)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(like_combine_kernel, dim3(p.R), dim3(256), 0, s, p);
    return hipGetLastError();
}

// One wave per request, four requests per workgroup.  Per chunk of 64 entries each lane tests its entry's id against the request's used
// example ids; the ballot of the kept lanes and a running offset place them, in order, in the caller's list.
__global__ __launch_bounds__(256) void like_drop_examples_kernel(LikeDrop p) {
    const int r = (int)(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (r >= p.R) return;  // (wave-uniform, like everything below but the lane's own slots)
    const int k = p.k, kk = p.kk, m = p.m;
    const float *q = p.q + (size_t)r * p.dim;
    bool any = false;
    for (int j0 = 0; j0 < p.dim && !any; j0 += 64) any = __ballot(j0 + lane < p.dim && q[j0 + lane] != 0.0f) != 0ull;
    int n = any ? p.in_nfound[r] : 0;  // an all-zero query: a blank request
    n = n < 0 ? 0 : n > kk ? kk : n;
    const uint32_t used = p.exclude ? p.used[r] : 0u;
    const uint64_t *own = p.own + (size_t)r * m;
    const uint64_t *iid = p.in_ids + (size_t)r * kk;
    const float *isc = p.in_scores + (size_t)r * kk;
    const float *idi = p.in_dists + (size_t)r * kk;
    uint64_t *oid = p.ids + (size_t)r * k;
    float *osc = p.scores + (size_t)r * k;
    float *odi = p.dists ? p.dists + (size_t)r * k : nullptr;
    int found = 0;
    for (int i0 = 0; i0 < n && found < k; i0 += 64) {
        const int i = i0 + lane;
        bool keep = i < n;
        const uint64_t id = keep ? iid[i] : 0;
        for (uint32_t u = used; u && keep; u &= u - 1)
            if (own[__builtin_ctz(u)] == id) keep = false;
        const unsigned long long kept = __ballot(keep);
        const int at = found + __popcll(kept & ((1ull << lane) - 1ull));
        if (keep && at < k) {
            oid[at] = id;
            osc[at] = isc[i];
            if (odi) odi[at] = idi[i];
        }
        found += __popcll(kept);
    }
    found = found < k ? found : k;
    for (int j = found + lane; j < k; j += 64) {
        oid[j] = 0;
        osc[j] = 0.0f;
        if (odi) odi[j] = INFINITY;
    }
    if (lane == 0) p.n_found[r] = found;
}

hipError_t launch_like_drop_examples(hipStream_t s, const LikeDrop &p) {
    if (p.R <= 0) return hipSuccess;
    if (p.m < 1 || p.m > kLikeMaxExamples || p.k < 1 || p.kk < p.k || p.dim < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(like_drop_examples_kernel, dim3((p.R + 3) / 4), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace mx
