// prep_wide.hip -- query preparation for rows wider than every scan (mx_index_open accepts up to 65536 dims).  A translation unit of
// its own: the code object of index_kernels.hip, which holds kernels of the headline path, stays what it was.  Exact arithmetic: built
// without FMA contraction, like index_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "index_kernels.h"

namespace mx {

// Rows wider than every scan (ds > kMaxKC16 chunks, up to 65536 dims): no filter copy exists, so there is neither an 8-bit
// form nor a centre, and a whole query no longer fits the LDS a workgroup may ask for (256 KiB at 65536 dims).  The query
// passes through LDS in chunks of kPrepChunk floats; thread 0 walks every chunk in element order, so the norm chain -- and
// with it qnorm2's bits -- is the one prep_queries_kernel runs.  The padded query, the flags and the a-priori bound are
// what that kernel leaves without a filter copy; query fragments are not written, because no scan exists to read them.
constexpr int kPrepChunk = 4096;  // floats per LDS chunk (16 KiB)

__global__ __launch_bounds__(256) void prep_queries_wide_kernel(const float *__restrict__ q, int B, int d, int ds,
                                                                float *__restrict__ qpad, double *__restrict__ qnorm2,
                                                                float *__restrict__ theta, float *__restrict__ e1,
                                                                uint32_t *__restrict__ overflow,
                                                                uint32_t *__restrict__ flags, float *__restrict__ qa,
                                                                float *__restrict__ qb) {
    __shared__ float s_chunk[kPrepChunk];
    __shared__ uint32_t s_bad[4];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const bool live = b < B;  // (block-uniform)
    const float *qrow = q + (size_t)(live ? b : 0) * d;
    bool bad = false;
    double na = 0.0;  // thread 0's chain; a padded slot's query is all zeros: its sum is 0 without the walk
    if (live) {
        for (int c0 = 0; c0 < d; c0 += kPrepChunk) {
            const int len = d - c0 < kPrepChunk ? d - c0 : kPrepChunk;
            __syncthreads();  // the previous chunk has been consumed
            for (int i = tid; i < len; i += 256) {
                const float v = qrow[c0 + i];
                s_chunk[i] = v;
                bad |= !isfinite(v);
            }
            __syncthreads();
            if (tid == 0) {
                for (int i = 0; i < len; ++i) {  // sequential, f32 products: DistCosine's query-norm chain
                    const float v = s_chunk[i];
                    na += (double)__fmul_rn(v, v);
                }
            }
        }
    }
    if (tid == 0) {
        qnorm2[b] = na;
        const bool usable = live && na > 0.0 && isfinite(na);
        theta[b] = usable ? -INFINITY : INFINITY;
        overflow[b] = 0;
    }
    for (int dim = tid; dim < ds; dim += 256)  // the EXACT path and the row-touching forms read the query as it came
        qpad[(size_t)b * ds + dim] = live && dim < d ? qrow[dim] : 0.0f;
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if ((tid & 63) == 0) s_bad[tid >> 6] = anybad ? 1u : 0u;
    __syncthreads();
    if (tid == 0) {
        flags[b] = live ? (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) : 0u;
        e1[b] = kApproxErr;  // no filter copy: the a-priori bound (no scan reads it at this width)
        qa[b] = kApproxErr;
        qb[b] = 0.0f;
    }
}

hipError_t launch_prep_queries_wide(hipStream_t s, const float *q, int B, int d, int ds, float *qpad, double *qnorm2, float *theta,
                                    float *e1, uint32_t *overflow, uint32_t *flags, float *qa, float *qb) {
    if (ds <= kMaxKC16 * kChunkFloats || d < 1 || d > ds) return hipErrorInvalidValue;
    // one block per query slot, as launch_prep_queries: 256 slots, 512 for a batch of more than 256
    hipLaunchKernelGGL(prep_queries_wide_kernel, dim3(B > kPassBatch ? kMaxBatch : kPassBatch), dim3(256), 0, s, q, B, d, ds, qpad, qnorm2,
                       theta, e1, overflow, flags, qa, qb);
    return hipGetLastError();
}

}  // namespace mx
