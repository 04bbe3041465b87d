// boost_kernels.hip -- the kernels of boosted search (mx_prior, mx_index_search_boosted).  A translation unit
// of their own, like group_kernels.hip: the code object of index_kernels.hip, which holds kernels of the headline path, stays what it
// was.  The one piece of arithmetic is c = (double)score + (double)w * (double)prior: the product of two f32 values is exact in f64,
// so c is rounded once, with or without contraction (the unit is built with -ffp-contract=off all the same).  The edits and the get
// of a prior are the grouping's kernels: a value moves as its 32 bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "index_kernels.h"

namespace mx {

namespace {

constexpr int kBoostPer = kBoostMaxFetch / kBoostThreads;  // entries a thread owns: t, t + 1024, ...
constexpr int kBoostWaves = kBoostThreads / 64;

// kBoostMaxBlocks workgroups stride over the rows; each leaves the maximum of 0 and its live rows' values in part[w]
__global__ __launch_bounds__(kBoostThreads) void prior_max_kernel(const float *__restrict__ vals, uint64_t n,
                                                                  const uint64_t *__restrict__ dead, float *__restrict__ part) {
    __shared__ float s_m[kBoostWaves];
    const int tid = threadIdx.x;
    float m = 0.0f;
    for (uint64_t r = (uint64_t)blockIdx.x * kBoostThreads + tid; r < n; r += (uint64_t)kBoostMaxBlocks * kBoostThreads) {
        if (dead && ((dead[r >> 6] >> (r & 63u)) & 1ull)) continue;
        m = fmaxf(m, vals[r]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) s_m[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        float a = 0.0f;
#pragma unroll
        for (int w = 0; w < kBoostWaves; ++w) a = fmaxf(a, s_m[w]);
        part[blockIdx.x] = a;
    }
}

// One workgroup per query.  Thread t takes entries t, t + 1024, ...: id -> global row -> prior, c = score + w * prior in f64, into LDS
// (32 KiB at fetch = 4096, padded with -inf to an even count: every c is finite, so a pad neither exceeds nor equals one).  After the
// barrier every thread walks the whole array, two values per LDS read (every lane reads the same 16 bytes: a broadcast), and counts
// for each of its entries those that precede it in the order (c descending, position ascending): m / 2 reads and 2 m compares per
// owned entry.  The ranks are a permutation of 0 .. m - 1, so every output slot below min(k, m) has exactly one writer.
__global__ __launch_bounds__(kBoostThreads) void boost_rank_kernel(BoostRank p) {
    __shared__ __attribute__((aligned(16))) double sc[kBoostMaxFetch];
    const int b = blockIdx.x, tid = threadIdx.x, k = p.k, fetch = p.fetch;
    const int m = min(max(p.cand_nf[b], 0), fetch), m2 = (m + 1) & ~1;  // (m2 <= kBoostMaxFetch: even itself)
    const size_t lbase = (size_t)b * fetch, obase = (size_t)b * k;
    const uint64_t *cid = p.cand_ids + lbase;
    const float *csc = p.cand_scores + lbase;
    const double w = (double)(p.weights ? p.weights[b] : 1.0f);
    float pr[kBoostPer];
    double c[kBoostPer];
#pragma unroll
    for (int e = 0; e < kBoostPer; ++e) {
        const int j = e * kBoostThreads + tid;
        pr[e] = 0.0f;
        c[e] = -INFINITY;
        if (j < m) {
            const uint64_t id = cid[j];
            if (id > p.id_offset && id - p.id_offset - 1 < p.len) pr[e] = p.vals[id - p.id_offset - 1];
            c[e] = (double)csc[j] + w * (double)pr[e];
        }
        if (j < m2) sc[j] = c[e];
    }
    __syncthreads();
    int rank[kBoostPer];
#pragma unroll
    for (int e = 0; e < kBoostPer; ++e) rank[e] = 0;
    if (tid < m) {  // (a thread whose first entry is past the list owns none)
        for (int i = 0; i < m2; i += 2) {
            const double2 v = *reinterpret_cast<const double2 *>(sc + i);
#pragma unroll
            for (int e = 0; e < kBoostPer; ++e) {
                const int j = e * kBoostThreads + tid;
                const double cj = c[e];
                rank[e] += (int)(v.x > cj || (v.x == cj && i < j)) + (int)(v.y > cj || (v.y == cj && i + 1 < j));
            }
        }
    }
    const int nf = min(m, k);
#pragma unroll
    for (int e = 0; e < kBoostPer; ++e) {
        const int j = e * kBoostThreads + tid;
        if (j >= m || rank[e] >= k) continue;
        const size_t dst = obase + rank[e];
        p.ids[dst] = cid[j];
        p.scores[dst] = csc[j];
        if (p.dists) p.dists[dst] = p.cand_dists[lbase + j];
        if (p.priors) p.priors[dst] = pr[e];
        if (p.combined) p.combined[dst] = c[e];
        // the k-th reported entry against the bound on every row outside a full list (m == fetch >= k: this thread exists)
        if (p.complete && m == fetch && rank[e] == k - 1) p.complete[b] = c[e] > (double)csc[m - 1] + w * (double)p.hi ? 1 : 0;
    }
    for (int s = nf + tid; s < k; s += kBoostThreads) {
        const size_t dst = obase + s;
        p.ids[dst] = 0;
        p.scores[dst] = 0.0f;
        if (p.dists) p.dists[dst] = INFINITY;
        if (p.priors) p.priors[dst] = 0.0f;
        if (p.combined) p.combined[dst] = 0.0;
    }
    if (tid == 0) {
        p.n_found[b] = nf;
        if (p.complete && m < fetch) p.complete[b] = 1;  // the list holds every row
    }
}

}  // namespace

hipError_t launch_prior_max(hipStream_t s, const float *vals, uint64_t n, const uint64_t *dead, float *part) {
    if (!part || (n && !vals)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prior_max_kernel, dim3(kBoostMaxBlocks), dim3(kBoostThreads), 0, s, vals, n, dead, part);
    return hipGetLastError();
}

hipError_t launch_boost_rank(hipStream_t s, const BoostRank &p) {
    if (p.B <= 0) return hipSuccess;
    if (p.k < 1 || p.fetch < p.k || p.fetch > kBoostMaxFetch || (p.len && !p.vals) || !p.cand_ids || !p.cand_scores || !p.cand_nf || !p.ids ||
        !p.scores || !p.n_found || (p.dists && !p.cand_dists))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(boost_rank_kernel, dim3(p.B), dim3(kBoostThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mx
