// group_kernels.hip -- the kernels of grouped search (mx_grouping, mx_index_search_grouped).  A translation
// unit of their own, like score_kernels.hip: the code object of index_kernels.hip, which holds kernels of the headline path, stays
// what it was.  Integer work only: keys are compared, list entries are copied unchanged.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "index_kernels.h"

namespace mx {

namespace {

constexpr int kGroupPer = kGroupMaxFetch / kGroupThreads;  // entries a thread owns: t, t + 1024, ...
constexpr int kGroupWaves = kGroupThreads / 64;
constexpr int kEditThreads = 256;

// One thread per row of [row0, row1): the last range that starts at or before the row, by binary search; the row takes its key if
// the range covers it.  The ranges are sorted by lo and disjoint, so at most one covers a row.
__global__ __launch_bounds__(kEditThreads) void grouping_range_edit_kernel(const uint64_t *__restrict__ ranges,
                                                                            const uint32_t *__restrict__ rkeys, uint32_t n_ranges,
                                                                            uint64_t row0, uint64_t row1, uint32_t *__restrict__ keys) {
    const uint64_t r = row0 + (uint64_t)blockIdx.x * kEditThreads + threadIdx.x;
    if (r >= row1) return;
    uint32_t lo = 0, hi = n_ranges;  // the first range with lo > r is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ranges[2 * (size_t)mid] <= r) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return;
    const uint32_t i = lo - 1;
    if (r < ranges[2 * (size_t)i + 1]) keys[r] = rkeys[i];
}

__global__ __launch_bounds__(kEditThreads) void grouping_id_edit_kernel(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ ikeys,
                                                                         uint64_t n_ids, uint64_t id_offset, uint64_t limit,
                                                                         uint32_t *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * kEditThreads + threadIdx.x;
    if (i >= n_ids) return;
    const uint64_t id = ids[i];
    if (id <= id_offset || id - id_offset > limit) return;
    keys[id - id_offset - 1] = ikeys[i];  // (an id named twice carries the same key both times: the host checked)
}

__global__ __launch_bounds__(kEditThreads) void grouping_get_kernel(const uint64_t *__restrict__ ids, uint64_t n_ids, uint64_t id_offset,
                                                                     uint64_t limit, const uint32_t *__restrict__ keys,
                                                                     uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kEditThreads + threadIdx.x;
    if (i >= n_ids) return;
    const uint64_t id = ids[i];
    out[i] = (id <= id_offset || id - id_offset > limit) ? 0u : keys[id - id_offset - 1];
}

// kGroupCountBlocks workgroups stride over the rows; each leaves its two sums in part[2 w], part[2 w + 1]
__global__ __launch_bounds__(kGroupThreads) void grouping_count_kernel(const uint32_t *__restrict__ keys, uint64_t n,
                                                                       const uint64_t *__restrict__ dead, uint64_t *__restrict__ part) {
    __shared__ uint32_t s_a[kGroupWaves], s_l[kGroupWaves];
    const int tid = threadIdx.x;
    uint32_t a = 0, l = 0;  // (a thread sees at most n / (kGroupCountBlocks * kGroupThreads) + 1 rows: no overflow below 2^50 rows)
    for (uint64_t r = (uint64_t)blockIdx.x * kGroupThreads + tid; r < n; r += (uint64_t)kGroupCountBlocks * kGroupThreads) {
        if (keys[r] == 0) continue;
        a += 1;
        l += (dead && ((dead[r >> 6] >> (r & 63u)) & 1ull)) ? 0u : 1u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        l += __shfl_xor(l, o);
    }
    if ((tid & 63) == 0) {
        s_a[tid >> 6] = a;
        s_l[tid >> 6] = l;
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t sa = 0, sl = 0;
#pragma unroll
        for (int w = 0; w < kGroupWaves; ++w) {
            sa += s_a[w];
            sl += s_l[w];
        }
        part[2 * blockIdx.x] = sa;
        part[2 * blockIdx.x + 1] = sl;
    }
}

// One workgroup per query.  Thread t takes entries t, t + 1024, ...: id -> global row -> key, into LDS (16 KiB at fetch = 4096, padded
// with zeros to a multiple of four entries).  After the barrier every thread walks the whole key array, four keys per LDS read (every
// lane reads the same 16 bytes: a broadcast), and counts for each of its entries the equal keys before it and in total: m / 4 reads and
// 4 m compares per owned entry, m^2 / 4 reads per query.  The head flags are then numbered in list order, 1024 entries per round: a
// ballot and a popcount within the wave, the waves' sums through LDS.
__global__ __launch_bounds__(kGroupThreads) void group_heads_kernel(GroupHeads p) {
    __shared__ __attribute__((aligned(16))) uint32_t skey[kGroupMaxFetch];
    __shared__ uint32_t s_wsum[kGroupWaves];
    const int b = blockIdx.x, tid = threadIdx.x, k = p.k, fetch = p.fetch;
    const int m = min(max(p.cand_nf[b], 0), fetch), m4 = (m + 3) & ~3;  // (m4 <= kGroupMaxFetch: a multiple of four itself)
    const int rounds = (m + kGroupThreads - 1) / kGroupThreads;
    const uint64_t *cid = p.cand_ids + (size_t)b * fetch;
    uint32_t key[kGroupPer];
#pragma unroll
    for (int e = 0; e < kGroupPer; ++e) {
        const int j = e * kGroupThreads + tid;
        key[e] = 0;
        if (j < m) {
            const uint64_t id = cid[j];
            if (id > p.id_offset && id - p.id_offset - 1 < p.len) key[e] = p.keys[id - p.id_offset - 1];
        }
        if (j < m4) skey[j] = key[e];
    }
    __syncthreads();
    uint32_t before[kGroupPer], total[kGroupPer];
#pragma unroll
    for (int e = 0; e < kGroupPer; ++e) before[e] = total[e] = 0;
    bool keyed = false;
#pragma unroll
    for (int e = 0; e < kGroupPer; ++e) keyed = keyed || key[e] != 0;
    if (keyed) {
        for (int i = 0; i < m4; i += 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(skey + i);
#pragma unroll
            for (int e = 0; e < kGroupPer; ++e) {
                const int j = e * kGroupThreads + tid;
                const uint32_t kj = key[e];  // (an entry with key 0 counts the zeros: never read)
                const uint32_t c0 = v.x == kj, c1 = v.y == kj, c2 = v.z == kj, c3 = v.w == kj;
                total[e] += c0 + c1 + c2 + c3;
                before[e] += (c0 & (uint32_t)(i < j)) + (c1 & (uint32_t)(i + 1 < j)) + (c2 & (uint32_t)(i + 2 < j)) +
                             (c3 & (uint32_t)(i + 3 < j));
            }
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
    uint64_t *oid = p.ids + (size_t)b * k;
    int base = 0;  // heads in the rounds before this one (the same in every thread)
#pragma unroll
    for (int e = 0; e < kGroupPer; ++e) {
        if (e >= rounds || base >= k) break;  // (block-uniform)
        const int j = e * kGroupThreads + tid;
        const bool head = j < m && (key[e] == 0 || before[e] == 0);
        const unsigned long long bal = __ballot(head);
        if (lane == 0) s_wsum[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        int wbase = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kGroupWaves; ++w) {
            const int v = (int)s_wsum[w];
            wbase += w < wave ? v : 0;
            tot += v;
        }
        const int slot = base + wbase + (int)__popcll(bal & ((1ull << lane) - 1ull));
        if (head && slot < k) {
            const size_t src = (size_t)b * fetch + j, dst = (size_t)b * k + slot;
            oid[slot] = cid[j];
            p.scores[dst] = p.cand_scores[src];
            if (p.dists) p.dists[dst] = p.cand_dists[src];
            if (p.out_keys) p.out_keys[dst] = key[e];
            if (p.group_rows) p.group_rows[dst] = key[e] == 0 ? 1 : (int32_t)total[e];
        }
        base += tot;
        __syncthreads();  // s_wsum is written again in the next round
    }
    const int nf = min(base, k);
    for (int s = nf + tid; s < k; s += kGroupThreads) {
        const size_t dst = (size_t)b * k + s;
        oid[s] = 0;
        p.scores[dst] = 0.0f;
        if (p.dists) p.dists[dst] = INFINITY;
        if (p.out_keys) p.out_keys[dst] = 0;
        if (p.group_rows) p.group_rows[dst] = 0;
    }
    if (tid == 0) {
        p.n_found[b] = nf;
        if (p.complete) p.complete[b] = (nf == k || m < fetch) ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_grouping_range_edit(hipStream_t s, const uint64_t *ranges, const uint32_t *rkeys, uint32_t n_ranges, uint64_t row0,
                                      uint64_t row1, uint32_t *keys) {
    if (n_ranges == 0 || row0 >= row1) return hipSuccess;
    const uint64_t blocks = (row1 - row0 + kEditThreads - 1) / kEditThreads;
    if (!ranges || !rkeys || !keys || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grouping_range_edit_kernel, dim3((unsigned)blocks), dim3(kEditThreads), 0, s, ranges, rkeys, n_ranges, row0, row1, keys);
    return hipGetLastError();
}

hipError_t launch_grouping_id_edit(hipStream_t s, const uint64_t *ids, const uint32_t *ikeys, uint64_t n_ids, uint64_t id_offset,
                                   uint64_t limit, uint32_t *keys) {
    if (n_ids == 0 || limit == 0) return hipSuccess;
    const uint64_t blocks = (n_ids + kEditThreads - 1) / kEditThreads;
    if (!ids || !ikeys || !keys || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grouping_id_edit_kernel, dim3((unsigned)blocks), dim3(kEditThreads), 0, s, ids, ikeys, n_ids, id_offset, limit, keys);
    return hipGetLastError();
}

hipError_t launch_grouping_get(hipStream_t s, const uint64_t *ids, uint64_t n_ids, uint64_t id_offset, uint64_t limit, const uint32_t *keys,
                               uint32_t *out) {
    if (n_ids == 0) return hipSuccess;
    const uint64_t blocks = (n_ids + kEditThreads - 1) / kEditThreads;
    if (!ids || !out || (limit && !keys) || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grouping_get_kernel, dim3((unsigned)blocks), dim3(kEditThreads), 0, s, ids, n_ids, id_offset, limit, keys, out);
    return hipGetLastError();
}

hipError_t launch_grouping_count(hipStream_t s, const uint32_t *keys, uint64_t n, const uint64_t *dead, uint64_t *part) {
    if (!part || (n && !keys)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grouping_count_kernel, dim3(kGroupCountBlocks), dim3(kGroupThreads), 0, s, keys, n, dead, part);
    return hipGetLastError();
}

hipError_t launch_group_heads(hipStream_t s, const GroupHeads &p) {
    if (p.B <= 0) return hipSuccess;
    if (p.k < 1 || p.fetch < p.k || p.fetch > kGroupMaxFetch || (p.len && !p.keys) || !p.cand_ids || !p.cand_scores || !p.cand_nf || !p.ids ||
        !p.scores || !p.n_found || (p.dists && !p.cand_dists))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_heads_kernel, dim3(p.B), dim3(kGroupThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mx
