// group_rows_kernels.hip -- the kernels of grouped search with members (mx_index_search_group_rows, mx_index_search_capped,
// mx_grouping_key_counts).  A translation unit of their own: the code objects of group_kernels.hip and of the
// headline path stay what they were.  Integer work only: keys are compared, list entries are copied unchanged.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "index_kernels.h"

namespace mx {

namespace {

constexpr int kGroupPer = kGroupMaxFetch / kGroupThreads;  // entries a thread owns: t, t + 1024, ...
constexpr int kGroupWaves = kGroupThreads / 64;
constexpr int kCountThreads = 256;
constexpr uint32_t kNoHead = 0xffffu;  // (a head's number is below k <= 4096)

// One workgroup per query, the layout of group_heads_kernel: thread t takes entries t, t + 1024, ...: id -> global row -> key, into LDS
// (padded with zeros to a multiple of four entries).  One walk over the key array, four keys per LDS read, gives each owned entry its
// RANK (the equal keys before it) and, for the group-rows form, the TOTAL under its key and the index of the FIRST equal key: its
// head.  The selected entries -- the heads; capped: key 0 or rank < per_key -- are numbered in list order, 1024 per round (ballot and
// popcount in the wave, the waves' sums through LDS).
//   capped      a selected entry with number s < k goes to slot s.
//   group rows  a head with number h < k leaves h in s_num[its index], writes slot [h, 0], the per-head outputs and the blanks of its
//               own row; after a barrier an entry with 0 < rank < n reads h = s_num[first] and, if h < k, writes slot [h, rank].
// Every output word is written by exactly one thread, with plain stores.
template <bool kCapped>
__global__ __launch_bounds__(kGroupThreads) void group_rows_kernel(GroupRows p) {
    __shared__ __attribute__((aligned(16))) uint32_t skey[kGroupMaxFetch];
    __shared__ uint16_t s_num[kGroupMaxFetch];
    __shared__ uint32_t s_wsum[kGroupWaves];
    const int b = blockIdx.x, tid = threadIdx.x, k = p.k, n = kCapped ? 1 : p.n, fetch = p.fetch;
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
        if (!kCapped) s_num[j] = (uint16_t)kNoHead;
    }
    __syncthreads();
    uint32_t before[kGroupPer], total[kGroupPer], first[kGroupPer];
#pragma unroll
    for (int e = 0; e < kGroupPer; ++e) {
        before[e] = total[e] = 0;
        first[e] = (uint32_t)(e * kGroupThreads + tid);  // (no equal key lies behind the entry's own index and before it at once)
    }
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
                before[e] += (c0 & (uint32_t)(i < j)) + (c1 & (uint32_t)(i + 1 < j)) + (c2 & (uint32_t)(i + 2 < j)) +
                             (c3 & (uint32_t)(i + 3 < j));
                if (!kCapped) {
                    total[e] += c0 + c1 + c2 + c3;
                    const uint32_t f = c0 ? (uint32_t)i : c1 ? (uint32_t)(i + 1) : c2 ? (uint32_t)(i + 2) : c3 ? (uint32_t)(i + 3) : kNoHead;
                    first[e] = min(first[e], f);
                }
            }
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
    int base = 0;  // selected entries in the rounds before this one (the same in every thread)
#pragma unroll
    for (int e = 0; e < kGroupPer; ++e) {
        if (e >= rounds || base >= k) break;  // (block-uniform)
        const int j = e * kGroupThreads + tid;
        const bool sel = j < m && (key[e] == 0 || before[e] < (uint32_t)(kCapped ? p.per_key : 1));
        const unsigned long long bal = __ballot(sel);
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
        if (sel && slot < k) {
            const size_t src = (size_t)b * fetch + j, head = (size_t)b * k + slot, dst = head * n;
            p.ids[dst] = cid[j];
            p.scores[dst] = p.cand_scores[src];
            if (p.dists) p.dists[dst] = p.cand_dists[src];
            if (p.out_keys) p.out_keys[head] = key[e];
            if (!kCapped) {
                const int rows = key[e] == 0 ? 1 : (int)total[e], mem = min(n, rows);
                s_num[j] = (uint16_t)slot;
                if (p.group_rows) p.group_rows[head] = rows;
                if (p.n_members) p.n_members[head] = mem;
                if (p.members_complete) p.members_complete[head] = (mem == n || m < fetch || key[e] == 0) ? 1 : 0;
                for (int r = mem; r < n; ++r) {  // the slots of this group no entry of the list fills
                    p.ids[dst + r] = 0;
                    p.scores[dst + r] = 0.0f;
                    if (p.dists) p.dists[dst + r] = INFINITY;
                }
            }
        }
        base += tot;
        __syncthreads();  // s_wsum is written again in the next round; s_num is read below
    }
    const int nf = min(base, k);
    if (!kCapped && n > 1) {
#pragma unroll
        for (int e = 0; e < kGroupPer; ++e) {
            const int j = e * kGroupThreads + tid;
            if (j >= m || key[e] == 0 || before[e] == 0 || before[e] >= (uint32_t)n) continue;
            const uint32_t h = s_num[first[e]];  // (first < j < m)
            if (h >= (uint32_t)k) continue;      // its head is behind the first k
            const size_t src = (size_t)b * fetch + j, dst = ((size_t)b * k + h) * n + before[e];
            p.ids[dst] = cid[j];
            p.scores[dst] = p.cand_scores[src];
            if (p.dists) p.dists[dst] = p.cand_dists[src];
        }
    }
    for (int s = nf * n + tid; s < k * n; s += kGroupThreads) {
        const size_t dst = (size_t)b * k * n + s;
        p.ids[dst] = 0;
        p.scores[dst] = 0.0f;
        if (p.dists) p.dists[dst] = INFINITY;
    }
    for (int s = nf + tid; s < k; s += kGroupThreads) {
        const size_t head = (size_t)b * k + s;
        if (p.out_keys) p.out_keys[head] = 0;
        if (!kCapped) {
            if (p.group_rows) p.group_rows[head] = 0;
            if (p.n_members) p.n_members[head] = 0;
            if (p.members_complete) p.members_complete[head] = 0;
        }
    }
    if (tid == 0) {
        p.n_found[b] = nf;
        if (p.complete) p.complete[b] = (nf == k || m < fetch) ? 1 : 0;
    }
}

// One thread per row of [0, rows): its key (0 at or past len) is looked up in the sorted list of distinct keys by binary search; a row
// whose key is listed adds one to that key's row counter and, when its bit in `dead` is clear, to its live counter.  Integer sums.
__global__ __launch_bounds__(kCountThreads) void grouping_key_counts_kernel(const uint32_t *__restrict__ keys, uint64_t len, uint64_t rows,
                                                                            const uint64_t *__restrict__ dead,
                                                                            const uint32_t *__restrict__ sorted, uint32_t n_sorted,
                                                                            unsigned long long *__restrict__ counts) {
    const uint64_t r = (uint64_t)blockIdx.x * kCountThreads + threadIdx.x;
    if (r >= rows) return;
    const uint32_t key = r < len ? keys[r] : 0u;
    uint32_t lo = 0, hi = n_sorted;  // the first listed key >= key is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    if (lo == n_sorted || sorted[lo] != key) return;
    atomicAdd(counts + 2 * (size_t)lo, 1ull);
    if (!(dead && ((dead[r >> 6] >> (r & 63u)) & 1ull))) atomicAdd(counts + 2 * (size_t)lo + 1, 1ull);
}

}  // namespace

hipError_t launch_group_rows(hipStream_t s, const GroupRows &p) {
    if (p.B <= 0) return hipSuccess;
    const bool capped = p.per_key > 0;
    if (p.k < 1 || p.fetch < p.k || p.fetch > kGroupMaxFetch || (p.len && !p.keys) || !p.cand_ids || !p.cand_scores || !p.cand_nf || !p.ids ||
        !p.scores || !p.n_found || (p.dists && !p.cand_dists))
        return hipErrorInvalidValue;
    if (capped ? p.n != 1 : (p.n < 1 || p.n > kGroupMaxMembers || (long long)p.k * p.n > kGroupMaxFetch)) return hipErrorInvalidValue;
    if (capped) hipLaunchKernelGGL(group_rows_kernel<true>, dim3(p.B), dim3(kGroupThreads), 0, s, p);
    else hipLaunchKernelGGL(group_rows_kernel<false>, dim3(p.B), dim3(kGroupThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_grouping_key_counts(hipStream_t s, const uint32_t *keys, uint64_t len, uint64_t rows, const uint64_t *dead,
                                      const uint32_t *sorted, uint32_t n_sorted, uint64_t *counts) {
    if (rows == 0 || n_sorted == 0) return hipSuccess;
    const uint64_t blocks = (rows + kCountThreads - 1) / kCountThreads;
    if (!sorted || !counts || (len && !keys) || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grouping_key_counts_kernel, dim3((unsigned)blocks), dim3(kCountThreads), 0, s, keys, len, rows, dead, sorted, n_sorted,
                       reinterpret_cast<unsigned long long *>(counts));
    return hipGetLastError();
}

}  // namespace mx
