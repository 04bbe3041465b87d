// score_kernels.hip -- the kernels of the scoring of named rows (mx_index_score_ids).  A translation unit of
// their own: the code object of index_kernels.hip, which holds kernels of the headline path, stays what it was.  Exact arithmetic:
// built without FMA contraction, like index_kernels.hip, and through the same exact_dist_stored (mx_exact_dist.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "index_kernels.h"
#include "mx_exact_dist.h"

namespace mx {

namespace {

constexpr int kScorePer = kScoreMaxIds / kScoreThreads;  // entries a thread owns: t, t + 1024, ...
constexpr int kScoreWaves = kScoreThreads / 64;
constexpr uint32_t kInfBits = 0x7f800000u;
// One workgroup's LDS, used twice: the raw padded query while the entries are scored (kMmrMaxDs floats, 32 KiB), then the keys of
// the ranking -- ids [kScoreMaxIds] u64 (0: the entry is not found; no row has id 0) and dist bits [kScoreMaxIds] u32, 48 KiB
constexpr int kScoreLdsBytes = kScoreMaxIds * 12;
static_assert(kMmrMaxDs * 4 <= kScoreLdsBytes, "the query must fit the key area");

// id -> local row of the index (a shard: of its own blocks only, as filter_id_edit_kernel translates); false: the id names no row
// of this index
__device__ __forceinline__ bool score_locate(uint64_t id, const IdMap &im, uint64_t total, uint64_t n_rows, uint32_t *row) {
    if (id <= im.id_offset) return false;
    uint64_t r = id - im.id_offset - 1;
    if (r >= total) return false;
    if (im.block_rows) {  // a shard: rows of its own blocks only, global block b -> local block b / G
        const uint64_t b = r / im.block_rows;
        if (b % im.n_shards != im.shard) return false;
        r = (b / im.n_shards) * im.block_rows + r % im.block_rows;
    }
    if (r >= n_rows) return false;
    *row = (uint32_t)r;
    return true;
}

// The ranking of one query's m entries, whose keys the workgroup has in LDS (kid[j] = 0: entry j is not found): n_found = the found
// entries, order[rank] = j for every found entry, rank = the found entries with a smaller (dist bits, id, j); -1 behind them.  Keys are
// unique by j: every slot is written exactly once.  order null: the count alone.
__device__ __forceinline__ void score_rank(const uint64_t *kid, const uint32_t *kd, int m, int32_t *order, int32_t *n_found,
                                           uint32_t *s_cnt) {
    const int tid = threadIdx.x;
    uint32_t cnt = 0;
    for (int j = tid; j < m; j += kScoreThreads) cnt += kid[j] != 0 ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    uint32_t nf = 0;
#pragma unroll
    for (int w = 0; w < kScoreWaves; ++w) nf += s_cnt[w];
    if (tid == 0 && n_found) *n_found = (int32_t)nf;
    if (!order) return;
    for (int j = tid; j < m; j += kScoreThreads) {
        const uint64_t idj = kid[j];
        if (idj == 0) continue;
        const uint32_t dj = kd[j];
        uint32_t rank = 0;
        for (int i = 0; i < m; ++i) {  // (every lane reads the same key: LDS broadcasts)
            const uint64_t idi = kid[i];
            const uint32_t di = kd[i];
            const bool lt = di < dj || (di == dj && (idi < idj || (idi == idj && i < j)));
            rank += (idi != 0 && lt) ? 1u : 0u;
        }
        order[rank] = j;
    }
    for (int r = (int)nf + tid; r < m; r += kScoreThreads) order[r] = -1;
}

// One workgroup per query.  Thread t takes entries t, t + 1024, ...: id -> local row, the row's bit in `dead`, exact_dist_stored.
// Plain form (part null): dist and score into the caller's order, blank (score 0, dist +inf) where the entry is not found, then the
// ranking.  Shard form: the dist bits alone into part[b, j] -- kScoreNotMine where the id names no row of this shard, kScoreBlank for a
// row of this shard that is removed or has a NaN dist.
template <bool CMP>
__global__ __launch_bounds__(kScoreThreads) void score_ids_kernel(ScoreIds p) {
    __shared__ __attribute__((aligned(16))) char ssm[kScoreLdsBytes];
    __shared__ uint32_t s_cnt[kScoreWaves];
    float *qv = reinterpret_cast<float *>(ssm);
    const int b = blockIdx.x, tid = threadIdx.x, m = p.m, ds = p.ds;
    for (int i = tid; i < ds; i += kScoreThreads) qv[i] = p.qpad[(size_t)b * ds + i];
    __syncthreads();
    const double na = p.qnorm2[b];
    const uint64_t *cand = p.cand + (size_t)b * m;
    uint64_t id[kScorePer];
    uint32_t db[kScorePer];
#pragma unroll
    for (int e = 0; e < kScorePer; ++e) {
        const int j = e * kScoreThreads + tid;
        id[e] = 0;
        db[e] = p.part ? kScoreNotMine : kInfBits;
        if (j >= m) continue;
        const uint64_t cid = cand[j];
        uint32_t row;
        if (score_locate(cid, p.idmap, p.total, p.n_rows, &row)) {
            bool found = !(p.dead && ((p.dead[row >> 6] >> (row & 63u)) & 1ull));
            float d = 0.0f;
            if (found) {
                d = exact_dist_stored<CMP>(qv, p.x, p.xh, ds, row, na);
                found = d == d;  // a NaN dist: blank
            }
            id[e] = found ? cid : 0;
            db[e] = found ? __float_as_uint(d) : (p.part ? kScoreBlank : kInfBits);
        }
        if (p.part) {
            p.part[(size_t)b * m + j] = db[e];
        } else {
            p.scores[(size_t)b * m + j] = id[e] ? score_from_dist(__uint_as_float(db[e])) : 0.0f;
            if (p.dists) p.dists[(size_t)b * m + j] = __uint_as_float(db[e]);
        }
    }
    if (p.part || (!p.order && !p.n_found)) return;  // (block-uniform)
    __syncthreads();  // every thread is done with the query: the keys take its place
    uint64_t *kid = reinterpret_cast<uint64_t *>(ssm);
    uint32_t *kd = reinterpret_cast<uint32_t *>(ssm + sizeof(uint64_t) * kScoreMaxIds);
#pragma unroll
    for (int e = 0; e < kScorePer; ++e) {
        const int j = e * kScoreThreads + tid;
        if (j < m) {
            kid[j] = id[e];
            kd[j] = db[e];
        }
    }
    __syncthreads();
    score_rank(kid, kd, m, p.order ? p.order + (size_t)b * m : nullptr, p.n_found ? p.n_found + b : nullptr, s_cnt);
}

// One workgroup per query, on the device of the handle's first shard: entry (b, j) takes the one value among the G shard blocks that
// is not kScoreNotMine (none: the id names no row, blank), writes dist and score, and the ranking runs on the combined entries.
__global__ __launch_bounds__(kScoreThreads) void score_merge_kernel(ScoreMerge p) {
    __shared__ __attribute__((aligned(16))) char ssm[kScoreLdsBytes];
    __shared__ uint32_t s_cnt[kScoreWaves];
    uint64_t *kid = reinterpret_cast<uint64_t *>(ssm);
    uint32_t *kd = reinterpret_cast<uint32_t *>(ssm + sizeof(uint64_t) * kScoreMaxIds);
    const int b = blockIdx.x, tid = threadIdx.x, m = p.m;
    for (int j = tid; j < m; j += kScoreThreads) {
        const size_t at = (size_t)b * m + j;
        uint32_t v = kScoreNotMine;
        for (int g = 0; g < p.G && v == kScoreNotMine; ++g) v = p.parts[(size_t)g * p.stride + at];
        const bool found = v != kScoreNotMine && v != kScoreBlank;
        const float d = found ? __uint_as_float(v) : INFINITY;
        p.scores[at] = found ? score_from_dist(d) : 0.0f;
        if (p.dists) p.dists[at] = d;
        kid[j] = found ? p.cand[at] : 0;
        kd[j] = found ? v : kInfBits;
    }
    if (!p.order && !p.n_found) return;  // (block-uniform)
    __syncthreads();
    score_rank(kid, kd, m, p.order ? p.order + (size_t)b * m : nullptr, p.n_found ? p.n_found + b : nullptr, s_cnt);
}

}  // namespace

hipError_t launch_score_ids(hipStream_t s, const ScoreIds &p) {
    if (p.B <= 0) return hipSuccess;
    if (p.m < 1 || p.m > kScoreMaxIds || p.ds < 4 || p.ds > kMmrMaxDs || (p.ds & 3) || (!p.part && !p.scores)) return hipErrorInvalidValue;
    if (p.x) hipLaunchKernelGGL(score_ids_kernel<false>, dim3(p.B), dim3(kScoreThreads), 0, s, p);
    else hipLaunchKernelGGL(score_ids_kernel<true>, dim3(p.B), dim3(kScoreThreads), 0, s, p);  // compressed corpus
    return hipGetLastError();
}

hipError_t launch_score_merge(hipStream_t s, const ScoreMerge &p) {
    if (p.B <= 0) return hipSuccess;
    if (p.m < 1 || p.m > kScoreMaxIds || p.G < 1 || !p.scores) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_merge_kernel, dim3(p.B), dim3(kScoreThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mx
