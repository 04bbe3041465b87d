// compact.hip -- device side of mx_index_compact: where every live row goes, the in-place gather of
// the padded rows, and the re-listing of the side lists.  Everything here is a bitwise copy: the rescoring stages read the
// moved values, so nothing is recomputed.
#include <type_traits>

#include "index_kernels.h"

namespace mx {

namespace {

constexpr int kCountThreads = 256;
constexpr int kCountPer = kCompactTilesPerBlock / kCountThreads;  // tiles per thread
static_assert(kCompactTilesPerBlock % kCountThreads == 0, "tiles per block must divide over the block");

// live rows of 64-row tile t of an index of n rows: not removed, and below n
__device__ __forceinline__ uint64_t live_bits(const uint64_t *dead, uint64_t n, uint64_t t) {
    const uint64_t r0 = t * (uint64_t)kTile8Rows;
    const uint64_t valid = n - r0 >= (uint64_t)kTile8Rows ? ~0ull : (1ull << (n - r0)) - 1ull;
    return ~dead[t] & valid;
}

// exclusive prefix of v over the block's 256 threads; *total = the block's sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *lds, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kCountThreads / 64; ++i) {
        before += i < w ? lds[i] : 0u;
        all += lds[i];
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// level 1: per tile, the live rows before it within its block of kCompactTilesPerBlock tiles; per block, its live rows
__global__ __launch_bounds__(kCountThreads) void tile_count_kernel(const uint64_t *__restrict__ dead, uint64_t n, uint64_t tiles,
                                                                  uint32_t *__restrict__ tile_base, uint32_t *__restrict__ blk_sum) {
    __shared__ uint32_t lds[kCountThreads / 64];
    const uint64_t t0 = (uint64_t)blockIdx.x * kCompactTilesPerBlock + (uint64_t)threadIdx.x * kCountPer;
    uint32_t c[kCountPer], mine = 0;
#pragma unroll
    for (int i = 0; i < kCountPer; ++i) {
        c[i] = t0 + i < tiles ? (uint32_t)__popcll(live_bits(dead, n, t0 + i)) : 0u;
        mine += c[i];
    }
    uint32_t total = 0;
    uint32_t at = block_excl_scan(mine, lds, &total);
#pragma unroll
    for (int i = 0; i < kCountPer; ++i) {
        if (t0 + i < tiles) tile_base[t0 + i] = at;
        at += c[i];
    }
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
}

// level 2: exclusive prefix of the block sums in place (one workgroup walks them 256 at a time); blk_sum[nb] = live rows
__global__ __launch_bounds__(kCountThreads) void block_scan_kernel(uint32_t *__restrict__ blk_sum, uint32_t nb) {
    __shared__ uint32_t lds[kCountThreads / 64];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += kCountThreads) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < nb ? blk_sum[b] : 0u;
        uint32_t total = 0;
        const uint32_t ex = block_excl_scan(v, lds, &total);
        if (b < nb) blk_sum[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) blk_sum[nb] = carry;
}

// One workgroup per 64-row source tile: the tile's live rows are copied, in order, to rows dst_row(t, j) - dst0 of dst, where
// dst_row = (live rows before tile t) + (live rows of tile t below row j).  Rows are W floats (W / VEC vectors of VEC floats);
// consecutive threads take consecutive vectors of consecutive rows, so loads and stores stay coalesced.  src points at row
// 64 tile0 of the source; scale (optional) moves with its row.
template <int VEC>
__global__ __launch_bounds__(256) void compact_gather_kernel(const uint64_t *__restrict__ dead, uint64_t n, uint64_t tile0,
                                                             const uint32_t *__restrict__ tile_base, const uint32_t *__restrict__ blk_off,
                                                             const float *__restrict__ src, const float *__restrict__ src_scale, int W,
                                                             uint64_t dst0, float *__restrict__ dst, float *__restrict__ dst_scale) {
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    const uint64_t t = tile0 + blockIdx.x;
    const uint64_t live = live_bits(dead, n, t);
    if (live == 0) return;
    const uint64_t base = (uint64_t)tile_base[t] + blk_off[t / kCompactTilesPerBlock] - dst0;
    const int nv = W / VEC;
    const int total = kTile8Rows * nv;
    const V *s = reinterpret_cast<const V *>(src + (uint64_t)blockIdx.x * kTile8Rows * (uint64_t)W);
    V *d = reinterpret_cast<V *>(dst);
    constexpr int kUnroll = 4;  // loads of four vectors in flight before their stores
    for (int i0 = threadIdx.x; i0 < total; i0 += 256 * kUnroll) {
        V v[kUnroll];
        int j[kUnroll], c[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int i = i0 + u * 256;
            j[u] = i / nv;
            c[u] = i - j[u] * nv;
            if (i < total && ((live >> j[u]) & 1ull)) v[u] = s[i];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int i = i0 + u * 256;
            if (i < total && ((live >> j[u]) & 1ull)) {
                const uint64_t r = base + (uint64_t)__popcll(live & ((1ull << j[u]) - 1ull));
                d[r * (uint64_t)nv + (uint64_t)c[u]] = v[u];
            }
        }
    }
    if (src_scale && threadIdx.x < kTile8Rows) {
        const int jj = threadIdx.x;
        if ((live >> jj) & 1ull) {
            const uint64_t r = base + (uint64_t)__popcll(live & ((1ull << jj) - 1ull));
            dst_scale[r] = src_scale[(uint64_t)blockIdx.x * kTile8Rows + jj];
        }
    }
}

// f32 corpus: rows [0, n) -> the zero-norm list (1/|c| = 0, every value zero) and the list of rows with an out-of-range norm
// (1/|c| = 0, values kept: ingest_kernel's raw & 2 rule), counted in flags[3] / flags[4] behind whatever they hold
__global__ __launch_bounds__(256) void relist_kernel(const float *__restrict__ x, const float *__restrict__ scale, uint64_t n, int ds,
                                                     uint32_t *flags, uint32_t *__restrict__ zero_rows, uint32_t *__restrict__ wild_rows) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) {
        if (scale[r] != 0.0f) continue;
        bool any = false;
        const float *row = x + r * (uint64_t)ds;
        for (int c = 0; c < ds && !any; ++c) any = row[c] != 0.0f;
        if (any) {
            const uint32_t at = atomicAdd(&flags[4], 1u);
            if (at < (uint32_t)kWildCap) wild_rows[at] = (uint32_t)r;
        } else {
            const uint32_t at = atomicAdd(&flags[3], 1u);
            if (at < (uint32_t)kZeroCap) zero_rows[at] = (uint32_t)r;
        }
    }
}

}  // namespace

uint32_t compact_count_blocks(uint64_t tiles) { return (uint32_t)((tiles + kCompactTilesPerBlock - 1) / kCompactTilesPerBlock); }

hipError_t launch_compact_prefix(hipStream_t s, const uint64_t *dead, uint64_t n, uint32_t *tile_base, uint32_t *blk_off) {
    const uint64_t tiles = (n + kTile8Rows - 1) / kTile8Rows;
    const uint32_t nb = compact_count_blocks(tiles);
    if (nb == 0) return hipMemsetAsync(blk_off, 0, sizeof(uint32_t), s);
    hipLaunchKernelGGL(tile_count_kernel, dim3(nb), dim3(kCountThreads), 0, s, dead, n, tiles, tile_base, blk_off);
    hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(kCountThreads), 0, s, blk_off, nb);
    return hipGetLastError();
}

hipError_t launch_compact_gather(hipStream_t s, const uint64_t *dead, uint64_t n, uint64_t tile0, uint64_t tiles, const uint32_t *tile_base,
                                 const uint32_t *blk_off, const float *src, const float *src_scale, int W, uint64_t dst0, float *dst,
                                 float *dst_scale) {
    if (tiles == 0) return hipSuccess;
    if (W % 4 == 0)
        hipLaunchKernelGGL(compact_gather_kernel<4>, dim3((unsigned)tiles), dim3(256), 0, s, dead, n, tile0, tile_base, blk_off, src, src_scale, W,
                           dst0, dst, dst_scale);
    else
        hipLaunchKernelGGL(compact_gather_kernel<1>, dim3((unsigned)tiles), dim3(256), 0, s, dead, n, tile0, tile_base, blk_off, src, src_scale, W,
                           dst0, dst, dst_scale);
    return hipGetLastError();
}

hipError_t launch_relist(hipStream_t s, const float *x, const float *scale, uint64_t n, int ds, uint32_t *flags, uint32_t *zero_rows,
                         uint32_t *wild_rows) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(relist_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, scale, n, ds, flags, zero_rows, wild_rows);
    return hipGetLastError();
}

}  // namespace mx
