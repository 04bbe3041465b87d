// where_kernels.hip -- the kernels that build a resident filter from what the rows already carry (mx_filter_set_where,
// mx_filter_set_keys, mx_filter_combine, mx_filter_invert).  A translation unit of their own, like
// group_kernels.hip and boost_kernels.hip: the code object of index_kernels.hip, which holds kernels of the headline path, stays what
// it was.  The two predicate kernels write a SELECTION bitmap, one bit per global row of the handle; filter_words_kernel folds a
// selection, or another filter's bits, into a filter's words.  The only arithmetic is two IEEE f32 compares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "index_kernels.h"

namespace mx {

namespace {

// lanes of a wave hold 64 consecutive rows that start at a multiple of 64: their ballot is the selection word of those rows
static_assert(kWhereThreads % 64 == 0, "a wave of where_*_kernel owns whole selection words");

// One thread per row, grid-stride over the rows rounded up to whole words.  A row at or past `len` reads 0, as mx_prior_get reads it;
// a lane at or past `rows` votes 0, which masks the tail word.  Lane 0 of each wave stores the wave's word: sel[w], w < (rows + 63) / 64,
// has exactly one writer.
__global__ __launch_bounds__(kWhereThreads) void where_range_kernel(const float *__restrict__ vals, uint64_t len, uint64_t rows, float lo,
                                                                    float hi, uint64_t *__restrict__ sel) {
    const uint64_t step = (uint64_t)gridDim.x * kWhereThreads;
    for (uint64_t base = (uint64_t)blockIdx.x * kWhereThreads + (threadIdx.x & ~63u); base < rows; base += step) {
        const uint64_t r = base + (threadIdx.x & 63u);
        const float v = r < len ? vals[r] : 0.0f;
        const uint64_t word = __ballot(r < rows && lo <= v && v <= hi);
        if ((threadIdx.x & 63u) == 0) sel[base >> 6] = word;
    }
}

// The same shape; the predicate is a binary search of the row's key (0 at or past `len`) in sorted[0, n_sorted), ascending and without
// repeats, n_sorted >= 1.
__global__ __launch_bounds__(kWhereThreads) void where_keys_kernel(const uint32_t *__restrict__ keys, uint64_t len, uint64_t rows,
                                                                   const uint32_t *__restrict__ sorted, uint32_t n_sorted,
                                                                   uint64_t *__restrict__ sel) {
    const uint64_t step = (uint64_t)gridDim.x * kWhereThreads;
    for (uint64_t base = (uint64_t)blockIdx.x * kWhereThreads + (threadIdx.x & ~63u); base < rows; base += step) {
        const uint64_t r = base + (threadIdx.x & 63u);
        const uint32_t key = r < len ? keys[r] : 0u;
        uint32_t a = 0, b = n_sorted;  // the first entry >= key is in [a, b]
        while (a < b) {
            const uint32_t m = a + (b - a) / 2;
            if (sorted[m] < key) a = m + 1;
            else b = m;
        }
        const uint64_t word = __ballot(r < rows && a < n_sorted && sorted[a] == key);
        if ((threadIdx.x & 63u) == 0) sel[base >> 6] = word;
    }
}

// One thread per word: dst[w] = a[w] OP b[w].  b null: the word of the pattern "every row below size".  dst may be a or b and a may be
// b (a thread reads its two words before it writes its one), so none of the three is __restrict__.
__global__ __launch_bounds__(kWhereThreads) void filter_words_kernel(uint64_t *dst, const uint64_t *a, const uint64_t *b, uint64_t words,
                                                                     int op, uint64_t size) {
    const uint64_t w = (uint64_t)blockIdx.x * kWhereThreads + threadIdx.x;
    if (w >= words) return;
    const uint64_t x = a[w];
    uint64_t y;
    if (b) y = b[w];
    else y = size >= (w + 1) * 64 ? ~0ull : size <= w * 64 ? 0ull : (1ull << (size - w * 64)) - 1ull;
    dst[w] = op == kFilterAnd ? x & y : op == kFilterOr ? x | y : op == kFilterAndNot ? x & ~y : x ^ y;
}

unsigned where_blocks(uint64_t rows) {
    return (unsigned)std::min<uint64_t>((rows + kWhereThreads - 1) / kWhereThreads, kWhereMaxBlocks);
}

}  // namespace

hipError_t launch_where_range(hipStream_t s, const float *vals, uint64_t len, uint64_t rows, float lo, float hi, uint64_t *sel) {
    if (rows == 0) return hipSuccess;
    if (!sel || (len && !vals)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(where_range_kernel, dim3(where_blocks(rows)), dim3(kWhereThreads), 0, s, vals, len, rows, lo, hi, sel);
    return hipGetLastError();
}

hipError_t launch_where_keys(hipStream_t s, const uint32_t *keys, uint64_t len, uint64_t rows, const uint32_t *sorted, uint32_t n_sorted,
                             uint64_t *sel) {
    if (rows == 0) return hipSuccess;
    if (!sel || (len && !keys) || !sorted || n_sorted == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(where_keys_kernel, dim3(where_blocks(rows)), dim3(kWhereThreads), 0, s, keys, len, rows, sorted, n_sorted, sel);
    return hipGetLastError();
}

hipError_t launch_filter_words(hipStream_t s, uint64_t *dst, const uint64_t *a, const uint64_t *b, uint64_t words, int op, uint64_t size) {
    if (words == 0) return hipSuccess;
    if (!dst || !a || op < kFilterAnd || op > kFilterXor || words > 0x7fffffffull * kWhereThreads) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_words_kernel, dim3((unsigned)((words + kWhereThreads - 1) / kWhereThreads)), dim3(kWhereThreads), 0, s, dst, a, b,
                       words, op, size);
    return hipGetLastError();
}

}  // namespace mx
