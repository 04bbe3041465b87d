// scan_common.h -- what the four streaming scans (scan.hip, scan16.hip, scan16w.hip, scan8.hip) share: vector types, the LDS-DMA
// operation, compile-time loops, the tile geometry, the tile epilogue that writes the records finish_kernel reads, and the
// variant table that drives both a scan's set-up and its launch.  Each scan file says only what is different about it.
#pragma once
#include <climits>
#include <cstddef>
#include <type_traits>

#include "index_kernels.h"

namespace mx {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef __attribute__((address_space(3))) void lds_void;

// 16 bytes per lane from a buffer descriptor straight into LDS (no VGPR staging); the LDS image is lane-linear
#define MX_LDS_DMA16(rsrc, ldsptr, voff, soff, aux) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds((rsrc), (lds_void *)(ldsptr), 16, (voff), (soff), 0, (aux))

template <int N>
using ic = std::integral_constant<int, N>;
// f(ic<B>{}), ..., f(ic<E - 1>{}): a loop whose index is a compile-time constant in the body ("n" asm operands, if constexpr)
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (B < E) {
        f(ic<B>{});
        static_for<B + 1, E>(f);
    }
}

// DMA operations a wave has issued after the last one of slot j+1 when it waits for that slot: the slots lo .. hi (relative to
// the tile start; RING - 3 of them, 13 with the 16-slot ring), DPS operations each (a wave's share of a slot's eight 1-KiB
// pieces), plus the TOPS per-tile operations of every tile that starts among them.  The scans' wait schedules are these
// numbers; each kernel keeps static_asserts on the ones it relies on.
template <int KC, int DPS = 1, int TOPS = 2>
constexpr int ops_after(int lo, int hi) {
    int n = 0;
    for (int i = lo; i <= hi; ++i) n += DPS + (i % KC == 0 ? TOPS : 0);
    return n;
}

// One barrier per slot behind the counted wait for it: the slot is in LDS for every wave of the workgroup, and the ring position
// that is refilled next is free.
template <int VM>
__device__ __forceinline__ void wait_slot() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
    __builtin_amdgcn_s_barrier();
}
// ... at a tile's first slot in a DEAD kernel: also fetches the tile's 64-row word of removed rows, with one SCALAR load whose
// latency hides under the slot wait and the barrier.  (A plain load would be a vector load outside the ring's counted vmcnt
// waits, and the compiler's vmcnt(0) in front of its use would drain the ring once per tile.)  lgkmcnt(0) sits behind them in
// the same statement, so that no LDS wait the compiler counts runs while the load is in flight.
template <int VM>
__device__ __forceinline__ uint64_t wait_slot_dead(const uint64_t *word) {
    uint64_t dw;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt vmcnt(%2)\n\ts_barrier\n\ts_waitcnt lgkmcnt(0)" : "=s"(dw) : "s"(word), "n"(VM) : "memory");
    return dw;
}

// Tiles of a workgroup: t0 + i * tstep for i < nT (workgroup b handles tile_begin + (b + i * grid) * tile_stride < tile_end).
// The bf16 and int8 streams keep issuing past their last tile on a descriptor of 0 bytes: every lane is out of range, the
// operation reads no memory, and the loop needs no "is there more?" branch and keeps uniform vmcnt arithmetic.
// tile_stride > 1 spreads the sample evenly over the corpus (a contiguous head can be unrepresentative: the first documents ingested).
struct TileSpan {
    uint32_t t0, tstep, nT;
};
__device__ __forceinline__ TileSpan tile_span(const ScanParams &p) {
    const uint32_t grid = gridDim.x;
    const uint32_t stride = p.tile_stride;
    const uint32_t t0 = p.tile_begin + blockIdx.x * stride;
    const uint32_t tstep = grid * stride;
    return {t0, tstep, (t0 < p.tile_end) ? (p.tile_end - t0 + tstep - 1) / tstep : 0};
}

// ---- tile epilogue --------------------------------------------------------------------------------------------------------
// With A = corpus rows and B = queries, an MFMA lane ends a 32-row tile holding the 16 scores of ONE query (column lane & 31)
// against rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  Lane buffers are laid out [thread-in-workgroup][workgroup], so everything
// one query ever receives (2 lanes x all workgroups) is contiguous for the gathers of theta_kernel and finish_kernel, which know
// of the scan that ran only whether its records hold floats or integers.
//   MODE 1 (collect): a lane whose maximum reaches the query's pass threshold (one wave-uniform ballot branch, taken by a few
//     percent of the tiles) stores ALL 16 scores as one record -- 4 x f32x4 in lane_rec plus the 32-row tile index in lane_tile
//     -- and counts it in lane_cnt; which rows pass is sorted out by finish_kernel, so the stream carries no per-row code.  The
//     int8 scan (scan8_kernel) stores its 16 integer sums instead, in the same 64 bytes (INT_MIN for a removed row): the
//     readers, finish_kernel and range_finish_kernel, turn a sum into ((float)sum * s_h) * s_q -- the value the scan compared
//     with the threshold -- on the threads that hold a record (FinishParams::rec_int), so the wave-wide branch here is stores only.  A
//     lane has room for kRecCap records; one more sets overflow[query].  The count and the overflow flag are a kernel's own
//     registers: scan_kernel and scan16_kernel keep them apart, next to the lane's two buffer addresses; scan16w_kernel and
//     scan8_kernel are short of registers, keep the flag in bit 31 of the count and rebuild the addresses where a record is stored.
//   MODE 0 (sample): only the lane's running maximum is kept (lane_max).  The k-th largest of a query's lane maxima is a
//     certified lower bound of its k-th best approximate score, which theta_kernel turns into the collect launch's threshold:
//     no score of the sample is ever written to HBM.
// Removed rows (ScanParams::dead) get a fill value that passes no test and is no lower bound for the sample.
// hipcc optimises a kernel once before it inlines these helpers and once after.  They take values and lambdas (no ScanParams, no
// nested helper calls) and form an address where it is used: other shapes of the same arithmetic move the kernels' instruction
// order and register allocation.  scan_kernel's code moved with every shape tried, so scan.hip keeps its epilogue written out.

// the lane's 16 values (a vector) with `fill` in place of its removed rows; `half` = the dead-row bits of the values' 32 rows
template <class V, class T>
__device__ __forceinline__ V mask_dead16(V v, uint32_t half, int lane, T fill) {
    if (half) {
        const uint32_t lb = lane_dead16(half, (uint32_t)lane >> 5);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if ((lb >> r) & 1u) v[r] = fill;
    }
    return v;
}

__device__ __forceinline__ float max2(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int max2(int a, int b) { return max(a, b); }
// maximum of v[0 .. 15] (an array or a 16-element vector) as a v_max3 tree
template <class V>
__device__ __forceinline__ auto max16(const V &v) {
    auto mx = max2(max2(v[0], v[1]), v[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) mx = max2(max2(mx, v[r]), v[r + 1]);
    return max2(mx, v[15]);
}

// Record number `at` of the buffers rec (floats or f32x4) / tiles: score(0) .. score(15), then the 32-row tile index tile().
// `at` is a number, or a function of none where the kernel rebuilds the number at each use.  `score` is a function of r, or the
// lane's 16 integer sums as a vector (scan8_kernel), which go out as they are.
template <class R, class A, class T, class F>
__device__ __forceinline__ void store_record(R *rec, uint32_t *tiles, A at, T tile, F score) {
    constexpr int k = 64 / sizeof(R);  // a record in units of R
    f32x4 *dst;
    if constexpr (std::is_invocable_v<A &>) dst = reinterpret_cast<f32x4 *>(rec + at() * k);
    else dst = reinterpret_cast<f32x4 *>(rec + at * k);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (std::is_invocable_v<F &, int>) dst[i] = f32x4{score(4 * i), score(4 * i + 1), score(4 * i + 2), score(4 * i + 3)};
        else reinterpret_cast<i32x4 *>(dst)[i] = i32x4{score[4 * i], score[4 * i + 1], score[4 * i + 2], score[4 * i + 3]};
    }
    if constexpr (std::is_invocable_v<A &>) tiles[at()] = tile();
    else tiles[at] = tile();
}

// what a lane leaves behind at the end of the launch: entry lane() of lane_max, or of lane_cnt and (set only) its query's overflow word;
// a sample launch that tracks which row gave the maximum (scan8_kernel, plain copy) also leaves that row in lane_arg
template <int MODE, class L>
__device__ __forceinline__ void write_lane(float *lane_max, uint32_t *lane_cnt, uint32_t *overflow, L lane, int query, float best, uint32_t cnt, uint32_t ovf,
                                           uint32_t *lane_arg = nullptr, uint32_t arg = kNoRow) {
    if (MODE == 0) {
        lane_max[lane()] = best;
        if (lane_arg) lane_arg[lane()] = arg;
    } else {
        lane_cnt[lane()] = cnt;
        if (ovf) overflow[query] = 1;
    }
}

// ---- variant table (host) -------------------------------------------------------------------------------------------------
// A scan kernel exists once per slot count KC, MODE (0 = sample, 1 = collect: distinct symbols, so rocprofv3 --stats averages them
// separately) and DEAD (the variant that honours ScanParams::dead, launched only when the index has removed rows).  A family is
// the list of its slot counts with the four instances of each, its dynamic LDS size and its workgroup size.  Set-up walks the
// list and launch looks the instance up in the same list, so nothing can be launched that set-up has not visited.
using ScanKernel = void (*)(const ScanParams);
struct ScanEntry {
    int kc;
    ScanKernel fn[2][2];  // [MODE][DEAD]
};
struct ScanFamily {
    const ScanEntry *entries;
    int n, lds_bytes, threads;
    template <int N>
    constexpr ScanFamily(const ScanEntry (&e)[N], int lds, int thr) : entries(e), n(N), lds_bytes(lds), threads(thr) {}
};

inline hipError_t scan_family_setup(const ScanFamily &f) {  // one-time function attributes (dynamic LDS size)
    for (int i = 0; i < f.n; ++i)
        for (int v = 0; v < 4; ++v) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(f.entries[i].fn[v >> 1][v & 1]),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, f.lds_bytes);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

inline hipError_t scan_family_launch(const ScanFamily &f, hipStream_t s, int kc, bool collect, int nwg, const ScanParams &p) {
    for (int i = 0; i < f.n; ++i) {
        if (f.entries[i].kc != kc) continue;
        void *args[] = {const_cast<ScanParams *>(&p)};
        (void)hipLaunchKernel(reinterpret_cast<const void *>(f.entries[i].fn[collect][p.dead != nullptr]), dim3(nwg), dim3(f.threads),
                              args, f.lds_bytes, s);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

}  // namespace mx
