// index_kernels.hip -- everything around the streaming scan: row ingest (K8), query preparation,
// candidate-pool maintenance, exact DistCosine rescoring + ordering (K7), the all-f64 EXACT path
// and the multi-GPU merge.  Compiled with -ffp-contract=off: the exact arithmetic below must
// round exactly like the reference's scalar Rust code.
//
// Reference arithmetic being reproduced (hnsw_rs 0.1.20 DistCosine, called from
// lib/libmemex/src/storage/local.rs:65,76; score formula local.rs:86):
//   dot = sum_i f64(f32(q_i*c_i)), na = sum_i f64(f32(q_i*q_i)), nb = sum_i f64(f32(c_i*c_i))
//   dist = (na>0 && nb>0) ? f32(max(1 - dot/sqrt(na*nb), 0)) : 0 ;  score = 1 - (1/(1/dist)) in f32
#include <cmath>

#include "index_kernels.h"
#include "mx_exact_dist.h"
#include "mx_rotate.h"

namespace mx {

typedef __attribute__((ext_vector_type(4))) float f32x4;

// ---------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f32_key(float f) {  // order-preserving map f32 -> u32
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}
// (score_from_dist, dist_from_sums, row_load4 and exact_dist_stored: mx_exact_dist.h)

// block-wide sum of a small unsigned value; every thread gets the result.  blockDim = 256.
__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t *lds4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}


// k-th largest of the u32 keys a block holds in registers (PER per thread; valid[e] marks real
// entries).  MSB-first radix select over the bits in which the keys actually differ (scores of one
// query share sign, exponent and leading mantissa bits), up to 8 bits per pass: LDS histogram of the
// digit among the keys that still match the prefix, one wave walks the bins from the top.
// hist: 256 words of LDS; s_pick: 2 words.  Requires 1 <= k <= number of valid keys, blockDim <= 1024.
template <int PER>
__device__ __forceinline__ uint32_t block_kth_largest(const uint32_t (&key)[PER], const bool (&valid)[PER], uint32_t k,
                                                      uint32_t *hist, uint32_t *s_pick) {
    const int tid = threadIdx.x;
    uint32_t kmax = 0, kmin = 0xffffffffu;
#pragma unroll
    for (int e = 0; e < PER; ++e)
        if (valid[e]) {
            kmax = key[e] > kmax ? key[e] : kmax;
            kmin = key[e] < kmin ? key[e] : kmin;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t a = __shfl_xor(kmax, o), b = __shfl_xor(kmin, o);
        kmax = a > kmax ? a : kmax;
        kmin = b < kmin ? b : kmin;
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        hist[tid >> 6] = kmax;
        hist[16 + (tid >> 6)] = kmin;
    }
    __syncthreads();
    const int nw = (int)(blockDim.x >> 6);
    for (int w = 0; w < nw; ++w) {
        kmax = hist[w] > kmax ? hist[w] : kmax;
        kmin = hist[16 + w] < kmin ? hist[16 + w] : kmin;
    }
    const uint32_t diff = kmax ^ kmin;
    if (diff == 0) return kmax;
    int hi = 31 - __clz((int)diff);  // highest bit in which two keys differ
    uint32_t mask = hi == 31 ? 0u : ~((2u << hi) - 1u);
    uint32_t prefix = kmax & mask;
#pragma unroll 1
    while (hi >= 0) {
        const int lo = hi >= 7 ? hi - 7 : 0;
        const uint32_t dmask = (1u << (hi - lo + 1)) - 1u;
        __syncthreads();  // the previous pass's picks / the reduction slots are consumed
        for (int i = tid; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PER; ++e)
            if (valid[e] && (key[e] & mask) == prefix) atomicAdd(&hist[(key[e] >> lo) & dmask], 1u);
        __syncthreads();
        if (tid < 64) {
            // lane l owns bins 4l .. 4l+3; above(l) = keys in bins owned by higher lanes
            const uint32_t b0 = hist[4 * tid], b1 = hist[4 * tid + 1], b2 = hist[4 * tid + 2], b3 = hist[4 * tid + 3];
            const uint32_t mine = b0 + b1 + b2 + b3;
            uint32_t inc = mine;  // inclusive suffix sum over lanes
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_down(inc, o);
                if (tid + o < 64) inc += t;
            }
            const uint32_t above = inc - mine;
            if (above < k && k <= inc) {  // the k-th largest key has its digit in one of my bins
                uint32_t a = above;
                int dg;
                if (a + b3 >= k) dg = 3;
                else if ((a += b3) + b2 >= k) dg = 2;
                else if ((a += b2) + b1 >= k) dg = 1;
                else { a += b1; dg = 0; }
                s_pick[0] = (uint32_t)(4 * tid + dg);
                s_pick[1] = k - a;  // rank inside that bin
            }
        }
        __syncthreads();
        prefix |= s_pick[0] << lo;
        mask |= dmask << lo;
        k = s_pick[1];
        hi = lo - 1;
    }
    return prefix;
}

// k-th largest of n keys that sit in LDS (ckey, 16-byte aligned; 1 <= k <= n), by rank: the thread that owns a key counts the
// keys above it with broadcast reads, four per read; the keys with fewer than k above them are the k largest (ties included)
// and the smallest of those is the answer: a wave minimum, then one LDS atomic per wave into *out, which holds 0xffffffff
// when the barrier in front of this call is passed.  The caller puts a barrier behind it.  A compare and an add per pair on the
// SIMDs' 4-cycle cadence: about n^2 / 32 cycles once n keys fill the four SIMDs -- 0.9 us at 256 keys, 3.5 at 512, which is what the
// radix passes above take (a dozen barriers and 3 * PER LDS atomics per thread, whatever n is): kRankCap.
constexpr uint32_t kRankCap = 512;
__device__ __forceinline__ void lds_rank_select(const uint32_t *ckey, uint32_t n, uint32_t k, uint32_t *out) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t i0 = threadIdx.x - lane; i0 < n; i0 += blockDim.x) {  // wave-uniform
        const uint32_t i = i0 + lane;
        const uint32_t mine = i < n ? ckey[i] : 0u;
        uint32_t gt = 0, j = 0;
        for (; j + 4 <= n; j += 4) {
            const uint4 o = *reinterpret_cast<const uint4 *>(ckey + j);
            gt += o.x > mine ? 1u : 0u;
            gt += o.y > mine ? 1u : 0u;
            gt += o.z > mine ? 1u : 0u;
            gt += o.w > mine ? 1u : 0u;
        }
        for (; j < n; ++j) gt += ckey[j] > mine ? 1u : 0u;
        uint32_t cand = i < n && gt < k ? mine : 0xffffffffu;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t t = __shfl_xor(cand, o);
            cand = t < cand ? t : cand;
        }
        if (lane == 0 && cand != 0xffffffffu) atomicMin(out, cand);
    }
}

// block_kth_largest for a small k among many keys (k <= kPreMaxK): select among the keys at or above a pivot that at least k keys
// reach.  Every wave takes the kw-th largest of the 64 keys its threads hold in slot 0, kw = ceil(k / nfull) with nfull the waves
// that nvalid keys could fill; a wave with fewer than kw valid keys there stands aside.  pivot = the smallest of these: each of the c
// waves that took part holds kw keys >= its own value >= pivot, so c * kw >= k keys reach the pivot, the k-th largest key of all is among
// them and is their k-th largest.  They are compacted into ckey (LDS, kRankCap words, 16-byte aligned; may be storage whose
// earlier contents every thread has read before the call: the first barrier here stands in front of the first write) and ranked there.
// Too few waves took part, or more than kRankCap keys reach the pivot: the radix passes, unchanged.  With keys in no particular
// order about 5 % of the keys of a 16-wave block reach the pivot at k <= 16.
// s_pre: nwaves + 2 words.  Requires 1 <= k <= number of valid keys, blockDim a multiple of 64 and <= 1024.
constexpr uint32_t kPreMaxK = 32;
template <int PER>
__device__ __forceinline__ uint32_t block_kth_largest_pre(const uint32_t (&key)[PER], const bool (&valid)[PER], uint32_t k,
                                                          uint32_t nvalid, uint32_t *ckey, uint32_t *s_pre, uint32_t *hist,
                                                          uint32_t *s_pick) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nw = blockDim.x >> 6;
    uint32_t nfull = nvalid >> 6;
    nfull = nfull < 1u ? 1u : nfull > nw ? nw : nfull;
    const uint32_t kw = (k + nfull - 1) / nfull;
    uint32_t *s_n = s_pre + nw, *s_out = s_pre + nw + 1;
    {
        const uint32_t mk = valid[0] ? key[0] : 0u;
        const uint32_t have = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(valid[0]));
        uint32_t wp;
        if (kw == 1) {  // the wave's largest key
            wp = mk;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t t = __shfl_xor(wp, o);
                wp = t > wp ? t : wp;
            }
        } else {  // its kw-th largest: the smallest of the keys with fewer than kw above them
            uint32_t gt = 0;
#pragma unroll
            for (int j = 0; j < 64; ++j) gt += (uint32_t)__builtin_amdgcn_readlane((int)mk, j) > mk ? 1u : 0u;  // (a scalar read per lane: no LDS crossbar)
            wp = valid[0] && gt < kw ? mk : 0xffffffffu;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t t = __shfl_xor(wp, o);
                wp = t < wp ? t : wp;
            }
        }
        if (lane == 0) s_pre[wave] = have >= kw ? wp : 0xffffffffu;
        if (tid == 0) *s_n = 0, *s_out = 0xffffffffu;
    }
    __syncthreads();
    uint32_t pivot = 0xffffffffu, took = 0;
    for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t wp = s_pre[w];
        took += wp != 0xffffffffu ? 1u : 0u;  // (a wave whose kw-th key is 0xffffffff, the key of one NaN pattern, stands aside too)
        pivot = wp < pivot ? wp : pivot;
    }
    if (took * kw < k) return block_kth_largest<PER>(key, valid, k, hist, s_pick);  // block-uniform
    uint32_t cnt = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) cnt += valid[e] && key[e] >= pivot ? 1u : 0u;
    uint32_t inc = cnt;  // one LDS atomic per wave, as in finish_kernel's gather
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += t;
    }
    uint32_t wbase = 0;
    if (lane == 63 && inc) wbase = atomicAdd(s_n, inc);
    wbase = __shfl(wbase, 63);
    uint32_t at = wbase + inc - cnt;
    if (cnt) {
#pragma unroll
        for (int e = 0; e < PER; ++e)
            if (valid[e] && key[e] >= pivot) {
                if (at < kRankCap) ckey[at] = key[e];
                ++at;
            }
    }
    __syncthreads();
    const uint32_t n = *s_n;
    if (n > kRankCap) return block_kth_largest<PER>(key, valid, k, hist, s_pick);  // block-uniform
    lds_rank_select(ckey, n, k, s_out);
    __syncthreads();
    return *s_out;
}

// ---------------------------------------------------------------------------------------------
// ingest: copy rows into the padded store and compute 1/|c|   (replaces hnsw.insert, local.rs:65)
// ---------------------------------------------------------------------------------------------
// raw & 1: the rows are stored values of a compressed corpus coming back from disk (unit length up to
// bf16 rounding): they must be stored as they are, so 1/|c| is replaced by 1.  raw & 2 (f32 corpus): rows whose norm is
// outside [1e-15, 1e15] are stored as zeros and listed in wild_rows (below).
__global__ __launch_bounds__(256) void ingest_kernel(const float *__restrict__ src, uint64_t n, int d,
                                                     float *__restrict__ x, float *__restrict__ scale,
                                                     uint64_t first, int ds, uint32_t *flags, int raw,
                                                     uint32_t *__restrict__ zero_rows, uint32_t *__restrict__ wild_rows,
                                                     uint64_t row_base) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = wave0; r < n; r += nwaves) {
        const float *s = src + r * (uint64_t)d;
        float *o = x + (first + r) * (uint64_t)ds;
        double acc = 0.0;
        bool bad = false;
        for (int c = lane; c < ds; c += 64) {
            const float v = c < d ? s[c] : 0.0f;
            o[c] = v;
            bad |= !isfinite(v);
            acc += (double)v * (double)v;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
        if (lane == 0) {
            float sc;
            const bool wild = acc > 0.0 && (acc < 1e-30 || acc > 1e30) && isfinite(acc);
            if (wild) atomicAdd(&flags[1], 1u);
            if (wild && (raw & 2) && !anybad) {
                // a norm outside [1e-15, 1e15]: the f32 stages are not certified for it (1/|c| and c/|c| leave the
                // f32 range).  The row is stored as zeros in every filter copy (1/|c| kept as 0) and listed: the scan
                // and the f32 stages never see it, finish_kernel hands it to its f64 stage for EVERY query, beside
                // the survivors.  One such row costs one more f64 chain per query, not the whole collection its fast path.
                sc = 0.0f;
                const uint32_t at = atomicAdd(&flags[4], 1u);
                if (at < (uint32_t)kWildCap) wild_rows[at] = (uint32_t)(row_base + r);
            } else if (acc > 0.0) {
                sc = (raw & 1) ? 1.0f : (float)(1.0 / sqrt(acc));
            } else {
                // zero-norm row: exact dist is 0 for every query (DistCosine else-branch).  It is stored as
                // zeros (scan score 0) and remembered in the index's zero-row list, from which
                // finish_kernel adds it to every query's candidates.
                sc = 0.0f;
                if (!anybad && acc == 0.0) {
                    const uint32_t at = atomicAdd(&flags[3], 1u);
                    if (at < (uint32_t)kZeroCap) zero_rows[at] = (uint32_t)(row_base + r);
                }
            }
            if (anybad || !isfinite(acc)) atomicAdd(&flags[0], 1u);
            scale[first + r] = sc;
        }
    }
}

hipError_t launch_ingest(hipStream_t s, const float *src, uint64_t n, int d, float *x, float *scale,
                         uint64_t first, int ds, uint32_t *flags, int raw, uint32_t *zero_rows, uint32_t *wild_rows, uint64_t row_base) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(ingest_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, n, d, x, scale, first, ds, flags, raw, zero_rows, wild_rows, row_base);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// query preparation: one block per query slot (256 slots)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_queries_kernel(const float *__restrict__ q, int B, int d, int ds,
                                                           __bf16 *__restrict__ qfrag, float *__restrict__ qpad,
                                                           double *__restrict__ qnorm2, float *__restrict__ theta,
                                                           float *__restrict__ e1, const uint32_t *__restrict__ ec_max,
                                                           uint32_t *__restrict__ overflow, uint32_t *__restrict__ flags,
                                                           int filt8, float *__restrict__ qscale,
                                                           float *__restrict__ qa, float *__restrict__ qb,
                                                           const float *__restrict__ mean, float *__restrict__ qmean,
                                                           const uint32_t *__restrict__ rc_max) {
    extern __shared__ __attribute__((aligned(16))) char psm[];
    float *s_row = reinterpret_cast<float *>(psm);  // [d] this query (coalesced load; the chain reads LDS)
    __shared__ float s_inv;
    __shared__ uint32_t s_red[4];
    __shared__ uint32_t s_bad[4];
    __shared__ double s_dot[4];
    __shared__ float s_rq[4];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const bool live = b < B;
    bool bad = false;
    for (int i = tid; i < d; i += 256) {
        const float v = live ? q[(size_t)b * d + i] : 0.0f;
        s_row[i] = v;
        bad |= !isfinite(v);
    }
    __syncthreads();
    if (tid == 0) {
        double na = 0.0;
        for (int i = 0; i < d; ++i) {  // sequential, f32 products: DistCosine's query-norm chain
            const float v = s_row[i];
            na += (double)__fmul_rn(v, v);
        }
        qnorm2[b] = na;
        const bool usable = live && na > 0.0 && isfinite(na);
        s_inv = usable ? (float)(1.0 / sqrt(na)) : 0.0f;
        theta[b] = usable ? -INFINITY : INFINITY;  // zero / padded queries never pass the scan filter
        overflow[b] = 0;
    }
    __syncthreads();
    const float inv = s_inv;
    const int w = b >> 5, col = b & 31;
    float r2 = 0.0f;  // |stored(q/|q|) - q/|q||^2: this query's share of the scan's error bound
    if (filt8) {
        // 8-bit filter copy (scan8.hip): the normalised query goes through the same rotation as the rows
        // (mx_rotate.h), then q8 = rint(rotated / s_q), s_q = max |rotated_i| / 127
        float *rin = s_row + d, *rot = rin + ds, *mixq = rot + ds;  // behind the query: [ds] | [ds] | [144]
        // centred copy: a_q = (q/|q|) . mean in f64, the quantiser sees r_q = q/|q| - a_q mean (as the rows' builder, shadow8_kernel)
        float aq8 = 0.0f, rq2 = 0.0f;
        if (mean) {
            double dp = 0.0;
            for (int dim = tid; dim < d; dim += 256) dp += (double)(s_row[dim] * inv) * (double)mean[dim];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dp += __shfl_xor(dp, o);
            if ((tid & 63) == 0) s_dot[tid >> 6] = dp;
            __syncthreads();
            aq8 = (float)(s_dot[0] + s_dot[1] + s_dot[2] + s_dot[3]);
            if (tid == 0) qmean[b] = aq8;
        }
        for (int dim = tid; dim < ds; dim += 256) {
            float vn = dim < d ? s_row[dim] * inv : 0.0f;
            if (mean && dim < d) vn = __builtin_fmaf(-aq8, mean[dim], vn);
            rin[dim] = vn;
            rq2 += vn * vn;
        }
        if (mean) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) rq2 += __shfl_xor(rq2, o);
            if ((tid & 63) == 0) s_rq[tid >> 6] = rq2;
        }
        rot_fill_mix(mixq, ds >> 7, tid, 256);
        __syncthreads();
        if (tid < 64) rot_wave(rin, rot, ds >> 7, tid, mixq);
        __syncthreads();
        float mx = 0.0f;
        for (int dim = tid; dim < ds; dim += 256) mx = fmaxf(mx, fabsf(rot[dim]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if ((tid & 63) == 0) s_red[tid >> 6] = __float_as_uint(mx);
        __syncthreads();
        mx = fmaxf(fmaxf(__uint_as_float(s_red[0]), __uint_as_float(s_red[1])), fmaxf(__uint_as_float(s_red[2]), __uint_as_float(s_red[3])));
        __syncthreads();  // s_red is reused for the residual below
        // (centred copy: the step stays at or above kMinStep8, as the rows' does -- scan8.hip's accumulator start a_q a_c / (s_h s_q)
        // must fit an int32; a query whose residual is that short loses nothing it can measure: r2 below is its actual residual.
        // Also when the residual is exactly 0 -- a usable query ON the mean axis: its codes are all 0 and a_q a_c enters through the
        // accumulator start alone.  A step of 0 stays the mark of an unusable query, which scan8_kernel scores 0 for every row.)
        const bool floored = mean && inv > 0.0f;
        const float sq = floored ? fmaxf(mx / 127.0f, kMinStep8) : mx / 127.0f;
        const float qinv = floored ? 1.0f / sq : (mx > 0.0f ? 127.0f / mx : 0.0f);
        if (tid == 0) qscale[b] = sq;
        const int ksteps = ds / 32;
        int8_t *q8 = reinterpret_cast<int8_t *>(qfrag);
        for (int dim = tid; dim < ds; dim += 256) {
            const float v = dim < d ? s_row[dim] : 0.0f;
            qpad[(size_t)b * ds + dim] = v;  // the rescoring stages read the query as it came
            // v_mfma_i32_32x32x32_i8 B-operand: lane l holds B[k = 16*(l>>5)+i][n = l&31], 16 int8
            const int ks = dim >> 5, hh = (dim >> 4) & 1, i = dim & 15;
            const int lane = hh * 32 + col;
            const float vn = rot[dim];
            const float qv = fminf(fmaxf(rintf(vn * qinv), -127.0f), 127.0f);
            q8[(((size_t)w * ksteps + ks) * 64 + lane) * 16 + i] = (int8_t)(int)qv;
            const float r = qv * sq - vn;
            r2 += r * r;
        }
    } else {
        // centred bf16 copy (ScanParams::amean): a_q = (q/|q|) . mean in f64, the fragments hold r_q = q/|q| - a_q mean
        float aq = 0.0f;
        if (mean) {
            double dp = 0.0;
            for (int dim = tid; dim < d; dim += 256) dp += (double)(s_row[dim] * inv) * (double)mean[dim];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dp += __shfl_xor(dp, o);
            if ((tid & 63) == 0) s_dot[tid >> 6] = dp;
            __syncthreads();
            aq = (float)(s_dot[0] + s_dot[1] + s_dot[2] + s_dot[3]);
            if (tid == 0) qmean[b] = aq;
        }
        const int ksteps = ds / 16;
        float rq2 = 0.0f;  // |r_q|^2 (centred) -- the factor of the rows' residual in the bound
        for (int dim = tid; dim < ds; dim += 256) {
            const float v = dim < d ? s_row[dim] : 0.0f;
            qpad[(size_t)b * ds + dim] = v;
            // MFMA 32x32x16 B-operand: lane l holds B[k = 8*(l>>5)+i][n = l&31]
            const int ks = dim >> 4, hh = (dim >> 3) & 1, i = dim & 7;
            const int lane = hh * 32 + col;
            float vn = v * inv;
            if (mean && dim < d) vn = __builtin_fmaf(-aq, mean[dim], vn);
            const __bf16 vb = (__bf16)vn;
            qfrag[(((size_t)w * ksteps + ks) * 64 + lane) * 8 + i] = vb;
            const float r = (float)vb - vn;
            r2 += r * r;
            rq2 += vn * vn;
        }
        if (mean) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) rq2 += __shfl_xor(rq2, o);
            if ((tid & 63) == 0) s_rq[tid >> 6] = rq2;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r2 += __shfl_xor(r2, o);
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if ((tid & 63) == 0) {
        s_red[tid >> 6] = __float_as_uint(r2);
        s_bad[tid >> 6] = anybad ? 1u : 0u;
    }
    __syncthreads();
    if (tid == 0) {
        // non-finite query: the call fails with MX_EINVAL.  One word per query slot, written by every launch:
        // nothing to clear between calls
        flags[b] = live ? (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) : 0u;
        // |approx - cos| <= |c^ - c| + |q^ - q| + |c^ - c||q^ - q| + f32 accumulation (unit vectors,
        // Cauchy-Schwarz).  ec_max is the largest row residual the filter copy holds (shadow_kernel);
        // without a filter copy (f32 scan: rows are rounded unnormalised) the a-priori bound is used.
        const float eq = sqrtf(__uint_as_float(s_red[0]) + __uint_as_float(s_red[1]) + __uint_as_float(s_red[2]) +
                               __uint_as_float(s_red[3])) * 1.01f + 1e-6f;
        float e = kApproxErr;
        if (ec_max) {
            const float ec = __uint_as_float(*ec_max) * 1.01f + 1e-6f;
            e = ec + eq + ec * eq + kAccSlack;
            if (!filt8) e = fminf(kApproxErr + ec * ec, e);  // two bf16 roundings have an a-priori bound as well
            if (mean && !filt8) {
                // centred copy: cos = a_q a_c + r_q . r_c exactly (a_c, a_q are the stored f32 values, r := unit vector - a m),
                // |r^_q . r^_c - r_q . r_c| <= |r_q| Ec + (|r_c| + Ec) Eq <= |r_q| Ec + Eq + Ec Eq   (|r_c| <= 1 + 1e-6)
                const float rq = sqrtf(s_rq[0] + s_rq[1] + s_rq[2] + s_rq[3]) * 1.001f + 1e-6f;
                e = fminf(e, rq * ec + eq * 1.0001f + ec * eq + kAccSlack);
            }
        }
        // the bound of ONE row is a + b * (its residual): with a residual per half tile (8-bit copy, scan8.hip) the
        // rows of a well-conditioned half tile get a tighter bound than e1, which is the bound of the worst one;
        // the other scans know one residual for all rows: a = e1, b = 0
        float a8 = eq + kAccSlack, b8 = 1.0f + eq;
        if (mean && filt8) {
            // centred int8 copy: cos = a_q a_c + r_q . r_c exactly; |r^_q . r^_c - r_q . r_c| <= |r_q| e_h + (|r_c| + e_h) Eq
            //   = Eq |r_c| + (|r_q| + Eq) e_h,  |r_c| <= rc_max (measured by the builder; 1 + 1e-6 without it)
            const float rq = sqrtf(s_rq[0] + s_rq[1] + s_rq[2] + s_rq[3]) * 1.001f + 1e-6f;
            const float rc = rc_max ? fminf(__uint_as_float(*rc_max) * 1.001f + 1e-6f, 1.0f + 1e-6f) : 1.0f + 1e-6f;
            a8 = eq * rc * 1.0001f + kAccSlack;
            b8 = rq + eq;
            if (ec_max) e = a8 + b8 * (__uint_as_float(*ec_max) * 1.01f + 1e-6f);  // the bound of a row of the worst half tile
        }
        e1[b] = e;
        qa[b] = filt8 ? a8 : e;
        qb[b] = filt8 ? b8 : 0.0f;
    }
}

hipError_t launch_prep_queries(hipStream_t s, const float *q, int B, int d, int ds, void *qfrag, float *qpad,
                               double *qnorm2, float *theta, float *e1, const uint32_t *ec_max, uint32_t *overflow,
                               uint32_t *flags, float *qa, float *qb, bool filt8, float *qscale, const float *mean, float *qmean,
                               const uint32_t *rc_max) {
    if (ds > kMaxKC16 * kChunkFloats) {
        if (filt8 || ec_max) return hipErrorInvalidValue;  // no filter copy exists at this width (index.hip, build_filter_copy)
        return launch_prep_queries_wide(s, q, B, d, ds, qpad, qnorm2, theta, e1, overflow, flags, qa, qb);  // prep_wide.hip
    }
    if (!qmean) mean = nullptr;
    // one block per query slot: 256 slots (a pass computes all of them), 512 for a batch of more than 256
    hipLaunchKernelGGL(prep_queries_kernel, dim3(B > kPassBatch ? kMaxBatch : kPassBatch), dim3(256),
                       sizeof(float) * ((size_t)d + (filt8 ? 2 * (size_t)ds + kRotMaxBlocks * kRotMaxBlocks : 0)), s, q, B, d, ds,
                       (__bf16 *)qfrag, qpad, qnorm2, theta, e1, ec_max, overflow, flags, filt8 ? 1 : 0, qscale, qa, qb, mean, qmean, rc_max);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// mean direction of the normalised rows (the centre of a centred bf16 copy, launch_shadow)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mean_sum_kernel(const float *__restrict__ x, const float *__restrict__ scale, uint64_t n, int ds,
                                                       float *__restrict__ msum) {
    // a workgroup walks a contiguous share of the rows; thread t sums columns t, t + 256, ... (coalesced along a row)
    const uint64_t per = (n + gridDim.x - 1) / gridDim.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * per, r1 = r0 + per < n ? r0 + per : n;
    for (int c = threadIdx.x; c < ds; c += 256) {
        float acc = 0.0f;
        for (uint64_t r = r0; r < r1; ++r) acc = __builtin_fmaf(x[r * (uint64_t)ds + c], scale[r], acc);
        atomicAdd(&msum[c], acc);
    }
}

__global__ __launch_bounds__(256) void mean_norm_kernel(float *__restrict__ msum, int ds, float *__restrict__ mean) {
    __shared__ double s_p[4];
    double p = 0.0;
    for (int c = threadIdx.x; c < ds; c += 256) p += (double)msum[c] * (double)msum[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
    if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = p;
    __syncthreads();
    const double n2 = s_p[0] + s_p[1] + s_p[2] + s_p[3];
    const double inv = n2 > 1e-30 && n2 < 1e30 ? 1.0 / sqrt(n2) : 0.0;  // a vanishing (or non-finite) sum: no centre
    for (int c = threadIdx.x; c < ds; c += 256) mean[c] = (float)((double)msum[c] * inv);
    __syncthreads();
    if (threadIdx.x == 0) msum[ds] = (float)sqrt(n2);  // |sum of the unit rows|: the host decides whether centring pays
}

hipError_t launch_mean_dir(hipStream_t s, const float *x, const float *scale, uint64_t n, int ds, float *msum, float *mean) {
    hipError_t e = hipMemsetAsync(msum, 0, (size_t)ds * sizeof(float), s);
    if (e != hipSuccess) return e;
    if (n > 0) {
        const unsigned blocks = (unsigned)(n < 2048 ? n : 2048);
        hipLaunchKernelGGL(mean_sum_kernel, dim3(blocks), dim3(256), 0, s, x, scale, n, ds, msum);
    }
    hipLaunchKernelGGL(mean_norm_kernel, dim3(1), dim3(256), 0, s, msum, ds, mean);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// theta: pass threshold of the collect launch from the sample launch's lane maxima
// ---------------------------------------------------------------------------------------------
// A query's 2*nwg lane maxima are approximate scores of 2*nwg DISTINCT rows, so the k-th largest of
// them, a_k, is a lower bound of the k-th best approximate score, the exact k-th best cosine is
// >= a_k - e1, and every row of the exact top-k has an approximate score >= a_k - 2*e1.
// Per-row bounds (scan8_kernel): the lane maxima already are lower bounds of cosines, L_k is a lower bound of the
// k-th best cosine, a row of the top-k has score + (qa + qb * residual) >= L_k, and the scan tests
// score >= theta - qb * residual with theta = L_k - qa.  `raw` = 1: lane maxima are plain scores, theta = a_k - 2*qa
// (qa = e1 there).
// Exact form (ThetaExact in index_kernels.h, the plain int8 copy: DESIGN.md section 3.1): the sample launch also left the ROW
// behind every lane maximum (lane_arg).  The C = min(lanes, max(32, 2k + 12)) lanes with the largest maxima name C distinct stored rows; they are rescored in f32
// against the raw query with the arithmetic and the bound e2 of finish_kernel's stage 2 (one wave per row, eight rows in flight), rows
// without a norm and lanes without a row left out.  L' = the k-th largest s2 - e2 (-inf when fewer than k rows were rescored) is a lower
// bound of the k-th best cosine that does not carry the scan's a-priori bracket qa + qb * residual, and so is max(L_k, L'):
// theta = max(L_k - qa, L' - qa).  Both terms are certified thresholds, so the collect launch's records are a subset of those under
// L_k - qa alone.
constexpr int kThetaMaxC = 2 * 256 + 12;  // C at the largest k of the scan pipeline
constexpr int kThetaRows = 8;             // rows a wave rescores together

// PER values per thread: 2 up to 256 workgroups, 4 up to 512 (the int8 scan's two-workgroup form)
template <int PER, bool EXACT>
__device__ __forceinline__ void theta_query(int k, int nwg, const float *__restrict__ lane_max, const float *__restrict__ qa, int raw,
                                            float *__restrict__ theta, const ThetaExact &x) {
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_pick[2];
    __shared__ uint32_t s_nvalid[4];
    __shared__ uint32_t s_crow[EXACT ? kThetaMaxC : 1];  // rows of the C best lanes, then (as float bits) their s2 - e2
    __shared__ uint32_t s_ckey[EXACT ? kThetaMaxC : 1];  // ... and their lane maxima (keys)
    __shared__ uint32_t s_cn, s_kth;
    __shared__ float s_lp;
    const int q = blockIdx.x;
    const int tid = threadIdx.x;
    const int n = 2 * nwg;  // <= 256 * PER
    const uint32_t t0 = (uint32_t)(q >> 5) * 64 + (uint32_t)(q & 31);
    uint32_t key[PER], arg[EXACT ? PER : 1];
    bool valid[PER];
    if (EXACT && tid == 0) s_cn = 0, s_lp = -INFINITY;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int i = e * 256 + tid;
        float v = -INFINITY;
        if (i < n) {
            const int hh = i / nwg, w = i - hh * nwg;
            v = lane_max[(size_t)(t0 + 32 * hh) * nwg + w];
            if constexpr (EXACT) arg[e] = x.lane_arg[(size_t)(t0 + 32 * hh) * nwg + w];  // (fetched with the maximum: no second round trip)
        }
        valid[e] = v > -INFINITY;  // a lane that saw no row keeps -inf
        key[e] = f32_key(v);
    }
    uint32_t nv = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) nv += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(valid[e]));
    if ((tid & 63) == 0) s_nvalid[tid >> 6] = nv;
    __syncthreads();
    nv = s_nvalid[0] + s_nvalid[1] + s_nvalid[2] + s_nvalid[3];
    // fewer than k lanes saw a row: no threshold that could drop a row -- every filter score of a row lies far above -8 -- but a
    // finite one, which the -inf of masked rows (a removal or a filter that leaves few rows in the sample) does not reach: such
    // rows then take no record slot in the collect launch
    float kth = -8.0f;
    bool exact = false;  // (uniform over the workgroup)
    uint32_t C = 0;
    double na = 0.0;
    if constexpr (EXACT) {
        na = x.qnorm2[q];
        C = (uint32_t)min(n, max(32, 2 * k + 12));
        exact = nv >= (uint32_t)k && k > 0 && C <= (uint32_t)kThetaMaxC && theta[q] != INFINITY && na > 0.0 && na < INFINITY;
    }
    if (!exact && nv >= (uint32_t)k && k > 0) kth = key_f32(block_kth_largest<PER>(key, valid, (uint32_t)k, s_hist, s_pick));
    float th = 0.0f;
    if constexpr (EXACT) {
        if (exact) {
            // ---- the C lanes with the largest maxima, C >= k: ONE radix select (none when at most C lanes saw a row); the k-th largest
            // maximum is then ranked among those C.  Ties at the C-th value beyond C are dropped: every larger value is kept, so the
            // k-th largest of what is kept is the k-th largest of all, and any C of the lanes would do for the rows.
            const uint32_t cut = nv > C ? block_kth_largest<PER>(key, valid, C, s_hist, s_pick) : 0u;
#pragma unroll
            for (int e = 0; e < PER; ++e)
                if (valid[e] && key[e] >= cut) {
                    const uint32_t at = atomicAdd(&s_cn, 1u);
                    if (at < C) s_crow[at] = arg[e], s_ckey[at] = key[e];
                }
            __syncthreads();
            const uint32_t nc = s_cn < C ? s_cn : C;  // >= k
            for (uint32_t i = tid; i < nc; i += 256) {
                const uint32_t mine = s_ckey[i];
                uint32_t gt = 0, ge = 0;
                for (uint32_t j = 0; j < nc; ++j) {
                    const uint32_t o = s_ckey[j];
                    gt += o > mine ? 1u : 0u;
                    ge += o >= mine ? 1u : 0u;
                }
                if (gt < (uint32_t)k && (uint32_t)k <= ge) s_kth = mine;  // ties write the same value
            }
            // ---- f32 rescoring: s2 = sum fma(q_i/|q|, c_i/|c|), |s2 - cos| <= e2 (finish_kernel's stage 2)
            const int lane = tid & 63, wave = tid >> 6;
            const float invq = (float)(1.0 / sqrt(na));
            const int nc4 = x.ds >> 2;
            const float4 *qv = reinterpret_cast<const float4 *>(x.qpad + (size_t)q * x.ds);
            for (uint32_t base = (uint32_t)wave * kThetaRows; base < nc; base += 4 * kThetaRows) {
                float dot[kThetaRows], sc[kThetaRows];
                const float4 *rp[kThetaRows];
#pragma unroll
                for (int j = 0; j < kThetaRows; ++j) {
                    const uint32_t row = base + j < nc ? s_crow[base + j] : kNoRow;
                    const bool ok = row != kNoRow && (uint64_t)row < x.n_rows;
                    sc[j] = ok ? x.scale[row] : 0.0f;
                    rp[j] = reinterpret_cast<const float4 *>(x.x + (size_t)(ok ? row : 0u) * x.ds);  // (does not wait for the norm)
                    dot[j] = 0.0f;
                }
                for (int tb = 0; tb * 64 < nc4; tb += kMaxKC / 2) {
                    float4 c[kThetaRows][kMaxKC / 2];
#pragma unroll
                    for (int t = 0; t < kMaxKC / 2; ++t) {
                        const int c4 = lane + 64 * (tb + t);
                        if (c4 < nc4) {
#pragma unroll
                            for (int j = 0; j < kThetaRows; ++j) c[j][t] = rp[j][c4];
                        }
                    }
#pragma unroll
                    for (int t = 0; t < kMaxKC / 2; ++t) {
                        const int c4 = lane + 64 * (tb + t);
                        if (c4 < nc4) {
                            const float4 a = qv[c4];
#pragma unroll
                            for (int j = 0; j < kThetaRows; ++j) {
                                dot[j] = fmaf(a.x * invq, c[j][t].x * sc[j], dot[j]);
                                dot[j] = fmaf(a.y * invq, c[j][t].y * sc[j], dot[j]);
                                dot[j] = fmaf(a.z * invq, c[j][t].z * sc[j], dot[j]);
                                dot[j] = fmaf(a.w * invq, c[j][t].w * sc[j], dot[j]);
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < kThetaRows; ++j) {
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) dot[j] += __shfl_xor(dot[j], o);
                }
                // (a wave reads and rewrites its own slots of s_crow only: no barrier, and none could stand in this wave-dependent loop)
#pragma unroll
                for (int j = 0; j < kThetaRows; ++j)
                    if (lane == j && base + j < nc) {
                        const float lb = dot[j] - x.e2;
                        // no row, a row without a norm (1/|c| kept as 0), or a score that is no number: not counted
                        s_crow[base + j] = __float_as_uint(sc[j] > 0.0f && sc[j] < INFINITY && lb == lb ? lb : -INFINITY);
                    }
            }
            __syncthreads();
            // ---- L' = the k-th largest lower bound (nc >= k entries, -inf for the rows left out)
            for (uint32_t i = tid; i < nc; i += 256) {
                const float mine = __uint_as_float(s_crow[i]);
                uint32_t gt = 0, ge = 0;
                for (uint32_t j = 0; j < nc; ++j) {
                    const float o = __uint_as_float(s_crow[j]);
                    gt += o > mine ? 1u : 0u;
                    ge += o >= mine ? 1u : 0u;
                }
                if (gt < (uint32_t)k && (uint32_t)k <= ge) s_lp = mine;  // ties write the same value
            }
            __syncthreads();
            kth = key_f32(s_kth);
            th = fmaxf(kth - qa[q], s_lp - qa[q]);
        }
    }
    if (!exact) th = kth - (raw ? 2.0f : 1.0f) * qa[q];
    if (tid == 0 && theta[q] != INFINITY) theta[q] = th;
}

template <int PER>
__global__ __launch_bounds__(256) void theta_kernel(int k, int nwg, const float *__restrict__ lane_max,
                                                    const float *__restrict__ qa, int raw, float *__restrict__ theta) {
    theta_query<PER, false>(k, nwg, lane_max, qa, raw, theta, ThetaExact{});
}
template <int PER>
__global__ __launch_bounds__(256) void theta_exact_kernel(int k, int nwg, const float *__restrict__ lane_max,
                                                          const float *__restrict__ qa, float *__restrict__ theta, const ThetaExact x) {
    theta_query<PER, true>(k, nwg, lane_max, qa, 0, theta, x);
}

hipError_t launch_theta(hipStream_t s, int B, int k, int nwg, const float *lane_max, const float *qa, bool raw, float *theta,
                        const ThetaExact *ex) {
    if (B <= 0) return hipSuccess;
    if (nwg > kMaxScanWGs) return hipErrorInvalidValue;
    if (ex && ex->lane_arg) {
        if (raw || !ex->x || !ex->scale || !ex->qpad || !ex->qnorm2) return hipErrorInvalidValue;
        const ThetaExact x = *ex;
        if (nwg <= 256)
            hipLaunchKernelGGL(theta_exact_kernel<2>, dim3(B), dim3(256), 0, s, k, nwg, lane_max, qa, theta, x);
        else
            hipLaunchKernelGGL(theta_exact_kernel<4>, dim3(B), dim3(256), 0, s, k, nwg, lane_max, qa, theta, x);
        return hipGetLastError();
    }
    if (nwg <= 256)
        hipLaunchKernelGGL(theta_kernel<2>, dim3(B), dim3(256), 0, s, k, nwg, lane_max, qa, raw ? 1 : 0, theta);
    else
        hipLaunchKernelGGL(theta_kernel<4>, dim3(B), dim3(256), 0, s, k, nwg, lane_max, qa, raw ? 1 : 0, theta);
    return hipGetLastError();
}

// retry launch: queries whose lane buffers overflowed are scanned again with the tight threshold
// finish_kernel derived from what was collected; every other query is parked at +inf
__global__ void retry_setup_kernel(float *theta, const float *theta_retry, uint32_t *overflow, uint32_t *todo) {
    const int q = threadIdx.x;
    const bool again = overflow[q] == 1;
    todo[q] = again ? 1u : 0u;
    theta[q] = again ? theta_retry[q] : INFINITY;
    if (again) overflow[q] = 0;
}

hipError_t launch_retry_setup(hipStream_t s, float *theta, const float *theta_retry, uint32_t *overflow, uint32_t *todo) {
    hipLaunchKernelGGL(retry_setup_kernel, dim3(1), dim3(kMaxBatch), 0, s, theta, theta_retry, overflow, todo);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// finish: gather a query's candidates, prune by approximate score, rescore in f32, prune again,
// exact DistCosine on the survivors, order by (dist, id), emit            (K7)
// ---------------------------------------------------------------------------------------------
// row_load4<CMP> (4 consecutive dims of a stored row) and exact_dist_stored<CMP> (exact DistCosine of a query in LDS against a stored
// row): mx_exact_dist.h

__device__ __forceinline__ float exact_dist_row(const float *__restrict__ qv, const float *__restrict__ row, int ds,
                                                double na, double *cos_out) {
    // sequential f64 accumulation of f32 products, element order 0..d-1 (zero padding adds +0.0)
    double dot = 0.0, nb = 0.0;
    const float4 *r4 = reinterpret_cast<const float4 *>(row);
#pragma unroll 8
    for (int i = 0; i < ds / 4; ++i) {  // ds is a multiple of 128: 8 independent loads in flight per trip
        const float4 c = r4[i];
        const float4 a = *reinterpret_cast<const float4 *>(qv + 4 * i);
        dot += (double)__fmul_rn(a.x, c.x); nb += (double)__fmul_rn(c.x, c.x);
        dot += (double)__fmul_rn(a.y, c.y); nb += (double)__fmul_rn(c.y, c.y);
        dot += (double)__fmul_rn(a.z, c.z); nb += (double)__fmul_rn(c.z, c.z);
        dot += (double)__fmul_rn(a.w, c.w); nb += (double)__fmul_rn(c.w, c.w);
    }
    if (cos_out) *cos_out = (na > 0.0 && nb > 0.0) ? dot / sqrt(na * nb) : 1.0;
    return dist_from_sums(dot, na, nb);
}

// one of exact_dist_row's two chains: sum_i f64(f32(a_i * c_i)) in element order (a = the query: dot; a = c: nb)
__device__ __forceinline__ double f64_chain(const float *__restrict__ a, const float *__restrict__ c, int ds) {
    double s = 0.0;
    const float4 *a4 = reinterpret_cast<const float4 *>(a), *c4 = reinterpret_cast<const float4 *>(c);
#pragma unroll 8
    for (int i = 0; i < ds / 4; ++i) {
        const float4 u = a4[i], v = c4[i];
        s += (double)__fmul_rn(u.x, v.x);
        s += (double)__fmul_rn(u.y, v.y);
        s += (double)__fmul_rn(u.z, v.z);
        s += (double)__fmul_rn(u.w, v.w);
    }
    return s;
}

constexpr int kFinThreads = 1024;
constexpr int kFinishTailBytes = 128 + (2 * kMaxScanWGs + 1 + 3) * 4;  // staged row ids [32] + scanned record counts
constexpr int kFinWaves = kFinThreads / 64;
constexpr int kFinPer = kCandCap / kFinThreads;  // candidates held per thread
static_assert(kCandCap % kFinThreads == 0, "candidate capacity must divide over the block");

// block-wide exclusive scan of a small unsigned value over 1024 threads; total in *total
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t v, uint32_t *lds_w, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) lds_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kFinWaves; ++w) {
        const uint32_t c = lds_w[w];
        base += w < wave ? c : 0u;
        tot += c;
    }
    *total = tot;
    return base + inc - v;
}

// A record of the int8 scan (FinishParams::rec_int) holds the lane's 16 integer sums, loaded here as float bits: each becomes the
// score scan8_kernel tested, ((float)sum * s_h) * s_q -- two multiplications in this order (this file is built without FMA
// contraction, and there is no addition to contract with), so the bits are those the scan compared with the threshold.
__device__ __forceinline__ void int_record_scores(float (&v)[16], float s_h, float s_q) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = ((float)__float_as_int(v[r]) * s_h) * s_q;
}

template <bool CMP>
__device__ __forceinline__ void finish_query(const FinishParams &p) {
    extern __shared__ __attribute__((aligned(16))) char fsm[];
    Cand *ent = reinterpret_cast<Cand *>(fsm);                                        // [kCandCap]
    uint64_t *keys = reinterpret_cast<uint64_t *>(fsm);                               // same storage, later
    float *qv = reinterpret_cast<float *>(fsm + sizeof(Cand) * (size_t)kCandCap);     // [ds] raw query
    __shared__ uint32_t s_w[kFinWaves];
    __shared__ uint32_t s_sel[2][kFinWaves];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_pick[2];
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_pre[kFinWaves + 2];  // block_kth_largest_pre's
    __shared__ uint32_t s_err;                 // profiling: the workgroup's largest |s2 - filter score| as float bits

    const int q = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (p.todo && !p.todo[q]) return;
    const int k = p.k, ds = p.ds;
    const uint64_t want64 = p.n_live < (uint64_t)k ? p.n_live : (uint64_t)k;  // removed rows are never found
    const int want = (int)want64;
    uint64_t *oid = p.ids + (size_t)q * k;
    float *osc = p.scores + (size_t)q * k;
    float *odi = p.dists ? p.dists + (size_t)q * k : nullptr;
    if (tid == 0) {
        p.n_found[q] = want;
        p.cand_cnt[q] = 0;
    }
    for (int j = tid; j < k; j += kFinThreads) {  // defaults for unused slots
        oid[j] = 0;
        osc[j] = 0.0f;
        if (odi) odi[j] = INFINITY;
    }
    if (want == 0) return;
    const double na = p.qnorm2[q];
    if (!(na > 0.0)) {
        // zero-norm query: DistCosine returns 0 for every row -> ties broken by id (local.rs:63 ids): the first `want` live rows
        if (!p.dead) {
            for (int j = tid; j < want; j += kFinThreads) {
                oid[j] = p.idmap.id_of((uint32_t)j);
                osc[j] = 1.0f;
                if (odi) odi[j] = 0.0f;
            }
        } else {
            // block-wide: 1024 dead-row words per trip, a scan of their live counts places each word's live rows
            uint32_t found = 0;  // block-uniform
            for (uint64_t w0 = 0; found < (uint32_t)want && w0 * 64 < p.n_rows; w0 += kFinThreads) {
                const uint64_t w = w0 + (uint64_t)tid;
                uint64_t live = 0;
                if (w * 64 < p.n_rows) {
                    live = ~p.dead[w];
                    const uint64_t rem = p.n_rows - w * 64;
                    if (rem < 64) live &= (1ull << rem) - 1ull;
                }
                uint32_t tot;
                uint32_t j = found + block_scan_1024((uint32_t)__popcll(live), s_w, &tot);
                for (; live && j < (uint32_t)want; ++j) {
                    const uint64_t row = w * 64 + (uint64_t)__builtin_ctzll(live);
                    live &= live - 1;
                    oid[j] = p.idmap.id_of((uint32_t)row);
                    osc[j] = 1.0f;
                    if (odi) odi[j] = 0.0f;
                }
                found += tot;
            }
        }
        return;
    }
    const uint32_t lane_ovf = p.overflow[q];
    // bound of a row's filter score: qa + qb * (residual of its half tile); one residual for all rows: qb = 0, qa = e1
    const float qa = p.qa[q], qb = p.qb[q];
    auto resid = [&](uint32_t row) { return p.terr ? p.terr[kTscaleFloats * (size_t)(row >> 6) + 2 + ((row >> 5) & 1u)] : 0.0f; };
    for (int i = tid; i < ds; i += kFinThreads) qv[i] = p.qpad[(size_t)q * ds + i];

    // ---- gather.  Scan workgroup w kept this query's records in lanes L0 and L0+32 of wave q/32
    // ([thread-in-workgroup][workgroup] layout): a record = the lane's 16 scores of one tile, rows
    // tile*32 + 4*hh + (r&3) + 8*(r>>2).  Thread i < 2*nwg owns one lane buffer: count the scores
    // >= theta (what the old per-row append code did on the stream), scan, then write (score, row).
    // The index's zero-norm rows score 0 in the scan (stored as zeros); their exact dist is 0, so they
    // join every query's candidates here with cosine 1 -- and are dropped from the records, should a
    // threshold <= 0 have let them through.
    const int nwg = p.nwg;
    const float th = p.theta[q];
    const uint32_t nz = p.n_zero;
    // rows with a norm outside the f32 stages' range (stored as zeros, like the zero-norm rows, but their cosine is
    // not known): they never become candidates; stage 3 evaluates them in f64 for every query, beside the survivors
    const uint32_t nw = p.n_wild;
    auto in_list = [&](const uint32_t *list, uint32_t n, uint32_t row) {  // ascending lists
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (list[mid] < row) lo = mid + 1;
            else hi = mid;
        }
        return lo < n && list[lo] == row;
    };
    auto is_zero_row = [&](uint32_t row) { return (nz && in_list(p.zero_rows, nz, row)) || (nw && in_list(p.wild_rows, nw, row)); };
    // removed rows: the masked scans give them scores no threshold passes, but a half tile of zeros (step 0) scores them 0, and
    // theta may be -inf.  The lists above may name masked rows: a removal prunes them, a filter does not (the per-call mask of
    // mx_index_search_filtered), so every listed row's bit is tested.  No mask: p.dead is null and this is never asked.
    auto is_dead = [&](uint32_t row) { return p.dead && ((p.dead[row >> 6] >> (row & 63u)) & 1ull) != 0; };
    // (a) record counts of this query's 2*nwg lane buffers -> exclusive scan in LDS
    uint32_t *s_off = reinterpret_cast<uint32_t *>(qv + ds) + 32;  // [2*kMaxScanWGs + 1], behind the staged-row ids
    uint32_t nrec = 0;
    if (tid < 2 * nwg) {
        const uint32_t hh0 = (uint32_t)(tid / nwg);
        const int w = tid - (int)hh0 * nwg;
        nrec = p.lane_cnt[(size_t)((uint32_t)(q >> 5) * 64 + (uint32_t)(q & 31) + 32u * hh0) * nwg + w];
        nrec = nrec > (uint32_t)kRecCap ? (uint32_t)kRecCap : nrec;
    }
    uint32_t R;
    const uint32_t roff = block_scan_1024(nrec, s_w, &R);
    if (tid < 2 * nwg) s_off[tid] = roff;
    if (tid == 0) s_off[2 * nwg] = R;  // (2 * nwg = kFinThreads with the int8 scan's two-workgroup form)
    if (tid == 0) s_cnt = 0, s_err = 0;
    __syncthreads();
    // (b) one record per thread and trip (all of a query's records are in flight together): find its
    // lane buffer by binary search in the scanned counts, test the 16 scores, append the passing rows
    auto put = [&](uint32_t at, float sc, uint32_t row) {
        if (at < (uint32_t)kCandCap) {
            Cand cd;
            cd.score = sc;
            cd.row = row;
            ent[at] = cd;
        }
    };
    for (uint32_t j0 = 0; j0 < R; j0 += kFinThreads) {  // block-uniform trip count
        const uint32_t j = j0 + tid;
        uint32_t mask = 0, rowb = 0;
        float v[16];
        if (j < R) {
            uint32_t lo = 0, hi = (uint32_t)(2 * nwg) - 1;  // last lane buffer i with s_off[i] <= j
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (s_off[mid] <= j) lo = mid;
                else hi = mid - 1;
            }
            const uint32_t e = j - s_off[lo], hh = lo / (uint32_t)nwg, w = lo - hh * (uint32_t)nwg;
            const size_t l = (size_t)((uint32_t)(q >> 5) * 64 + (uint32_t)(q & 31) + 32u * hh) * nwg + w;
            const f32x4 *rec = reinterpret_cast<const f32x4 *>(p.lane_rec + l * (kRecCap * 16)) + e * 4;
            const uint32_t t32 = p.lane_tile[l * kRecCap + e];
            rowb = t32 * kTileRows + 4u * hh;
            // removed rows of the record: its 16 rows lie in one half tile, one word loaded beside the scores
            const uint32_t dm = p.dead ? lane_dead16(dead_half(p.dead, t32), hh) : 0u;
            const f32x4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = a[r], v[4 + r] = b[r], v[8 + r] = c[r], v[12 + r] = d[r];
            if (p.rec_int) int_record_scores(v, p.terr[kTscaleFloats * (size_t)(t32 >> 1) + (t32 & 1u)], p.qscale[q]);
            const float er = resid(rowb);                  // one half tile per record
            const float thr = fmaf(-qb, er, th), eb = fmaf(qb, er, qa);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t row = rowb + (r & 3) + 8 * (r >> 2);
                const bool pass = v[r] >= thr && (uint64_t)row < p.n_rows && !(v[r] == 0.0f && (nz | nw) && is_zero_row(row)) && !((dm >> r) & 1u);
                mask |= pass ? (1u << r) : 0u;
                v[r] -= eb;                                // candidates carry the LOWER bound of their cosine
            }
        }
        // one LDS atomic per WAVE (a per-thread atomicAdd on the one counter serialises: ~1800 of them
        // cost 19 us against 13 this way): wave-inclusive scan of the pass counts, lane 63 reserves the range
        const uint32_t cnt = (uint32_t)__popc(mask);
        uint32_t inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        uint32_t wbase = 0;
        if (lane == 63 && inc) wbase = atomicAdd(&s_cnt, inc);
        wbase = __shfl(wbase, 63);
        uint32_t at = wbase + inc - cnt;
        if (mask) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (mask & (1u << r)) put(at++, v[r], rowb + (r & 3) + 8 * (r >> 2));
        }
    }
    // the zero-norm rows
    for (uint32_t z = tid; z < nz; z += kFinThreads)
        if ((uint64_t)p.zero_rows[z] < p.n_rows && !is_dead(p.zero_rows[z])) put(atomicAdd(&s_cnt, 1u), 1.0f, p.zero_rows[z]);
    __syncthreads();
    uint32_t M = s_cnt;
    const bool too_many = M > (uint32_t)kCandCap;  // more than the block can hold: keep what fits (any subset yields a
                                                    // valid rescan threshold) and flag the query for the rescan
    if (too_many) M = kCandCap;
    __syncthreads();
    if (M < (uint32_t)want) {  // cannot happen unless candidates were lost: leave it to the host
        if (tid == 0) p.overflow[q] = lane_ovf ? 3u : 2u;
        return;
    }

    // ---- stage 1: L = k-th best lower bound; keep the rows whose upper bound (lower + 2 * own bound) reaches L;
    // the survivors carry their filter score again (lower + own bound)
    uint32_t key[kFinPer], row[kFinPer];
    bool valid[kFinPer];
#pragma unroll
    for (int e = 0; e < kFinPer; ++e) {
        const uint32_t i = (uint32_t)e * kFinThreads + tid;
        valid[e] = i < M;
        if (valid[e]) {
            const Cand cd = ent[i];
            key[e] = f32_key(cd.score);
            row[e] = cd.row;
        } else {
            key[e] = 0;
            row[e] = 0xffffffffu;
        }
    }
    {
        // (every thread holds its entries in registers, so the prefiltered select may compact its keys into ent[]'s storage)
        const uint32_t kth = (p.serial & kSerialPre) && (uint32_t)want <= kPreMaxK && M >= 64u
                                 ? block_kth_largest_pre<kFinPer>(key, valid, (uint32_t)want, M, reinterpret_cast<uint32_t *>(fsm), s_pre, s_hist, s_pick)
                                 : block_kth_largest<kFinPer>(key, valid, (uint32_t)want, s_hist, s_pick);
        const float L1 = key_f32(kth);
        if (tid == 0) s_cnt = 0;
        __syncthreads();  // also: every thread has its entries in registers, ent[] may be overwritten
        uint32_t mine = 0;
        float eb[kFinPer];
#pragma unroll
        for (int e = 0; e < kFinPer; ++e) {
            eb[e] = valid[e] ? fmaf(qb, resid(row[e]), qa) : 0.0f;
            valid[e] = valid[e] && key_f32(key[e]) + 2.0f * eb[e] >= L1;
            mine += valid[e] ? 1u : 0u;
        }
        uint32_t at = mine ? atomicAdd(&s_cnt, mine) : 0;
#pragma unroll
        for (int e = 0; e < kFinPer; ++e)
            if (valid[e]) {
                Cand cd;
                cd.score = key_f32(key[e]) + eb[e];
                cd.row = row[e];
                ent[at++] = cd;
            }
        __syncthreads();
    }
    const uint32_t m1 = s_cnt;
    if (tid == 0) p.cand_cnt[q] = m1;

    // ---- stage 2: f32 rescoring of the m1 survivors (one wave per row, 4 rows in flight per wave):
    // s2 = sum fma(q_i/|q|, c_i/|c|), |s2 - cos| <= e2 (any summation order)
    const float invq = (float)(1.0 / sqrt(na));
    const int nc4 = ds >> 2;
    float err = 0.0f;
    for (uint32_t base = (uint32_t)wave * 4; base < m1; base += kFinWaves * 4) {
        float dot[4];
        float sc[4];   // f32 store: 1/|c| of the row; compressed: sum of squares of the stored (near-unit) row
        uint32_t rr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = base + j < m1 ? base + j : base;
            rr[j] = ent[i].row;
            sc[j] = CMP ? 0.0f : p.scale[rr[j]];
            dot[j] = 0.0f;
        }
        // per pass of 768 dims: at most 3 float4 per lane and row, all 12 row loads in flight together (the rows
        // are random 1.5-3 KB reads in a multi-GB array: every one is a TLB miss); wide rows take two passes
        for (int tb = 0; tb * 64 < nc4; tb += kMaxKC / 2) {
            float4 x[4][kMaxKC / 2];
#pragma unroll
            for (int t = 0; t < kMaxKC / 2; ++t) {
                const int c4 = lane + 64 * (tb + t);
                if (c4 < nc4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[j][t] = row_load4<CMP>(p.x, p.xh, ds, rr[j], c4);
                }
            }
#pragma unroll
            for (int t = 0; t < kMaxKC / 2; ++t) {
                const int c4 = lane + 64 * (tb + t);
                if (c4 < nc4) {
                    const float4 a = *reinterpret_cast<const float4 *>(qv + 4 * c4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float m = CMP ? 1.0f : sc[j];
                        dot[j] = fmaf(a.x * invq, x[j][t].x * m, dot[j]);
                        dot[j] = fmaf(a.y * invq, x[j][t].y * m, dot[j]);
                        dot[j] = fmaf(a.z * invq, x[j][t].z * m, dot[j]);
                        dot[j] = fmaf(a.w * invq, x[j][t].w * m, dot[j]);
                        if (CMP) sc[j] = fmaf(x[j][t].x, x[j][t].x, fmaf(x[j][t].y, x[j][t].y, fmaf(x[j][t].z, x[j][t].z, fmaf(x[j][t].w, x[j][t].w, sc[j]))));
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                dot[j] += __shfl_xor(dot[j], o);
                if (CMP) sc[j] += __shfl_xor(sc[j], o);
            }
        }
        if (lane < 4 && base + lane < m1) {
            const float d0 = lane == 0 ? dot[0] : lane == 1 ? dot[1] : lane == 2 ? dot[2] : dot[3];
            const float s0 = lane == 0 ? sc[0] : lane == 1 ? sc[1] : lane == 2 ? sc[2] : sc[3];
            // zero-norm row (f32 store: its 1/|c| is kept as 0; compressed: every element is 0): dist 0
            const bool zero_row = !(s0 > 0.0f);
            const float s2 = zero_row ? 1.0f : (CMP ? d0 * __frsqrt_rn(s0) : d0);
            if (p.max_err && !zero_row) err = fmaxf(err, fabsf(s2 - ent[base + lane].score));
            ent[base + lane].score = s2;
        }
    }
    if (p.max_err) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) err = fmaxf(err, __shfl_xor(err, o));
        // one atomic per workgroup on the batch's word, not one per wave (all on one address)
        if (lane == 0 && err > 0.0f) atomicMax(&s_err, __float_as_uint(err));
    }
    __syncthreads();
    if (p.max_err && tid == 0 && s_err) atomicMax(reinterpret_cast<unsigned int *>(p.max_err), s_err);

    // ---- k-th best f32 score L; keep [L - 2*e2, +inf); publish the retry threshold
#pragma unroll
    for (int e = 0; e < kFinPer; ++e) {
        const uint32_t i = (uint32_t)e * kFinThreads + tid;
        valid[e] = i < m1;
        if (valid[e]) {
            const Cand cd = ent[i];
            key[e] = f32_key(cd.score);
            row[e] = cd.row;
        } else {
            key[e] = 0;
            row[e] = 0xffffffffu;
        }
    }
    {
        uint32_t kth;
        if (m1 <= 64u) {
            // the usual case (a few dozen survivors): wave 0 ranks them with shuffles, no histogram passes
            if (wave == 0) {
                const uint32_t mk = key[0];  // entry `lane` (kFinThreads >= 64: entry e = 0 of threads 0..63)
                uint32_t gt = 0, ge = 0;
                for (int j = 0; j < 64; ++j) {
                    const uint32_t o = __shfl(mk, j);
                    const bool ov = (uint32_t)j < m1;
                    gt += (ov && o > mk) ? 1u : 0u;
                    ge += (ov && o >= mk) ? 1u : 0u;
                }
                if (valid[0] && gt < (uint32_t)want && (uint32_t)want <= ge) s_pick[0] = mk;  // ties write the same value
            }
            __syncthreads();
            kth = s_pick[0];
        } else {
            kth = block_kth_largest<kFinPer>(key, valid, (uint32_t)want, s_hist, s_pick);
        }
        const float L = key_f32(kth);
        if (tid == 0) {
            p.theta_retry[q] = L - p.e2 - qa - 1e-6f;  // a row of the top-k: score + qa + qb * residual >= L - e2
            s_cnt = 0;
        }
        if (lane_ovf || too_many) {  // incomplete candidate set: the host rescans this query with theta_retry
            if (tid == 0) p.overflow[q] = 1;
            return;
        }
        const uint32_t keep = f32_key(L - 2.0f * p.e2);
        __syncthreads();
        uint32_t mine = 0;
#pragma unroll
        for (int e = 0; e < kFinPer; ++e) mine += (valid[e] && key[e] >= keep) ? 1u : 0u;
        uint32_t at = mine ? atomicAdd(&s_cnt, mine) : 0;
#pragma unroll
        for (int e = 0; e < kFinPer; ++e)
            if (valid[e] && key[e] >= keep) {
                Cand cd;
                cd.score = key_f32(key[e]);
                cd.row = row[e];
                ent[at++] = cd;
            }
        __syncthreads();
    }
    const uint32_t m2 = s_cnt;

    // ---- stage 3: exact DistCosine: sequential f64 chain, one thread per row, key = (dist_bits << 32 |
    // row).  Up to kStageRows survivors (the usual case: k plus a few) are first copied to LDS by the
    // whole block -- one coalesced fetch instead of a dozen dependent ones per chain; beyond that the
    // chains read global memory (the rows are L2-warm from stage 2).
    constexpr int kStageRows = 32;
    uint32_t *srow = reinterpret_cast<uint32_t *>(qv + ds);                     // [kStageRows] row ids
    float *stage = reinterpret_cast<float *>(fsm) + 2 * kStageRows;            // behind kStageRows keys
    const int pitch = ds + 4;                                                   // +16 B: conflict-free ds_read_b128 across rows
    // rows that fit behind the keys in ent[]'s storage: 32 up to 1020 dims, 21 at 1536
    const uint32_t stage_rows = min((uint32_t)kStageRows, (uint32_t)((sizeof(Cand) * kCandCap - 2 * kStageRows * sizeof(float)) / (pitch * sizeof(float))));
    // the listed wide-norm rows join here: mt keys in all
    uint32_t nwv = 0;  // those of them below n_rows (a rolled-back append may have left later ones)
    for (uint32_t i = 0; i < nw; ++i) nwv += (uint64_t)p.wild_rows[i] < p.n_rows ? 1u : 0u;  // ascending: a prefix
    const uint32_t mt = m2 + nwv;
    if (mt > (uint32_t)kCandCap) {
        // keys[] shares ent[]'s kCandCap entries and the raw query sits right behind them: a duplicate-heavy corpus can
        // keep (nearly) kCandCap survivors, and the wide-norm rows on top would run into qv[].  Workgroup-uniform: the
        // host rescans the query with theta_retry and, if that overflows as well, answers it on the EXACT path.
        if (tid == 0) p.overflow[q] = 1;
        return;
    }
    if (mt <= stage_rows) {
        if (tid < (int)m2) srow[tid] = ent[tid].row;
        else if (tid < (int)mt) srow[tid] = p.wild_rows[tid - (int)m2];
        __syncthreads();  // row ids are out of ent[]: its storage becomes keys + staged rows
        const uint32_t nc4s = (uint32_t)ds >> 2;
        for (uint32_t i = tid; i < mt * nc4s; i += kFinThreads) {
            const uint32_t r = i / nc4s, c4 = i - r * nc4s;
            *reinterpret_cast<float4 *>(stage + (size_t)r * pitch + 4 * c4) = row_load4<CMP>(p.x, p.xh, ds, srow[r], (int)c4);
        }
        __syncthreads();
        if (p.serial & kSerialSplit) {
            // two lanes per row, one per chain (2 * mt <= 64: one wave): lane 2r sums dot, lane 2r + 1 nb, each in exact_dist_row's
            // element order, so the sums keep their bits; the even lane fetches nb and finishes the row
            if (wave == 0) {
                const uint32_t r = (uint32_t)lane >> 1;
                const bool second = (lane & 1) != 0;
                const float *rowp = stage + (size_t)(r < mt ? r : 0u) * pitch;
                const double acc = r < mt ? f64_chain(second ? rowp : qv, rowp, ds) : 0.0;
                const double nb = __shfl_down(acc, 1);
                if (!second && r < mt) {
                    const float d = dist_from_sums(acc, na, nb);
                    keys[r] = r >= m2 && is_dead(srow[r]) ? ~0ull : ((uint64_t)__float_as_uint(d) << 32) | srow[r];  // as below
                }
            }
        } else if (tid < (int)mt) {
            const float d = exact_dist_row(qv, stage + (size_t)tid * pitch, ds, na, nullptr);
            keys[tid] = tid >= (int)m2 && is_dead(srow[tid]) ? ~0ull : ((uint64_t)__float_as_uint(d) << 32) | srow[tid];  // a masked listed row (the candidates are not): last
        }
    } else {
        // (keys[] shares ent[]'s storage, 8 bytes per entry both: thread cI reads ent[cI] and writes keys[cI] itself)
        for (uint32_t cI = tid; cI < mt; cI += kFinThreads) {
            const uint32_t r = cI < m2 ? ent[cI].row : p.wild_rows[cI - m2];
            const float d = exact_dist_stored<CMP>(qv, p.x, p.xh, ds, r, na);
            keys[cI] = cI >= m2 && is_dead(r) ? ~0ull : ((uint64_t)__float_as_uint(d) << 32) | r;  // a masked listed row (the candidates are not): last
        }
    }
    __syncthreads();

    // ---- order by (dist, row) and emit the first `want`
    uint64_t lim = ~0ull;  // keys above the want-th smallest need no rank
    if (mt > 2048u) {
        // many exact ties (duplicated rows): select the want-th smallest key first (64-bit radix,
        // MSB first), so that the quadratic ranking below runs on `want` keys only
        uint64_t prefix = 0;
        for (int bit = 63; bit >= 0; --bit) {
            const uint64_t trial = prefix | (1ull << bit);
            uint32_t cc = 0;
            for (uint32_t cI = tid; cI < mt; cI += kFinThreads) cc += keys[cI] < trial ? 1u : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cc += __shfl_xor(cc, o);
            uint32_t *slot = s_sel[bit & 1];
            if (lane == 0) slot[wave] = cc;
            __syncthreads();
            cc = 0;
#pragma unroll
            for (int w = 0; w < kFinWaves; ++w) cc += slot[w];
            if (cc < (uint32_t)want) prefix = trial;  // fewer than `want` keys below trial: the want-th is >= trial
        }
        lim = prefix;
    }
    for (uint32_t cI = tid; cI < mt; cI += kFinThreads) {
        const uint64_t me = keys[cI];
        if (me > lim) continue;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < mt; ++j) rank += keys[j] < me ? 1u : 0u;
        if (rank < (uint32_t)want) {
            const float d = __uint_as_float((uint32_t)(me >> 32));
            oid[rank] = p.idmap.id_of((uint32_t)me);
            osc[rank] = score_from_dist(d);
            if (odi) odi[rank] = d;
        }
    }
}

// One workgroup per query (finish_query above), then the completion signal of FinishParams.
template <bool CMP>
__global__ __launch_bounds__(kFinThreads) void finish_kernel(const FinishParams p) {
    finish_query<CMP>(p);  // every exit of it is workgroup-uniform
    if (!p.host_flags) return;
    __shared__ uint32_t s_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        // this workgroup's results and flag words before its tick (results in mapped host memory: visible to the host, which
        // reads them as soon as it sees the sequence number)
        if (p.host_out) __threadfence_system();
        else __threadfence();
        s_last = atomicAdd(p.done_ctr, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    // summary of the batch for the host (4 words + seq: one small write over PCIe; the per-query words stay
    // in HBM and are only fetched when the summary says some query overflowed)
    __shared__ uint32_t s_sum[4];
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
    __threadfence();
    __syncthreads();
    if ((int)threadIdx.x < p.n_queries) {
        const uint32_t ovf = __hip_atomic_load(&p.dev_flags[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t cnt = __hip_atomic_load(&p.dev_flags[kMaxBatch + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t bad = __hip_atomic_load(&p.dev_flags[3 * kMaxBatch + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ovf) atomicMax(&s_sum[0], ovf);
        atomicAdd(&s_sum[1], cnt);
        if (bad) atomicOr(&s_sum[2], 1u);
        // e1 is a positive float: the order of its bits is its order
        atomicMax(&s_sum[3], __hip_atomic_load(&p.dev_flags[2 * kMaxBatch + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        p.host_flags[0] = s_sum[0];  // 0: nobody overflowed; 1: some need the retry pass; >= 2: some need EXACT
        p.host_flags[1] = s_sum[1];  // candidates rescored in f32, whole batch
        p.host_flags[2] = s_sum[2];  // a query held non-finite values
        p.host_flags[3] = s_sum[3];  // largest e1 of the batch (the bound the profiling maximum is checked against)
        *p.done_ctr = 0;
        __hip_atomic_store(&p.host_flags[4], p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t finish_setup() {
    const int lds = (int)(sizeof(Cand) * (size_t)kCandCap + sizeof(float) * (size_t)kMaxKC16 * kChunkFloats + kFinishTailBytes);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&finish_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&finish_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

hipError_t launch_finish(hipStream_t s, int B, const FinishParams &p) {
    if (B <= 0) return hipSuccess;
    if (p.nwg > kMaxScanWGs || 2 * p.nwg > kFinThreads) return hipErrorInvalidValue;  // one lane buffer per thread
    const size_t lds = sizeof(Cand) * (size_t)kCandCap + sizeof(float) * (size_t)p.ds + kFinishTailBytes;  // candidates | query | staged row ids | record offsets
    if (p.x) hipLaunchKernelGGL(finish_kernel<false>, dim3(B), dim3(kFinThreads), lds, s, p);
    else hipLaunchKernelGGL(finish_kernel<true>, dim3(B), dim3(kFinThreads), lds, s, p);  // compressed corpus: rows come from xh
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// EXACT path: f64 DistCosine on every row, then a 64-step MSB-first select on (dist,row) keys
// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// EXACT path, batched: every row against a GROUP of up to 32 queries in one pass (k > 256, more listed rows than
// finish_kernel takes, rows wider than the scans, MX_SEARCH_EXACT, and queries whose neighbourhood overflowed twice).
// The reference answers any vector and any limit at one price (local.rs:71-91); so must this: a group costs about one
// f32 scan of the corpus plus five light passes over its 4-byte distances, whatever k is.
//   exact_dist_batch_kernel   dist[g][row] = DistCosine(query g, row): f32 products, sequential f64 sums in element
//                             order (one chain per pair), as the oracle; a workgroup = 64 rows x 32 queries, the rows and
//                             the queries of a 128-dim chunk in LDS (rows padded: conflict-free), thread = 1 row x 8 queries
//   xsel_hist / xsel_pick     3-pass radix select (12 + 12 + 8 bits) of the kk-th smallest distance per query
//   xsel_count / xsel_collect rows below it, plus the lowest-numbered rows equal to it (ties are ordered by row: slices
//                             are contiguous and ascending, a tie's rank is a prefix count)
//   xsel_emit_kernel          order the kk keys by (dist, row), emit ids / scores / dists
// ---------------------------------------------------------------------------------------------
constexpr int kXRows = 64;      // rows per workgroup pass
constexpr int kXChunk = 128;    // dims per LDS chunk
constexpr int kXPitch = kXChunk + 4;  // row pitch in floats: lanes (rows) hit distinct bank groups with 16-byte reads

// QPT = queries per thread: the workgroup's four waves take QPT queries each (4 QPT per pass over the rows); the host picks
// the smallest QPT that holds the group, so that four queries do not pay for thirty-two
template <bool CMP, int QPT>
__global__ __launch_bounds__(256) void exact_dist_batch_kernel(int ds, const float *__restrict__ x, const void *__restrict__ xh,
                                                               uint64_t n_rows, const float *__restrict__ qpad,
                                                               const double *__restrict__ qnorm2, ExactGroup grp,
                                                               uint32_t *__restrict__ dist, const uint64_t *__restrict__ dead) {
    __shared__ __attribute__((aligned(16))) float s_rows[kXRows * kXPitch];
    __shared__ __attribute__((aligned(16))) float s_q[kExactGroup * kXChunk];
    const int tid = threadIdx.x, lr = tid & 63, qg = tid >> 6;  // local row, query group of the wave (QPT queries)
    const int nq = grp.n;
    double na[QPT];
#pragma unroll
    for (int j = 0; j < QPT; ++j) na[j] = qg * QPT + j < nq ? qnorm2[grp.q[qg * QPT + j]] : 0.0;
    const uint64_t tiles = (n_rows + kXRows - 1) / kXRows;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t r0 = t * kXRows;
        double dot[QPT], nb = 0.0;
#pragma unroll
        for (int j = 0; j < QPT; ++j) dot[j] = 0.0;
        for (int c0 = 0; c0 < ds; c0 += kXChunk) {
            __syncthreads();  // the previous chunk has been consumed
            for (int i = tid; i < kXRows * (kXChunk / 4); i += 256) {  // coalesced: 32 consecutive float4 per row
                const int r = i / (kXChunk / 4), c4 = i % (kXChunk / 4);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r0 + r < n_rows) v = row_load4<CMP>(x, xh, ds, (uint32_t)(r0 + r), c0 / 4 + c4);
                *reinterpret_cast<float4 *>(s_rows + r * kXPitch + 4 * c4) = v;
            }
            for (int i = tid; i < 4 * QPT * (kXChunk / 4); i += 256) {
                const int g = i / (kXChunk / 4), c4 = i % (kXChunk / 4);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (g < nq) v = *reinterpret_cast<const float4 *>(qpad + (size_t)grp.q[g] * ds + c0 + 4 * c4);
                *reinterpret_cast<float4 *>(s_q + g * kXChunk + 4 * c4) = v;
            }
            __syncthreads();
            const float *rw = s_rows + lr * kXPitch;
            const float *qw = s_q + qg * QPT * kXChunk;
#pragma unroll 2
            for (int i = 0; i < kXChunk / 4; ++i) {
                const float4 c = *reinterpret_cast<const float4 *>(rw + 4 * i);
                nb += (double)__fmul_rn(c.x, c.x);
                nb += (double)__fmul_rn(c.y, c.y);
                nb += (double)__fmul_rn(c.z, c.z);
                nb += (double)__fmul_rn(c.w, c.w);
#pragma unroll
                for (int j = 0; j < QPT; ++j) {
                    const float4 a = *reinterpret_cast<const float4 *>(qw + j * kXChunk + 4 * i);  // same address in every lane
                    dot[j] += (double)__fmul_rn(a.x, c.x);
                    dot[j] += (double)__fmul_rn(a.y, c.y);
                    dot[j] += (double)__fmul_rn(a.z, c.z);
                    dot[j] += (double)__fmul_rn(a.w, c.w);
                }
            }
        }
        if (r0 + lr < n_rows) {
            // a removed row: the largest key, which no distance has -- never among the min(k, live rows) selected
            const bool gone = dead && ((dead[(r0 + lr) >> 6] >> ((r0 + lr) & 63u)) & 1ull) != 0;
#pragma unroll
            for (int j = 0; j < QPT; ++j)
                if (qg * QPT + j < nq)
                    dist[(size_t)(qg * QPT + j) * n_rows + r0 + lr] = gone ? 0xffffffffu : __float_as_uint(dist_from_sums(dot[j], na[j], nb));
        }
    }
}

// per query g of the group: state[g] = {prefix, need, -, cursor}; hist[g][4096]
constexpr int kXBins = 4096;
__global__ void xsel_init_kernel(uint32_t kk, uint32_t *state) {
    state[4 * threadIdx.x] = 0;
    state[4 * threadIdx.x + 1] = kk;
    state[4 * threadIdx.x + 2] = 0;
    state[4 * threadIdx.x + 3] = 0;
}
__global__ __launch_bounds__(256) void xsel_hist_kernel(const uint32_t *__restrict__ dist, uint64_t n_rows, int pass,
                                                        const uint32_t *__restrict__ state, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[kXBins];
    const int g = blockIdx.y;
    for (int i = threadIdx.x; i < kXBins; i += 256) h[i] = 0;
    __syncthreads();
    const uint32_t prefix = state[4 * g];
    const int shift = pass == 0 ? 20 : pass == 1 ? 8 : 0;
    const uint32_t bmask = pass == 2 ? 0xffu : 0xfffu;
    const uint32_t pmask = pass == 0 ? 0u : pass == 1 ? 0xfff00000u : 0xffffff00u;
    const uint64_t per = (n_rows + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = lo + per < n_rows ? lo + per : n_rows;
    const uint32_t *d = dist + (size_t)g * n_rows;
    for (uint64_t r = lo + threadIdx.x; r < hi; r += 256) {
        const uint32_t key = d[r];
        if ((key & pmask) == prefix) atomicAdd(&h[(key >> shift) & bmask], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kXBins; i += 256)
        if (h[i]) atomicAdd(&hist[(size_t)g * kXBins + i], h[i]);
}
// one workgroup per query: the bin that holds the need-th smallest remaining key; clears the histogram for the next pass
__global__ __launch_bounds__(256) void xsel_pick_kernel(int pass, uint32_t *__restrict__ state, uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_part[256];
    __shared__ uint32_t s_res[2];
    const int g = blockIdx.x, tid = threadIdx.x;
    uint32_t *h = hist + (size_t)g * kXBins;
    const int nb = pass == 2 ? 256 : kXBins, per = nb / 256;  // bins per thread, ascending
    uint32_t mine = 0;
    for (int i = 0; i < per; ++i) mine += h[tid * per + i];
    s_part[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        const uint32_t need = state[4 * g + 1];
        uint32_t below = 0;
        int t = 0;
        for (; t < 255 && below + s_part[t] < need; ++t) below += s_part[t];
        int bin = t * per;
        for (; bin < t * per + per - 1 && below + h[bin] < need; ++bin) below += h[bin];
        const int shift = pass == 0 ? 20 : pass == 1 ? 8 : 0;
        s_res[0] = state[4 * g] | ((uint32_t)bin << shift);
        s_res[1] = need - below;
    }
    __syncthreads();
    for (int i = tid; i < kXBins; i += 256) h[i] = 0;
    if (tid == 0) {
        state[4 * g] = s_res[0];           // pass 2: the kk-th smallest key T itself
        state[4 * g + 1] = s_res[1];       // pass 2: how many rows equal to T are wanted
    }
}
// rows equal to T per slice (slices = contiguous ascending row ranges)
__global__ __launch_bounds__(256) void xsel_count_kernel(const uint32_t *__restrict__ dist, uint64_t n_rows,
                                                         const uint32_t *__restrict__ state, uint32_t *__restrict__ eq_cnt) {
    __shared__ uint32_t s4[4];
    const int g = blockIdx.y;
    const uint32_t T = state[4 * g];
    const uint64_t per = (n_rows + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = lo + per < n_rows ? lo + per : n_rows;
    const uint32_t *d = dist + (size_t)g * n_rows;
    uint32_t c = 0;
    for (uint64_t r = lo + threadIdx.x; r < hi; r += 256) c += d[r] == T ? 1u : 0u;
    c = block_sum_256(c, s4);
    if (threadIdx.x == 0) eq_cnt[(size_t)g * gridDim.x + blockIdx.x] = c;
}
// sel[g][kk]: keys (dist << 32 | row) of the rows below T (any order) and of the first `need` rows equal to T
__global__ __launch_bounds__(256) void xsel_collect_kernel(const uint32_t *__restrict__ dist, uint64_t n_rows, uint32_t kk,
                                                           uint32_t *__restrict__ state, const uint32_t *__restrict__ eq_cnt,
                                                           uint64_t *__restrict__ sel) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_base;
    const int g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t T = state[4 * g], need = state[4 * g + 1], n_lt = kk - need;
    const uint64_t per = (n_rows + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = lo + per < n_rows ? lo + per : n_rows;
    const uint32_t *d = dist + (size_t)g * n_rows;
    uint64_t *out = sel + (size_t)g * kk;
    if (tid == 0) {
        uint32_t b = 0;
        for (unsigned i = 0; i < blockIdx.x; ++i) b += eq_cnt[(size_t)g * gridDim.x + i];
        s_base = b;
    }
    __syncthreads();
    uint32_t eq_base = s_base;  // ties in lower-numbered rows
    for (uint64_t r0 = lo; r0 < hi; r0 += 256) {  // block-uniform trip count
        const uint64_t r = r0 + tid;
        const uint32_t key = r < hi ? d[r] : 0xffffffffu;
        const bool lt = r < hi && key < T, eq = r < hi && key == T;
        if (lt) {
            const uint32_t at = atomicAdd(&state[4 * g + 3], 1u);
            if (at < n_lt) out[at] = ((uint64_t)key << 32) | (uint32_t)r;
        }
        // rank of a tie among the ties of this slice, in row order
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(eq);
        const uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), wtot = (uint32_t)__popcll(bal);
        __syncthreads();
        if (lane == 0) s_w[wave] = wtot;
        __syncthreads();
        uint32_t wbase = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            wbase += w < wave ? s_w[w] : 0u;
            tot += s_w[w];
        }
        if (eq) {
            const uint32_t rank = eq_base + wbase + before;
            if (rank < need) out[n_lt + rank] = ((uint64_t)key << 32) | (uint32_t)r;
        }
        eq_base += tot;
    }
}
__global__ __launch_bounds__(256) void xsel_emit_kernel(int k, uint32_t kk, IdMap idmap, ExactGroup grp,
                                                        const uint64_t *__restrict__ sel_all, uint64_t *ids_all,
                                                        float *scores_all, float *dists_all, int32_t *n_found) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const int q = grp.q[g];
    const uint64_t *sel = sel_all + (size_t)g * kk;
    uint64_t *ids = ids_all + (size_t)q * k;
    float *scores = scores_all + (size_t)q * k;
    float *dists = dists_all ? dists_all + (size_t)q * k : nullptr;
    if (tid == 0) n_found[q] = (int32_t)kk;
    for (int j = tid; j < k; j += 256) {
        ids[j] = 0;
        scores[j] = 0.0f;
        if (dists) dists[j] = INFINITY;
    }
    __syncthreads();
    for (uint32_t c = tid; c < kk; c += 256) {
        const uint64_t me = sel[c];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < kk; ++j) rank += sel[j] < me ? 1u : 0u;
        const float d = __uint_as_float((uint32_t)(me >> 32));
        ids[rank] = idmap.id_of((uint32_t)me);
        scores[rank] = score_from_dist(d);
        if (dists) dists[rank] = d;
    }
}

// scratch layout: hist | state | eq_cnt | sel (the fixed part, sized for a full group) | dist [gcap][n_rows]
static size_t exact_fixed_bytes(uint64_t kk) {
    size_t b = (size_t)kExactGroup * kXBins * sizeof(uint32_t)               // hist
               + (size_t)kExactGroup * 4 * sizeof(uint32_t)                  // state
               + (size_t)kExactGroup * kExactSlices * sizeof(uint32_t);      // eq_cnt
    b = (b + 15) & ~(size_t)15;
    b += (size_t)kExactGroup * (kk ? kk : 1) * sizeof(uint64_t);             // sel
    return (b + 255) & ~(size_t)255;
}

size_t exact_group_scratch_bytes(uint64_t n_rows, int k, int gcap) {
    const uint64_t kk = n_rows < (uint64_t)k ? n_rows : (uint64_t)k;
    return exact_fixed_bytes(kk) + (size_t)gcap * n_rows * sizeof(uint32_t) + 64;
}

hipError_t launch_exact_group(hipStream_t s, int k, int ds, const float *x, const void *xh, uint64_t n_rows, const IdMap &idmap,
                              const float *qpad, const double *qnorm2, const ExactGroup &grp, void *scratch, uint64_t *ids,
                              float *scores, float *dists, int32_t *n_found, const uint64_t *dead, uint64_t n_live) {
    if (grp.n <= 0) return hipSuccess;
    const uint64_t live = n_live < n_rows ? n_live : n_rows;
    const uint32_t kk = (uint32_t)(live < (uint64_t)k ? live : (uint64_t)k);
    char *base = static_cast<char *>(scratch);
    uint32_t *hist = reinterpret_cast<uint32_t *>(base);
    uint32_t *state = hist + (size_t)kExactGroup * kXBins;
    uint32_t *eq_cnt = state + kExactGroup * 4;
    uint64_t *sel = reinterpret_cast<uint64_t *>(((uintptr_t)(eq_cnt + (size_t)kExactGroup * kExactSlices) + 15) & ~(uintptr_t)15);
    uint32_t *dist = reinterpret_cast<uint32_t *>(base + exact_fixed_bytes(kk));  // [grp.n][n_rows]: the caller sized it for >= grp.n queries
    if (kk > 0) {
        hipError_t e = hipMemsetAsync(hist, 0, ((size_t)kExactGroup * kXBins + kExactGroup * 4) * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(xsel_init_kernel, dim3(1), dim3(kExactGroup), 0, s, kk, state);
        const uint64_t tiles = (n_rows + kXRows - 1) / kXRows;
        const unsigned blocks = (unsigned)(tiles < 2048 ? tiles : 2048);
#define MX_XDIST(CMP_, QPT_) hipLaunchKernelGGL((exact_dist_batch_kernel<CMP_, QPT_>), dim3(blocks), dim3(256), 0, s, ds, x, xh, n_rows, qpad, qnorm2, grp, dist, dead)
        if (x) {
            if (grp.n <= 4) MX_XDIST(false, 1);
            else if (grp.n <= 8) MX_XDIST(false, 2);
            else if (grp.n <= 16) MX_XDIST(false, 4);
            else MX_XDIST(false, 8);
        } else {
            if (grp.n <= 4) MX_XDIST(true, 1);
            else if (grp.n <= 8) MX_XDIST(true, 2);
            else if (grp.n <= 16) MX_XDIST(true, 4);
            else MX_XDIST(true, 8);
        }
#undef MX_XDIST
        const unsigned slices = (unsigned)((n_rows + 4095) / 4096 < (uint64_t)kExactSlices ? (n_rows + 4095) / 4096 : (uint64_t)kExactSlices);
        const dim3 sg(slices ? slices : 1, grp.n);
        for (int pass = 0; pass < 3; ++pass) {
            hipLaunchKernelGGL(xsel_hist_kernel, sg, dim3(256), 0, s, dist, n_rows, pass, state, hist);
            hipLaunchKernelGGL(xsel_pick_kernel, dim3(grp.n), dim3(256), 0, s, pass, state, hist);
        }
        hipLaunchKernelGGL(xsel_count_kernel, sg, dim3(256), 0, s, dist, n_rows, state, eq_cnt);
        hipLaunchKernelGGL(xsel_collect_kernel, sg, dim3(256), 0, s, dist, n_rows, kk, state, eq_cnt, sel);
    }
    hipLaunchKernelGGL(xsel_emit_kernel, dim3(grp.n), dim3(256), 0, s, k, kk, idmap, grp, sel, ids, scores, dists, n_found);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// multi-GPU merge of per-shard top-k lists (after the RCCL all-gather)
// ---------------------------------------------------------------------------------------------
// shard g's lists: ids at ids_base + g*ids_stride, dists at dists_base + g*dists_stride (bytes), each [B, k]
__global__ __launch_bounds__(256) void merge_kernel(const char *__restrict__ ids_base, size_t ids_stride,
                                                    const char *__restrict__ dists_base, size_t dists_stride,
                                                    int G, int B, int k, uint64_t *out_ids, float *out_dists,
                                                    float *out_scores) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int total = G * k;
    for (int j = tid; j < k; j += 256) {
        out_ids[(size_t)b * k + j] = 0;
        out_dists[(size_t)b * k + j] = INFINITY;
        if (out_scores) out_scores[(size_t)b * k + j] = 0.0f;
    }
    __syncthreads();
    for (int c = tid; c < total; c += 256) {
        const int g = c / k, j = c % k;
        const size_t o = (size_t)b * k + j;
        const uint64_t id = reinterpret_cast<const uint64_t *>(ids_base + (size_t)g * ids_stride)[o];
        if (id == 0) continue;
        const float d = reinterpret_cast<const float *>(dists_base + (size_t)g * dists_stride)[o];
        int rank = 0;
        for (int c2 = 0; c2 < total; ++c2) {
            const int g2 = c2 / k;
            const size_t o2 = (size_t)b * k + (c2 % k);
            const uint64_t id2 = reinterpret_cast<const uint64_t *>(ids_base + (size_t)g2 * ids_stride)[o2];
            if (id2 == 0) continue;
            const float d2 = reinterpret_cast<const float *>(dists_base + (size_t)g2 * dists_stride)[o2];
            rank += (d2 < d || (d2 == d && id2 < id)) ? 1 : 0;
        }
        if (rank < k) {
            out_ids[(size_t)b * k + rank] = id;
            out_dists[(size_t)b * k + rank] = d;
            if (out_scores) out_scores[(size_t)b * k + rank] = score_from_dist(d);
        }
    }
}

// compressed corpus -> rows [row0, row0 + n) as f32 [n, d] (exact widening; zero-norm rows come out as zeros)
__global__ __launch_bounds__(256) void unshadow_kernel(const void *__restrict__ xh, int ds, int d, uint64_t row0, uint64_t n,
                                                       float *__restrict__ out) {
    const int nc4 = (d + 3) / 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n * (uint64_t)nc4; i += (uint64_t)gridDim.x * 256) {
        const uint64_t r = i / nc4;
        const int c4 = (int)(i - r * nc4);
        const float4 v = row_load4<true>(nullptr, xh, ds, (uint32_t)(row0 + r), c4);
        float *o = out + r * (uint64_t)d + 4 * c4;
        if (4 * c4 + 0 < d) o[0] = v.x;
        if (4 * c4 + 1 < d) o[1] = v.y;
        if (4 * c4 + 2 < d) o[2] = v.z;
        if (4 * c4 + 3 < d) o[3] = v.w;
    }
}

hipError_t launch_unshadow(hipStream_t s, const void *xh, int ds, int d, uint64_t row0, uint64_t n, float *out) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n * (uint64_t)((d + 3) / 4) + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(unshadow_kernel, dim3((unsigned)blocks), dim3(256), 0, s, xh, ds, d, row0, n, out);
    return hipGetLastError();
}

__global__ void fill_nfound_kernel(int32_t *nf, int B, int32_t v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) nf[i] = v;
}

hipError_t launch_fill_nfound(hipStream_t s, int32_t *nf, int B, int32_t v) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(fill_nfound_kernel, dim3((B + 255) / 256), dim3(256), 0, s, nf, B, v);
    return hipGetLastError();
}

hipError_t launch_merge(hipStream_t s, const void *ids, size_t ids_stride, const void *dists, size_t dists_stride,
                        int G, int B, int k, uint64_t *out_ids, float *out_dists, float *out_scores) {
    if (B <= 0 || k <= 0) return hipSuccess;
    hipLaunchKernelGGL(merge_kernel, dim3(B), dim3(256), 0, s, static_cast<const char *>(ids), ids_stride,
                       static_cast<const char *>(dists), dists_stride, G, B, k, out_ids, out_dists, out_scores);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// filtered search (mx_index_search_filtered)
// ---------------------------------------------------------------------------------------------
// mask[t] = dead[t] | ~allow(t) for every 64-row word t < words.  allow(t): the bits of the rows of word t that lie in one of the
// n_ranges sorted, disjoint, non-adjacent local ranges [lo, hi) (u64 pairs); a binary search finds the first range that ends past
// the word, and at most 32 such ranges can meet one word.  One thread per word, one vector store each.
__global__ __launch_bounds__(256) void filter_mask_kernel(const uint64_t *__restrict__ dead, const uint64_t *__restrict__ ranges,
                                                          uint32_t n_ranges, uint64_t words, uint64_t *__restrict__ mask) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= words) return;
    const uint64_t r0 = t * 64, r1 = r0 + 64;
    uint32_t lo = 0, hi = n_ranges;  // first range with end > r0
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ranges[2 * mid + 1] <= r0) lo = mid + 1;
        else hi = mid;
    }
    uint64_t allow = 0;
    for (uint32_t i = lo; i < n_ranges && ranges[2 * i] < r1; ++i) {
        const uint64_t a = (ranges[2 * i] > r0 ? ranges[2 * i] : r0) - r0;
        const uint64_t b = (ranges[2 * i + 1] < r1 ? ranges[2 * i + 1] : r1) - r0;  // a < b <= 64
        const uint64_t upto = b == 64 ? ~0ull : (1ull << b) - 1ull;
        allow |= upto & ~((1ull << a) - 1ull);
    }
    mask[t] = (dead ? dead[t] : 0ull) | ~allow;
}

hipError_t launch_filter_mask(hipStream_t s, const uint64_t *dead, const uint64_t *ranges, uint32_t n_ranges, uint64_t words,
                              uint64_t *mask) {
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(filter_mask_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, dead, ranges, n_ranges, words, mask);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// resident filters (mx_filter): one allow bit per local row, kept in HBM next to the rows
// ---------------------------------------------------------------------------------------------
// The rows of word t inside one of the sorted, disjoint ranges, found as filter_mask_kernel finds them.
__device__ __forceinline__ uint64_t word_selection(const uint64_t *__restrict__ ranges, uint32_t n_ranges, uint64_t t) {
    const uint64_t r0 = t * 64, r1 = r0 + 64;
    uint32_t lo = 0, hi = n_ranges;  // first range with end > r0
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ranges[2 * mid + 1] <= r0) lo = mid + 1;
        else hi = mid;
    }
    uint64_t sel = 0;
    for (uint32_t i = lo; i < n_ranges && ranges[2 * i] < r1; ++i) {
        const uint64_t a = (ranges[2 * i] > r0 ? ranges[2 * i] : r0) - r0;
        const uint64_t b = (ranges[2 * i + 1] < r1 ? ranges[2 * i + 1] : r1) - r0;  // a < b <= 64
        const uint64_t upto = b == 64 ? ~0ull : (1ull << b) - 1ull;
        sel |= upto & ~((1ull << a) - 1ull);
    }
    return sel;
}

// One thread per word of [w0, w1): a word belongs to one thread, so the read-modify-write needs no atomic.
__global__ __launch_bounds__(256) void filter_range_edit_kernel(const uint64_t *__restrict__ ranges, uint32_t n_ranges, uint64_t w0,
                                                                uint64_t w1, int allow, uint64_t *__restrict__ bits) {
    const uint64_t t = w0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= w1) return;
    const uint64_t sel = word_selection(ranges, n_ranges, t);
    if (sel == 0) return;
    bits[t] = allow ? bits[t] | sel : bits[t] & ~sel;
}

hipError_t launch_filter_range_edit(hipStream_t s, const uint64_t *ranges, uint32_t n_ranges, uint64_t w0, uint64_t w1, bool allow,
                                    uint64_t *bits) {
    if (w1 <= w0 || n_ranges == 0) return hipSuccess;
    hipLaunchKernelGGL(filter_range_edit_kernel, dim3((unsigned)((w1 - w0 + 255) / 256)), dim3(256), 0, s, ranges, n_ranges, w0, w1,
                       allow ? 1 : 0, bits);
    return hipGetLastError();
}

// One thread per id; ids repeat and several ids share a word, hence the atomics.
__global__ __launch_bounds__(256) void filter_id_edit_kernel(const uint64_t *__restrict__ ids, uint64_t n_ids, uint64_t total, IdMap idmap,
                                                             int allow, unsigned long long *bits, uint64_t bit_words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ids) return;
    const uint64_t id = ids[i];
    if (id <= idmap.id_offset) return;
    uint64_t r = id - idmap.id_offset - 1;
    if (r >= total) return;
    if (idmap.block_rows) {  // a shard: rows of its own blocks only, global block b -> local block b / G
        const uint64_t b = r / idmap.block_rows;
        if (b % idmap.n_shards != idmap.shard) return;
        r = (b / idmap.n_shards) * idmap.block_rows + r % idmap.block_rows;
    }
    if ((r >> 6) >= bit_words) return;
    const unsigned long long bit = 1ull << (r & 63);
    if (allow) atomicOr(bits + (r >> 6), bit);
    else atomicAnd(bits + (r >> 6), ~bit);
}

hipError_t launch_filter_id_edit(hipStream_t s, const uint64_t *ids, uint64_t n_ids, uint64_t total, const IdMap &idmap, bool allow,
                                 uint64_t *bits, uint64_t bit_words) {
    if (n_ids == 0 || bit_words == 0) return hipSuccess;
    hipLaunchKernelGGL(filter_id_edit_kernel, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, s, ids, n_ids, total, idmap,
                       allow ? 1 : 0, reinterpret_cast<unsigned long long *>(bits), bit_words);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void filter_apply_kernel(const uint64_t *__restrict__ dead, const uint64_t *__restrict__ bits,
                                                           uint64_t bit_words, uint64_t words, uint64_t *__restrict__ mask) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= words) return;
    mask[t] = t < bit_words ? (dead ? dead[t] : 0ull) | ~bits[t] : ~0ull;
}

hipError_t launch_filter_apply(hipStream_t s, const uint64_t *dead, const uint64_t *bits, uint64_t bit_words, uint64_t words,
                               uint64_t *mask) {
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(filter_apply_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, dead, bits, bit_words, words, mask);
    return hipGetLastError();
}

// One workgroup.  Thread i owns the consecutive words [w0 + i * per, w0 + (i + 1) * per): it counts their live allowed rows, an
// inclusive scan over the 1024 counts gives it the position of its first row, and it writes its rows in ascending order.
constexpr int kListThreads = 1024;
__global__ __launch_bounds__(kListThreads) void filter_list_kernel(const uint64_t *__restrict__ dead, const uint64_t *__restrict__ bits,
                                                                   uint64_t w0, uint64_t w1, uint32_t *__restrict__ rows, uint32_t cap) {
    __shared__ uint32_t s_scan[kListThreads];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (w1 - w0 + kListThreads - 1) / kListThreads;
    const uint64_t a = w0 + (uint64_t)tid * per < w1 ? w0 + (uint64_t)tid * per : w1;
    const uint64_t b = a + per < w1 ? a + per : w1;
    uint32_t cnt = 0;
    for (uint64_t t = a; t < b; ++t) cnt += (uint32_t)__popcll(bits[t] & ~(dead ? dead[t] : 0ull));
    s_scan[tid] = cnt;
    __syncthreads();
    for (uint32_t o = 1; o < (uint32_t)kListThreads; o <<= 1) {
        const uint32_t v = tid >= o ? s_scan[tid - o] : 0u;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    uint32_t pos = s_scan[tid] - cnt;
    for (uint64_t t = a; t < b; ++t) {
        uint64_t live = bits[t] & ~(dead ? dead[t] : 0ull);
        while (live) {
            const uint32_t bit = (uint32_t)__ffsll((unsigned long long)live) - 1u;
            live &= live - 1;
            if (pos < cap) rows[pos] = (uint32_t)(t * 64 + bit);
            ++pos;
        }
    }
}

hipError_t launch_filter_list(hipStream_t s, const uint64_t *dead, const uint64_t *bits, uint64_t w0, uint64_t w1, uint32_t *rows,
                              uint32_t cap) {
    if (w1 <= w0) return hipSuccess;
    hipLaunchKernelGGL(filter_list_kernel, dim3(1), dim3(kListThreads), 0, s, dead, bits, w0, w1, rows, cap);
    return hipGetLastError();
}

// Small filters: one workgroup per query against the m listed rows (ascending local rows, m <= kSubsetCap).  Each thread takes
// rows i = tid, tid + 1024, ...: exact DistCosine through exact_dist_stored -- the f64 chain of finish_kernel's stage 3 and of the
// EXACT path, so zero-norm, wide-norm and compressed rows get the same bits there and here -- into the key
// (dist_bits << 32) | i.  The list is ascending in local row and a shard's local order is its id order, so ordering keys orders by
// (dist, id).  Up to 2048 rows every key is ranked against all of them; above, an MSB-first select over the bits a key can have
// (dist bits, 14 position bits) finds the want-th smallest key, the want keys at or below it move to the front, and only they
// are ranked.  Keys are unique (the position), so exactly `want` of them qualify and every output slot is written once.
constexpr int kSubsetPer = kSubsetCap / kFinThreads;
constexpr int kSubsetPosBits = 14;
static_assert((1 << kSubsetPosBits) == kSubsetCap, "position bits of a subset key");
template <bool CMP>
__global__ __launch_bounds__(kFinThreads) void subset_topk_kernel(int k, int ds, const float *__restrict__ x, const void *__restrict__ xh,
                                                                 const uint32_t *__restrict__ rows, uint32_t m, IdMap idmap,
                                                                 const float *__restrict__ qpad, const double *__restrict__ qnorm2,
                                                                 uint64_t *ids, float *scores, float *dists, int32_t *n_found) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    uint64_t *keys = reinterpret_cast<uint64_t *>(ssm);                        // [kSubsetCap]
    float *qv = reinterpret_cast<float *>(ssm + sizeof(uint64_t) * kSubsetCap);  // [ds] raw query
    __shared__ uint32_t s_sel[2][kFinWaves];
    __shared__ uint32_t s_cnt;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t want = m < (uint32_t)k ? m : (uint32_t)k;
    uint64_t *oid = ids + (size_t)q * k;
    float *osc = scores + (size_t)q * k;
    float *odi = dists ? dists + (size_t)q * k : nullptr;
    if (tid == 0) n_found[q] = (int32_t)want;
    for (int j = (int)want + tid; j < k; j += kFinThreads) {  // unused slots (the first `want` are written below)
        oid[j] = 0;
        osc[j] = 0.0f;
        if (odi) odi[j] = INFINITY;
    }
    if (want == 0) return;
    for (int i = tid; i < ds; i += kFinThreads) qv[i] = qpad[(size_t)q * ds + i];
    __syncthreads();
    const double na = qnorm2[q];
    for (uint32_t i = tid; i < m; i += kFinThreads) {
        const float d = exact_dist_stored<CMP>(qv, x, xh, ds, rows[i], na);
        keys[i] = ((uint64_t)__float_as_uint(d) << 32) | i;
    }
    __syncthreads();
    uint32_t mt = m;  // keys[0, mt) are ranked
    if (m > 2048u && m > want) {
        uint64_t prefix = 0;
        for (int bit = 63; bit >= 0; --bit) {
            if (bit < 32 && bit >= kSubsetPosBits) continue;  // zero in every key (and so in the want-th smallest)
            const uint64_t trial = prefix | (1ull << bit);
            uint32_t cc = 0;
            for (uint32_t i = tid; i < m; i += kFinThreads) cc += keys[i] < trial ? 1u : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cc += __shfl_xor(cc, o);
            uint32_t *slot = s_sel[bit & 1];  // bits 32 and 13 are consecutive passes: the slots still alternate
            if (lane == 0) slot[wave] = cc;
            __syncthreads();
            cc = 0;
#pragma unroll
            for (int w = 0; w < kFinWaves; ++w) cc += slot[w];
            if (cc < want) prefix = trial;  // fewer than `want` keys below trial: the want-th smallest is >= trial
        }
        uint64_t v[kSubsetPer];
        bool sel[kSubsetPer];
#pragma unroll
        for (int e = 0; e < kSubsetPer; ++e) {
            const uint32_t i = (uint32_t)e * kFinThreads + tid;
            sel[e] = i < m && keys[i] <= prefix;
            v[e] = sel[e] ? keys[i] : 0ull;
        }
        if (tid == 0) s_cnt = 0;
        __syncthreads();  // every key is in registers: the front of keys[] may be overwritten
#pragma unroll
        for (int e = 0; e < kSubsetPer; ++e)
            if (sel[e]) keys[atomicAdd(&s_cnt, 1u)] = v[e];
        __syncthreads();
        mt = want;
    }
    for (uint32_t c = tid; c < mt; c += kFinThreads) {
        const uint64_t me = keys[c];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < mt; ++j) rank += keys[j] < me ? 1u : 0u;
        if (rank < want) {
            const float d = __uint_as_float((uint32_t)(me >> 32));
            oid[rank] = idmap.id_of(rows[(uint32_t)me]);
            osc[rank] = score_from_dist(d);
            if (odi) odi[rank] = d;
        }
    }
}

static size_t subset_lds_bytes(int ds) { return sizeof(uint64_t) * (size_t)kSubsetCap + sizeof(float) * (size_t)ds; }

hipError_t subset_setup() {
    const int lds = (int)subset_lds_bytes(kMaxKC16 * kChunkFloats);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&subset_topk_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&subset_topk_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

hipError_t launch_subset_topk(hipStream_t s, int B, int k, int ds, const float *x, const void *xh, const uint32_t *rows, uint32_t m,
                              const IdMap &idmap, const float *qpad, const double *qnorm2, uint64_t *ids, float *scores, float *dists,
                              int32_t *n_found) {
    if (B <= 0) return hipSuccess;
    if (m > (uint32_t)kSubsetCap || ds > kMaxKC16 * kChunkFloats) return hipErrorInvalidValue;
    const size_t lds = subset_lds_bytes(ds);
    if (x) hipLaunchKernelGGL(subset_topk_kernel<false>, dim3(B), dim3(kFinThreads), lds, s, k, ds, x, xh, rows, m, idmap, qpad, qnorm2, ids, scores, dists, n_found);
    else hipLaunchKernelGGL(subset_topk_kernel<true>, dim3(B), dim3(kFinThreads), lds, s, k, ds, x, xh, rows, m, idmap, qpad, qnorm2, ids, scores, dists, n_found);  // compressed corpus
    return hipGetLastError();
}


// ---------------------------------------------------------------------------------------------
// range search (mx_index_search_range): every row whose score reaches the query's threshold t.  The host
// turns t into an exclusive bound on the f32 dist's bits, dlim (in range <=> bits(dist) < dlim; 0 = nothing, t > 1), and the collect
// launch runs with theta = 1 - D - eps - qa (range_theta_kernel): every in-range row reaches the lane records.
// ---------------------------------------------------------------------------------------------
__global__ void range_theta_kernel(int B, const uint32_t *__restrict__ dlim, float eps, const float *__restrict__ qa,
                                   float *__restrict__ theta) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B || theta[q] == INFINITY) return;  // zero-norm and padded queries stay parked
    const uint32_t lim = dlim[q];
    theta[q] = lim == 0 ? INFINITY : 1.0f - __uint_as_float(lim - 1u) - eps - qa[q];
}

hipError_t launch_range_theta(hipStream_t s, int B, const uint32_t *dlim, float eps, const float *qa, float *theta) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(range_theta_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, dlim, eps, qa, theta);
    return hipGetLastError();
}

// One workgroup per query.  Gather exactly as finish_query does; then decide every candidate: by its filter bounds (certainly in /
// certainly out / undecided), the undecided by f32 rescoring (error e2), what is still undecided -- and the listed wide-norm rows --
// by the exact f64 DistCosine against dlim.  n_in_range = the rows decided in.  Emit: all of them when they are at most cap, else the
// cap-th best lower bound L and the rows whose upper bound reaches L - 2 eps; exact dists for those, order by (dist, row), first
// min(cap, n_in_range).  A lane-buffer overflow, or more candidates than the block holds, flags the query for the EXACT path (2).
template <bool CMP>
__device__ __forceinline__ void range_query(const RangeParams &rp) {
    const FinishParams &p = rp.f;
    extern __shared__ __attribute__((aligned(16))) char fsm[];
    Cand *ent = reinterpret_cast<Cand *>(fsm);                                        // [kCandCap]
    uint64_t *keys = reinterpret_cast<uint64_t *>(fsm);                               // same storage, at the end
    float *qv = reinterpret_cast<float *>(fsm + sizeof(Cand) * (size_t)kCandCap);     // [ds] raw query
    __shared__ uint32_t s_w[kFinWaves];
    __shared__ uint32_t s_sel[2][kFinWaves];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_pick[2];
    __shared__ uint32_t s_cnt;

    const int q = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int cap = p.k, ds = p.ds;
    const uint32_t dlim = rp.dlim[q];
    const float eps = rp.eps;
    uint64_t *oid = p.ids + (size_t)q * cap;
    float *osc = p.scores + (size_t)q * cap;
    float *odi = p.dists ? p.dists + (size_t)q * cap : nullptr;
    if (tid == 0) {
        p.n_found[q] = 0;
        rp.n_in_range[q] = 0;
        p.cand_cnt[q] = 0;
    }
    for (int j = tid; j < cap; j += kFinThreads) {
        oid[j] = 0;
        osc[j] = 0.0f;
        if (odi) odi[j] = INFINITY;
    }
    if (dlim == 0 || p.n_live == 0) return;  // threshold above 1, or no live row
    const double na = p.qnorm2[q];
    if (!(na > 0.0)) {
        // zero-norm query: dist 0 (score 1) against every row, so every live row is in range; the first cap of them by id
        const uint32_t want = (uint32_t)(p.n_live < (uint64_t)cap ? p.n_live : (uint64_t)cap);
        if (tid == 0) {
            p.n_found[q] = (int32_t)want;
            rp.n_in_range[q] = p.n_live;
        }
        uint32_t found = 0;  // block-uniform
        for (uint64_t w0 = 0; found < want && w0 * 64 < p.n_rows; w0 += kFinThreads) {
            const uint64_t w = w0 + (uint64_t)tid;
            uint64_t live = 0;
            if (w * 64 < p.n_rows) {
                live = p.dead ? ~p.dead[w] : ~0ull;
                const uint64_t rem = p.n_rows - w * 64;
                if (rem < 64) live &= (1ull << rem) - 1ull;
            }
            uint32_t tot;
            uint32_t j = found + block_scan_1024((uint32_t)__popcll(live), s_w, &tot);
            for (; live && j < want; ++j) {
                const uint64_t row = w * 64 + (uint64_t)__builtin_ctzll(live);
                live &= live - 1;
                oid[j] = p.idmap.id_of((uint32_t)row);
                osc[j] = 1.0f;
                if (odi) odi[j] = 0.0f;
            }
            found += tot;
        }
        return;
    }
    const float D = __uint_as_float(dlim - 1u);
    const float cin = 1.0f - D + eps, cout = 1.0f - D - eps;  // cosine >= cin: certainly in; < cout: certainly out
    const uint32_t lane_ovf = p.overflow[q];
    const float qa = p.qa[q], qb = p.qb[q];
    auto resid = [&](uint32_t row) { return p.terr ? p.terr[kTscaleFloats * (size_t)(row >> 6) + 2 + ((row >> 5) & 1u)] : 0.0f; };
    for (int i = tid; i < ds; i += kFinThreads) qv[i] = p.qpad[(size_t)q * ds + i];

    // ---- gather (finish_query's, unchanged): candidates carry the lower bound of their cosine
    const int nwg = p.nwg;
    const float th = p.theta[q];
    const uint32_t nz = p.n_zero, nw = p.n_wild;
    auto in_list = [&](const uint32_t *list, uint32_t n, uint32_t row) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (list[mid] < row) lo = mid + 1;
            else hi = mid;
        }
        return lo < n && list[lo] == row;
    };
    auto is_zero_row = [&](uint32_t row) { return (nz && in_list(p.zero_rows, nz, row)) || (nw && in_list(p.wild_rows, nw, row)); };
    auto is_dead = [&](uint32_t row) { return p.dead && ((p.dead[row >> 6] >> (row & 63u)) & 1ull) != 0; };
    uint32_t *s_off = reinterpret_cast<uint32_t *>(qv + ds) + 32;
    uint32_t nrec = 0;
    if (tid < 2 * nwg) {
        const uint32_t hh0 = (uint32_t)(tid / nwg);
        const int w = tid - (int)hh0 * nwg;
        nrec = p.lane_cnt[(size_t)((uint32_t)(q >> 5) * 64 + (uint32_t)(q & 31) + 32u * hh0) * nwg + w];
        nrec = nrec > (uint32_t)kRecCap ? (uint32_t)kRecCap : nrec;
    }
    uint32_t R;
    const uint32_t roff = block_scan_1024(nrec, s_w, &R);
    if (tid < 2 * nwg) s_off[tid] = roff;
    if (tid == 0) s_off[2 * nwg] = R;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    auto put = [&](uint32_t at, float sc, uint32_t row) {
        if (at < (uint32_t)kCandCap) {
            Cand cd;
            cd.score = sc;
            cd.row = row;
            ent[at] = cd;
        }
    };
    for (uint32_t j0 = 0; j0 < R; j0 += kFinThreads) {
        const uint32_t j = j0 + tid;
        uint32_t mask = 0, rowb = 0;
        float v[16];
        if (j < R) {
            uint32_t lo = 0, hi = (uint32_t)(2 * nwg) - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (s_off[mid] <= j) lo = mid;
                else hi = mid - 1;
            }
            const uint32_t e = j - s_off[lo], hh = lo / (uint32_t)nwg, w = lo - hh * (uint32_t)nwg;
            const size_t l = (size_t)((uint32_t)(q >> 5) * 64 + (uint32_t)(q & 31) + 32u * hh) * nwg + w;
            const f32x4 *rec = reinterpret_cast<const f32x4 *>(p.lane_rec + l * (kRecCap * 16)) + e * 4;
            const uint32_t t32 = p.lane_tile[l * kRecCap + e];
            rowb = t32 * kTileRows + 4u * hh;
            const uint32_t dm = p.dead ? lane_dead16(dead_half(p.dead, t32), hh) : 0u;
            const f32x4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = a[r], v[4 + r] = b[r], v[8 + r] = c[r], v[12 + r] = d[r];
            if (p.rec_int) int_record_scores(v, p.terr[kTscaleFloats * (size_t)(t32 >> 1) + (t32 & 1u)], p.qscale[q]);
            const float er = resid(rowb);
            const float thr = fmaf(-qb, er, th), eb = fmaf(qb, er, qa);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t row = rowb + (r & 3) + 8 * (r >> 2);
                const bool pass = v[r] >= thr && (uint64_t)row < p.n_rows && !(v[r] == 0.0f && (nz | nw) && is_zero_row(row)) && !((dm >> r) & 1u);
                mask |= pass ? (1u << r) : 0u;
                v[r] -= eb;
            }
        }
        const uint32_t cnt = (uint32_t)__popc(mask);
        uint32_t inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        uint32_t wbase = 0;
        if (lane == 63 && inc) wbase = atomicAdd(&s_cnt, inc);
        wbase = __shfl(wbase, 63);
        uint32_t at = wbase + inc - cnt;
        if (mask) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (mask & (1u << r)) put(at++, v[r], rowb + (r & 3) + 8 * (r >> 2));
        }
    }
    for (uint32_t z = tid; z < nz; z += kFinThreads)
        if ((uint64_t)p.zero_rows[z] < p.n_rows && !is_dead(p.zero_rows[z])) put(atomicAdd(&s_cnt, 1u), 1.0f, p.zero_rows[z]);
    __syncthreads();
    const uint32_t M = s_cnt;
    uint32_t nwv = 0;  // listed wide-norm rows below n_rows (ascending: a prefix)
    for (uint32_t i = 0; i < nw; ++i) nwv += (uint64_t)p.wild_rows[i] < p.n_rows ? 1u : 0u;
    if (lane_ovf || M + nwv > (uint32_t)kCandCap) {  // an incomplete or too large candidate set: the EXACT range path
        if (tid == 0) p.overflow[q] = 2;
        return;
    }

    // ---- stage A: filter bounds.  ent becomes [in (nA) | undecided (nU)]
    uint32_t row[kFinPer];
    float lb[kFinPer];
    uint32_t st[kFinPer];  // 0 out, 1 in, 2 undecided
    uint32_t mi = 0, mu = 0;
#pragma unroll
    for (int e = 0; e < kFinPer; ++e) {
        const uint32_t i = (uint32_t)e * kFinThreads + tid;
        st[e] = 0;
        row[e] = 0;
        lb[e] = 0.0f;
        if (i < M) {
            const Cand cd = ent[i];
            row[e] = cd.row;
            lb[e] = cd.score;
            st[e] = lb[e] >= cin ? 1u : lb[e] + 2.0f * fmaf(qb, resid(cd.row), qa) < cout ? 0u : 2u;
            mi += st[e] == 1u ? 1u : 0u;
            mu += st[e] == 2u ? 1u : 0u;
        }
    }
    uint32_t nA, nU;
    {
        uint32_t pi = block_scan_1024(mi, s_w, &nA);
        uint32_t pu = block_scan_1024(mu, s_w, &nU);  // (every entry is in registers: both scans synchronise the block)
        pu += nA;
#pragma unroll
        for (int e = 0; e < kFinPer; ++e) {
            if (st[e] == 0u) continue;
            Cand cd;
            cd.score = lb[e];
            cd.row = row[e];
            ent[st[e] == 1u ? pi++ : pu++] = cd;
        }
        __syncthreads();
    }
    if (tid == 0) p.cand_cnt[q] = nU;

    // ---- stage B: f32 rescoring of the undecided (finish_query's stage 2): s2, |s2 - cos| <= e2
    const float invq = (float)(1.0 / sqrt(na));
    const int nc4 = ds >> 2;
    for (uint32_t base = (uint32_t)wave * 4; base < nU; base += kFinWaves * 4) {
        float dot[4];
        float sc[4];
        uint32_t rr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = base + j < nU ? base + j : base;
            rr[j] = ent[nA + i].row;
            sc[j] = CMP ? 0.0f : p.scale[rr[j]];
            dot[j] = 0.0f;
        }
        for (int tb = 0; tb * 64 < nc4; tb += kMaxKC / 2) {
            float4 x[4][kMaxKC / 2];
#pragma unroll
            for (int t = 0; t < kMaxKC / 2; ++t) {
                const int c4 = lane + 64 * (tb + t);
                if (c4 < nc4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[j][t] = row_load4<CMP>(p.x, p.xh, ds, rr[j], c4);
                }
            }
#pragma unroll
            for (int t = 0; t < kMaxKC / 2; ++t) {
                const int c4 = lane + 64 * (tb + t);
                if (c4 < nc4) {
                    const float4 a = *reinterpret_cast<const float4 *>(qv + 4 * c4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float m = CMP ? 1.0f : sc[j];
                        dot[j] = fmaf(a.x * invq, x[j][t].x * m, dot[j]);
                        dot[j] = fmaf(a.y * invq, x[j][t].y * m, dot[j]);
                        dot[j] = fmaf(a.z * invq, x[j][t].z * m, dot[j]);
                        dot[j] = fmaf(a.w * invq, x[j][t].w * m, dot[j]);
                        if (CMP) sc[j] = fmaf(x[j][t].x, x[j][t].x, fmaf(x[j][t].y, x[j][t].y, fmaf(x[j][t].z, x[j][t].z, fmaf(x[j][t].w, x[j][t].w, sc[j]))));
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                dot[j] += __shfl_xor(dot[j], o);
                if (CMP) sc[j] += __shfl_xor(sc[j], o);
            }
        }
        if (lane < 4 && base + lane < nU) {
            const float d0 = lane == 0 ? dot[0] : lane == 1 ? dot[1] : lane == 2 ? dot[2] : dot[3];
            const float s0 = lane == 0 ? sc[0] : lane == 1 ? sc[1] : lane == 2 ? sc[2] : sc[3];
            const bool zero_row = !(s0 > 0.0f);
            ent[nA + base + lane].score = zero_row ? 1.0f : (CMP ? d0 * __frsqrt_rn(s0) : d0);
        }
    }
    __syncthreads();
    // ... the undecided region becomes [in (nB) | undecided (n2)]
    uint32_t nB, n2;
    {
        mi = mu = 0;
#pragma unroll
        for (int e = 0; e < kFinPer; ++e) {
            const uint32_t i = (uint32_t)e * kFinThreads + tid;
            st[e] = 0;
            if (i < nU) {
                const Cand cd = ent[nA + i];
                row[e] = cd.row;
                lb[e] = cd.score;
                st[e] = cd.score - p.e2 >= cin ? 1u : cd.score + p.e2 < cout ? 0u : 2u;
                mi += st[e] == 1u ? 1u : 0u;
                mu += st[e] == 2u ? 1u : 0u;
            }
        }
        uint32_t pi = block_scan_1024(mi, s_w, &nB);
        uint32_t pu = block_scan_1024(mu, s_w, &n2);
        pi += nA;
        pu += nA + nB;
#pragma unroll
        for (int e = 0; e < kFinPer; ++e) {
            if (st[e] == 0u) continue;
            Cand cd;
            cd.score = lb[e];
            cd.row = row[e];
            ent[st[e] == 1u ? pi++ : pu++] = cd;
        }
        __syncthreads();
    }

    // ---- stage C: exact DistCosine of the still undecided and of the listed wide-norm rows; the entry keeps its row and gets the
    // exact dist as its score when the row is in range, -1 when it is not (or is masked)
    const uint32_t c0 = nA + nB, nC = n2 + nwv;  // c0 + nC <= M + nwv <= kCandCap
    for (uint32_t i = tid; i < nC; i += kFinThreads) {
        const uint32_t r = i < n2 ? ent[c0 + i].row : p.wild_rows[i - n2];
        const float d = exact_dist_stored<CMP>(qv, p.x, p.xh, ds, r, na);
        Cand cd;
        cd.score = (i >= n2 && is_dead(r)) || __float_as_uint(d) >= dlim ? -1.0f : d;
        cd.row = r;
        ent[c0 + i] = cd;
    }
    __syncthreads();

    // ---- count, and the rows to order: [0, nA) filter-certified (lower bound), [nA, c0) f32-certified (s2), [c0, T) exact.
    // stm: two bits per entry (0 not in range, 1 in range by bounds, 3 in range with its exact dist in ent[].score)
    const uint32_t T = c0 + nC;
    uint32_t stm = 0, mine = 0;
#pragma unroll
    for (int e = 0; e < kFinPer; ++e) {
        const uint32_t i = (uint32_t)e * kFinThreads + tid;
        lb[e] = 0.0f;
        row[e] = 0;
        if (i < T) {
            const Cand cd = ent[i];
            row[e] = cd.row;
            uint32_t s = 0;
            if (i < nA) lb[e] = cd.score, s = 1;
            else if (i < c0) lb[e] = cd.score - p.e2, s = 1;
            else if (cd.score >= 0.0f) lb[e] = 1.0f - cd.score - eps, s = 3;
            stm |= s << (2 * e);
            mine += s ? 1u : 0u;
        }
    }
    uint32_t C;
    (void)block_scan_1024(mine, s_w, &C);
    const uint32_t want = C < (uint32_t)cap ? C : (uint32_t)cap;
    if (tid == 0) {
        p.n_found[q] = (int32_t)want;
        rp.n_in_range[q] = C;
    }
    if (C == 0) return;
    if (C > (uint32_t)cap) {
        // more than cap: L = the cap-th best lower bound; a row whose upper bound stays below L - 2 eps has cap rows strictly ahead
        // of it
        uint32_t key[kFinPer];
        bool valid[kFinPer];
#pragma unroll
        for (int e = 0; e < kFinPer; ++e) {
            valid[e] = ((stm >> (2 * e)) & 3u) != 0u;
            key[e] = valid[e] ? f32_key(lb[e]) : 0u;
        }
        const float L = key_f32(block_kth_largest<kFinPer>(key, valid, (uint32_t)cap, s_hist, s_pick)) - 2.0f * eps;
#pragma unroll
        for (int e = 0; e < kFinPer; ++e) {
            const uint32_t s = (stm >> (2 * e)) & 3u;
            if (!s) continue;
            const uint32_t i = (uint32_t)e * kFinThreads + tid;
            const float v = ent[i].score;  // (ent[] is intact until the keys are written)
            const float ubv = i < nA ? v + 2.0f * fmaf(qb, resid(row[e]), qa) : i < c0 ? v + p.e2 : 1.0f - v + eps;
            if (!(ubv >= L)) stm &= ~(3u << (2 * e));
        }
    }
    uint32_t K;
    {
        mine = 0;
#pragma unroll
        for (int e = 0; e < kFinPer; ++e) {
            const uint32_t s = (stm >> (2 * e)) & 3u;
            mine += s ? 1u : 0u;
            if (s == 3u) lb[e] = ent[(uint32_t)e * kFinThreads + tid].score;  // the exact dist
        }
        uint32_t at = block_scan_1024(mine, s_w, &K);
        __syncthreads();  // every entry is in registers: ent[]'s storage becomes the keys
#pragma unroll
        for (int e = 0; e < kFinPer; ++e) {
            const uint32_t s = (stm >> (2 * e)) & 3u;
            if (!s) continue;
            const uint64_t hi = s == 3u ? (uint64_t)__float_as_uint(lb[e]) : 0xffffffffull;  // all ones: dist still to compute
            keys[at++] = (hi << 32) | row[e];
        }
        __syncthreads();
    }
    // exact dists of the rows certified by bounds
    for (uint32_t cI = tid; cI < K; cI += kFinThreads) {
        const uint64_t me = keys[cI];
        if ((me >> 32) != 0xffffffffull) continue;
        const uint32_t r = (uint32_t)me;
        const float d = exact_dist_stored<CMP>(qv, p.x, p.xh, ds, r, na);
        keys[cI] = ((uint64_t)__float_as_uint(d) << 32) | r;
    }
    __syncthreads();

    // ---- order by (dist, row) and emit the first `want` (finish_query's ranking)
    uint64_t lim = ~0ull;
    if (K > 2048u) {
        uint64_t prefix = 0;
        for (int bit = 63; bit >= 0; --bit) {
            const uint64_t trial = prefix | (1ull << bit);
            uint32_t cc = 0;
            for (uint32_t cI = tid; cI < K; cI += kFinThreads) cc += keys[cI] < trial ? 1u : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cc += __shfl_xor(cc, o);
            uint32_t *slot = s_sel[bit & 1];
            if (lane == 0) slot[wave] = cc;
            __syncthreads();
            cc = 0;
#pragma unroll
            for (int w = 0; w < kFinWaves; ++w) cc += slot[w];
            if (cc < want) prefix = trial;
        }
        lim = prefix;
    }
    for (uint32_t cI = tid; cI < K; cI += kFinThreads) {
        const uint64_t me = keys[cI];
        if (me > lim) continue;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < K; ++j) rank += keys[j] < me ? 1u : 0u;
        if (rank < want) {
            const float d = __uint_as_float((uint32_t)(me >> 32));
            oid[rank] = p.idmap.id_of((uint32_t)me);
            osc[rank] = score_from_dist(d);
            if (odi) odi[rank] = d;
        }
    }
}

// One workgroup per query (range_query above), then finish_kernel's completion signal: the summary words of the batch's flag block
// into host-mapped memory, the sequence number behind them
template <bool CMP>
__global__ __launch_bounds__(kFinThreads) void range_finish_kernel(const RangeParams rp) {
    range_query<CMP>(rp);  // every exit of it is workgroup-uniform
    const FinishParams &p = rp.f;
    if (!p.host_flags) return;
    __shared__ uint32_t s_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (p.host_out) __threadfence_system();
        else __threadfence();
        s_last = atomicAdd(p.done_ctr, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __shared__ uint32_t s_sum[4];
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
    __threadfence();
    __syncthreads();
    if ((int)threadIdx.x < p.n_queries) {
        const uint32_t ovf = __hip_atomic_load(&p.dev_flags[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t cnt = __hip_atomic_load(&p.dev_flags[kMaxBatch + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t bad = __hip_atomic_load(&p.dev_flags[3 * kMaxBatch + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ovf) atomicMax(&s_sum[0], ovf);
        atomicAdd(&s_sum[1], cnt);
        if (bad) atomicOr(&s_sum[2], 1u);
        atomicMax(&s_sum[3], __hip_atomic_load(&p.dev_flags[2 * kMaxBatch + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        p.host_flags[0] = s_sum[0];
        p.host_flags[1] = s_sum[1];
        p.host_flags[2] = s_sum[2];
        p.host_flags[3] = s_sum[3];
        *p.done_ctr = 0;
        __hip_atomic_store(&p.host_flags[4], p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t range_setup() {
    const int lds = (int)(sizeof(Cand) * (size_t)kCandCap + sizeof(float) * (size_t)kMaxKC16 * kChunkFloats + kFinishTailBytes);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&range_finish_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&range_finish_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

hipError_t launch_range_finish(hipStream_t s, int B, const RangeParams &rp) {
    if (B <= 0) return hipSuccess;
    const FinishParams &p = rp.f;
    if (p.nwg > kMaxScanWGs || 2 * p.nwg > kFinThreads || p.ds > kMaxKC16 * kChunkFloats) return hipErrorInvalidValue;
    const size_t lds = sizeof(Cand) * (size_t)kCandCap + sizeof(float) * (size_t)p.ds + kFinishTailBytes;
    if (p.x) hipLaunchKernelGGL(range_finish_kernel<false>, dim3(B), dim3(kFinThreads), lds, s, rp);
    else hipLaunchKernelGGL(range_finish_kernel<true>, dim3(B), dim3(kFinThreads), lds, s, rp);
    return hipGetLastError();
}

// EXACT range path: in-range rows of each query of the group per row slice (dist key < dlim; masked rows carry the all-ones key)
__global__ __launch_bounds__(256) void xrange_count_kernel(const uint32_t *__restrict__ dist, uint64_t n_rows, ExactGroup grp,
                                                           const uint32_t *__restrict__ dlim, uint32_t *__restrict__ cnt) {
    __shared__ uint32_t s4[4];
    const int g = blockIdx.y;
    const uint32_t lim = dlim[grp.q[g]];
    const uint64_t per = (n_rows + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = lo + per < n_rows ? lo + per : n_rows;
    const uint32_t *d = dist + (size_t)g * n_rows;
    uint32_t c = 0;
    for (uint64_t r = lo + threadIdx.x; r < hi; r += 256) c += d[r] < lim ? 1u : 0u;
    c = block_sum_256(c, s4);
    if (threadIdx.x == 0) cnt[(size_t)g * gridDim.x + blockIdx.x] = c;
}
// the count over the slices; the emitted list (the kk best rows, best first) trimmed to min(cap, count)
__global__ __launch_bounds__(256) void xrange_trim_kernel(int cap, uint32_t kk, unsigned slices, ExactGroup grp,
                                                          const uint32_t *__restrict__ cnt, uint64_t *ids_all, float *scores_all,
                                                          float *dists_all, int32_t *n_found, uint64_t *n_in_range) {
    __shared__ uint32_t s4[4];
    const int g = blockIdx.x, q = grp.q[g];
    uint32_t c = 0;
    if (cnt)
        for (unsigned i = threadIdx.x; i < slices; i += 256) c += cnt[(size_t)g * slices + i];
    c = block_sum_256(c, s4);
    const uint32_t nf = c < (uint32_t)cap ? c : (uint32_t)cap;
    if (threadIdx.x == 0) {
        n_found[q] = (int32_t)nf;
        n_in_range[q] = c;
    }
    for (uint32_t j = nf + threadIdx.x; j < kk; j += 256) {
        ids_all[(size_t)q * cap + j] = 0;
        scores_all[(size_t)q * cap + j] = 0.0f;
        if (dists_all) dists_all[(size_t)q * cap + j] = INFINITY;
    }
}

hipError_t launch_exact_range_group(hipStream_t s, int cap, int ds, const float *x, const void *xh, uint64_t n_rows, const IdMap &idmap,
                                    const float *qpad, const double *qnorm2, const ExactGroup &grp, void *scratch, const uint32_t *dlim,
                                    uint64_t *ids, float *scores, float *dists, int32_t *n_found, uint64_t *n_in_range,
                                    const uint64_t *dead, uint64_t n_live) {
    if (grp.n <= 0) return hipSuccess;
    hipError_t e = launch_exact_group(s, cap, ds, x, xh, n_rows, idmap, qpad, qnorm2, grp, scratch, ids, scores, dists, n_found, dead, n_live);
    if (e != hipSuccess) return e;
    // the layout launch_exact_group used: the histogram area is free again (xsel_pick_kernel cleared it) and holds the slice counts
    const uint64_t live = n_live < n_rows ? n_live : n_rows;
    const uint32_t kk = (uint32_t)(live < (uint64_t)cap ? live : (uint64_t)cap);
    char *base = static_cast<char *>(scratch);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(base);
    const uint32_t *dist = reinterpret_cast<const uint32_t *>(base + exact_fixed_bytes(kk));
    const unsigned slices = (unsigned)((n_rows + 4095) / 4096 < (uint64_t)kExactSlices ? (n_rows + 4095) / 4096 : (uint64_t)kExactSlices);
    if (kk > 0) hipLaunchKernelGGL(xrange_count_kernel, dim3(slices ? slices : 1, grp.n), dim3(256), 0, s, dist, n_rows, grp, dlim, cnt);
    hipLaunchKernelGGL(xrange_trim_kernel, dim3(grp.n), dim3(256), 0, s, cap, kk, slices ? slices : 1u, grp, kk > 0 ? cnt : nullptr,
                       ids, scores, dists, n_found, n_in_range);
    return hipGetLastError();
}

// sharded handle: n_in_range[b] = sum over the G shards' counts (counts of shard g at base + g * stride bytes), n_found = min(cap, it)
__global__ void range_sum_kernel(const char *__restrict__ base, size_t stride, int G, int B, int cap, uint64_t *n_in_range,
                                 int32_t *n_found) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint64_t c = 0;
    for (int g = 0; g < G; ++g) c += reinterpret_cast<const uint64_t *>(base + (size_t)g * stride)[b];
    n_in_range[b] = c;
    n_found[b] = (int32_t)(c < (uint64_t)cap ? c : (uint64_t)cap);
}

hipError_t launch_range_sum(hipStream_t s, const void *counts, size_t stride, int G, int B, int cap, uint64_t *n_in_range, int32_t *n_found) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(range_sum_kernel, dim3((B + 255) / 256), dim3(256), 0, s, static_cast<const char *>(counts), stride, G, B, cap,
                       n_in_range, n_found);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// diversified search (mx_index_search_mmr): the stored rows of the candidates, widened to f32, and the
// greedy MMR selection over them
// ---------------------------------------------------------------------------------------------
// stage[i, ds] = the stored row rows[i] (zero padding included), one workgroup per row
template <bool CMP>
__global__ __launch_bounds__(256) void mmr_gather_kernel(const float *__restrict__ x, const void *__restrict__ xh, int ds,
                                                         const uint32_t *__restrict__ rows, float *__restrict__ stage) {
    const uint32_t row = rows[blockIdx.x];
    float4 *dst = reinterpret_cast<float4 *>(stage + (size_t)blockIdx.x * ds);
    for (int c4 = threadIdx.x; c4 < ds / 4; c4 += 256) dst[c4] = row_load4<CMP>(x, xh, ds, row, c4);
}

hipError_t launch_mmr_gather(hipStream_t s, int ds, const float *x, const void *xh, const uint32_t *rows, uint32_t n, float *stage) {
    if (n == 0) return hipSuccess;
    if (x) hipLaunchKernelGGL(mmr_gather_kernel<false>, dim3(n), dim3(256), 0, s, x, xh, ds, rows, stage);
    else hipLaunchKernelGGL(mmr_gather_kernel<true>, dim3(n), dim3(256), 0, s, x, xh, ds, rows, stage);
    return hipGetLastError();
}

// order-preserving map f64 -> u64 (a NaN ranks with -inf); every key is > 0
__device__ __forceinline__ uint64_t mmr_key(double v) {
    if (!(v == v)) v = -INFINITY;
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
// (key descending, position ascending)
__device__ __forceinline__ void mmr_better(uint64_t &key, uint32_t &pos, uint64_t k2, uint32_t p2) {
    if (k2 > key || (k2 == key && p2 < pos)) {
        key = k2;
        pos = p2;
    }
}

// One workgroup per query, one candidate per thread (blockDim >= fetch).  Candidate i of query q is the i-th entry of the
// candidate stage's lists (ids / rel / dists at q * fetch + i, m = cand_nf[q] of them) and its stored row is row
// pos[q * fetch + i] of stage.  Every thread keeps its candidate's norm sum, its penalty and its state in registers; per
// pick the row picked last is staged in LDS and every unselected candidate runs ONE sequential f64 chain against it (the
// summation order is the contract: a chain is never split across lanes), then the block takes the arg-max of the MMR value.
__global__ __launch_bounds__(1024) void mmr_select_kernel(int k, int fetch, int ds, float lambda, const float *__restrict__ stage,
                                                          const uint32_t *__restrict__ pos, const uint64_t *__restrict__ cand_ids,
                                                          const float *__restrict__ cand_rel, const float *__restrict__ cand_dists,
                                                          const int32_t *__restrict__ cand_nf, uint64_t *__restrict__ ids,
                                                          float *__restrict__ scores, float *__restrict__ dists,
                                                          int32_t *__restrict__ n_found) {
    extern __shared__ __attribute__((aligned(16))) char mmr_lds[];
    float *sel_row = reinterpret_cast<float *>(mmr_lds);                               // [ds]
    uint64_t *wkey = reinterpret_cast<uint64_t *>(mmr_lds + (size_t)ds * sizeof(float));  // [16] per-wave winners
    uint32_t *wpos = reinterpret_cast<uint32_t *>(wkey + 16);                          // [16]
    double *sel_nb = reinterpret_cast<double *>(wpos + 16);                            // [1] norm sum of the staged row
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = (blockDim.x + 63) >> 6;
    const size_t c0 = (size_t)q * fetch, o0 = (size_t)q * k;
    int m = cand_nf[q];
    m = m < 0 ? 0 : m > fetch ? fetch : m;
    const int found = k < m ? k : m;
    // unused output slots, and the count
    for (int t = found + tid; t < k; t += blockDim.x) {
        ids[o0 + t] = 0;
        scores[o0 + t] = 0.0f;
        if (dists) dists[o0 + t] = INFINITY;
    }
    if (tid == 0) n_found[q] = found;
    if (found == 0) return;  // (block-uniform)

    const bool mine = tid < m;
    const float4 *my4 = reinterpret_cast<const float4 *>(stage + (size_t)(mine ? pos[c0 + tid] : 0u) * ds);
    const double lam = (double)lambda, one_minus = __dsub_rn(1.0, lam);
    const float rel = mine ? cand_rel[c0 + tid] : 0.0f;
    const double lam_rel = __dmul_rn(lam, (double)rel);
    double nb = 0.0;  // the candidate's own norm sum: DistCosine's third chain, independent of the dot chain
    if (mine && found > 1) {
#pragma unroll 8
        for (int i = 0; i < ds / 4; ++i) {
            const float4 c = my4[i];
            nb += (double)__fmul_rn(c.x, c.x);
            nb += (double)__fmul_rn(c.y, c.y);
            nb += (double)__fmul_rn(c.z, c.z);
            nb += (double)__fmul_rn(c.w, c.w);
        }
    }
    float pen = -INFINITY;
    bool open = mine;  // not selected yet
    uint32_t sel = 0;  // the first pick is candidate 0
    for (int t = 0;; ++t) {
        if (tid == (int)sel) {
            open = false;
            ids[o0 + t] = cand_ids[c0 + sel];
            scores[o0 + t] = rel;
            if (dists) dists[o0 + t] = cand_dists[c0 + sel];
            *sel_nb = nb;
        }
        if (t + 1 == found) break;
        // stage the row just picked
        const float4 *s4 = reinterpret_cast<const float4 *>(stage + (size_t)pos[c0 + sel] * ds);
        for (int c4 = tid; c4 < ds / 4; c4 += blockDim.x) reinterpret_cast<float4 *>(sel_row)[c4] = s4[c4];
        __syncthreads();
        uint64_t key = 0;
        uint32_t at = 0xffffffffu;
        if (open) {
            double dot = 0.0;
#pragma unroll 8
            for (int i = 0; i < ds / 4; ++i) {
                const float4 c = my4[i];
                const float4 a = *reinterpret_cast<const float4 *>(sel_row + 4 * i);
                dot += (double)__fmul_rn(a.x, c.x);
                dot += (double)__fmul_rn(a.y, c.y);
                dot += (double)__fmul_rn(a.z, c.z);
                dot += (double)__fmul_rn(a.w, c.w);
            }
            float sim = score_from_dist(dist_from_sums(dot, *sel_nb, nb));
            if (!(sim == sim)) sim = 1.0f;
            pen = sim > pen ? sim : pen;
            key = mmr_key(__dsub_rn(lam_rel, __dmul_rn(one_minus, (double)pen)));
            at = (uint32_t)tid;
        }
        // block arg-max: within the wave by shuffles, across the waves through LDS
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), o), lo = (uint32_t)__shfl_xor((int)(uint32_t)key, o);
            const uint32_t p2 = (uint32_t)__shfl_xor((int)at, o);
            mmr_better(key, at, ((uint64_t)hi << 32) | lo, p2);
        }
        if (lane == 0) {
            wkey[wave] = key;
            wpos[wave] = at;
        }
        __syncthreads();
        key = wkey[0];
        at = wpos[0];
        for (int w = 1; w < nwaves; ++w) mmr_better(key, at, wkey[w], wpos[w]);
        sel = at;
        __syncthreads();  // wkey / wpos / sel_row / sel_nb are rewritten in the next round
    }
}

size_t mmr_select_lds_bytes(int ds) { return (size_t)ds * sizeof(float) + 16 * sizeof(uint64_t) + 16 * sizeof(uint32_t) + 16; }

hipError_t launch_mmr_select(hipStream_t s, int B, int k, int fetch, int ds, float lambda, const float *stage, const uint32_t *pos,
                             const uint64_t *cand_ids, const float *cand_scores, const float *cand_dists, const int32_t *cand_nf,
                             uint64_t *ids, float *scores, float *dists, int32_t *n_found) {
    if (B <= 0) return hipSuccess;
    if (fetch < 1 || fetch > kMmrMaxFetch || k < 1 || k > fetch || ds < 4 || ds > kMmrMaxDs || ds % 4) return hipErrorInvalidValue;
    const int threads = (fetch + 63) / 64 * 64;
    hipLaunchKernelGGL(mmr_select_kernel, dim3(B), dim3(threads), mmr_select_lds_bytes(ds), s, k, fetch, ds, lambda, stage, pos, cand_ids,
                       cand_scores, cand_dists, cand_nf, ids, scores, dists, n_found);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// search by stored row (mx_index_search_by_id / mx_index_search_range_by_id): the stored rows as a query
// block, and the own row taken out of the lists the pass returns
// ---------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup: lane l copies the 16 bytes l, l + 64, ... of the row, so a wave reads and writes 1 KiB of
// consecutive addresses per trip (an f32 corpus; the compressed corpus reads the 8-byte halves of its fragments).  Rows of the block
// are dim floats apart: 16-byte stores when that keeps them aligned, element stores otherwise.
template <bool CMP>
__global__ __launch_bounds__(256) void byid_gather_kernel(int dim, int ds, const float *__restrict__ x, const void *__restrict__ xh,
                                                          const uint32_t *__restrict__ rows, uint32_t n, float *__restrict__ q) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n) return;  // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint32_t row = rows[i];
    float *dst = q + (size_t)i * dim;
    if ((dim & 3) == 0) {
        for (int c4 = lane; c4 < dim / 4; c4 += 64) reinterpret_cast<float4 *>(dst)[c4] = row_load4<CMP>(x, xh, ds, row, c4);
    } else {
        for (int c4 = lane; c4 < (dim + 3) / 4; c4 += 64) {  // (ds >= dim rounded up to a multiple of 4: the load stays inside the row)
            const float4 v = row_load4<CMP>(x, xh, ds, row, c4);
            const int c = 4 * c4;
            dst[c] = v.x;
            if (c + 1 < dim) dst[c + 1] = v.y;
            if (c + 2 < dim) dst[c + 2] = v.z;
            if (c + 3 < dim) dst[c + 3] = v.w;
        }
    }
}

hipError_t launch_byid_gather(hipStream_t s, int dim, int ds, const float *x, const void *xh, const uint32_t *rows, uint32_t n, float *q) {
    if (n == 0) return hipSuccess;
    if (dim < 1 || ds < dim || ds % 4) return hipErrorInvalidValue;
    if (x) hipLaunchKernelGGL(byid_gather_kernel<false>, dim3((n + 3) / 4), dim3(256), 0, s, dim, ds, x, xh, rows, n, q);
    else hipLaunchKernelGGL(byid_gather_kernel<true>, dim3((n + 3) / 4), dim3(256), 0, s, dim, ds, x, xh, rows, n, q);
    return hipGetLastError();
}

// One wave per query, four queries per workgroup.  Reads the internal lists, writes the caller's: never in place.
__global__ __launch_bounds__(256) void byid_drop_self_kernel(ByIdDrop p) {
    const int b = (int)(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (b >= p.B) return;  // (wave-uniform, like everything below but the lane's own slots)
    const int k = p.k, kk = p.kk;
    const uint32_t src = p.src[b];
    const bool live = src != kByIdNone;
    const uint64_t *iid = p.in_ids + (size_t)(live ? src : 0u) * kk;
    const float *isc = p.in_scores + (size_t)(live ? src : 0u) * kk;
    const float *idi = p.in_dists + (size_t)(live ? src : 0u) * kk;
    int m = live ? p.in_nfound[src] : 0;
    m = m < 0 ? 0 : m > kk ? kk : m;
    int at = m;  // where the own row is listed; m: nowhere
    if (live && p.exclude) {
        const uint64_t own = p.own[b];
        for (int i0 = 0; i0 < m && at == m; i0 += 64) {
            const int i = i0 + lane;
            const unsigned long long hit = __ballot(i < m && iid[i] == own);
            if (hit) at = i0 + __builtin_ctzll(hit);
        }
    }
    const int left = m - (at < m ? 1 : 0), found = left < k ? left : k;
    uint64_t *oid = p.ids + (size_t)b * k;
    float *osc = p.scores + (size_t)b * k;
    float *odi = p.dists ? p.dists + (size_t)b * k : nullptr;
    for (int j = lane; j < k; j += 64) {
        const int i = j < at ? j : j + 1;  // (j < found: i < m)
        oid[j] = j < found ? iid[i] : 0;
        osc[j] = j < found ? isc[i] : 0.0f;
        if (odi) odi[j] = j < found ? idi[i] : INFINITY;
    }
    if (lane != 0) return;
    p.n_found[b] = found;
    if (!p.n_in_range) return;
    uint64_t nr = live ? p.in_nrange[src] : 0;
    if (live && p.exclude) {
        if (at < m) {
            nr -= 1;
        } else if (nr > (uint64_t)m) {
            // the list was cut before the own row, if it is in range at all: the plain path's membership test for it.  Query and row
            // are the same values, so DistCosine's three chains are one: 0 unless na * na leaves the f64 range (a wide-norm row)
            const float *v = p.q + (size_t)src * p.dim;
            double na = 0.0;
            for (int i = 0; i < p.dim; ++i) na += (double)__fmul_rn(v[i], v[i]);
            if (__float_as_uint(dist_from_sums(na, na, na)) < p.dlim[src]) nr -= 1;
        }
    }
    p.n_in_range[b] = nr;
}

hipError_t launch_byid_drop_self(hipStream_t s, const ByIdDrop &p) {
    if (p.B <= 0) return hipSuccess;
    if (p.k < 1 || p.kk < p.k || p.kk > p.k + 1 || (p.in_nrange && !p.n_in_range)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(byid_drop_self_kernel, dim3((p.B + 3) / 4), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// fused search (mx_index_search_fused): one ranked list from the candidate lists of a request's sub-queries
// ---------------------------------------------------------------------------------------------
// a record is (a, b): sorted by (b >> 31, a, b), i.e. the records whose top bit of b is set (padding, dropped entries) go last
__device__ __forceinline__ bool fuse_less(uint64_t a1, uint32_t b1, uint64_t a2, uint32_t b2) {
    const uint32_t v1 = b1 >> 31, v2 = b2 >> 31;
    if (v1 != v2) return v1 < v2;
    if (a1 != a2) return a1 < a2;
    return b1 < b2;
}

// bitonic network over the P (a power of two) records of the block, ascending; ends with a barrier
__device__ __forceinline__ void fuse_sort(uint64_t *ka, uint32_t *kb, int P) {
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P / 2; t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;  // (i < l < P)
                const uint64_t ai = ka[i], al = ka[l];
                const uint32_t bi = kb[i], bl = kb[l];
                const bool up = (i & k2) == 0;
                if (up ? fuse_less(al, bl, ai, bi) : fuse_less(ai, bi, al, bl)) {
                    ka[i] = al; kb[i] = bl;
                    ka[l] = ai; kb[l] = bi;
                }
            }
            __syncthreads();
        }
    }
}

constexpr uint32_t kFusePad = 0x80000000u;  // b of a record that is no entry
constexpr int kFusePer = 4;                 // records per thread at the largest block: 4096 / 1024

// One workgroup per request; P = the power of two >= m * fetch (at least 128), blockDim = min(P / 2, 1024).  The entries of the
// consulted lists go to LDS as (id, sub << 8 | rank) -- 12 bytes each, 48 KiB at 4096 -- and are sorted by (id, sub): the entries of one
// row become a run in ascending sub.  The head of each run walks it (at most m entries): the f64 sum in that order, the best (dist, sub)
// with the dists re-read from the lists.  The heads are then sorted in the same LDS by the mode's key; the head's position in the
// first order stands in for its id (both ascend together) and travels with the best entry's (sub, rank), from which the outputs are
// re-read.  No atomics: every record is written by one thread between two barriers.
__global__ __launch_bounds__(1024) void fuse_kernel(FuseArgs p, int P) {
    extern __shared__ __attribute__((aligned(16))) char fuse_lds[];
    uint64_t *ka = reinterpret_cast<uint64_t *>(fuse_lds);                        // [P]
    uint32_t *kb = reinterpret_cast<uint32_t *>(fuse_lds + (size_t)P * 8);        // [P]
    float *w = reinterpret_cast<float *>(fuse_lds + (size_t)P * 12);              // [kFuseMaxSub]
    int *nfl = reinterpret_cast<int *>(w + kFuseMaxSub);                          // [kFuseMaxSub]
    int *heads = nfl + kFuseMaxSub;                                               // [1]
    const int r = blockIdx.x, tid = threadIdx.x, T = blockDim.x, m = p.m, fetch = p.fetch, k = p.k, N = m * fetch;
    const size_t l0 = (size_t)r * m * fetch, o0 = (size_t)r * k;  // the request's lists; its outputs
    if (tid < m) {
        const float wi = p.weights[(size_t)r * m + tid];
        int n = p.cand_nf[(size_t)r * m + tid];
        n = n < 0 ? 0 : n > fetch ? fetch : n;
        w[tid] = wi;
        nfl[tid] = wi > 0.0f ? n : 0;  // an absent sub-query: its list is never consulted
    }
    if (tid == 0) *heads = 0;
    __syncthreads();
    for (int e = tid; e < P; e += T) {
        bool valid = false;
        uint32_t sub = 0, rank = 0;
        if (e < N) {
            sub = (uint32_t)(e / fetch);
            rank = (uint32_t)(e % fetch);
            valid = (int)rank < nfl[sub];
        }
        ka[e] = valid ? p.cand_ids[l0 + e] : 0;
        kb[e] = valid ? (sub << 8 | rank) : kFusePad;
    }
    __syncthreads();
    fuse_sort(ka, kb, P);

    uint64_t hk[kFusePer];
    uint32_t hb[kFusePer];
#pragma unroll
    for (int i = 0; i < kFusePer; ++i) {
        const int e = tid + i * T;
        hk[i] = 0;
        hb[i] = kFusePad;
        if (e >= P || (kb[e] >> 31)) continue;
        const uint64_t id = ka[e];
        if (e > 0 && ka[e - 1] == id) continue;  // (the record before a valid one is valid: they sort first)
        double sum = 0.0;
        float bd = 0.0f;
        uint32_t best = 0;
        for (int j = e; j < P && !(kb[j] >> 31) && ka[j] == id; ++j) {
            const uint32_t b = kb[j], sub = b >> 8, rank = b & 255u;
            if (p.mode == 1) sum = __dadd_rn(sum, __ddiv_rn((double)w[sub], __dadd_rn(p.rrf_c, (double)(rank + 1u))));
            const float d = p.cand_dists[l0 + (size_t)sub * fetch + rank];
            if (j == e || d < bd) {  // (ascending sub: an equal dist keeps the earlier list)
                bd = d;
                best = b;
            }
        }
        // descending fused = ascending ~key; dists are >= +0, so their bits order them
        hk[i] = p.mode == 1 ? ~mmr_key(sum) : (uint64_t)__float_as_uint(bd) << 32;
        hb[i] = (uint32_t)e << 12 | best;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kFusePer; ++i) {
        const int e = tid + i * T;
        if (e < P) {
            ka[e] = hk[i];
            kb[e] = hb[i];
        }
    }
    __syncthreads();
    fuse_sort(ka, kb, P);
    for (int e = tid; e < P; e += T)
        if (!(kb[e] >> 31) && (e + 1 == P || (kb[e + 1] >> 31))) *heads = e + 1;  // the last head: one thread at most
    __syncthreads();
    const int found = *heads < k ? *heads : k;
    for (int t = tid; t < k; t += T) {  // (k <= fetch <= P)
        const bool have = t < found;
        const uint32_t b = have ? kb[t] : 0u, sub = (b >> 8) & 15u;
        const size_t src = l0 + (size_t)sub * fetch + (b & 255u);  // (entry 0 of list 0 for a blank slot: read, not used)
        const float sc = have ? p.cand_scores[src] : 0.0f;
        p.ids[o0 + t] = have ? p.cand_ids[src] : 0;
        p.scores[o0 + t] = sc;
        if (p.dists) p.dists[o0 + t] = have ? p.cand_dists[src] : INFINITY;
        if (p.best_sub) p.best_sub[o0 + t] = have ? (int32_t)sub : -1;
        if (p.fused) {
            double f = 0.0;
            if (have && p.mode == 1) {
                const uint64_t key = ~ka[t];  // mmr_key of the sum, undone
                f = __longlong_as_double((long long)((key >> 63) ? key ^ 0x8000000000000000ull : ~key));
            } else if (have) {
                f = (double)sc;
            }
            p.fused[o0 + t] = f;
        }
    }
    if (tid == 0) p.n_found[r] = found;
}

hipError_t launch_fuse(hipStream_t s, const FuseArgs &p) {
    if (p.R <= 0) return hipSuccess;
    if (p.m < 1 || p.m > kFuseMaxSub || p.fetch < 1 || p.fetch > kFuseMaxFetch || p.k < 1 || p.k > p.fetch || (p.mode != 0 && p.mode != 1))
        return hipErrorInvalidValue;
    int P = 128;
    while (P < p.m * p.fetch) P <<= 1;  // <= 4096 = kFusePer * 1024
    const int threads = P / 2 < 1024 ? P / 2 : 1024;
    const size_t lds = (size_t)P * 12 + kFuseMaxSub * (sizeof(float) + sizeof(int)) + sizeof(int);
    hipLaunchKernelGGL(fuse_kernel, dim3(p.R), dim3(threads), lds, s, p, P);
    return hipGetLastError();
}

}  // namespace mx
