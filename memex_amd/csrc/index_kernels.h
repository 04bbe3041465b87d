// index_kernels.h -- device-side contract of the flat cosine index (launch wrappers + shared
// constants).  The streaming scans live in scan.hip (f32 rows), scan16.hip / scan16w.hip (bf16 filter
// copy, with its builder) and scan8.hip (int8 filter copy, with its builder), what they share in
// scan_common.h; compaction in compact.hip, the search by examples in like_kernels.hip, the scoring of named rows in score_kernels.hip, every other kernel in index_kernels.hip; index.hip holds
// the host logic behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mx {

// ---- geometry of the streaming scan (scan.hip) --------------------------------------------
constexpr int kScanThreads = 512;  // 8 waves: 2 per SIMD
constexpr int kScanWaves = 8;
constexpr int kTileRows = 32;      // one 32x32x16 MFMA A-operand worth of corpus rows
constexpr int kChunkFloats = 128;  // k-chunk: 32 rows x 128 f32 = one 16 KiB LDS slot
constexpr int kSlotBytes = kTileRows * kChunkFloats * 4;
constexpr int kNumSlots = 8;       // f32 LDS ring: 8 x 16 KiB = 128 KiB, all of it in flight
constexpr int kPrefetch = 8;
constexpr int kScaleRing = 16;     // per-tile 1/|c| vectors (128 B each)
// ring + two padded bf16 tiles (32 rows x 272 B) + scale ring
constexpr int kScanLdsBytes = kNumSlots * kSlotBytes + 2 * kTileRows * (kChunkFloats * 2 + 16) + kScaleRing * kTileRows * 4;
constexpr int kMaxKC = 6;          // k-chunks per row the MFMA scan supports (dim_pad <= 768)

// ---- scan over the bf16 filter copy (scan16_kernel): a slot is 32 rows x 128 bf16 = 8 KiB, already
// in MFMA A-fragment order in HBM, so the LDS image is a linear copy and needs no conversion pass
constexpr int kSlot16Bytes = kTileRows * kChunkFloats * 2;
constexpr int kRing16 = 16;        // 16 x 8 KiB = 128 KiB ring, 15 slots in flight
constexpr int kMeanRing16 = 32;    // tiles whose a_c values (centred copy: 128 B per tile in a 256-B entry) can be in flight
constexpr int kScan16LdsBytes = kRing16 * kSlot16Bytes + kMeanRing16 * 256 + 1024;  // slot ring | a_c ring | a_q of the 256 queries
// wide rows (scan16w_kernel, 768 < dim_pad <= 1536): the k-steps of a row are dealt to two waves, 128 queries per
// launch; the ring plus 16 KiB in which the even-slot waves hand their partial sums to the odd-slot waves
constexpr int kMaxKC16 = 12;
constexpr int kWideBatch = 128;
constexpr int kScan16WideLdsBytes = kRing16 * kSlot16Bytes + 4 * 64 * 16 * 4;

constexpr int kPassBatch = 256;    // queries per scan pass (8 waves x 32 MFMA columns)
constexpr int kMaxBatch = 512;     // queries per pipeline batch: a pass of the int8 scan with two query groups per wave (up to
                                   // 512 dims) serves 512; everything else splits a batch into passes of 256 (128: scan16w)
constexpr int kMaxKC8x2 = 4;       // ... up to this many 128-dim slots per row
constexpr int kRecCap = 64;        // lane-private records per collect launch: one record = the lane's 16 scores of a tile
constexpr int kMaxScanCUs = 256;   // CUs a scan spreads over: persistent workgroups, one per CU
constexpr int kMaxScanWGs = 2 * kMaxScanCUs;  // ... two per CU in the int8 scan's two-workgroup form (Scan8Geom::kPair)
constexpr int kCandCap = 16384;    // candidates finish_kernel holds per query (LDS); more = rescan with a tight threshold
constexpr int kZeroCap = 1024;     // zero-norm rows an index tracks in its list (more: EXACT path)
constexpr int kWildCap = 64;       // rows with a norm outside [1e-15, 1e15] an f32 index lists (more: EXACT path)

// MEMEX_HIP_DEBUG=serial=N (mx_debug.h): which of the short serial stages of finish_kernel take their newer form, a sum of the
// items below.  Either item leaves every answer, threshold and candidate set as it is; 0 = the older form throughout
// (tests/test_serial_stages_gpu.py holds the two against each other).
constexpr int kSerialPre = 1;      // the first select (the k-th best lower bound) selects among the keys at or above a pivot
constexpr int kSerialSplit = 2;    // stage 3: two lanes per staged row, one per f64 chain
constexpr int kSerialAll = 3;

// cosine-unit bounds on |approx - exact| of the bf16 scan.
//   a priori:  two bf16 roundings (unit roundoff 2^-8 each) of unit vectors, Cauchy-Schwarz:
//              2^-7 + 2^-16, + kAccSlack for f32 accumulation/normalisation  ->  kApproxErr
//   per query: e1 = min(kApproxErr, Ec + Eq + Ec*Eq + kAccSlack) with the MEASURED residual norms
//              Ec = max_rows |bf16(c/|c|) - c/|c|| (tracked while the filter copy is built) and
//              Eq = |bf16(q/|q|) - q/|q|| (prep_queries_kernel): typically 0.0045.
constexpr float kApproxErr = 0.0081f;
constexpr float kAccSlack = 2.7e-4f;

struct Cand {
    float score;   // approximate cosine
    uint32_t row;  // local row
};

// local row -> id reported to the caller.  Default (block_rows = 0): id_offset + row + 1, the
// reference's dense 1-based insertion ids (local.rs:63).  A shard of a block-cyclic sharded index
// (shard g of G, blocks of block_rows rows) owns global rows ((row / R) * G + g) * R + row % R.
struct IdMap {
    uint64_t id_offset;
    uint32_t block_rows, n_shards, shard;
    __host__ __device__ uint64_t id_of(uint32_t row) const {
        const uint64_t r = block_rows ? ((uint64_t)(row / block_rows) * n_shards + shard) * block_rows + row % block_rows
                                      : (uint64_t)row;
        return id_offset + r + 1;
    }
};

struct ScanParams {
    const float *x;          // [cap_rows, ds] f32 corpus (ds = padded dim, multiple of 128)
    const void *xh;          // bf16 filter copy in fragment order (see launch_shadow); scan16 only
    const float *scale;      // [cap_rows] 1/|c| (f32; +inf for zero rows)
    const void *qfrag;       // bf16 query fragments [8 waves][ds/16][64 lanes][8]
    const float *theta;      // [256] pass threshold per query (cosine units)
    uint64_t n_rows;         // valid rows
    uint32_t tile_begin;     // workgroup b handles tiles tile_begin + (b + i*grid)*tile_stride < tile_end
    uint32_t tile_end;
    uint32_t tile_stride;    // 1 = every tile; > 1 = the evenly spread sample
    uint32_t ds;             // floats per stored row
    uint32_t wave_mask = 0xff;  // bit w: wave w (queries 32w .. 32w+31) has a query that is wanted; the others skip their MFMAs
                                // (two query groups per wave: one bit per group of 32, 16 bits)
    // collect launch: a lane whose 16 scores of a tile contain one >= theta stores ALL 16 (one record =
    // 64 bytes + the tile index); finish_kernel picks the passing rows.  No per-row code on the stream.
    float *lane_rec;         // [512][nwg][kRecCap][16]  (thread-in-workgroup major; [1024] with two query groups per wave);
                             // scan8_kernel stores 16 int32 sums per record in place of the floats (FinishParams::rec_int)
    uint32_t *lane_tile;     // [512][nwg][kRecCap] tile index of each record
    uint32_t *lane_cnt;      // [512][nwg] records written
    float *lane_max;         // [512][nwg] sample mode: running maximum of each lane
    uint32_t *overflow;      // [256]
    // 8-bit filter copy (scan8_kernel): xh holds int8 fragments, tiles are 64 rows
    const float *tscale = nullptr;  // [cap_rows / 64][kTscaleFloats]: quantisation steps of a tile's two halves, their residual bounds, 1 / step of a centred copy
    const float *qscale = nullptr;  // [256] quantisation step of each query
    const float *qa = nullptr, *qb = nullptr;  // [256] a row's bound is qa + qb * residual (launch_prep_queries)
    // centred bf16 copy (scan16_kernel, launch_shadow): the copy holds r_c = c/|c| - a_c m for a fixed unit direction m (the
    // corpus mean direction), amean[row] = a_c; the query fragments hold r_q = q/|q| - a_q m, qmean[q] = a_q; a row's score
    // is a_q a_c + (MFMA sum over r_q r_c).  null: the copy holds c/|c| itself.
    const float *amean = nullptr;   // [cap_rows]
    const float *qmean = nullptr;   // [256]
    // removed rows (mx_index_remove): bit j of dead[t] = row 64t + j.  null: nothing removed, and the launchers run the kernels
    // without the mask; otherwise the masked variants score a removed row so low that it passes no test
    const uint64_t *dead = nullptr;  // [cap_rows / 64]
    // sample launch of the plain int8 copy: the row that gave each lane its maximum, laid out like lane_max (kNoRow: the lane saw
    // no row); theta_kernel rescores the best of them exactly.  null: not wanted
    uint32_t *lane_arg = nullptr;    // [512][nwg]
};
constexpr uint32_t kNoRow = 0xffffffffu;  // ScanParams::lane_arg of a lane without a row

// The 16 rows an MFMA lane holds of a 32-row half tile are (r & 3) + 8 (r >> 2) + 4h (h = lane >> 5): bit r of the result is
// bit (r & 3) + 8 (r >> 2) + 4h of `half`, the half tile's 32 dead-row bits
__device__ __forceinline__ uint32_t lane_dead16(uint32_t half, uint32_t h) {
    const uint32_t w = half >> (4u * h);
    return (w & 0xfu) | ((w >> 4) & 0xf0u) | ((w >> 8) & 0xf00u) | ((w >> 12) & 0xf000u);
}
// the half tile of 32-row tile t (t / 2 is its 64-row word)
__device__ __forceinline__ uint32_t dead_half(const uint64_t *dead, uint32_t t) { return (uint32_t)(dead[t >> 1] >> (32u * (t & 1u))); }

// launches ---------------------------------------------------------------------------------
hipError_t scan_setup();  // one-time function attributes (dynamic LDS size)
hipError_t scan16_setup();
// collect = false: sample launch (lane maxima only); collect = true: survivors of theta are appended
hipError_t launch_scan(hipStream_t s, int kc, bool collect, int nwg, const ScanParams &p);
hipError_t launch_scan16(hipStream_t s, int kc, bool collect, int nwg, const ScanParams &p);
// scan over the 8-bit filter copy: kc = ds / 128 in 1 .. 12, tile_begin / tile_end / tile_stride count 64-row tiles
constexpr int kTile8Rows = 64;
constexpr int kTscaleFloats = 8;  // per 64-row tile: steps of its two halves | residual bounds | 1 / step (centred copy, else 0) | 0
constexpr float kMinStep8 = 1.0f / 32768.0f;  // smallest quantisation step of a CENTRED int8 copy and of its queries (scan8.hip: |a_q a_c / (s_h s_q)| < 2^30)
constexpr int kScaleRing8 = 32;  // tiles whose scales can be in flight (15 slots ahead at one slot per tile, + the tile being multiplied)
constexpr int kScale8Entry = 512;  // per tile: [0, 16) the steps and residual bounds of its halves | [256, 512) a_c of its 64 rows (centred copy)
constexpr int kScan8LdsBytes = kRing16 * kSlot16Bytes + kScaleRing8 * kScale8Entry + 256;  // ... | 256 B that absorb the empty a_c operations
// Two-workgroup form of the plain int8 scan (256 queries, up to kMaxKC8x2 slots): 4-wave workgroups, two resident per CU,
// each wave holding two query groups, each workgroup with its own 8-slot ring (7 in flight) and a 16-tile scale ring of
// 256-byte entries (the scales' DMA operation writes 64 lanes x 4 B): 72 KiB, so two fit in the CU's 160 KiB.  The two
// workgroups of a CU meet at separate barriers -- one's tile epilogue and DMA waits can run under the other's MFMAs.
constexpr int kScan8PairWaves = 4;
constexpr int kScan8PairRing = 8;
constexpr int kScan8PairScaleRing = 16;
constexpr int kScan8PairEntry = 256;
constexpr int kScan8PairLdsBytes = kScan8PairRing * kSlot16Bytes + kScan8PairScaleRing * kScan8PairEntry;
static_assert(2 * kScan8PairLdsBytes <= 160 * 1024, "two workgroups of the pair form must fit one CU's LDS");
enum class Scan8Geom {
    k256,   // one 8-wave workgroup per CU, 256 queries (every batch size; idle waves skip their MFMAs)
    k512,   // one 8-wave workgroup per CU, two query groups per wave: 512 queries (up to kMaxKC8x2 slots)
    kPair,  // two 4-wave workgroups per CU, two query groups per wave: 256 queries (up to kMaxKC8x2 slots); nwg = 2 x CUs
};
hipError_t scan8_setup();
hipError_t launch_scan8(hipStream_t s, int kc, bool collect, int nwg, const ScanParams &p, Scan8Geom geom = Scan8Geom::k256);
// (re)build half tiles [half0, half1) (32 rows each) of the 8-bit filter copy from the padded f32 store: per half
// tile one quantisation step = max |c_i/|c|| / 127 over its rows below row_hi (rows at or above row_hi, and zero-norm
// rows, are stored as zeros) and one residual bound = 1.01 * max_rows |c/|c| - step * c8| + 1e-6; both go to
// tscale[kTscaleFloats * (h / 2) + (h & 1)] and [.. + 2] (then 1 / step of the halves of a centred copy): the 32 bytes of a 64-row scan tile;
// ec_max as launch_shadow.
// Centred form (mean != nullptr, f32 corpora up to kMaxKC slots): the quantiser sees r_c = c/|c| - a_c mean, amean[row] = a_c
// (f32; zero for the zero rows), steps and residual bounds are those of the shorter vectors, rc_max (device word, atomicMax'ed
// float bits) = max |r_c|
hipError_t launch_shadow8(hipStream_t s, const float *x, const float *scale, int ds, uint32_t half0, uint32_t half1,
                          uint64_t row_hi, void *x8, float *tscale, uint32_t *ec_max, const float *mean = nullptr,
                          float *amean = nullptr, uint32_t *rc_max = nullptr);
hipError_t scan16w_setup();
hipError_t launch_scan16w(hipStream_t s, int kc, bool collect, int nwg, const ScanParams &p);  // kc in {8, 10, 12}, <= 128 queries

// (re)build tiles [tile0, tile1) of the bf16 filter copy from the padded f32 store.  Layout: tile t
// (32 rows), k-step s (16 dims), MFMA lane l -> 8 bf16 at ((t*(ds/16) + s)*64 + l)*8, holding row
// 32t + (l&31), dims 16s + 8(l>>5) .. +7: exactly the A operand of v_mfma_f32_32x32x16_bf16.
// Values are bf16(c_i * 1/|c|); a zero-norm row is stored as zeros (it scores 0 in the scan and reaches
// finish_kernel through the index's zero-row list instead).
// ec_max: device word, atomicMax'ed with the float bits of the largest |bf16(c/|c|) - c/|c|| built.
// src_tile0: x / scale hold the rows of tiles src_tile0 .. (a staging window; 0 = the whole store).
// Only rows in [row_lo, row_hi) are (re)written: a 16-byte fragment belongs to ONE row, so rows of a
// tile that are already in the copy stay untouched.
// Centred form (mean != nullptr; f32 corpora only): with a_c = (c/|c|) . mean the copy holds bf16(c/|c| - a_c mean) and
// amean[row] = a_c; ec_max then tracks |stored - (c/|c| - a_c mean)|.  Embedding corpora sit in a cone around a common
// direction: what is left after removing it is several times shorter than the unit vector, and so is its bf16 rounding
// error -- the scan's certificate.
hipError_t launch_shadow(hipStream_t s, const float *x, const float *scale, int ds, uint32_t tile0, uint32_t tile1,
                         void *xh, uint32_t *ec_max, uint32_t src_tile0 = 0, uint64_t row_lo = 0, uint64_t row_hi = ~0ull,
                         const float *mean = nullptr, float *amean = nullptr);
// mean[ds] = normalised sum of c/|c| over rows [0, n) (zeros when the sum vanishes); msum: [ds + 1] f32 scratch, on return
// msum[ds] = |sum of c/|c||
hipError_t launch_mean_dir(hipStream_t s, const float *x, const float *scale, uint64_t n, int ds, float *msum, float *mean);
// compressed corpus -> f32 rows [n, d]
hipError_t launch_unshadow(hipStream_t s, const void *xh, int ds, int d, uint64_t row0, uint64_t n, float *out);

// rows [n, d] (device) -> x[first.., ds] zero-padded + scale (0 for a zero-norm row); flags[0] += non-finite
// rows, flags[1] += rows whose norm is outside the range the bf16 scan is certified for, flags[3] +=
// zero-norm rows, whose local row numbers (row_base + r) go to zero_rows[] (first kZeroCap); raw & 2: flags[4] += rows
// with such a norm, stored as zeros and listed in wild_rows[] (first kWildCap)
hipError_t launch_ingest(hipStream_t s, const float *src, uint64_t n, int d, float *x, float *scale,
                         uint64_t first, int ds, uint32_t *flags, int raw, uint32_t *zero_rows, uint32_t *wild_rows, uint64_t row_base);

// queries [B, d] (device) -> qfrag (normalised bf16 fragments), qpad [256, ds] f32 original
// values zero padded, qnorm2 [256] f64 (sequential DistCosine accumulation), theta init, e1 [256]
// per-query error bound of the scan (ec_max: device word holding the filter copy's largest row
// residual as float bits, or null = a-priori bound); flags[0] |= 1 when a query is not finite
hipError_t launch_prep_queries(hipStream_t s, const float *q, int B, int d, int ds, void *qfrag,
                               float *qpad, double *qnorm2, float *theta, float *e1, const uint32_t *ec_max,
                               uint32_t *overflow, uint32_t *flags, float *qa, float *qb, bool filt8 = false,
                               float *qscale = nullptr, const float *mean = nullptr, float *qmean = nullptr,
                               const uint32_t *rc_max = nullptr);
// mean / qmean: the centred copy (ScanParams::amean; bf16 or int8): fragments of q/|q| - a_q mean, qmean[q] = a_q;
// rc_max (int8 copy): device word with max |r_c| over the rows as float bits (launch_shadow8)
// qa / qb [256]: the bound of one row's filter score is qa + qb * (residual of the row's half tile); scans that know
// one residual for all rows get qa = e1, qb = 0
// filt8: fragments for the 8-bit filter copy (scan8.hip: int8 [8 waves][ds/32][64 lanes][16]) and qscale[256] = the
// query's quantisation step (0 for an unusable query); ec_max then is that copy's residual word (required)
// ds > kMaxKC16 * kChunkFloats (no scan, no filter copy: filt8 false and ec_max null, anything else is hipErrorInvalidValue): the
// call goes to launch_prep_queries_wide, which stages the query through LDS in fixed chunks and leaves qfrag alone.
hipError_t launch_prep_queries_wide(hipStream_t s, const float *q, int B, int d, int ds, float *qpad, double *qnorm2, float *theta,
                                    float *e1, uint32_t *overflow, uint32_t *flags, float *qa, float *qb);

// theta[q] = (k-th largest of query q's lane maxima) - 2*e1[q]
// raw: the lane maxima are plain scores (theta = k-th - 2 * qa); otherwise they are lower bounds of cosines already
// (scan8_kernel: theta = k-th - qa)
// ex (with a lane_arg; the plain int8 copy, raw = false): theta = max(that, L' - qa), L' = the k-th largest s2 - e2 over the rows behind
// the max(32, 2k + 12) largest lane maxima, rescored in f32 like finish_kernel's stage 2.  null, or no lane_arg: the kernel above alone
struct ThetaExact {
    const uint32_t *lane_arg;  // [lanes] like lane_max: the row of each lane maximum (ScanParams::lane_arg), kNoRow for none
    const float *x;            // [cap_rows, ds] f32 rows
    const float *scale;        // [cap_rows] 1/|c| (0: a row without a norm, which is left out)
    const float *qpad;         // [256, ds] raw queries
    const double *qnorm2;      // [256]
    uint64_t n_rows;
    int ds;
    float e2;                  // FinishParams::e2
};
hipError_t launch_theta(hipStream_t s, int B, int k, int nwg, const float *lane_max, const float *qa, bool raw, float *theta,
                        const ThetaExact *ex = nullptr);

// per query: gather the collect launch's lane buffers -> keep [kth approx - 2*e1, inf) -> f32
// rescoring (error e2) -> keep [kth - 2*e2, inf) -> exact DistCosine -> order by (dist, id) -> emit.
// overflow[q] (in: 1 = a lane buffer overflowed) out: 0 = answered, 1 = rescan with theta_retry[q],
// >= 2 = answer on the EXACT path.
struct FinishParams {
    int k, ds, nwg;
    int serial;                 // kSerial* items
    const float *x;             // [cap_rows, ds] f32 rows; null = compressed corpus (rows are read from xh)
    const void *xh;             // bf16 filter copy (fragment order)
    const float *scale;         // [cap_rows] 1/|c| (f32 rows only)
    uint64_t n_rows;
    IdMap idmap;
    const float *qpad;          // [256, ds]
    const double *qnorm2;       // [256]
    const float *e1;            // [256]
    const float *qa, *qb;       // [256] bound of a row's filter score: qa + qb * residual(row)
    const float *terr;          // the 8-bit copy's tscale array (residual of row r: [kTscaleFloats * (r / 64) + 2 + (r / 32 & 1)]); null: 0
    float e2;                   // bound on |f32 rescoring - cosine|
    const float *lane_rec;      // records of the collect launch (ScanParams)
    int rec_int;                // the records hold the int8 scan's integer sums: a score is ((float)sum * s_h) * qscale[q], s_h = terr[kTscaleFloats * (r / 64) + (r / 32 & 1)]
    const float *qscale;        // [256] the batch's query steps (ScanParams::qscale); read only with rec_int
    const uint32_t *lane_tile;
    const uint32_t *lane_cnt;
    const float *theta;         // [256] the collect launch's pass threshold
    const uint32_t *zero_rows;  // [kZeroCap] zero-norm rows of the index (their stored scores are 0: they enter here)
    uint32_t n_zero;
    const uint32_t *wild_rows;  // [kWildCap] rows with a norm outside the f32 stages' range, ascending: stage 3 takes them all
    uint32_t n_wild;
    const uint64_t *dead;       // removed rows (ScanParams::dead), or the per-call mask of a filtered search; null: none.  The
                                // side lists above may name masked rows (a filter does not prune them): every listed row's bit is tested
    uint64_t n_live;            // rows not masked: a query finds min(k, n_live)
    uint32_t *overflow;         // [256]
    const uint32_t *todo;       // null = every query; else only queries with todo[q] != 0
    float *theta_retry;         // [256]
    uint32_t *cand_cnt;         // [256] candidates rescored in f32 (statistics)
    uint64_t *ids;
    float *scores, *dists;
    int32_t *n_found;
    float *max_err;             // null unless profiling
    // completion signal: the LAST workgroup of the launch writes a 4-word summary of the batch's flag block
    // (dev_flags: [overflow 256 | cand_cnt 256 | e1 256 | qbad 256]) into host-mapped memory and then stores
    // seq behind it (system scope) -- the host polls that word instead of queueing a D2H copy (and a flag memset) and waiting in
    // hipStreamSynchronize.  host_flags == nullptr: no signal.
    uint32_t *done_ctr;         // device word, 0 between launches
    const uint32_t *dev_flags;
    uint32_t *host_flags;       // [5]: max overflow code, sum of cand_cnt, any bad query, e1[0], seq
    int n_queries;              // B
    int host_out;               // ids / scores / dists / n_found are pinned host memory (mx_index_search): system-scope fence before the tick
    uint32_t seq;
};
hipError_t finish_setup();
hipError_t launch_finish(hipStream_t s, int B, const FinishParams &p);
hipError_t launch_retry_setup(hipStream_t s, float *theta, const float *theta_retry, uint32_t *overflow, uint32_t *todo);

// range search (mx_index_search_range).  dlim[q]: row r is in range for query q iff the bits of its f32 dist
// are < dlim[q] (0: nothing is).  theta[q] = 1 - D - eps - qa[q] for the collect launch (D: the largest dist in range), zero-norm and
// padded queries stay at +inf.
hipError_t launch_range_theta(hipStream_t s, int B, const uint32_t *dlim, float eps, const float *qa, float *theta);
// finish stage of a range batch: f.k = cap; the exact count of in-range live rows per query goes to n_in_range, the best
// min(cap, count) of them to ids / scores / dists / n_found (best first, unused slots id 0, score 0, dist +inf).  overflow[q] = 2: the
// query needs the EXACT range path.  Completion signal as finish_kernel's.
struct RangeParams {
    FinishParams f;
    const uint32_t *dlim;  // [256]
    float eps;             // bound on |cos - (1 - dist)| of the f64 chain and the f32 rounding of dist, with slack
    uint64_t *n_in_range;
};
hipError_t range_setup();
hipError_t launch_range_finish(hipStream_t s, int B, const RangeParams &rp);

// EXACT path, batched: a group of up to kExactGroup queries against every row in one pass (f32 products, sequential f64
// sums per pair: DistCosine), then a 3-pass radix select per query with ties ordered by row.  Queries are named by
// their slot in qpad / qnorm2 / the output arrays; scratch holds exact_group_scratch_bytes(n_rows, k).
constexpr int kExactGroup = 32;
constexpr int kExactSlices = 256;  // row slices per query in the selection passes
struct ExactGroup {
    int n;
    int q[kExactGroup];
};
size_t exact_group_scratch_bytes(uint64_t n_rows, int k, int gcap);  // gcap: queries per pass the dist array holds (<= kExactGroup)
// dead / n_live: removed rows (ScanParams::dead, null: none) get a distance key that is never selected; min(k, n_live) found
hipError_t launch_exact_group(hipStream_t s, int k, int ds, const float *x, const void *xh, uint64_t n_rows, const IdMap &idmap,
                              const float *qpad, const double *qnorm2, const ExactGroup &grp, void *scratch, uint64_t *ids,
                              float *scores, float *dists, int32_t *n_found, const uint64_t *dead = nullptr, uint64_t n_live = ~0ull);

// compaction (compact.hip, mx_index_compact).  The destination of every live row comes from a two-level scan over the 64-row
// tiles of the dead-row mask of an index of n rows: tile_base[t] = live rows before tile t within its block of
// kCompactTilesPerBlock tiles, blk_off[b] = live rows before block b, blk_off[compact_count_blocks(tiles)] = all live rows.
constexpr int kCompactTilesPerBlock = 1024;
uint32_t compact_count_blocks(uint64_t tiles);
hipError_t launch_compact_prefix(hipStream_t s, const uint64_t *dead, uint64_t n, uint32_t *tile_base, uint32_t *blk_off);
// live rows of tiles [tile0, tile0 + tiles) -> dst rows (destination - dst0), W floats each (bitwise); src holds row 64 tile0
// onwards; scale (optional) moves along.  dst may be the source array itself when no destination reaches an unread source row.
hipError_t launch_compact_gather(hipStream_t s, const uint64_t *dead, uint64_t n, uint64_t tile0, uint64_t tiles, const uint32_t *tile_base,
                                 const uint32_t *blk_off, const float *src, const float *src_scale, int W, uint64_t dst0, float *dst,
                                 float *dst_scale);
// f32 corpus rows [0, n): the zero-norm list and the out-of-range-norm list afresh (flags[3] / flags[4] count, zeroed by the caller)
hipError_t launch_relist(hipStream_t s, const float *x, const float *scale, uint64_t n, int ds, uint32_t *flags, uint32_t *zero_rows,
                         uint32_t *wild_rows);

// filtered search (mx_index_search_filtered).  mask[t] = dead[t] | ~allow(t) for every 64-row word
// t < words (dead null: no removals), allow(t) = the rows of word t inside one of the n_ranges sorted, disjoint, non-adjacent
// local row ranges [lo, hi), passed as u64 pairs.  The result is the dead-row mask (ScanParams::dead) of the filtered search.
hipError_t launch_filter_mask(hipStream_t s, const uint64_t *dead, const uint64_t *ranges, uint32_t n_ranges, uint64_t words,
                              uint64_t *mask);
// Small filters: the m <= kSubsetCap rows of an ascending list of local rows, exact DistCosine (finish_kernel's stage-3 arithmetic)
// for B queries (qpad / qnorm2 of launch_prep_queries), the min(k, m) smallest by (dist, row) emitted like finish_kernel.  One
// workgroup per query, the keys in LDS (128 KiB).
constexpr int kSubsetCap = 16384;
hipError_t subset_setup();
hipError_t launch_subset_topk(hipStream_t s, int B, int k, int ds, const float *x, const void *xh, const uint32_t *rows, uint32_t m,
                              const IdMap &idmap, const float *qpad, const double *qnorm2, uint64_t *ids, float *scores, float *dists,
                              int32_t *n_found);

// resident filters (mx_filter): `bits` holds one allow bit per local row, [bit_words] 64-row words.
// Range edit: the rows of the n_ranges sorted, disjoint local ranges (u64 pairs) are ORed into (allow) or ANDed out of the words
// [w0, w1) of bits (w1 <= bit_words), one thread per word and no atomics.
hipError_t launch_filter_range_edit(hipStream_t s, const uint64_t *ranges, uint32_t n_ranges, uint64_t w0, uint64_t w1, bool allow,
                                    uint64_t *bits);
// Id edit: one thread per id.  Global row = id - id_offset - 1 (ids outside [id_offset + 1, id_offset + total] are skipped); a
// shard (idmap.block_rows != 0) keeps the rows of its own blocks only, as local rows.  atomicOr / atomicAnd on the 64-bit word.
hipError_t launch_filter_id_edit(hipStream_t s, const uint64_t *ids, uint64_t n_ids, uint64_t total, const IdMap &idmap, bool allow,
                                 uint64_t *bits, uint64_t bit_words);
// Apply: mask[t] = dead[t] | ~bits[t] for t < bit_words and all ones for bit_words <= t < words (dead null: no removals): the
// per-call mask of a masked pass, every word of the capacity.
hipError_t launch_filter_apply(hipStream_t s, const uint64_t *dead, const uint64_t *bits, uint64_t bit_words, uint64_t words,
                               uint64_t *mask);
// List: the rows of bits & ~dead in the words [w0, w1), ascending, into rows[0, cap) (the caller knows the count and that it fits);
// one workgroup, a block-wide prefix sum over per-thread popcounts.
hipError_t launch_filter_list(hipStream_t s, const uint64_t *dead, const uint64_t *bits, uint64_t w0, uint64_t w1, uint32_t *rows,
                              uint32_t cap);

hipError_t launch_fill_nfound(hipStream_t s, int32_t *nf, int B, int32_t v);
// EXACT range path: launch_exact_group with k = cap, the in-range count of every query of the group (dist key < dlim[q]) into
// n_in_range[q], and each list trimmed to min(cap, count)
hipError_t launch_exact_range_group(hipStream_t s, int cap, int ds, const float *x, const void *xh, uint64_t n_rows, const IdMap &idmap,
                                    const float *qpad, const double *qnorm2, const ExactGroup &grp, void *scratch, const uint32_t *dlim,
                                    uint64_t *ids, float *scores, float *dists, int32_t *n_found, uint64_t *n_in_range,
                                    const uint64_t *dead = nullptr, uint64_t n_live = ~0ull);
// sharded range search: n_in_range[b] = sum of the G per-shard counts (shard g's [B] u64 at counts + g * stride bytes), n_found[b] =
// min(cap, n_in_range[b])
hipError_t launch_range_sum(hipStream_t s, const void *counts, size_t stride, int G, int B, int cap, uint64_t *n_in_range, int32_t *n_found);
hipError_t launch_merge(hipStream_t s, const void *ids, size_t ids_stride, const void *dists, size_t dists_stride,
                        int G, int B, int k, uint64_t *out_ids, float *out_dists, float *out_scores);

// diversified search (mx_index_search_mmr)
constexpr int kMmrMaxFetch = 1024;               // candidates per query: one thread each in mmr_select_kernel
constexpr int kMmrMaxDs = 8192;                  // padded row width the selection stages in LDS (32 KiB)
constexpr size_t kMmrStageBytes = 64u << 20;     // gathered rows per chunk of queries
// stage[i, ds] = stored row rows[i] of the index (x: f32 rows, or null: the compressed corpus xh), widened to f32, i < n
hipError_t launch_mmr_gather(hipStream_t s, int ds, const float *x, const void *xh, const uint32_t *rows, uint32_t n, float *stage);
// greedy MMR selection of min(k, cand_nf[q]) of query q's candidates (lists [B, fetch] in (dist, id) order; the stored row of candidate i
// of query q is row pos[q * fetch + i] of stage) into ids / scores / dists [B, k] in selection order and n_found [B]; unused slots id 0,
// score 0, dist +inf; dists may be null.  1 <= k <= fetch <= kMmrMaxFetch, ds <= kMmrMaxDs.
hipError_t launch_mmr_select(hipStream_t s, int B, int k, int fetch, int ds, float lambda, const float *stage, const uint32_t *pos,
                             const uint64_t *cand_ids, const float *cand_scores, const float *cand_dists, const int32_t *cand_nf,
                             uint64_t *ids, float *scores, float *dists, int32_t *n_found);

// search by stored row (mx_index_search_by_id / mx_index_search_range_by_id)
constexpr uint32_t kByIdNone = 0xffffffffu;      // ByIdDrop::src of a query whose id names no live row
// q[i, dim] = the first dim values of stored row rows[i] of the index (x: f32 rows, or null: the compressed corpus xh), widened to
// f32, i < n: a query block as the search entry points take it (rows dim apart, no padding)
hipError_t launch_byid_gather(hipStream_t s, int dim, int ds, const float *x, const void *xh, const uint32_t *rows, uint32_t n, float *q);
// The internal lists [*, kk] (kk = k + exclude) of a pass whose queries are stored rows -> the caller's outputs [B, k].  Query b's lists
// are row src[b] of the internal ones (the pass orders its queries by shard and leaves out ids that name no live row: src = kByIdNone,
// blank outputs); own[b] is the id it was asked under.  With exclude, the entry whose id is own[b] is dropped if it is listed and the
// later ones move up; either way the list is cut to k.  A range pass (in_nrange != null) also corrects the count: minus one when the own
// row is listed, or when the list was cut short of the count and the own row is in range by the plain path's own test, bits(dist) <
// dlim[src] with dist = DistCosine(row, row) on the gathered row q[src].  Unused slots id 0 / score 0 / dist +inf; dists may be null.
struct ByIdDrop {
    int B, k, kk, exclude, dim;
    const uint32_t *src;
    const uint64_t *own;
    const uint64_t *in_ids;
    const float *in_scores, *in_dists;
    const int32_t *in_nfound;
    const uint64_t *in_nrange;
    const uint32_t *dlim;
    const float *q;
    uint64_t *ids;
    float *scores, *dists;
    int32_t *n_found;
    uint64_t *n_in_range;
};
hipError_t launch_byid_drop_self(hipStream_t s, const ByIdDrop &p);

// fused search (mx_index_search_fused)
constexpr int kFuseMaxSub = 16;                  // sub-queries per request
constexpr int kFuseMaxFetch = 256;               // entries per list: kFuseMaxSub * kFuseMaxFetch = 4096 entries sorted in LDS per request
// One ranked list [R, k] per request from the m candidate lists of its sub-queries: list i of request r is row r * m + i of cand_*
// [R * m, fetch] ((dist, id) order, cand_nf entries) and is consulted iff weights[r * m + i] > 0.  A row of the union is reported with
// the entry of its best list (smallest (dist, sub-query)) and that list's index; mode 0 orders by (best dist, id), mode 1 by
// (fused descending, id) with fused = the f64 sum over the consulted lists that hold the row, in ascending i, of
// (double)weight / (rrf_c + 1-based rank); fused of mode 0 is (double)score.  n_found = min(k, rows in the union); unused slots id 0 /
// score 0 / dist +inf / best_sub -1 / fused 0.  dists, best_sub and fused may be null.  1 <= m <= kFuseMaxSub, 1 <= k <= fetch <=
// kFuseMaxFetch.
struct FuseArgs {
    int R, m, fetch, k, mode;
    double rrf_c;
    const float *weights;
    const uint64_t *cand_ids;
    const float *cand_scores, *cand_dists;
    const int32_t *cand_nf;
    uint64_t *ids;
    float *scores, *dists;
    int32_t *best_sub;
    double *fused;
    int32_t *n_found;
};
hipError_t launch_fuse(hipStream_t s, const FuseArgs &p);

// search by examples (mx_index_search_like)
constexpr int kLikeMaxExamples = 16;             // example slots per request: the used ones fit one 32-bit mask
constexpr uint32_t kLikeNone = 0xffffffffu;      // LikeCombine::src of a slot that is absent (weight 0) or names no live row
// One f32 query per request from its terms: the caller vector q[r] (q null: none) under weight wq[r], then example slot i = 0 .. m - 1,
// gathered row src[r * m + i] of `rows` (launch_byid_gather's block) under weight w[r * m + i].  A term is USED when its weight is not 0,
// it has a vector (q given / src != kLikeNone) and na != 0 (stored rows: na > 0; a NaN of a non-finite caller vector counts as used), na = the
// f64 sum in element order of fl32(v_j * v_j).  Per column, from +0.0
// and in that order over the used terms:  c_j += (double)weight * ((double)v_j / sqrt(na))  (IEEE f64, round to nearest, a true square
// root and division, nothing contracted); out[r, j] = (float)c_j, also written to combined[r, j] when given.  used[r]: bit i set when
// example i is used; n_used[r] (may be null) their count.  A request without a used term gets zeros.  1 <= m <= kLikeMaxExamples.
struct LikeCombine {
    int R, m, dim;
    const float *rows;
    const uint32_t *src;
    const float *w;
    const float *q;
    const float *wq;
    float *out;
    float *combined;
    uint32_t *used;
    int32_t *n_used;
};
hipError_t launch_like_combine(hipStream_t s, const LikeCombine &p);
// The internal lists [R, kk] of the pass over LikeCombine::out -> the caller's outputs [R, k], k <= kk.  With exclude, every entry whose
// id is own[r * m + i] for a set bit i of used[r] is dropped and the later ones move up, in order; either way the list is cut to k.  A
// request whose query q[r] is all zeros (no used term, or terms that cancel) is BLANK: n_found 0.  Unused slots id 0 / score 0 / dist
// +inf; dists may be null.  Reads the internal lists, writes the caller's: never in place.
struct LikeDrop {
    int R, m, k, kk, exclude, dim;
    const uint64_t *own;
    const uint32_t *used;
    const float *q;
    const uint64_t *in_ids;
    const float *in_scores, *in_dists;
    const int32_t *in_nfound;
    uint64_t *ids;
    float *scores, *dists;
    int32_t *n_found;
};
hipError_t launch_like_drop_examples(hipStream_t s, const LikeDrop &p);

// scoring of named rows (mx_index_score_ids; score_kernels.hip)
constexpr int kScoreMaxIds = 4096;               // entries per query: their ranking keys (dist bits, id, position) fit 48 KiB of LDS
constexpr int kScoreThreads = 1024;              // one workgroup per query; thread t owns entries t, t + 1024, ...
constexpr uint32_t kScoreNotMine = 0xffffffffu;  // ScoreIds::part of an entry whose id names no row of the shard (no dist has these bits:
constexpr uint32_t kScoreBlank = 0xfffffffeu;    // a NaN dist is blank) | ... of a row of the shard that is removed or has a NaN dist
// Exact DistCosine (exact_dist_stored: the f64 chain of finish_kernel's stage 3 and of the EXACT path) of query b (qpad / qnorm2 of
// launch_prep_queries) against the rows its m ids cand[b, 0 .. m) name, B queries.  An id names global row id - id_offset - 1 of the
// `total` rows of the handle; a shard (idmap.block_rows != 0) holds the rows of its own blocks, as local rows below n_rows.  An entry
// is FOUND when its id names a row of this index whose bit in `dead` (null: no removals) is clear and whose dist is not NaN.
// Plain form (part null): scores / dists [B, m] in the caller's order, score 0 and dist +inf where the entry is not found; n_found[b] =
// the found entries; order[b, r] for r < n_found[b] = the position j of the r-th smallest found entry by (dist bits, id, j), -1 behind
// them.  dists, order, n_found may be null.  Shard form (part given): the dist bits alone into part[b, j], kScoreNotMine / kScoreBlank
// otherwise; scores, dists, order, n_found are not touched.  1 <= m <= kScoreMaxIds, ds <= kMmrMaxDs.
struct ScoreIds {
    int B, m, ds;
    const float *x;            // [cap_rows, ds] f32 rows; null = compressed corpus (rows are read from xh)
    const void *xh;
    const uint64_t *dead;
    uint64_t n_rows, total;
    IdMap idmap;
    const float *qpad;
    const double *qnorm2;
    const uint64_t *cand;
    uint32_t *part;
    float *scores, *dists;
    int32_t *order, *n_found;
};
hipError_t launch_score_ids(hipStream_t s, const ScoreIds &p);
// The G shard blocks of a sharded handle (block g: parts + g * stride words, [B, m] each) -> the outputs of the plain form: entry (b, j)
// is the one value that is not kScoreNotMine (none: blank), cand[b, j] its id for the ranking.
struct ScoreMerge {
    int B, m, G;
    const uint32_t *parts;
    size_t stride;
    const uint64_t *cand;
    float *scores, *dists;
    int32_t *order, *n_found;
};
hipError_t launch_score_merge(hipStream_t s, const ScoreMerge &p);

// grouped search (mx_grouping / mx_index_search_grouped; group_kernels.hip)
constexpr int kGroupThreads = 1024;              // one workgroup per query
constexpr int kGroupMaxFetch = 4096;             // entries per list (the ABI's cap on k): kGroupMaxFetch / kGroupThreads per thread
constexpr int kGroupCountBlocks = 256;           // workgroups of the count; each writes its two partial sums
// The keys of a grouping: one u32 per GLOBAL row (id - id_offset - 1) of the handle, keys[0, len).  Every edit is a plain store of a
// value the host has made unambiguous (disjoint ranges; no id with two keys): no atomics, nothing depends on thread order.
// Range edit: one thread per row of [row0, row1); ranges holds n_ranges pairs [lo, hi) of rows sorted by lo and pairwise disjoint,
// rkeys the key of each; a row some range covers gets that range's key.  row1 <= len.
hipError_t launch_grouping_range_edit(hipStream_t s, const uint64_t *ranges, const uint32_t *rkeys, uint32_t n_ranges, uint64_t row0,
                                      uint64_t row1, uint32_t *keys);
// Id edit: one thread per id; ids outside [id_offset + 1, id_offset + limit] are skipped (limit <= len).
hipError_t launch_grouping_id_edit(hipStream_t s, const uint64_t *ids, const uint32_t *ikeys, uint64_t n_ids, uint64_t id_offset,
                                   uint64_t limit, uint32_t *keys);
// Get: out[i] = the key of the row ids[i] names, 0 for an id outside [id_offset + 1, id_offset + limit] (limit <= len).
hipError_t launch_grouping_get(hipStream_t s, const uint64_t *ids, uint64_t n_ids, uint64_t id_offset, uint64_t limit, const uint32_t *keys,
                               uint32_t *out);
// Count: part[2 w] = rows r < n of workgroup w's share with keys[r] != 0, part[2 w + 1] = those of them whose bit in `dead` (one bit per
// global row, null: no removals) is clear; kGroupCountBlocks workgroups, the host adds the partial sums.
hipError_t launch_grouping_count(hipStream_t s, const uint32_t *keys, uint64_t n, const uint64_t *dead, uint64_t *part);
// One list [B, k] of group heads per query from its candidate list (row b of cand_* [B, fetch], (dist, id) order, cand_nf entries).  The
// key of an entry is keys[id - id_offset - 1], 0 when that row is not below len.  Entry i is a HEAD when its key is 0 or no entry
// before it has its key; the first k heads are written in list order with the entry's id, score and dist unchanged, the key, and
// group_rows = the entries of the list with that key (1 for key 0).  n_found = min(k, heads); the slots behind them hold id 0, score
// 0, dist +inf, key 0, group_rows 0; complete = n_found == k or the list holds fewer than fetch entries.  dists, out_keys, group_rows
// and complete may be null.  1 <= k <= fetch <= kGroupMaxFetch.
struct GroupHeads {
    int B, k, fetch;
    uint64_t id_offset, len;
    const uint32_t *keys;
    const uint64_t *cand_ids;
    const float *cand_scores, *cand_dists;
    const int32_t *cand_nf;
    uint64_t *ids;
    float *scores, *dists;
    uint32_t *out_keys;
    int32_t *group_rows, *n_found;
    uint8_t *complete;
};
hipError_t launch_group_heads(hipStream_t s, const GroupHeads &p);

// grouped search with members (mx_index_search_group_rows / mx_index_search_capped / mx_grouping_key_counts, DESIGN.md section 3.19;
// group_rows_kernels.hip).  Lists, keys and heads as for GroupHeads.
constexpr int kGroupMaxMembers = 16;             // n: rows reported per group; k * n <= kGroupMaxFetch
constexpr uint64_t kGroupMaxCountKeys = 1ull << 20;
// per_key == 0, the GROUP-ROWS form: the first k heads in list order, each with the first n entries of the list under its key (a key-0
// head: itself alone) in list order: ids, scores, dists [B, k, n], unused slots id 0 / score 0 / dist +inf; per head [B, k] the key,
// group_rows = the entries of the list under the key (1 for key 0), n_members = min(n, group_rows), members_complete = n_members == n
// or the list holds fewer than fetch entries or the key is 0; all four 0 behind the heads found.  1 <= n <= kGroupMaxMembers.
// per_key >= 1, the CAPPED form (n = 1): an entry is accepted when its key is 0 or fewer than per_key entries before it have its key;
// the first k accepted entries unchanged with their key, [B, k]; group_rows, n_members and members_complete are not written.
// Both: n_found = min(k, heads or accepted entries); complete = n_found == k or the list holds fewer than fetch entries.  dists,
// out_keys, group_rows, n_members, members_complete and complete may be null.  1 <= k <= fetch <= kGroupMaxFetch.
struct GroupRows {
    int B, k, n, per_key, fetch;
    uint64_t id_offset, len;
    const uint32_t *keys;
    const uint64_t *cand_ids;
    const float *cand_scores, *cand_dists;
    const int32_t *cand_nf;
    uint64_t *ids;
    float *scores, *dists;
    uint32_t *out_keys;
    int32_t *group_rows, *n_members;
    uint8_t *members_complete;
    int32_t *n_found;
    uint8_t *complete;
};
hipError_t launch_group_rows(hipStream_t s, const GroupRows &p);
// Key counts: counts[2 i] += the rows r < rows whose key (keys[r], 0 at or past len) is sorted[i], counts[2 i + 1] += those of them
// whose bit in `dead` (one bit per global row, null: no removals) is clear.  sorted: n_sorted distinct keys, ascending; the caller
// zeroes counts [2 * n_sorted] first.  One thread per row, a binary search, global integer adds.
hipError_t launch_grouping_key_counts(hipStream_t s, const uint32_t *keys, uint64_t len, uint64_t rows, const uint64_t *dead,
                                      const uint32_t *sorted, uint32_t n_sorted, uint64_t *counts);

// boosted search (mx_prior / mx_index_search_boosted; boost_kernels.hip)
constexpr int kBoostThreads = 1024;              // one workgroup per query
constexpr int kBoostMaxFetch = 4096;             // entries per list (the ABI's cap on k): kBoostMaxFetch / kBoostThreads per thread
constexpr int kBoostMaxBlocks = 256;             // workgroups of the maximum; each writes its partial maximum
// The values of a prior: one f32 per GLOBAL row (id - id_offset - 1) of the handle, vals[0, len).  They are edited and read back by
// the grouping's edit and get kernels, as their 32 bits.
// Maximum: part[w] = the largest of 0 and vals[r] over the rows r < n of workgroup w's share whose bit in `dead` (one bit per global
// row, null: no removals) is clear; kBoostMaxBlocks workgroups, the host folds the partial maxima.
hipError_t launch_prior_max(hipStream_t s, const float *vals, uint64_t n, const uint64_t *dead, float *part);
// One re-ranked list [B, k] per query from its candidate list (row b of cand_* [B, fetch], (dist, id) order, cand_nf = m entries).
// Entry j has prior vals[id - id_offset - 1] (0 when that row is not below len) and c_j = (double)score_j + (double)w * (double)prior_j
// with w = weights[b] (device memory; null: 1).  The entries are ranked by (c descending, j ascending) and the first min(k, m) written
// in that order: id, score and dist unchanged, the prior, and c.  n_found = min(k, m); the slots behind hold id 0, score 0, dist +inf,
// prior 0, combined 0.  complete = m < fetch, or the k-th reported c > (double)score_{m-1} + (double)w * (double)hi.  dists, priors,
// combined and complete may be null.  1 <= k <= fetch <= kBoostMaxFetch.
struct BoostRank {
    int B, k, fetch;
    uint64_t id_offset, len;
    const float *vals;
    const float *weights;
    float hi;
    const uint64_t *cand_ids;
    const float *cand_scores, *cand_dists;
    const int32_t *cand_nf;
    uint64_t *ids;
    float *scores, *dists, *priors;
    double *combined;
    int32_t *n_found;
    uint8_t *complete;
};
hipError_t launch_boost_rank(hipStream_t s, const BoostRank &p);

// filters from row attributes (mx_filter_set_where / set_keys / combine / invert; where_kernels.hip)
constexpr int kWhereThreads = 256;               // four waves; each wave and step owns one 64-row word of the selection
constexpr int kWhereMaxBlocks = 2048;            // workgroups of a predicate kernel: they stride over the rows
constexpr int kFilterAnd = 0, kFilterOr = 1, kFilterAndNot = 2, kFilterXor = 3;  // MX_FILTER_AND ... of the C ABI
// Range predicate: sel[w], w < (rows + 63) / 64, bit r & 63 of word r >> 6 = lo <= v_r && v_r <= hi (IEEE f32) for the GLOBAL row
// r < rows, v_r = vals[r] below len and 0 from there on.  Bits at or past `rows` are 0.  sel holds (rows + 63) / 64 words.
hipError_t launch_where_range(hipStream_t s, const float *vals, uint64_t len, uint64_t rows, float lo, float hi, uint64_t *sel);
// Key predicate: the same with "the key of row r (keys[r] below len, 0 from there on) is in sorted[0, n_sorted)", a device array in
// ascending order without repeats, n_sorted >= 1.
hipError_t launch_where_keys(hipStream_t s, const uint32_t *keys, uint64_t len, uint64_t rows, const uint32_t *sorted, uint32_t n_sorted,
                             uint64_t *sel);
// dst[w] = a[w] OP b[w] for w < words, OP one of kFilterAnd ... kFilterXor (kFilterAndNot: a & ~b); b null: b is the pattern that has
// one bit for every row below `size`.  One thread per word, no atomics; dst may be a or b, a may be b.
hipError_t launch_filter_words(hipStream_t s, uint64_t *dst, const uint64_t *a, const uint64_t *b, uint64_t words, int op, uint64_t size);

}  // namespace mx
