// index.hip -- host logic of the GPU-resident flat cosine index behind the C ABI
// (include/memex_hip.h).  Drop-in for memex's HnswStore (reference
// lib/libmemex/src/storage/local.rs:21-166) reached through the VectorStore trait
// (lib/libmemex/src/storage/mod.rs:55-66).
//
// Search pipeline per batch of <= 512 queries (one scan pass serves 256 of them -- 512 on the int8 copy up to 512
// dims, 128 on scan16w; kernels: scan8.hip / scan16.hip / scan16w.hip / scan.hip,
// index_kernels.hip):
//   prep      normalise queries -> MFMA fragments (int8 with the query's own step, or bf16); f64 query norms
//             (DistCosine order); the bound of a row's filter score, qa + qb * (residual of the row's half
//             tile), from measured residuals (one residual for all rows with the bf16 / f32 scans: qb = 0)
//   sample    scan an evenly spread 1/4 .. 1/64 of the tiles keeping only each lane's best lower bound
//   theta     k-th largest of those - qa = pass threshold (certified: keeps the exact top-k)
//   collect   scan every tile; a lane with a passing row stores its 16 scores as one record
//   finish    gather -> k-th best lower bound, keep the rows whose upper bound reaches it -> f32 rescoring
//             (error e2 ~ 5e-5) -> keep [kth - 2*e2, inf) -> exact f64 DistCosine -> order by (dist, id)
// Five launches; corpora of <= 2 tiles per workgroup skip sample/theta (theta = -inf).
// What the scan streams: an int8 or a bf16 filter copy kept next to the f32 rows (the library chooses by row
// width and demotes int8 to bf16 on a corpus too dense for its certificate), or the f32 rows themselves.
// A query whose lane buffers overflowed (dense neighbourhoods, weak sample threshold) is rescanned
// ONCE with the tight threshold finish derived from what it did collect (all such queries of the
// batch share that one extra pass); only if that overflows too -- more than ~16k rows within the bound of
// the k-th neighbour -- is it answered on the EXACT path (f64 on every row).
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <chrono>
#include <ctime>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "index_kernels.h"
#include "mx_common.h"
#include "mx_debug.h"
#include "mx_filter_bits.h"
#include "mx_owned.h"
#include "shard_pool.h"

namespace mx {

std::string &last_error_slot() {
    static thread_local std::string slot;
    return slot;
}

namespace {

// per-query words of a batch in HBM: [overflow 256 | cand_cnt 256 | e1 256 | qbad 256].  finish_kernel sends
// the host a 4-word summary + its sequence number (host_sum); the block itself is only copied when the
// summary reports an overflow, and on the EXACT path
constexpr int kFlagWords = 4 * kMaxBatch;
// Filter copy an f32 corpus keeps unless told otherwise: int8 up to 1024 dims, bf16 above.  The int8 certificate is
// ~0.016-0.026 wide whatever the width (quantisation noise of a unit vector does not depend on its length) while the
// spread of cosines shrinks like 1/sqrt(dim), so the int8 pass hands more rows to finish_kernel the wider the rows are.
// Measured on Gaussian rows, B = 256, k = 10, one box (scripts/r3_dims.sh; int8 at its best sample size / bf16, kQPS):
// 463 / 312 at 128 dims, 290 / 188 at 256, 188 / 117 at 384, 160 / 100 at 512, 102 / 70 at 768, 146 / 90 at 1024
// (4M rows), 51 / 61 at 1536 (4M rows).
constexpr int kAutoI8MaxDim = 1024;  // filter copy of an f32 corpus: int8 (scan8.hip) or bf16 (scan16.hip)
constexpr int kSumWords = 5;  // max overflow code, candidates, any bad query, e1 of query 0, seq

struct Scratch {
    Dev<void> qfrag;
    Dev<float> qpad;
    Dev<double> qnorm2;
    Dev<float> theta, theta_retry;
    Dev<uint32_t> todo;
    Dev<uint32_t> dev_flags;   // [kFlagWords]
    Pin<uint32_t> host_flags;  // pinned mirror of dev_flags [kFlagWords] (D2H copy, rare)
    Pin<uint32_t> host_sum;    // pinned, device-visible [kSumWords]: written by finish_kernel's last workgroup
    bool out_on_host = false;        // this batch's output pointers are mapped host memory (run_combined)
    Dev<uint32_t> done_ctr;    // finish_kernel's workgroup counter
    uint32_t flag_seq = 0;           // sequence number of the last finish launch
    uint32_t *overflow = nullptr, *cand_cnt = nullptr, *qflags = nullptr;  // views into dev_flags
    float *e1 = nullptr;
    float *lane_rec = nullptr;       // records of the collect launch (ScanParams); leased (LaneLease), like the four below
    uint32_t *lane_tile = nullptr;
    uint32_t *lane_cnt = nullptr;
    float *lane_max = nullptr;
    uint32_t *lane_arg = nullptr;    // the row behind each lane maximum (sample launch of the plain int8 copy)
    Dev<float> qstage;       // [256, dim] host->device query staging
    Dev<float> qscale;       // [256] quantisation step of each query (8-bit filter copy)
    Dev<float> qa, qb;       // [256] a row's filter-score bound is qa + qb * residual (launch_prep_queries)
    Dev<float> qmean;        // [256] a_q of the centred bf16 copy
    Dev<uint64_t> out_ids;   // [256, kcap] device outputs for the host API
    Dev<float> out_scores;
    Dev<float> out_dists;
    Dev<int32_t> out_nfound;
    int kcap = 0;
    Dev<void> exact_scratch;  // EXACT path: distances of a query group, selection state (exact_group_scratch_bytes)
    size_t exact_bytes = 0;
    Dev<float> max_err;
    // pinned staging of the host API: queries in, results out (one H2D / D2H per combined batch)
    Pin<float> h_q;
    Pin<uint64_t> h_ids;
    Pin<float> h_scores, h_dists;
    Pin<int32_t> h_nf;
    // range search (range_batch): per-query dist bound, device and pinned counts
    Dev<uint32_t> rlim;        // [kMaxBatch] dlim of the batch (launch_range_theta)
    Dev<uint64_t> out_nrange;  // [kMaxBatch] device n_in_range of a combined sharded pass
    Pin<uint64_t> h_nr;        // [kMaxBatch] pinned, mapped: n_in_range of a combined pass
    bool ready = false;
};

// The lane buffers of the scan (records of the collect launch: 64 per lane x 68 B, 0.57 GB per set at 256 workgroups x 512
// lanes; twice that for a 512-query pass of the int8 scan, which numbers 1024 lanes per workgroup, and for its two-workgroup
// form, 512 workgroups x 512 lanes) are
// only live inside one search_batch call, which returns host-synchronised.  They are therefore leased from a pool per
// device instead of owned by every index: a process with many resident collections holds as many sets as it has
// searches in flight on a device at the same time, not one per collection.  The pool is freed when the last index
// on the device closes.
struct LaneBufs {
    float *rec = nullptr;
    uint32_t *tile = nullptr, *cnt = nullptr;
    float *max = nullptr;
    uint32_t *arg = nullptr;  // ScanParams::lane_arg, sized like max
    int nwg = 0;
    int groups = 1;  // query groups per wave the set is sized for (2: a 512-query pass, or the int8 scan's two-workgroup form:
                     // twice the workgroups with half the waves, the same 1024 lanes per CU)
};
constexpr int kMaxDevices = 64;
struct LanePool {
    std::mutex mu;
    std::vector<LaneBufs> idle;
    int open_indexes = 0;
};
LanePool g_lanes[kMaxDevices];

void lane_free(LaneBufs &b) {
    if (b.rec) (void)hipFree(b.rec);
    if (b.tile) (void)hipFree(b.tile);
    if (b.cnt) (void)hipFree(b.cnt);
    if (b.max) (void)hipFree(b.max);
    if (b.arg) (void)hipFree(b.arg);
    b = LaneBufs{};
}

// RCCL entry points, resolved with dlopen the first time a sharded index spans more than one device
// (libmemex_hip.so itself links only the HIP runtime; a single-GPU host never loads RCCL)
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
};

}  // namespace
}  // namespace mx

using namespace mx;

struct mx_filter;

// one host-API search call waiting to be served (see mx_index_search)
struct SearchReq {
    const float *q;
    int B, k;
    uint64_t *ids;
    float *scores, *dists;
    int32_t *n_found;
    const std::vector<std::pair<uint64_t, uint64_t>> *filt = nullptr;  // mx_index_search_filtered: the normalised id ranges
    mx_filter *res = nullptr;           // mx_index_search_with_filter: the resident filter (never together with filt)
    const uint32_t *dlim = nullptr;     // mx_index_search_range: per-query dist bounds (k is the cap); null: a top-k request
    uint64_t *n_in_range = nullptr;
    int rc = MX_OK;
    std::string err;
    bool done = false;
};

struct mx_index {
    std::string key;
    int dim = 0, ds = 0, kc = 0, device = 0;
    int refs = 1;
    std::mutex mu;
    // request combining (mx_index_search): callers queue here; one of them, the leader, serves batches
    std::mutex cmu;
    std::condition_variable ccv;
    std::deque<SearchReq *> pending;
    bool leader = false;
    hipStream_t stream = nullptr;
    Dev<float> x;
    Dev<float> scale;
    Dev<void> xh;          // bf16 filter copy (fragment order), cap/32 tiles; null = not kept
    bool want_filter = true;     // keep a filter copy when HBM allows (mx_index_set_filter_copy)
    // 8-bit filter copy (scan8.hip): xh holds int8 fragments in 64-row tiles, tsc one quantisation step per 32-row
    // half tile.  An f32 corpus only; the compressed corpus keeps its bf16 rows.
    bool filter_i8 = false;
    bool filter_auto = true;     // the library picks the kind (by row width) and may demote int8 to bf16 when a batch overflows
    bool pooled = false;         // counted in its device's lane-buffer pool (open_plain)
    uint32_t i8_batches = 0, i8_retry_batches = 0;  // since the int8 copy was built: batches served, batches that needed the retry pass
    uint64_t plain_bf16_rows = 0;  // rows the index held when its bf16 copy was last built WITHOUT centring (0: no such copy): a collection
                                   // that started small, or off a cone, is looked at again once it has doubled (add_device_locked)
    uint64_t demoted_at_rows = 0;  // rows the index held when an automatic int8 copy was demoted to bf16 (0: never); the
                                   // int8 copy gets another try once the collection has doubled (add_device_locked)
    Dev<float> tsc;
    // centred bf16 copy (f32 corpus, up to kMaxKC slots; launch_shadow): `amean` lives with every such copy, `centred` says
    // whether it was built around `mean` (a full rebuild of a populated index: a demotion, mx_index_set_filter_copy)
    Dev<float> amean;      // [cap] a_c = (c/|c|) . mean
    Dev<float> mean;       // [ds] unit direction; msum: [ds] scratch of its computation
    Dev<float> msum;
    bool centred = false;
    // compressed corpus (mx_index_set_corpus_mode): xh is the ONLY copy of the rows; x / scale are not
    // allocated, appends pass through the small f32 staging window xs / ss
    bool compressed = false;
    bool raw_ingest = false;     // rows being appended are stored values coming back from disk: no renormalisation
    Dev<float> xs, ss;
    uint64_t xs_rows = 0;
    uint64_t n = 0, cap = 0;
    IdMap idmap{0, 0, 1, 0};
    Dev<uint32_t> flags;  // device: [0] non-finite rows, [1] out-of-range-norm rows (last add), [2] ec_max (float bits), [3] zero-norm rows, [4] listed out-of-range-norm rows,
                                // [5] rc_max (float bits): max |r_c| of a centred int8 copy
    uint64_t wild_rows = 0;         // rows with a norm outside [1e-15, 1e15] (a compressed corpus answers on the EXACT path then)
    Dev<uint32_t> zero_rows;  // device: [kZeroCap] local rows with zero norm, ascending (finish_kernel adds them to every query)
    uint64_t n_zero = 0;            // zero-norm rows in the index; more than kZeroCap -> EXACT path
    Dev<uint32_t> wild_list;  // device: [kWildCap] local rows with a norm outside [1e-15, 1e15] (f32 corpus), ascending
    uint64_t n_wild = 0;            // ... how many; more than kWildCap -> EXACT path
    int mode = MX_SEARCH_AUTO;
    bool profiling = false;
    int n_cu = 0, nwg = 0;       // nwg: workgroups of the one-per-CU scans (min(CUs, kMaxScanCUs))
    bool scan8_pair = true;      // plain int8 copy, 129-256 queries: the two-workgroup form (Scan8Geom::kPair, 2 x nwg workgroups)
    bool exact_theta = true;     // plain int8 copy: the collect threshold also from exact scores of the sample's best rows (launch_theta's
                                 // ThetaExact), and the smaller sample that threshold allows; MEMEX_HIP_EXACT_THETA=0: neither
    int sample_div = 0;          // MEMEX_HIP_DEBUG=sample_div=N as it stood when the index was created (0: the built-in sample sizes)
    int serial = kSerialAll;     // MEMEX_HIP_DEBUG=serial=N likewise: the kSerial* items of finish_kernel (0: the older forms)
    uint64_t crowded_at_rows = 0;  // rows the index held when a crowded f32 stage last had its plain int8 copy rebuilt (search_batch); 0: never
    bool print_records = false;  // MEMEX_HIP_DEBUG=records=1 (at creation): every batch prints the records of its first collect launch to stderr
    Scratch s;
    mx_index_stats stats{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_wait = nullptr;
    double wait_ema_us[4] = {0.0, 0.0, 0.0, 0.0};  // how long recent batches of <= 32 / 128 / 256 / more queries took from the
                                                   // finish launch to completion (sleeping wait)
    // removed rows (mx_index_remove): tombstones, ids stay.  A plain index (or shard) keeps one dead-row word per 64-row scan tile
    // on the device ([cap / 64], allocated at the first removal, grown with the capacity) and its host copy; the scans and
    // finish_kernel see the device mask only while n_dead > 0, so an index without removals runs the kernels it always ran
    Dev<uint64_t> dead;
    std::vector<uint64_t> dead_h;
    uint64_t n_dead = 0;            // rows removed (a composite: over its shards)
    std::vector<uint64_t> dead_log;  // the handle's removals in the order made, global rows without id offset (vectors.mxdead)
    uint64_t disk_dead = 0;          // ... how many of them vectors.mxdead in disk_dir holds
    // compaction (mx_index_compact): how many times the rows were renumbered -- the generation the store files carry (0: never,
    // and the 01 formats).  `failed`: a compaction met a device error after rows had moved; every call fails until clear / load
    uint64_t gen = 0;
    bool failed = false;
    // filtered search (mx_index_search_filtered): the per-call mask -- dead words | rows outside the filter, [cap / 64]
    // words, reallocated when the capacity grows past it and rewritten by filter_mask_kernel before every masked pass -- the
    // device copy of the local ranges it is built from, and the row list of the subset kernel ([kSubsetCap])
    Dev<uint64_t> filt;
    size_t filt_words = 0;
    Dev<uint64_t> filt_ranges;
    size_t filt_ranges_cap = 0;     // pairs
    Dev<uint32_t> subset_rows;
    bool last_subset = false;       // the last search_batch answered on the subset kernel
    // resident filters (mx_filter).  row_epoch (the handle's): how many times the rows were renumbered or replaced
    // (clear, load, a compaction that dropped rows) -- a filter made before the last one is stale.  dead_ver (every plain index or
    // shard): moves whenever its removal mask changes, so a filter knows when its cached live count and row list are out of date.
    uint64_t row_epoch = 0;
    uint64_t dead_ver = 0;
    // diversified search (mx_index_search_mmr), allocated at the first such call.  Every plain index or shard: the
    // row list of a gather launch and -- the handle's own index, or a shard on another device than shards[0] -- the block the
    // gathered rows go to (at most kMmrStageBytes).  The index that owns the stream (shards[0] of a composite) also holds the
    // candidate stage's lists [kMaxBatch, mmr_fcap], their pinned mirrors and the candidates' positions in the block.
    Dev<uint32_t> mmr_rows;
    Dev<float> mmr_stage;
    size_t mmr_stage_bytes = 0;
    Dev<uint64_t> mmr_ids; Pin<uint64_t> mmr_h_ids;
    Dev<float> mmr_scores, mmr_dists;
    Dev<int32_t> mmr_nf; Pin<int32_t> mmr_h_nf;
    Dev<uint32_t> mmr_pos;
    int mmr_fcap = 0;
    // search by stored row (mx_index_search_by_id), allocated at the first such call.  Every plain index or shard: the
    // row list of a gather launch [kMaxBatch] and -- a shard on another device than shards[0] -- the block its rows go to before the
    // peer copy [kMaxBatch, dim].  The index that owns the stream also holds the query block [kMaxBatch, dim], the pass's own lists
    // [kMaxBatch, byid_cap] with their counts, and per query its place in them, its id and its dist bound.
    Dev<uint32_t> byid_rows;
    Dev<float> byid_stage;
    Dev<float> byid_q;
    Dev<uint64_t> byid_ids, byid_nr, byid_own;
    Dev<float> byid_scores, byid_dists;
    Dev<int32_t> byid_nf;
    Dev<uint32_t> byid_src, byid_dlim;
    int byid_cap = 0;
    // fused search (mx_index_search_fused), allocated at the first such call on the index that owns the stream: a
    // chunk's weights [kMaxBatch] and, for the host-pointer variant, best_sub and fused [kMaxBatch, kFuseMaxFetch].  The candidate
    // lists are the diversified search's (mmr_ids ...).
    Dev<float> fuse_w;
    Dev<int32_t> fuse_best;
    Dev<double> fuse_val;
    // search by examples (mx_index_search_like), allocated at the first such call on the index that owns the stream:
    // the gathered example rows and the combined queries [kMaxBatch, dim] each, the pass's own lists [kMaxBatch, like_cap] with their
    // counts, and per pass the example ids, weights and places in the gathered block [kMaxBatch], the caller weights, the used-example
    // masks and their counts [kMaxBatch].  A shard's row list and peer-copy block are the by-id search's (byid_rows, byid_stage).
    Dev<float> like_rows, like_q;
    Dev<uint64_t> like_ids, like_own;
    Dev<float> like_scores, like_dists, like_w, like_wq;
    Dev<int32_t> like_nf, like_nused;
    Dev<uint32_t> like_src, like_used;
    int like_cap = 0;
    // scoring of named rows (mx_index_score_ids), allocated at the first such call and sized by kMaxBatch x score_cap.
    // Every plain index or shard: the id block of a batch.  The index that owns the stream: the outputs of the host-pointer variant.
    // A shard: its dist block when it lives on another device than shards[0], which holds the gather area of G such blocks.
    Dev<uint64_t> score_cand;
    Dev<float> score_scores, score_dists;
    Dev<int32_t> score_order, score_nf;
    Dev<uint32_t> score_part, score_gather;
    int score_cap = 0, score_out_cap = 0, score_part_cap = 0, score_gather_cap = 0;
    // persistence bookkeeping: what vectors.mxflat in `disk_dir` holds, as far as this handle knows
    std::string disk_dir;
    uint64_t disk_rows = 0;
    off_t disk_size = 0;
    struct timespec disk_mtime {};
    // ---- composite (mx_index_open_sharded): rows are dealt to `shards` in blocks of block_rows
    std::vector<mx_index *> shards;
    uint64_t block_rows = 0;
    uint64_t total = 0;
    bool use_rccl = false;
    std::vector<void *> comms;       // ncclComm_t per shard (RCCL exchange)
    std::vector<Dev<void>> sh_block;    // per shard, on its device: packed result block [ids | dists]
    std::vector<Dev<void>> sh_gather;   // per shard, on its device: [G] packed blocks (RCCL recv); [0] is the merge input
    std::vector<Dev<float>> sh_q, sh_scores;
    std::vector<Dev<int32_t>> sh_nf;
    int sh_kcap = 0;
    std::unique_ptr<ShardPool> pool;  // helper threads for shards 1 .. G-1 (shards on distinct devices only)
    bool composite() const { return !shards.empty(); }
    ~mx_index();  // with `device` current (free_index, open_plain); the buffers go as members, after the stream is idle
};

// A resident filter: one allow bit per row, kept on every plain index or shard of the handle it was made for,
// with a host mirror of the bits (kept the way dead_h is: counts, spans and the export come from it).  Every call that reads or
// edits a filter holds the handle's mutex.
struct FilterShard {
    int device = 0;                  // where the shard's rows live
    Dev<uint64_t> bits;        // device: [words], bit r & 63 of word r >> 6 = local row r is in the set
    size_t words = 0;                // grows to the index's capacity words at the next edit; rows past it are not in the set
    std::vector<uint64_t> bits_h;    // host mirror [words]
    Dev<uint64_t> stage;       // device: the ranges or ids of the edit in progress
    size_t stage_words = 0;
    Dev<uint32_t> list;        // device: [kSubsetCap] the live allowed rows, ascending (launch_filter_list), while list_ok
    // what a search needs, valid while `cached` and cached_dead == the index's dead_ver
    bool cached = false, list_ok = false;
    uint64_t cached_dead = 0;
    uint64_t n_allowed = 0, n_live = 0;  // rows in the set; those of them not removed
    uint64_t row_lo = 0, row_hi = 0;     // first row of the set, one past its last
};
struct mx_filter {
    mx_index *idx = nullptr;
    uint64_t epoch = 0;              // idx->row_epoch when the filter was made
    std::vector<FilterShard> sh;     // one per shard; a plain index: one
};

// A per-row column: one 32-bit word per GLOBAL row (id - id_offset - 1) of the handle it was made for, 0 where nothing
// was set, in one array on the device of the index that owns the stream (shards[0] of a composite: where the merged lists of a search
// end up).  No host mirror.  A grouping's keys and a prior's values are each one column; every call that reads or edits one holds the
// handle's mutex.
struct RowColumn {
    const char *noun;                // what the column is to its caller, for messages: "grouping" or "prior"
    mx_index *idx = nullptr;
    uint64_t epoch = 0;              // idx->row_epoch when the column was made
    int device = 0;                  // where the words live
    Dev<uint32_t> words;             // device: [len]; a row at or past len has the word 0
    uint64_t len = 0;
    Dev<void> stage;                 // device: the ranges, ids or keys of the call in progress and its words
    size_t stage_bytes = 0;
    Dev<uint64_t> dead;              // device: the removal mask by global row a sharded handle's reduction is taken against
    size_t dead_words = 0;
    const float *floats() const { return reinterpret_cast<const float *>(words.get()); }  // a prior's view of its words
};

// A grouping: a column of u32 keys, 0 = ungrouped.
struct mx_grouping {
    RowColumn col{"grouping"};
    Dev<uint64_t> part;              // device: [2 * kGroupCountBlocks] the partial sums of a count
    // outputs of the host-pointer search [kMaxBatch, out_cap] that the index's staging block has no room for
    Dev<uint32_t> out_keys;
    Dev<int32_t> out_rows;
    Dev<uint8_t> out_complete;
    int out_cap = 0;
    // the further per-head outputs of mx_index_search_group_rows [kMaxBatch, members_cap]
    Dev<int32_t> out_members;
    Dev<uint8_t> out_members_complete;
    int members_cap = 0;
};

// A prior: a column of f32 values.  hi >= every value of the column at all times: edits raise it on the host, a
// refresh replaces it by the exact maximum over the live rows and 0.
struct mx_prior {
    RowColumn col{"prior"};
    float hi = 0.0f;
    Dev<float> part;                 // device: [kBoostMaxBlocks] the partial maxima of a refresh
    Dev<float> weights;              // device: [kMaxBatch] the weights of the batch in progress
    // outputs of the host-pointer search [kMaxBatch, out_cap] that the index's staging block has no room for
    Dev<float> out_priors;
    Dev<double> out_combined;
    Dev<uint8_t> out_complete;
    int out_cap = 0;
};

namespace {

// the device buffers of a handle, released with their device current (under idx->mu)
void free_buffers(mx_filter *f) {
    for (FilterShard &fs : f->sh) {
        DeviceGuard dg(fs.device);
        fs.bits.reset();
        fs.stage.reset();
        fs.list.reset();
    }
}
void free_buffers(RowColumn &c) {
    c.words.reset();
    c.stage.reset();
    c.dead.reset();
}
void free_buffers(mx_grouping *g) {
    DeviceGuard dg(g->col.device);
    free_buffers(g->col);
    g->part.reset();
    g->out_keys.reset();
    g->out_rows.reset();
    g->out_complete.reset();
    g->out_members.reset();
    g->out_members_complete.reset();
}
void free_buffers(mx_prior *p) {
    DeviceGuard dg(p->col.device);
    free_buffers(p->col);
    p->part.reset();
    p->weights.reset();
    p->out_priors.reset();
    p->out_combined.reset();
    p->out_complete.reset();
}

std::mutex g_reg_mu;
std::map<std::string, mx_index *> g_registry;
std::once_flag g_scan_once;
hipError_t g_scan_setup_err = hipSuccess;
std::mutex g_rccl_mu;
Rccl g_rccl;
std::atomic<bool> g_rccl_broken{false};  // an initialisation hung: no further attempts in this process (indexes open concurrently)

bool load_rccl() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.lib) return g_rccl.ok;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        g_rccl.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.lib) break;
    }
    if (!g_rccl.lib) return false;
    auto sym = [&](const char *n) { return dlsym(g_rccl.lib, n); };
    g_rccl.CommInitAll = reinterpret_cast<int (*)(void **, int, const int *)>(sym("ncclCommInitAll"));
    g_rccl.CommDestroy = reinterpret_cast<int (*)(void *)>(sym("ncclCommDestroy"));
    g_rccl.AllGather = reinterpret_cast<int (*)(const void *, void *, size_t, int, void *, hipStream_t)>(sym("ncclAllGather"));
    g_rccl.GroupStart = reinterpret_cast<int (*)()>(sym("ncclGroupStart"));
    g_rccl.GroupEnd = reinterpret_cast<int (*)()>(sym("ncclGroupEnd"));
    g_rccl.GetErrorString = reinterpret_cast<const char *(*)(int)>(sym("ncclGetErrorString"));
    g_rccl.ok = g_rccl.CommInitAll && g_rccl.CommDestroy && g_rccl.AllGather && g_rccl.GroupStart && g_rccl.GroupEnd;
    return g_rccl.ok;
}

void free_composite_buffers(mx_index *idx) {
    for (size_t g = 0; g < idx->shards.size(); ++g) {
        DeviceGuard dg(idx->shards[g]->device);
        if (g < idx->sh_block.size()) idx->sh_block[g].reset();
        if (g < idx->sh_gather.size()) idx->sh_gather[g].reset();
        if (g < idx->sh_q.size()) idx->sh_q[g].reset();
        if (g < idx->sh_scores.size()) idx->sh_scores[g].reset();
        if (g < idx->sh_nf.size()) idx->sh_nf[g].reset();
    }
    idx->sh_block.clear(); idx->sh_gather.clear(); idx->sh_q.clear(); idx->sh_scores.clear(); idx->sh_nf.clear();
    idx->sh_kcap = 0;
}

}  // namespace

mx_index::~mx_index() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev_wait) (void)hipEventDestroy(ev_wait);
    if (stream) (void)hipStreamDestroy(stream);
    if (pooled && device >= 0 && device < kMaxDevices) {  // the last index on the device takes the lane-buffer pool with it
        LanePool &lp = g_lanes[device];
        std::lock_guard<std::mutex> lk(lp.mu);
        if (--lp.open_indexes <= 0) {
            lp.open_indexes = 0;
            for (LaneBufs &b : lp.idle) lane_free(b);
            lp.idle.clear();
        }
    }
}

namespace {

int free_index(mx_index *idx) {
    {   // nobody may still be inside a call on this handle (a combined search holds idx->mu)
        std::lock_guard<std::mutex> lk(idx->mu);
    }
    if (idx->composite()) {
        idx->pool.reset();  // joins the helper threads
        for (mx_index *sh : idx->shards) {
            DeviceGuard dg(sh->device);
            if (sh->stream) (void)hipStreamSynchronize(sh->stream);
        }
        free_composite_buffers(idx);
        for (void *c : idx->comms)
            if (c && g_rccl.ok) (void)g_rccl.CommDestroy(c);
        for (mx_index *sh : idx->shards) free_index(sh);
        idx->shards.clear();
    }
    DeviceGuard g(idx->device);
    delete idx;
    return MX_OK;
}

// a handle under construction: whatever it holds by then (a composite: its shards) goes with it on any failure
struct IndexCloser {
    void operator()(mx_index *idx) const { free_index(idx); }
};

// One set of lane buffers for the duration of a search_batch call (see LanePool).
struct LaneLease {
    mx_index *idx = nullptr;
    LaneBufs b;
    int take(mx_index *i, int groups) {
        if (i->device < 0 || i->device >= kMaxDevices) return fail(MX_EDEVICE, "device %d out of range", i->device);
        idx = i;
        LanePool &lp = g_lanes[i->device];
        {
            std::lock_guard<std::mutex> lk(lp.mu);
            for (size_t j = 0; j < lp.idle.size(); ++j)
                if (lp.idle[j].nwg == i->nwg && lp.idle[j].groups == groups) {
                    b = lp.idle[j];
                    lp.idle.erase(lp.idle.begin() + (long)j);
                    break;
                }
        }
        if (!b.rec) {
            b.nwg = i->nwg;
            b.groups = groups;
            const size_t lanes = (size_t)i->nwg * kScanThreads * (size_t)groups;  // a 512-query pass numbers 16 waves per workgroup
            hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.rec), lanes * kRecCap * 16 * sizeof(float));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b.tile), lanes * kRecCap * sizeof(uint32_t));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b.cnt), lanes * sizeof(uint32_t));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b.max), lanes * sizeof(float));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b.arg), lanes * sizeof(uint32_t));
            if (e != hipSuccess) {
                lane_free(b);
                idx = nullptr;
                return fail(MX_ENOMEM, "hipMalloc(lane buffers): %s", hipGetErrorString(e));
            }
        }
        Scratch &s = i->s;
        s.lane_rec = b.rec;
        s.lane_tile = b.tile;
        s.lane_cnt = b.cnt;
        s.lane_max = b.max;
        s.lane_arg = b.arg;
        return MX_OK;
    }
    void drop() {  // the caller is host-synchronised with everything that used the buffers
        if (!idx) return;
        Scratch &s = idx->s;
        s.lane_rec = nullptr;
        s.lane_tile = nullptr;
        s.lane_cnt = nullptr;
        s.lane_max = nullptr;
        s.lane_arg = nullptr;
        LanePool &lp = g_lanes[idx->device];
        std::lock_guard<std::mutex> lk(lp.mu);
        if (lp.open_indexes > 0) lp.idle.push_back(b);
        else lane_free(b);
        idx = nullptr;
        b = LaneBufs{};
    }
    ~LaneLease() { drop(); }
};

int ensure_scratch(mx_index *idx) {
    Scratch &s = idx->s;
    if (s.ready) return MX_OK;
    // a call that failed part-way left some of these allocated (zero-fills maybe still queued): alloc releases what a buffer held,
    // so nothing leaks, and the set is complete and zero-filled again before `ready` is set
    if (s.qfrag) MX_HIP(hipStreamSynchronize(idx->stream));
    const size_t ds = (size_t)idx->ds;
    const unsigned mapped = hipHostMallocMapped | hipHostMallocCoherent;
    MX_HIP(s.qfrag.alloc_bytes((size_t)kMaxBatch * ds * 2));
    MX_HIP(s.qpad.alloc((size_t)kMaxBatch * ds));
    MX_HIP(s.qnorm2.alloc(kMaxBatch));
    MX_HIP(s.theta.alloc(kMaxBatch));
    MX_HIP(s.theta_retry.alloc(kMaxBatch));
    MX_HIP(s.todo.alloc(kMaxBatch));
    MX_HIP(s.dev_flags.alloc(kFlagWords));
    MX_HIP(hipMemsetAsync(s.dev_flags, 0, kFlagWords * sizeof(uint32_t), idx->stream));
    s.overflow = s.dev_flags;
    s.cand_cnt = s.dev_flags + kMaxBatch;
    s.e1 = reinterpret_cast<float *>(s.dev_flags + 2 * kMaxBatch);
    s.qflags = s.dev_flags + 3 * kMaxBatch;
    MX_HIP(s.host_flags.alloc(kFlagWords, hipHostMallocDefault));
    MX_HIP(s.host_sum.alloc(kSumWords, mapped));
    memset(s.host_sum, 0, kSumWords * sizeof(uint32_t));
    MX_HIP(s.done_ctr.alloc(1));
    MX_HIP(hipMemsetAsync(s.done_ctr, 0, sizeof(uint32_t), idx->stream));
    MX_HIP(s.qstage.alloc((size_t)kMaxBatch * idx->dim));
    MX_HIP(s.qscale.alloc(kMaxBatch));
    MX_HIP(s.qa.alloc(kMaxBatch));
    MX_HIP(s.qb.alloc(kMaxBatch));
    MX_HIP(s.qmean.alloc(kMaxBatch));
    MX_HIP(hipMemsetAsync(s.qmean, 0, kMaxBatch * sizeof(float), idx->stream));
    MX_HIP(s.h_q.alloc((size_t)kMaxBatch * idx->dim, mapped));
    MX_HIP(s.h_nf.alloc(kMaxBatch, mapped));
    MX_HIP(s.max_err.alloc(1));
    MX_HIP(s.rlim.alloc(kMaxBatch));
    MX_HIP(s.out_nrange.alloc(kMaxBatch));
    MX_HIP(s.h_nr.alloc(kMaxBatch, mapped));
    MX_HIP(hipMemsetAsync(s.max_err, 0, sizeof(float), idx->stream));
    s.ready = true;
    return MX_OK;
}

int ensure_out(mx_index *idx, int k) {
    Scratch &s = idx->s;
    if (k <= s.kcap) return MX_OK;
    s.kcap = 0;
    const int kc = std::max(k, 16);
    const unsigned mapped = hipHostMallocMapped | hipHostMallocCoherent;
    MX_HIP(s.out_ids.alloc((size_t)kMaxBatch * kc));
    MX_HIP(s.out_scores.alloc((size_t)kMaxBatch * kc));
    MX_HIP(s.out_dists.alloc((size_t)kMaxBatch * kc));
    MX_HIP(s.out_nfound.alloc(kMaxBatch));
    MX_HIP(s.h_ids.alloc((size_t)kMaxBatch * kc, mapped));
    MX_HIP(s.h_scores.alloc((size_t)kMaxBatch * kc, mapped));
    MX_HIP(s.h_dists.alloc((size_t)kMaxBatch * kc, mapped));
    s.kcap = kc;
    return MX_OK;
}

// EXACT path scratch for passes of `gcap` queries (4 / 8 / 16 / 32: the kernel's query-per-thread buckets).  The EXACT path
// is the correctness backstop -- one doubly-overflowed query, one k > 256 search -- so it asks for what THIS batch needs
// (4 B per row and query of the pass), not for a full group, and on a full device it settles for smaller passes.
int ensure_exact(mx_index *idx, int k, int *gcap) {
    Scratch &s = idx->s;
    for (int g = *gcap;; g /= 2) {
        const size_t need = exact_group_scratch_bytes(idx->n, k, g);
        if (s.exact_bytes >= need) {
            *gcap = g;
            return MX_OK;
        }
        if (s.exact_scratch) MX_HIP(hipStreamSynchronize(idx->stream));
        s.exact_scratch.reset();
        s.exact_bytes = 0;
        const size_t want = need + need / 4;  // room for appends before the next reallocation
        if (s.exact_scratch.alloc_bytes(want) == hipSuccess) {
            s.exact_bytes = want;
        } else {
            (void)hipGetLastError();
            if (s.exact_scratch.alloc_bytes(need) == hipSuccess) s.exact_bytes = need;
            else (void)hipGetLastError();
        }
        if (s.exact_bytes >= need) {
            *gcap = g;
            return MX_OK;
        }
        if (g <= 4) return fail(MX_ENOMEM, "hipMalloc(EXACT-path scratch, %zu bytes) failed", need);
    }
}

// the dead-row mask covers `cap` rows (one word per 64-row tile); words past the old size start with no row removed
int grow_dead(mx_index *idx, uint64_t cap) {
    if (!idx->dead) return MX_OK;  // allocated by the first removal
    const size_t words = (size_t)(cap / kTile8Rows), have = idx->dead_h.size();
    if (words <= have) return MX_OK;
    Dev<uint64_t> nd;
    MX_HIP(nd.alloc(words));
    MX_HIP(hipMemcpyAsync(nd, idx->dead, have * sizeof(uint64_t), hipMemcpyDeviceToDevice, idx->stream));
    MX_HIP(hipMemsetAsync(nd + have, 0, (words - have) * sizeof(uint64_t), idx->stream));
    MX_HIP(hipStreamSynchronize(idx->stream));
    idx->dead = std::move(nd);
    idx->dead_h.resize(words, 0);
    return MX_OK;
}

int ensure_capacity(mx_index *idx, uint64_t rows) {
    if (rows <= idx->cap) return MX_OK;
    uint64_t want = std::max<uint64_t>(rows, idx->cap + idx->cap / 2);
    want = round_up(std::max<uint64_t>(want, 1024), kTile8Rows);
    if (int rc = grow_dead(idx, want); rc != MX_OK) return rc;
    if (idx->compressed) {  // the bf16 copy is the corpus: it must grow, there is nothing to fall back to
        Dev<void> nh2;
        const size_t hb = (size_t)want * idx->ds * 2;
        MX_HIP(nh2.alloc_bytes(hb));
        const size_t used = idx->xh ? (size_t)round_up(idx->n, kTileRows) * idx->ds * 2 : 0;
        if (used) MX_HIP(hipMemcpyAsync(nh2, idx->xh, used, hipMemcpyDeviceToDevice, idx->stream));
        MX_HIP(hipMemsetAsync(static_cast<char *>(nh2.get()) + used, 0, hb - used, idx->stream));
        MX_HIP(hipStreamSynchronize(idx->stream));
        idx->xh = std::move(nh2);
        idx->cap = want;
        return MX_OK;
    }
    Dev<float> nx, nsc, nts, nam;
    Dev<void> nh;
    const size_t rowb = (size_t)idx->ds * sizeof(float);
    MX_HIP(nx.alloc(want * (size_t)idx->ds));
    MX_HIP(nsc.alloc(want));
    float *fx = nx, *fsc = nsc;
    if (idx->n) {
        MX_HIP(hipMemcpyAsync(fx, idx->x, idx->n * rowb, hipMemcpyDeviceToDevice, idx->stream));
        MX_HIP(hipMemcpyAsync(fsc, idx->scale, idx->n * sizeof(float), hipMemcpyDeviceToDevice, idx->stream));
    }
    MX_HIP(hipMemsetAsync(fx + idx->n * (size_t)idx->ds, 0, (want - idx->n) * rowb, idx->stream));
    MX_HIP(hipMemsetAsync(fsc + idx->n, 0, (want - idx->n) * sizeof(float), idx->stream));
    if (idx->want_filter && idx->kc <= kMaxKC16) {
        // the filter copy is an accelerator, not a requirement: without HBM for it the index
        // keeps working on the f32 scan
        const size_t eb = idx->filter_i8 ? 1 : 2;  // bytes per stored element
        const size_t hb = (size_t)want * idx->ds * eb, tb = (size_t)(want / kTile8Rows) * kTscaleFloats * sizeof(float);
        if (nh.alloc_bytes(hb) != hipSuccess || (idx->filter_i8 && nts.alloc_bytes(tb) != hipSuccess)) {
            (void)hipGetLastError();
            nh.reset();
        } else {
            const uint64_t used_rows = idx->xh ? round_up(idx->n, kTile8Rows) : 0;
            const size_t used = (size_t)used_rows * idx->ds * eb;
            if (used) MX_HIP(hipMemcpyAsync(nh, idx->xh, used, hipMemcpyDeviceToDevice, idx->stream));
            MX_HIP(hipMemsetAsync(static_cast<char *>(nh.get()) + used, 0, hb - used, idx->stream));
            if (idx->filter_i8) {
                const size_t tused = (size_t)(used_rows / kTile8Rows) * kTscaleFloats * sizeof(float);
                if (tused) MX_HIP(hipMemcpyAsync(nts, idx->tsc, tused, hipMemcpyDeviceToDevice, idx->stream));
                MX_HIP(hipMemsetAsync(reinterpret_cast<char *>(nts.get()) + tused, 0, tb - tused, idx->stream));
                if (idx->centred && idx->xh && idx->amean) {
                    // the a_c array of a CENTRED int8 copy grows with it; without room for it the copy is rewritten plain from the rows
                    if (nam.alloc(want) == hipSuccess) {
                        const size_t aused = (size_t)used_rows * sizeof(float);
                        MX_HIP(hipMemcpyAsync(nam, idx->amean, std::min(aused, (size_t)idx->cap * sizeof(float)), hipMemcpyDeviceToDevice, idx->stream));
                        if (want * sizeof(float) > aused) MX_HIP(hipMemsetAsync(reinterpret_cast<char *>(nam.get()) + aused, 0, want * sizeof(float) - aused, idx->stream));
                    } else {
                        (void)hipGetLastError();
                        if (idx->n) {
                            const uint32_t t1c = (uint32_t)((idx->n + kTileRows - 1) / kTileRows);
                            MX_HIP(launch_shadow8(idx->stream, fx, fsc, idx->ds, 0, (uint32_t)round_up(t1c, 2), idx->n, nh, nts, idx->flags + 2));
                        }
                    }
                }
            } else if (idx->kc <= kMaxKC && nam.alloc(want) == hipSuccess) {
                // the a_c array of a (possibly centred) bf16 copy grows with it
                const size_t aused = idx->amean && idx->xh ? (size_t)idx->n * sizeof(float) : 0;
                if (aused) MX_HIP(hipMemcpyAsync(nam, idx->amean, aused, hipMemcpyDeviceToDevice, idx->stream));
                MX_HIP(hipMemsetAsync(reinterpret_cast<char *>(nam.get()) + aused, 0, want * sizeof(float) - aused, idx->stream));
            } else {
                (void)hipGetLastError();
                if (idx->centred && idx->xh && idx->n) {
                    // no room for the a_c array of a CENTRED copy: the fragments just copied hold c/|c| - a_c m and would be
                    // read as c/|c| -- rewrite the copy as a plain one from the rows (rare: 4 bytes per row did not fit)
                    const uint32_t t1c = (uint32_t)((idx->n + kTileRows - 1) / kTileRows);
                    MX_HIP(launch_shadow(idx->stream, fx, fsc, idx->ds, 0, t1c, nh, idx->flags + 2));
                }
            }
            if (!idx->xh && idx->n) {  // (re)enabled on a populated index
                const uint32_t t1 = (uint32_t)((idx->n + kTileRows - 1) / kTileRows);
                if (idx->filter_i8)
                    MX_HIP(launch_shadow8(idx->stream, fx, fsc, idx->ds, 0, t1, idx->n, nh, nts, idx->flags + 2));
                else
                    MX_HIP(launch_shadow(idx->stream, fx, fsc, idx->ds, 0, t1, nh, idx->flags + 2));
            }
        }
    }
    MX_HIP(hipStreamSynchronize(idx->stream));
    // (a centred copy stays centred only if its a_c array came along: a copy built afresh above is a plain one)
    const bool keep_centre = idx->centred && idx->xh && idx->amean && nh && nam;
    idx->x = std::move(nx);
    idx->scale = std::move(nsc);
    idx->xh = std::move(nh);
    idx->tsc = std::move(nts);
    idx->amean = std::move(nam);
    idx->centred = keep_centre;
    idx->cap = want;
    return MX_OK;
}

int build_filter_copy(mx_index *idx, bool i8);

// reads the ingest flags back; a batch with non-finite rows is rejected (zero-row list rolled back),
// otherwise the zero-norm rows it brought are committed (list kept ascending for finish_kernel)
int commit_ingest(mx_index *idx, uint32_t (&fl)[5]) {
    MX_HIP(hipMemcpyAsync(fl, idx->flags, sizeof(fl), hipMemcpyDeviceToHost, idx->stream));
    MX_HIP(hipStreamSynchronize(idx->stream));
    if (fl[0] != 0) {
        const uint32_t keep[2] = {(uint32_t)idx->n_zero, (uint32_t)idx->n_wild};
        MX_HIP(hipMemcpyAsync(idx->flags + 3, keep, sizeof(keep), hipMemcpyHostToDevice, idx->stream));
        MX_HIP(hipStreamSynchronize(idx->stream));
        return fail(MX_EINVAL, "%u row(s) contain non-finite values; nothing inserted", fl[0]);
    }
    if (fl[4] != idx->n_wild) {  // new listed rows arrive in atomic order: keep the list ascending
        const size_t have = std::min<size_t>(fl[4], kWildCap);
        if (have > std::min<uint64_t>(idx->n_wild, kWildCap)) {
            std::vector<uint32_t> z(have);
            MX_HIP(hipMemcpy(z.data(), idx->wild_list, have * sizeof(uint32_t), hipMemcpyDeviceToHost));
            std::sort(z.begin(), z.end());
            MX_HIP(hipMemcpy(idx->wild_list, z.data(), have * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        idx->n_wild = fl[4];
    }
    if (fl[3] != idx->n_zero) {
        const size_t have = std::min<size_t>(fl[3], kZeroCap);
        if (have > std::min<uint64_t>(idx->n_zero, kZeroCap)) {  // new entries arrive in atomic order: sort
            std::vector<uint32_t> z(have);
            MX_HIP(hipMemcpy(z.data(), idx->zero_rows, have * sizeof(uint32_t), hipMemcpyDeviceToHost));
            std::sort(z.begin(), z.end());
            MX_HIP(hipMemcpy(idx->zero_rows, z.data(), have * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        idx->n_zero = fl[3];
    }
    return MX_OK;
}

// rows already on the device ([n, dim]); appends and validates
int add_device_locked(mx_index *idx, const float *d_rows, uint64_t n, uint64_t *first_id) {
    if (n == 0) {
        if (first_id) *first_id = idx->idmap.id_of((uint32_t)idx->n);
        return MX_OK;
    }
    if (idx->n + n > 0xfffffff0ull) return fail(MX_EINSERT, "index shard limited to 2^32 rows");
    int rc = ensure_capacity(idx, idx->n + n);
    if (rc != MX_OK) return rc;
    MX_HIP(hipMemsetAsync(idx->flags, 0, 2 * sizeof(uint32_t), idx->stream));
    if (idx->compressed) {
        // rows -> f32 staging window (validated, padded, 1/|c|) -> bf16 fragments.  The window is aligned
        // to the tile of the first new row; rows of that tile that are already stored are not touched.
        constexpr uint64_t kWin = 65536;
        if (!idx->xs) {
            MX_HIP(idx->xs.alloc((size_t)(kWin + kTileRows) * idx->ds));
            MX_HIP(idx->ss.alloc((size_t)(kWin + kTileRows)));
            idx->xs_rows = kWin + kTileRows;
        }
        uint32_t fl[5] = {0, 0, 0, 0, 0};
        for (uint64_t done = 0; done < n; done += kWin) {
            const uint64_t m = std::min(kWin, n - done), g0 = idx->n + done;     // global rows [g0, g0 + m)
            const uint64_t t0 = g0 / kTileRows, off = g0 % kTileRows;
            MX_HIP(launch_ingest(idx->stream, d_rows + (size_t)done * idx->dim, m, idx->dim, idx->xs, idx->ss, off, idx->ds, idx->flags,
                                 idx->raw_ingest ? 1 : 0, idx->zero_rows, idx->wild_list, g0));
            MX_HIP(launch_shadow(idx->stream, idx->xs, idx->ss, idx->ds, (uint32_t)t0, (uint32_t)((g0 + m + kTileRows - 1) / kTileRows),
                                 idx->xh, idx->flags + 2, (uint32_t)t0, g0, g0 + m));
        }
        int rc2 = commit_ingest(idx, fl);
        if (rc2 != MX_OK) return rc2;  // rows past idx->n are never read by a search; the next append overwrites them
        idx->wild_rows += fl[1];
        if (first_id) *first_id = idx->idmap.id_of((uint32_t)idx->n);
        idx->n += n;
        return MX_OK;
    }
    MX_HIP(launch_ingest(idx->stream, d_rows, n, idx->dim, idx->x, idx->scale, idx->n, idx->ds, idx->flags, 2, idx->zero_rows, idx->wild_list, idx->n));
    // tiles touched by this append (the first one may already be partly filled; an 8-bit half tile is requantised
    // as a whole: its step depends on all of its rows)
    auto refilter = [&](uint64_t row_lo, uint64_t row_hi) -> hipError_t {
        const uint32_t h0 = (uint32_t)(row_lo / kTileRows), h1 = (uint32_t)((row_hi + kTileRows - 1) / kTileRows);
        const bool ctr = idx->centred && idx->amean && idx->mean;
        if (idx->filter_i8)  // both halves of the last 64-row scan tile: the one past row_hi becomes zeros with step 0
            return launch_shadow8(idx->stream, idx->x, idx->scale, idx->ds, h0, (uint32_t)round_up(std::max(h1, h0 + 1), 2), row_hi, idx->xh, idx->tsc, idx->flags + 2,
                                  ctr ? idx->mean : nullptr, ctr ? idx->amean : nullptr, ctr ? idx->flags + 5 : nullptr);
        return launch_shadow(idx->stream, idx->x, idx->scale, idx->ds, h0, std::max(h1, h0 + 1), idx->xh, idx->flags + 2, 0, 0, ~0ull,
                             ctr ? idx->mean : nullptr, ctr ? idx->amean : nullptr);
    };
    if (idx->xh) MX_HIP(refilter(idx->n, idx->n + n));
    uint32_t fl[5] = {0, 0, 0, 0, 0};
    rc = commit_ingest(idx, fl);
    if (rc != MX_OK) {
        // rows past idx->n are never read, but the filter copy's tile of row n may now hold garbage: rebuild it
        if (idx->xh) {
            const std::string keep = last_error_slot();
            MX_HIP(refilter(idx->n, idx->n));
            last_error_slot() = keep;
        }
        return rc;
    }
    idx->wild_rows += fl[1];
    if (first_id) *first_id = idx->idmap.id_of((uint32_t)idx->n);  // local.rs:63: next_id = len + 1
    idx->n += n;
    // A demotion is not for life: it was decided on the rows and the queries of its day.  Once the collection has doubled
    // since, the automatic choice gets its int8 copy back (one pass over the rows, as when it was first built) and the
    // demotion rule judges it afresh; mx_index_set_filter_copy(idx, 1) does the same at once.
    if (idx->filter_auto && idx->xh && !idx->filter_i8 && idx->demoted_at_rows && idx->n >= 2 * idx->demoted_at_rows &&
        idx->ds <= kAutoI8MaxDim) {
        const std::string keep = last_error_slot();
        if (build_filter_copy(idx, true) == MX_OK) {
            idx->demoted_at_rows = 0;
            idx->stats.filter_promotions += 1;
        } else {
            idx->demoted_at_rows = idx->n;  // no room now: ask again after the next doubling
            last_error_slot() = keep;
        }
    }
    // ... and a bf16 copy that was built plain (fewer than 256 rows at the time, or rows that did not sit in a cone) is rebuilt once the
    // collection has doubled: should the rows sit in a cone by now, it comes back centred (section 3.2c) -- one pass over the rows per
    // doubling.  (An automatic copy gets there through the promotion above; this is for a pinned bf16 copy.)
    // (plain_bf16_rows == 0: the copy grew with the index from empty and was never built in one piece: first look at 256 rows)
    if (idx->xh && !idx->filter_i8 && !idx->compressed && !idx->centred && idx->kc <= kMaxKC && idx->n >= 256 &&
        idx->n >= 2 * std::max<uint64_t>(idx->plain_bf16_rows, 128) && !(idx->filter_auto && idx->demoted_at_rows)) {
        const std::string keep = last_error_slot();
        if (build_filter_copy(idx, false) != MX_OK) {
            idx->plain_bf16_rows = idx->n;  // no room now: ask again after the next doubling
            last_error_slot() = keep;
        }
    }
    return MX_OK;
}

constexpr double kExactThetaDiv = 32.0;  // sample of the plain int8 copy up to 512 dims when theta_kernel rescores its best rows (below)
// how many tiles the sample launch visits: enough that the k-th largest of 2*nwg lane maxima is a
// useful threshold (expected survivors of the collect launch ~ k * N / sample, times the margin's
// share) and small enough to stay a few percent of the pass
uint32_t sample_stride(uint64_t full_tiles, int nwg, int k, bool filt8, int ds, bool exact_theta, int debug_div) {
    // 1/64 of the tiles for k <= 10.  Measured at 10M x 384 (B = 256): the sample launch costs 65 / 38 / 24 /
    // 17 us at 1/32, 1/64, 1/128, 1/256; a weaker threshold means more records for finish_kernel to sift
    // (62 / 63 / 72 us, and at 1/256 lanes start to overflow their 32 records), while the collect launch
    // hardly notices since appends became whole-record stores (1.76 / 1.77 / 1.79 ms).  1/64 is the
    // fastest end to end.  The int8 copy's certificate is four to five times wider, so a weak threshold costs it far
    // more rows: 1/16 of the tiles up to 512 dims, 1/8 at 768, 1/4 at 1024 (a smaller sample makes lanes overflow
    // their 64 records and the retry pass costs a whole scan: scripts/r3_i8_sample.sh, r3_dims.sh).
    // (A tuning constant: results do not depend on it.)
    // (MEMEX_HIP_DEBUG=sample_div=N tries others: a tuning knob, results do not depend on it.)
    // (a centred int8 copy, whose certificate is four to five times tighter again, gains nothing from a smaller sample: 1/32 against
    // 1/16 on the enc_like leg 169.3k against 169.0k queries/s; at 1/64 lanes overflow and the copy is demoted: gpurun_out/r6m_*)
    // The plain int8 copy with the exact threshold (launch_theta's ThetaExact: the best sampled rows rescored in f32, so the threshold no
    // longer carries the a-priori bracket): 1/32 of the tiles up to 512 dims.  10M x 384, B = 256, k = 10, queries/s at 1/16 | 1/32 |
    // 1/64 (and 1/16 without the exact threshold): Gaussian 244.2k | 249.6k | 245.3k (236.1k), clustered 241.1k | 248.6k | 247.6k
    // (243.4k), anisotropic 247.9k | 248.7k | 246.2k (233.1k); no retry query in any of them (profiles/exact_theta_sample_sweep.txt).
    double div = !filt8 ? 64.0 : ds <= 512 ? (exact_theta ? kExactThetaDiv : 16.0) : ds <= 768 ? 8.0 : 4.0;
    if (debug_div >= 2 && debug_div <= 4096) div = (double)debug_div;  // mx_index::sample_div
    // larger k: the sample grows like k / 640 for every copy (int8 at k = 30 / 100: 1.33 / 1.56 ms per step with
    // 1/16 / 0.16 of the tiles against 1.93 / 1.77 with three and ten times the k = 10 sample)
    const double f = std::min(0.5, std::max(1.0 / div, (double)k / 640.0));
    const uint64_t target = std::max<uint64_t>((uint64_t)nwg, (uint64_t)((double)full_tiles * f));
    return (uint32_t)std::max<uint64_t>(1, full_tiles / std::max<uint64_t>(target, 1));
}

constexpr size_t kExactKeepBytes = 256ull << 20;  // EXACT-path scratch kept between batches up to this size

// mask: removed rows, or the per-call mask of a filtered search (null: none); n_live: rows it leaves
int run_exact(mx_index *idx, const std::vector<int> &qs, int k, uint64_t *d_ids, float *d_scores, float *d_dists,
              int32_t *d_nfound, const uint64_t *mask, uint64_t n_live) {
    if (qs.empty()) return MX_OK;
    int gcap = qs.size() <= 4 ? 4 : qs.size() <= 8 ? 8 : qs.size() <= 16 ? 16 : kExactGroup;
    int rc = ensure_exact(idx, k, &gcap);
    if (rc != MX_OK) return rc;
    Scratch &s = idx->s;
    // groups of up to gcap (<= 32) queries share one pass over the rows (launch_exact_group); the groups of a batch reuse the
    // scratch in stream order
    for (size_t g0 = 0; g0 < qs.size(); g0 += (size_t)gcap) {
        ExactGroup grp{};
        grp.n = (int)std::min<size_t>((size_t)gcap, qs.size() - g0);
        for (int j = 0; j < grp.n; ++j) grp.q[j] = qs[g0 + j];
        MX_HIP(launch_exact_group(idx->stream, k, idx->ds, idx->compressed ? nullptr : idx->x, idx->xh, idx->n, idx->idmap, s.qpad,
                                  s.qnorm2, grp, s.exact_scratch, d_ids, d_scores, d_dists, d_nfound, mask, n_live));
    }
    return MX_OK;
}

// builds the filter copy of kind (i8 ? int8 : bf16) from the f32 rows, complete before it replaces whatever copy is resident
int build_filter_copy(mx_index *idx, bool i8) {
    Dev<void> nh;
    Dev<float> nts, nam;
    Dev<uint32_t> nec;
    const size_t hb = (size_t)idx->cap * idx->ds * (i8 ? 1 : 2), tb = (size_t)(idx->cap / kTile8Rows) * kTscaleFloats * sizeof(float);
    hipError_t e = nh.alloc_bytes(hb);
    if (e == hipSuccess && i8) e = nts.alloc_bytes(tb);
    if (e == hipSuccess) e = nec.alloc(2);  // [0] largest residual, [1] longest centred row (int8)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MX_ENOMEM, "hipMalloc(filter copy, %zu bytes): %s", hb, hipGetErrorString(e));
    }
    uint32_t *ec = nec;
    MX_HIP(hipMemsetAsync(nh, 0, hb, idx->stream));
    if (i8) MX_HIP(hipMemsetAsync(nts, 0, tb, idx->stream));
    MX_HIP(hipMemsetAsync(ec, 0, 2 * sizeof(uint32_t), idx->stream));
    const uint32_t t1 = (uint32_t)((idx->n + kTileRows - 1) / kTileRows);
    // A copy rebuilt from a populated index is CENTRED on the rows' mean direction (launch_shadow / launch_shadow8): a corpus
    // that a plain int8 certificate could not resolve is a dense one, and embedding corpora are dense because they sit in a
    // cone -- what is left of a row after its component along the cone's axis is removed is several times shorter, and so is
    // the rounding (bf16) or quantisation (int8: round 6) error the scan's certificate has to cover.
    const bool centre_ok = true;
    bool centre = false;
    if (idx->kc <= kMaxKC && !idx->compressed && nam.alloc((size_t)idx->cap) == hipSuccess) {
        MX_HIP(hipMemsetAsync(nam, 0, (size_t)idx->cap * sizeof(float), idx->stream));
        if (centre_ok && idx->n >= 256) {
            if (!idx->mean) MX_HIP(idx->mean.alloc((size_t)idx->ds));
            if (!idx->msum) MX_HIP(idx->msum.alloc((size_t)idx->ds + 1));
            MX_HIP(launch_mean_dir(idx->stream, idx->x, idx->scale, idx->n, idx->ds, idx->msum, idx->mean));
            // worth it only for a corpus that does sit in a cone: |mean of the unit rows| = the typical a_c; below 0.3 the
            // centred rows are < 5 % shorter and the scan's extra epilogue work buys nothing
            float msq = 0.f;
            MX_HIP(hipMemcpyAsync(&msq, idx->msum + idx->ds, sizeof(float), hipMemcpyDeviceToHost, idx->stream));
            MX_HIP(hipStreamSynchronize(idx->stream));
            centre = std::isfinite(msq) && msq / (float)idx->n >= 0.3f;
        }
    } else {
        (void)hipGetLastError();
    }
    if (i8 && !centre) nam.reset();  // (a plain int8 copy has no use for the a_c array)
    if (i8)
        MX_HIP(launch_shadow8(idx->stream, idx->x, idx->scale, idx->ds, 0, (uint32_t)round_up(t1, 2), idx->n, nh, nts, ec,
                              centre ? idx->mean : nullptr, centre ? nam : nullptr, centre ? ec + 1 : nullptr));
    else
        MX_HIP(launch_shadow(idx->stream, idx->x, idx->scale, idx->ds, 0, t1, nh, ec, 0, 0, ~0ull, centre ? idx->mean : nullptr,
                             centre ? nam : nullptr));
    MX_HIP(hipMemcpyAsync(idx->flags + 2, ec, sizeof(uint32_t), hipMemcpyDeviceToDevice, idx->stream));
    MX_HIP(hipMemcpyAsync(idx->flags + 5, ec + 1, sizeof(uint32_t), hipMemcpyDeviceToDevice, idx->stream));
    MX_HIP(hipStreamSynchronize(idx->stream));
    idx->xh = std::move(nh);
    idx->tsc = std::move(nts);
    idx->amean = std::move(nam);
    idx->centred = centre;
    idx->filter_i8 = i8;
    idx->plain_bf16_rows = (!i8 && !centre) ? std::max<uint64_t>(idx->n, 1) : 0;
    idx->i8_batches = idx->i8_retry_batches = 0;
    for (double &w : idx->wait_ema_us) w = 0.0;
    return MX_OK;
}

// int8 filter copy -> bf16 filter copy, rebuilt from the f32 rows (an automatic choice that did not suit the data).
// The bf16 copy is complete (and its residual word known) before the int8 copy is released: any failure leaves the
// index exactly as it was.  MX_ENOMEM: no room for the wider copy, the caller stays on int8.
int demote_filter(mx_index *idx) {
    const std::string keep = last_error_slot();
    const int rc = build_filter_copy(idx, false);
    if (rc == MX_ENOMEM) last_error_slot() = keep;
    if (rc == MX_OK) idx->demoted_at_rows = std::max<uint64_t>(idx->n, 1);
    return rc;
}

// ---- filtered search (mx_index_search_filtered) ------------------------------------------------------------------
// half-open [lo, hi) ranges of ids or of rows: Ranges (mx_filter_bits.h)

// sorted by lo, overlapping and adjacent ranges merged, empty ones dropped
void normalise_ranges(Ranges &r) {
    std::sort(r.begin(), r.end());
    size_t m = 0;
    for (const auto &x : r) {
        if (x.first >= x.second) continue;
        if (m && x.first <= r[m - 1].second) r[m - 1].second = std::max(r[m - 1].second, x.second);
        else r[m++] = x;
    }
    r.resize(m);
}

// normalised id ranges -> the rows [0, n) they select (row = id - id_offset - 1), still normalised
Ranges rows_of_ids(const Ranges &ids, uint64_t off, uint64_t n) {
    Ranges out;
    for (const auto &x : ids) {
        const uint64_t lo = x.first > off ? x.first - off - 1 : 0, hi = std::min(x.second > off ? x.second - off - 1 : 0, n);
        if (lo < hi) out.emplace_back(lo, hi);
    }
    return out;
}

// Global rows of a sharded handle -> the local rows of shard g.  Rows are dealt in blocks of R (global row r: block b = r / R, on
// shard b % G, local row (b / G) R + r % R), so the blocks of shard g inside a global range [lo, hi) -- b1, b1 + G, ..., b2 -- are
// consecutive local blocks b1 / G .. b2 / G: one global range is at most ONE local range per shard, from the local row of its first
// row on the shard to that of its last.  The mapping is monotone, so sorted ranges stay sorted.
Ranges shard_ranges(const Ranges &glob, uint64_t R, uint64_t G, uint64_t g) {
    Ranges out;
    for (const auto &x : glob) {
        const uint64_t b_lo = x.first / R, b_hi = (x.second - 1) / R;
        const uint64_t b1 = b_lo + (g + G - b_lo % G) % G;  // first block of shard g at or after b_lo
        if (b1 > b_hi) continue;
        const uint64_t b2 = b_hi - (b_hi % G + G - g) % G;  // last one at or before b_hi
        const uint64_t first = std::max(x.first, b1 * R), last = std::min(x.second - 1, b2 * R + R - 1);
        out.emplace_back((b1 / G) * R + first % R, (b2 / G) * R + last % R + 1);
    }
    normalise_ranges(out);  // (adjacent local ranges join)
    return out;
}

// rows of the (clipped) ranges that are not removed: a popcount over the host copy of the dead-row words
uint64_t count_allowed(const mx_index *t, const Ranges &r) {
    uint64_t c = 0;
    for (const auto &x : r) {
        c += x.second - x.first;
        if (!t->n_dead) continue;
        for (uint64_t w = x.first >> 6; w * 64 < x.second; ++w) {
            uint64_t bits = t->dead_h[w];
            const uint64_t a = std::max(x.first, w * 64) - w * 64, b = std::min(x.second, w * 64 + 64) - w * 64;
            bits &= (b == 64 ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull);
            c -= (uint64_t)__builtin_popcountll(bits);
        }
    }
    return c;
}

int ensure_mask_words(mx_index *idx, size_t words);

// the per-call mask of a masked pass over the ranges (clipped to the rows): every word of the capacity (the zero-query walk and
// the EXACT path read them all), dead words included when the index has removals
int build_filter_mask(mx_index *idx, const Ranges &r, std::vector<uint64_t> &flat) {
    const size_t words = (size_t)(idx->cap / kTile8Rows);
    if (int rc = ensure_mask_words(idx, words); rc != MX_OK) return rc;
    if (idx->filt_ranges_cap < std::max<size_t>(r.size(), 1)) {
        idx->filt_ranges_cap = 0;
        const size_t want = std::max<size_t>(r.size() + r.size() / 2, 64);
        MX_HIP(idx->filt_ranges.alloc(want * 2));
        idx->filt_ranges_cap = want;
    }
    flat.resize(2 * r.size());
    for (size_t i = 0; i < r.size(); ++i) {
        flat[2 * i] = r[i].first;
        flat[2 * i + 1] = r[i].second;
    }
    if (!flat.empty())
        MX_HIP(hipMemcpyAsync(idx->filt_ranges, flat.data(), flat.size() * sizeof(uint64_t), hipMemcpyHostToDevice, idx->stream));
    MX_HIP(launch_filter_mask(idx->stream, idx->n_dead ? idx->dead : nullptr, idx->filt_ranges, (uint32_t)r.size(), words, idx->filt));
    return MX_OK;
}

// Which path answers a filtered batch of B queries whose ranges leave m <= kSubsetCap rows over a span of span_rows rows
// (MEMEX_HIP_DEBUG=filt_subset=0|1 forces one).  A cost model fitted to profiles/filtered_10Mx384.txt (int8 copy, 384 dims,
// k = 10):
//   subset kernel     43 us + 0.053 us per row at 384 dims, whatever B up to 256 (one workgroup per query, each a chain of
//                     m / 1024 rows per thread: latency-bound, so B = 1 costs what B = 256 does); once more per further 256 queries
//   masked pipeline   75 us of fixed launches + the scan of the span: 0.065 ns per int8 byte at B <= 128, 0.10 ns above
// The kernel wins for scattered rows (the span is the collection) up to the cap, and for a contiguous run up to ~600 rows.
bool subset_pays(const mx_index *idx, int B, uint64_t m, uint64_t span_rows, int bytes_per_elem) {
    if (m > (uint64_t)kSubsetCap || idx->ds > kMaxKC16 * kChunkFloats) return false;
    const int force = debug_flag("filt_subset", -1);
    if (force == 0 || force == 1) return force == 1;
    const double w = (double)idx->ds / 384.0;
    const double subset_us = (double)((B + kPassBatch - 1) / kPassBatch) * (43.0 + 0.053 * w * (double)m);
    const double masked_us = 75.0 + (double)span_rows * w * bytes_per_elem * (B <= 128 ? 0.065e-3 : 0.10e-3);
    return subset_us <= masked_us;
}

// What restricts a filtered batch: the ranges of a per-call filter (search_batch: local rows; composite_batch: global rows), or a
// resident filter and the shard of it this index holds.
struct FilterArg {
    const Ranges *ranges = nullptr;
    mx_filter *res = nullptr;
    int shard = 0;
};

// the cached counts and span of one shard of a resident filter, recomputed from the host mirrors when the filter or the shard's
// removals have changed since they were taken (t: the plain index or shard that holds the rows)
void refresh_filter_shard(const mx_index *t, FilterShard &fs) {
    if (fs.cached && fs.cached_dead == t->dead_ver) return;
    fs.n_allowed = fs.n_live = 0;
    fs.row_lo = fs.row_hi = 0;
    const bool dead = t->n_dead != 0;
    for (size_t w = 0; w < fs.bits_h.size(); ++w) {
        const uint64_t b = fs.bits_h[w];
        if (!b) continue;
        if (!fs.n_allowed) fs.row_lo = (uint64_t)w * 64 + (uint64_t)__builtin_ctzll(b);
        fs.row_hi = (uint64_t)w * 64 + 64 - (uint64_t)__builtin_clzll(b);
        fs.n_allowed += (uint64_t)__builtin_popcountll(b);
        fs.n_live += (uint64_t)__builtin_popcountll(dead && w < t->dead_h.size() ? b & ~t->dead_h[w] : b);
    }
    fs.cached = true;
    fs.cached_dead = t->dead_ver;
    fs.list_ok = false;
}

// the index-owned mask buffer of a masked pass covers the capacity
int ensure_mask_words(mx_index *idx, size_t words) {
    if (idx->filt_words >= words) return MX_OK;
    idx->filt_words = 0;
    MX_HIP(idx->filt.alloc(words));  // (every batch before this one is host-synchronised)
    idx->filt_words = words;
    return MX_OK;
}

// the per-call mask of a masked pass with a resident filter: one launch over the capacity's words, no upload
int apply_filter_mask(mx_index *idx, const FilterShard &fs) {
    const size_t words = (size_t)(idx->cap / kTile8Rows);
    if (int rc = ensure_mask_words(idx, words); rc != MX_OK) return rc;
    MX_HIP(launch_filter_apply(idx->stream, idx->n_dead ? idx->dead : nullptr, fs.bits, std::min(fs.words, words), words, idx->filt));
    return MX_OK;
}

// Wait for the completion word of a finish launch (finish_kernel, range_finish_kernel) with sequence number seq, for a batch of B
// queries.  A kernel that never signals (fault) is caught by the synchronize after the spin budget.
int await_finish(mx_index *idx, int B, uint32_t seq) {
    Scratch &s = idx->s;
    // Default: a SLEEPING wait -- a server thread must not burn a core for the ~1 ms of a batch.  The HIP runtime's
    // own waits do not help: hipStreamSynchronize and hipEventSynchronize (also on a hipEventBlockingSync event)
    // poll with the default scheduling policy -- 100 % of a core in all three forms (scripts/gpu_wait_modes.py) --
    // and hipSetDeviceFlags(BlockingSync) is not this library's to set in a host process.  So: sleep for most of
    // what the last batches took (clock_nanosleep), then poll the completion word; the estimate follows the
    // workload (an EMA of the wait just observed).  MEMEX_HIP_SPIN=1 (bench.py sets it) polls from the start.
    static const bool no_spin = [] {
        const char *sp = getenv("MEMEX_HIP_SPIN");
        return !(sp && sp[0] == '1');
    }();
    const auto t0 = std::chrono::steady_clock::now();
    double &ema = idx->wait_ema_us[B <= 32 ? 0 : B <= 128 ? 1 : B <= 256 ? 2 : 3];
    bool overslept = false;  // the batch was already complete when the nap ended: the estimate is too long
    if (no_spin && ema > 150.0) {
        const double nap_us = 0.8 * ema - 60.0;  // timer slack and wake-up latency stay inside the estimate
        if (nap_us > 50.0) {
            struct timespec ts;
            ts.tv_sec = (time_t)(nap_us / 1e6);
            ts.tv_nsec = (long)((nap_us - (double)ts.tv_sec * 1e6) * 1e3);
            (void)clock_nanosleep(CLOCK_MONOTONIC, 0, &ts, nullptr);
            overslept = __atomic_load_n(&s.host_sum[4], __ATOMIC_ACQUIRE) == seq;
        }
    }
    bool done = false;
    for (unsigned spins = 1;; ++spins) {
        if (__atomic_load_n(&s.host_sum[4], __ATOMIC_ACQUIRE) == seq) {
            done = true;
            break;
        }
        if ((spins & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
        __builtin_ia32_pause();
    }
    if (done) {
        // what was observed includes the nap: when the batch had finished before the nap did (batches got faster: a
        // cleared or smaller index, another k) only an upper bound is known, so the estimate is halved instead of
        // creeping down 5 % per batch
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        ema = overslept ? 0.5 * ema : ema > 0.0 ? 0.75 * ema + 0.25 * us : us;
        return MX_OK;
    }
    MX_HIP(hipStreamSynchronize(idx->stream));  // a kernel that never signals (fault): the synchronize reports it
    if (__atomic_load_n(&s.host_sum[4], __ATOMIC_ACQUIRE) == seq) return MX_OK;
    return fail(MX_EDEVICE, "finish_kernel did not signal completion");
}

// ---- what search_batch and range_batch share: the geometry of a batch and the parameter blocks of its launches ------------------
// The geometry of one batch of B queries: which scan serves it, with how many workgroups and lane-buffer sets, and where it has to be
// split.  It follows from the index state, B and the kind of search alone; `trivial` (nothing can be found) is the caller's own rule.
enum class BatchKind { kTopK, kRange };
struct BatchPlan {
    bool filt8;     // 8-bit copy: 256 queries per pass at every width
    bool wide;      // wide rows (768 < dim_pad <= 1536) have their own scan kernel over the bf16 copy: 128 queries per pass
    bool fast;      // the scan pipeline answers the batch; otherwise the EXACT path does
    bool centred8;  // a centred int8 copy: passes of 256 (the two-group variant has no register left for the per-row epilogue)
    bool centred;   // the copy is centred on its rows' mean direction (build_filter_copy): queries are split the same way
    bool x2;        // more than 256 queries as ONE pass of the int8 scan with two query groups per wave (up to 512 dims)
    bool pair;      // 129-256 queries on a plain int8 copy up to 512 dims: two 4-wave workgroups per CU with two query groups per wave
                    // (DESIGN.md section 3.2e).  Smaller batches stay on the 8-wave form, whose idle waves skip their MFMAs.
    int nwg;        // workgroups of the scan launches; finish_kernel and theta_kernel follow
    int lanes;      // lane-buffer sets per workgroup (LaneLease::take): 2 for x2 and for pair (2 x nwg workgroups x 512 lanes)
    Scan8Geom geom;
    int split;      // 0: one pass serves the batch; else the batch is answered as [0, split) and the rest (kPassBatch or kWideBatch)
    uint64_t trows;      // rows per scan tile
    int bytes_per_elem;  // of what the scan streams
};

BatchPlan plan_batch(const mx_index *idx, int B, int k_or_cap, BatchKind kind, bool trivial) {
    BatchPlan pl;
    pl.filt8 = idx->xh != nullptr && idx->filter_i8 && !idx->compressed;
    pl.wide = idx->kc > kMaxKC && !pl.filt8;
    // (a range search has no k > 256 rule: its lists are cut from what the pass collects, whatever the cap)
    pl.fast = !trivial && idx->mode == MX_SEARCH_AUTO && (idx->kc > kMaxKC ? idx->xh != nullptr && idx->kc <= kMaxKC16 : true) &&
              (!idx->compressed || idx->wild_rows == 0) && (kind == BatchKind::kRange || k_or_cap <= 256) &&
              idx->n_zero <= (uint64_t)kZeroCap && idx->n_wild <= (uint64_t)kWildCap;
    pl.centred8 = idx->centred && pl.filt8 && idx->amean && idx->mean && idx->kc <= kMaxKC;
    const bool two_groups = pl.fast && pl.filt8 && !pl.centred8 && idx->kc <= kMaxKC8x2;
    pl.x2 = two_groups && B > kPassBatch;
    pl.pair = two_groups && B > kPassBatch / 2 && B <= kPassBatch && idx->scan8_pair;
    pl.centred = pl.centred8 || (idx->centred && idx->xh && !pl.filt8 && !pl.wide && !idx->compressed && idx->amean && idx->mean && idx->kc <= kMaxKC);
    pl.nwg = pl.pair ? 2 * idx->nwg : idx->nwg;
    pl.lanes = pl.x2 || pl.pair ? 2 : 1;
    pl.geom = pl.pair ? Scan8Geom::kPair : pl.x2 ? Scan8Geom::k512 : Scan8Geom::k256;
    pl.split = B > kPassBatch && !pl.x2 && !(pl.fast && pl.wide) ? kPassBatch : pl.fast && pl.wide && B > kWideBatch ? kWideBatch : 0;
    pl.trows = pl.filt8 ? kTile8Rows : kTileRows;
    pl.bytes_per_elem = pl.filt8 ? 1 : idx->xh ? 2 : 4;
    return pl;
}

int prep_queries(mx_index *idx, const BatchPlan &pl, const float *d_q, int B) {
    Scratch &s = idx->s;
    MX_HIP(launch_prep_queries(idx->stream, d_q, B, idx->dim, idx->ds, s.qfrag, s.qpad, s.qnorm2, s.theta, s.e1,
                               idx->xh ? idx->flags + 2 : nullptr, s.overflow, s.qflags, s.qa, s.qb, pl.filt8, s.qscale,
                               pl.centred ? idx->mean : nullptr, s.qmean, pl.centred8 ? idx->flags + 5 : nullptr));
    return MX_OK;
}

// the plain int8 copy of an f32 corpus, unless switched off: the sample launch names the rows behind its lane maxima and theta_kernel
// rescores the best of them (every geometry of scan8_kernel; the centred copy keeps the lane maxima alone)
bool exact_theta_for(const mx_index *idx, const BatchPlan &pl) { return idx->exact_theta && pl.filt8 && !pl.centred8 && idx->x != nullptr; }

// everything of a scan launch but its tiles (tile_begin / tile_end / tile_stride: the caller's, per launch); mask: ScanParams::dead
void fill_scan_params(ScanParams &p, const mx_index *idx, const BatchPlan &pl, int B, const uint64_t *mask) {
    const Scratch &s = idx->s;
    p.x = idx->x;
    p.xh = idx->xh;
    p.scale = idx->scale;
    p.qfrag = s.qfrag;
    p.theta = s.theta;
    p.n_rows = idx->n;
    p.ds = (uint32_t)idx->ds;
    p.wave_mask = (1u << ((B + 31) / 32)) - 1u;  // waves whose 32 columns are all padding skip their MFMAs
    p.lane_rec = s.lane_rec;
    p.lane_tile = s.lane_tile;
    p.lane_cnt = s.lane_cnt;
    p.lane_max = s.lane_max;
    p.lane_arg = exact_theta_for(idx, pl) ? s.lane_arg : nullptr;
    p.overflow = s.overflow;
    p.tscale = idx->tsc;
    p.qscale = s.qscale;
    p.qa = s.qa;
    p.qb = s.qb;
    p.amean = pl.centred ? idx->amean : nullptr;
    p.qmean = s.qmean;
    p.dead = mask;  // the masked kernels only for an index with removed rows, or a filtered search
}

hipError_t launch_scan_for(const mx_index *idx, const BatchPlan &pl, bool collect, const ScanParams &p) {
    if (pl.filt8) return launch_scan8(idx->stream, idx->kc, collect, pl.nwg, p, pl.geom);
    if (pl.wide) return launch_scan16w(idx->stream, idx->kc, collect, pl.nwg, p);
    return idx->xh ? launch_scan16(idx->stream, idx->kc, collect, pl.nwg, p) : launch_scan(idx->stream, idx->kc, collect, pl.nwg, p);
}

// The finish launch of a batch over all rows: k (or the cap), the mask and what it leaves, and the outputs are the caller's; so is
// what it sets afterwards (the retry pass's todo, max_err when profiling, no rows for a batch that can find nothing) and seq.
void fill_finish_params(FinishParams &fp, const mx_index *idx, const BatchPlan &pl, int B, int k, const uint64_t *mask, uint64_t n_live,
                        uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_nfound) {
    const Scratch &s = idx->s;
    fp.k = k;
    fp.ds = idx->ds;
    fp.nwg = pl.nwg;
    fp.serial = idx->serial;
    fp.x = idx->compressed ? nullptr : idx->x;
    fp.xh = idx->xh;
    fp.scale = idx->scale;
    fp.n_rows = idx->n;
    fp.idmap = idx->idmap;
    fp.qpad = s.qpad;
    fp.qnorm2 = s.qnorm2;
    fp.e1 = s.e1;
    fp.qa = s.qa;
    fp.qb = s.qb;
    fp.terr = pl.filt8 ? idx->tsc : nullptr;
    fp.e2 = (float)(idx->ds + 8) * 5.9604645e-8f + 1e-6f;  // f32 fma dot of <= ds terms of unit vectors, any order
    fp.lane_rec = s.lane_rec;
    fp.rec_int = pl.filt8 ? 1 : 0;
    fp.qscale = s.qscale;
    fp.lane_tile = s.lane_tile;
    fp.lane_cnt = s.lane_cnt;
    fp.theta = s.theta;
    fp.zero_rows = idx->zero_rows;
    fp.n_zero = (uint32_t)std::min<uint64_t>(idx->n_zero, kZeroCap);
    fp.wild_rows = idx->wild_list;
    fp.n_wild = (uint32_t)std::min<uint64_t>(idx->n_wild, kWildCap);
    fp.dead = mask;
    fp.n_live = n_live;
    fp.overflow = s.overflow;
    fp.todo = nullptr;
    fp.theta_retry = s.theta_retry;
    fp.cand_cnt = s.cand_cnt;
    fp.ids = d_ids;
    fp.scores = d_scores;
    fp.dists = d_dists;
    fp.n_found = d_nfound;
    fp.max_err = nullptr;
    fp.done_ctr = s.done_ctr;
    fp.dev_flags = s.dev_flags;
    fp.host_flags = s.host_sum;
    fp.n_queries = B;
    fp.host_out = s.out_on_host ? 1 : 0;
}

// the per-query flag words of the batch, host-synchronised (overflowed batches, the EXACT path and the subset kernel only)
int fetch_flags(mx_index *idx) {
    MX_HIP(hipMemcpyAsync(idx->s.host_flags, idx->s.dev_flags, kFlagWords * sizeof(uint32_t), hipMemcpyDeviceToHost, idx->stream));
    MX_HIP(hipStreamSynchronize(idx->stream));
    return MX_OK;
}

// a large exact scratch does not stay behind a fallback batch (the stream is idle)
void drop_large_exact_scratch(mx_index *idx) {
    if (idx->mode != MX_SEARCH_AUTO || idx->s.exact_bytes <= kExactKeepBytes) return;
    idx->s.exact_scratch.reset();
    idx->s.exact_bytes = 0;
}

// one batch (B <= 256) with queries and outputs on the device; filt: what a filtered search allows -- local rows (normalised
// ranges), or this index's shard of a resident filter
int search_batch(mx_index *idx, const float *d_q, int B, int k, uint64_t *d_ids, float *d_scores, float *d_dists,
                 int32_t *d_nfound, const FilterArg *filt = nullptr) {
    int rc = ensure_scratch(idx);
    if (rc != MX_OK) return rc;
    Scratch &s = idx->s;
    hipStream_t st = idx->stream;
    // a filtered batch: its ranges clipped to the rows, and the rows they allow that are not removed
    Ranges fr;
    uint64_t n_allow = 0, span_lo = 0, span_hi = 0;  // [span_lo, span_hi): from the first allowed row to the last
    FilterShard *res = filt && filt->res ? &filt->res->sh[(size_t)filt->shard] : nullptr;
    if (res) {  // a resident filter: nothing here grows with the rows or the ranges while the cached figures hold
        refresh_filter_shard(idx, *res);
        n_allow = res->n_live;
        span_lo = res->row_lo;
        span_hi = res->row_hi;
    } else if (filt) {
        for (const auto &x : *filt->ranges)
            if (x.first < std::min(x.second, idx->n)) fr.emplace_back(x.first, std::min(x.second, idx->n));
        n_allow = count_allowed(idx, fr);
        if (!fr.empty()) {
            span_lo = fr.front().first;
            span_hi = fr.back().second;
        }
    }
    idx->last_subset = false;
    const bool trivial = idx->n == 0 || k == 0 || (filt && n_allow == 0);
    if (idx->compressed && idx->kc > kMaxKC16 && !trivial)
        return fail(MX_EUNSUPPORTED, "a compressed corpus supports dim <= %d", kMaxKC16 * kChunkFloats);
    const BatchPlan pl = plan_batch(idx, B, k, BatchKind::kTopK, trivial);
    if (pl.split) {
        rc = search_batch(idx, d_q, pl.split, k, d_ids, d_scores, d_dists, d_nfound, filt);
        if (rc != MX_OK) return rc;
        const size_t o = (size_t)pl.split * k;
        return search_batch(idx, d_q + (size_t)pl.split * idx->dim, B - pl.split, k, d_ids + o, d_scores + o,
                            d_dists ? d_dists + o : nullptr, d_nfound + pl.split, filt);
    }
    const uint32_t *h_ovf = s.host_flags, *h_qfl = s.host_flags + 3 * kMaxBatch;
    auto any_bad_query = [&] {
        uint32_t bad = 0;
        for (int b = 0; b < B; ++b) bad |= h_qfl[b];
        return bad != 0;
    };
    if (filt && !trivial && subset_pays(idx, B, n_allow, span_hi - span_lo, pl.bytes_per_elem)) {
        // a small filter: the allowed live rows, ascending, and one subset_topk_kernel launch; no scan, no lane buffers
        std::vector<uint32_t> list;
        const uint32_t *rows_list = nullptr;
        if (res) {  // the filter's own list, compacted on the device and kept until the filter or the removals change
            if (!res->list) MX_HIP(res->list.alloc((size_t)kSubsetCap));
            if (!res->list_ok) {
                MX_HIP(hipMemsetAsync(res->list, 0, (size_t)kSubsetCap * sizeof(uint32_t), st));  // (no entry is ever an arbitrary row)
                MX_HIP(launch_filter_list(st, idx->n_dead ? idx->dead : nullptr, res->bits, span_lo >> 6, (span_hi + 63) >> 6, res->list,
                                          (uint32_t)kSubsetCap));
                res->list_ok = true;
            }
            rows_list = res->list;
        } else {
            list.reserve((size_t)n_allow);
            for (const auto &x : fr)
                for (uint64_t r = x.first; r < x.second; ++r)
                    if (!idx->n_dead || !((idx->dead_h[r >> 6] >> (r & 63)) & 1ull)) list.push_back((uint32_t)r);
            if (!idx->subset_rows) MX_HIP(idx->subset_rows.alloc((size_t)kSubsetCap));
            MX_HIP(hipMemcpyAsync(idx->subset_rows, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            rows_list = idx->subset_rows;
        }
        if ((rc = prep_queries(idx, pl, d_q, B)) != MX_OK) return rc;
        MX_HIP(launch_subset_topk(st, B, k, idx->ds, idx->compressed ? nullptr : idx->x, idx->xh, rows_list, (uint32_t)n_allow,
                                  idx->idmap, s.qpad, s.qnorm2, d_ids, d_scores, d_dists, d_nfound));
        if ((rc = fetch_flags(idx)) != MX_OK) return rc;  // (host-synchronised: also for outputs in mapped host memory)
        if (any_bad_query()) return fail(MX_EINVAL, "a query contains non-finite values");
        idx->last_subset = true;
        idx->stats.searches += 1;
        idx->stats.queries += (uint64_t)B;
        idx->stats.filtered_queries += (uint64_t)B;
        idx->stats.subset_queries += (uint64_t)B;
        return MX_OK;
    }
    // what masks the pipeline: the per-call mask of a filtered search, the removed rows, or nothing; the rows it leaves
    std::vector<uint64_t> flat_ranges;  // (alive until the batch is host-synchronised: the source of an async upload)
    if (filt && !trivial && (rc = res ? apply_filter_mask(idx, *res) : build_filter_mask(idx, fr, flat_ranges)) != MX_OK) return rc;
    const uint64_t *mask = filt ? idx->filt : idx->n_dead ? idx->dead : nullptr;
    const uint64_t n_live = filt ? n_allow : idx->n - idx->n_dead;
    LaneLease lease;  // every return below is host-synchronised with the kernels that used the lane buffers
    if ((rc = lease.take(idx, pl.lanes)) != MX_OK) return rc;
    if ((rc = prep_queries(idx, pl, d_q, B)) != MX_OK) return rc;
    bool timed = false;
    bool crowded = false;  // the plain int8 copy sent too many rows to the f32 stage (below)

    FinishParams fp;
    fill_finish_params(fp, idx, pl, B, k, mask, n_live, d_ids, d_scores, d_dists, d_nfound);
    if (trivial) fp.n_rows = fp.n_live = 0;
    // (nothing to find: finish_kernel writes the blanks and leaves before it stages the query, so rows wider than every scan ask for the
    // widest query the kernel's LDS limit was raised for, not for their own)
    if (trivial) fp.ds = std::min(fp.ds, kMaxKC16 * kChunkFloats);
    fp.max_err = idx->profiling ? s.max_err : nullptr;
    // finish + completion: the kernel's last workgroup writes the batch summary into pinned host memory and
    // stores the launch's sequence number behind it; the host spins on that word (no D2H copy command and no
    // memset between batches: the host gap between two batches drops from 45 to 22 us, the kernel grows by
    // 8: scripts/r2_step_gaps.sh; waiting in hipStreamSynchronize is as fast, see MEMEX_HIP_SPIN below).  A kernel that never signals (fault) is
    // caught by the synchronize after the spin budget.  -> the summary's overflow code
    auto finish_and_wait = [&]() -> int {
        fp.seq = ++s.flag_seq;
        MX_HIP(launch_finish(st, B, fp));
        return await_finish(idx, B, fp.seq);
    };
    std::vector<int> exact;
    if (trivial) {
        fp.seq = ++s.flag_seq;
        MX_HIP(launch_finish(st, B, fp));  // n_found = 0, empty slots
    } else if (pl.fast) {
        const uint64_t tiles = (idx->n + pl.trows - 1) / pl.trows, full = idx->n / pl.trows;
        // the tiles the scans visit: all of them, or the span of tiles a filter's ranges touch (the sample: its full tiles)
        const uint64_t ts0 = filt ? span_lo / pl.trows : 0, ts1 = filt ? (span_hi + pl.trows - 1) / pl.trows : tiles;
        const uint64_t full1 = std::min(ts1, full);
        ScanParams p;
        fill_scan_params(p, idx, pl, B, mask);
        auto collect = [&](bool first) -> int {
            p.tile_begin = (uint32_t)ts0;
            p.tile_end = (uint32_t)ts1;
            p.tile_stride = 1;
            // the first collect launch of a batch is the one the roofline is quoted on
            if (first && idx->profiling) MX_HIP(hipEventRecord(idx->ev0, st));
            MX_HIP(launch_scan_for(idx, pl, true, p));
            if (first && idx->profiling) {
                MX_HIP(hipEventRecord(idx->ev1, st));
                timed = true;
            }
            if (first) {
                idx->stats.scan_launches += 1;
                idx->stats.scan_bytes += (ts1 - ts0) * pl.trows * idx->ds * (uint64_t)pl.bytes_per_elem;
            }
            return MX_OK;
        };
        // a lane holds 16 scores per tile of its workgroup: up to 2 tiles per workgroup everything fits
        // in the lane buffers and no threshold is needed (counted per CU: the two-workgroup form samples the same corpora)
        if (ts1 - ts0 > 2ull * idx->nwg) {
            p.tile_begin = (uint32_t)ts0;
            p.tile_end = (uint32_t)full1;
            const bool exact_theta = exact_theta_for(idx, pl);
            p.tile_stride = sample_stride(full1 - ts0, pl.nwg, k, pl.filt8, idx->ds, exact_theta, idx->sample_div);
            MX_HIP(launch_scan_for(idx, pl, false, p));
            const ThetaExact tx{s.lane_arg, idx->x, idx->scale, s.qpad, s.qnorm2, idx->n, idx->ds, fp.e2};
            MX_HIP(launch_theta(st, B, k, pl.nwg, s.lane_max, s.qa, !pl.filt8, s.theta, exact_theta ? &tx : nullptr));
        }
        if ((rc = collect(true)) != MX_OK) return rc;
        if ((rc = finish_and_wait()) != MX_OK) return rc;
        if (idx->print_records) {  // measurement only: what the collect launch wrote, summed over the lanes (the stats do not carry it)
            std::vector<uint32_t> cnt((size_t)pl.nwg * kScanThreads * (pl.x2 ? 2 : 1));
            MX_HIP(hipMemcpy(cnt.data(), s.lane_cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint64_t rec = 0;
            for (const uint32_t c : cnt) rec += std::min<uint32_t>(c, (uint32_t)kRecCap);
            fprintf(stderr, "memex_hip: collect records %llu queries %d serial %d\n", (unsigned long long)rec, B, fp.serial);  // (serial: what finish_kernel was given)
        }
        if (timed) {
            float ms = 0.f;
            MX_HIP(hipEventElapsedTime(&ms, idx->ev0, idx->ev1));
            idx->stats.scan_ms += ms;
            timed = false;
        }
        if (s.host_sum[2]) return fail(MX_EINVAL, "a query contains non-finite values");
        idx->stats.candidates += s.host_sum[1];
        // The exact threshold keeps a plain int8 copy from overflowing on corpora whose certificate is nevertheless too wide: a cone
        // with cosines spread by 0.012 used to overflow finish_kernel's candidate list and was rebuilt centred for it (below); now it
        // fits, and 3000 rows per query reach the f32 stage where the centred copy sends 130.  So an automatic plain copy is also
        // rebuilt centred when a batch that fitted rescored more than 64 (k + 6) rows per query in f32 (four times the headline's
        // 250 at k = 10, twice the clustered and anisotropic corpora's 500) -- once per doubling of the index, after the batch is answered.
        crowded = !s.host_sum[0] && !filt && idx->filter_auto && exact_theta_for(idx, pl) && !idx->centred && idx->kc <= kMaxKC &&
                  idx->n >= 256 && idx->n >= 2 * idx->crowded_at_rows && (uint64_t)s.host_sum[1] > (uint64_t)B * 64u * (uint64_t)(k + 6);
        if (s.host_sum[0]) {
            if ((rc = fetch_flags(idx)) != MX_OK) return rc;
            int retry = 0;
            for (int b = 0; b < B; ++b) {
                if (h_ovf[b] == 1) ++retry;
                else if (h_ovf[b] >= 2) exact.push_back(b);
            }
            // (a filtered batch leaves the copy heuristics alone: a selective filter's overflows say nothing about the corpus)
            if (pl.filt8 && !filt) idx->i8_retry_batches += 1;
            // ... or the retry pass (a second whole scan) has become the rule: more than a quarter of the batches
            const bool habitual = pl.filt8 && idx->i8_batches >= 8 && idx->i8_retry_batches * 4 > idx->i8_batches;
            if (pl.filt8 && !filt && idx->filter_auto && ((size_t)(retry + (int)exact.size()) * 16 > (size_t)std::max(B, 16) || habitual)) {
                // More than 1/16 of the batch (and more than one query) did not fit the int8 pass: this corpus is too dense for the int8
                // certificate (neighbourhoods narrower than ~0.05 in cosine).  Rebuild the copy as bf16 (one pass
                // over the f32 rows) and answer the batch on it; the index stays on bf16.
                // Round 6: first the same copy CENTRED on the rows' mean direction (section 3.2c carried over to int8: what an encoder
                // produces sits in a cone, and the quantisation error of the short residual vectors is several times smaller); only
                // a corpus without a cone, or one that overflows the centred copy as well, goes to bf16.
                if (!idx->centred && idx->kc <= kMaxKC && idx->n >= 256) {
                    const std::string keep = last_error_slot();
                    if (build_filter_copy(idx, true) == MX_OK && idx->centred) {
                        lease.drop();
                        return search_batch(idx, d_q, B, k, d_ids, d_scores, d_dists, d_nfound);
                    }
                    last_error_slot() = keep;
                }
                const int drc = demote_filter(idx);
                if (drc == MX_OK) {
                    idx->stats.filter_demotions += 1;
                    lease.drop();
                    return search_batch(idx, d_q, B, k, d_ids, d_scores, d_dists, d_nfound);
                }
                if (drc != MX_ENOMEM) return drc;  // (no room for the wider copy: the batch finishes on int8 below)
            }
            if (retry) {
                // ONE more pass for all overflowed queries of the batch, with the threshold finish derived
                // from what they did collect (everyone else is parked at theta = +inf)
                idx->stats.retry_queries += (uint64_t)retry;
                p.wave_mask = 0;  // only the waves that hold a rescanned query multiply: the pass runs at the stream's rate
                for (int b = 0; b < B; ++b)
                    if (h_ovf[b] == 1) p.wave_mask |= 1u << (b >> 5);
                MX_HIP(launch_retry_setup(st, s.theta, s.theta_retry, s.overflow, s.todo));
                if ((rc = collect(false)) != MX_OK) return rc;
                fp.todo = s.todo;
                if ((rc = finish_and_wait()) != MX_OK) return rc;
                exact.clear();
                if (s.host_sum[0]) {
                    if ((rc = fetch_flags(idx)) != MX_OK) return rc;
                    for (int b = 0; b < B; ++b)
                        if (h_ovf[b] != 0) exact.push_back(b);
                }
            }
        }
        idx->stats.fallback_queries += exact.size();
    } else {
        if ((rc = fetch_flags(idx)) != MX_OK) return rc;
        if (any_bad_query()) return fail(MX_EINVAL, "a query contains non-finite values");
        for (int b = 0; b < B; ++b) exact.push_back(b);
    }
    if (!exact.empty() || trivial || !pl.fast) {
        rc = run_exact(idx, exact, k, d_ids, d_scores, d_dists, d_nfound, mask, n_live);
        if (rc != MX_OK) return rc;
        MX_HIP(hipStreamSynchronize(st));
        drop_large_exact_scratch(idx);
    }
    // (fast path with nothing left to do: finish_kernel's completion word was stored after every result of
    // the batch had been fenced to device scope -- the results are in HBM, nothing else is queued)
    idx->stats.searches += 1;
    idx->stats.queries += (uint64_t)B;
    if (filt) idx->stats.filtered_queries += (uint64_t)B;
    if (pl.filt8 && pl.fast && !filt) idx->i8_batches += 1;
    if (crowded) {  // (the batch is answered; a corpus without a cone gets its plain copy back, and no second try until it has doubled)
        idx->crowded_at_rows = idx->n;
        const std::string keep = last_error_slot();
        lease.drop();
        if (build_filter_copy(idx, true) != MX_OK) last_error_slot() = keep;
    }
    return MX_OK;
}

// ---- range search (mx_index_search_range) -----------------------------------------------------------------
// Score of a dist, exactly as the device computes it (score_from_dist) and as the reference reports it: f32 1 / (1 / d), 1 - that
float host_score_from_dist(float d) {
    const volatile float t = 1.0f / d;  // (volatile: each rounding to f32 happens, whatever the host compiler keeps in registers)
    const volatile float u = 1.0f / t;
    return 1.0f - u;
}

// The threshold t as a dist bound: score is a non-increasing function of the f32 dist (three monotone roundings), so "score >= t" is
// "dist <= D(t)" with D(t) the largest f32 in [0, 4] whose score reaches t -- found by bisection over the bit patterns, which order the
// non-negative floats.  Returned as bits(D) + 1 (in range <=> bits(dist) < it); 0 when t > 1 selects nothing.  t must not be NaN.
uint32_t range_dist_limit(float t) {
    if (!(t <= 1.0f)) return 0;                // score(0) = 1 is the largest score
    uint32_t lo = 0, hi = 0x40800000u;         // score(bits lo) >= t holds; 4.0 is past every dist (cos >= -1 - 2^-22)
    if (host_score_from_dist(4.0f) >= t) return hi + 1;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        float d;
        memcpy(&d, &mid, sizeof d);
        if (host_score_from_dist(d) >= t) lo = mid;
        else hi = mid;
    }
    return lo + 1;
}

// |cos - (1 - dist)| of the reference's chain on f32 rows: f32 products (relative 2^-24 each), f64 sums (ds 2^-53), the f64 sqrt /
// divide / subtract (a few 2^-53), then the f32 rounding of dist (at most 2^-24 below 2, 2^-23 up to 4): at most 2^-22 + 2^-23 + ...
// for |cos| <= 1.  kRangeEps = 2^-20 leaves room for the f32 arithmetic of the bounds it is combined with.
constexpr float kRangeEps = 9.5367431640625e-7f;

// EXACT range path for the queries qs of the batch
int run_exact_range(mx_index *idx, const std::vector<int> &qs, int cap, uint64_t *d_ids, float *d_scores, float *d_dists,
                    int32_t *d_nfound, uint64_t *d_nrange, const uint64_t *mask, uint64_t n_live) {
    if (qs.empty()) return MX_OK;
    int gcap = qs.size() <= 4 ? 4 : qs.size() <= 8 ? 8 : qs.size() <= 16 ? 16 : kExactGroup;
    int rc = ensure_exact(idx, cap, &gcap);
    if (rc != MX_OK) return rc;
    Scratch &s = idx->s;
    for (size_t g0 = 0; g0 < qs.size(); g0 += (size_t)gcap) {
        ExactGroup grp{};
        grp.n = (int)std::min<size_t>((size_t)gcap, qs.size() - g0);
        for (int j = 0; j < grp.n; ++j) grp.q[j] = qs[g0 + j];
        MX_HIP(launch_exact_range_group(idx->stream, cap, idx->ds, idx->compressed ? nullptr : idx->x, idx->xh, idx->n, idx->idmap, s.qpad,
                                        s.qnorm2, grp, s.exact_scratch, s.rlim, d_ids, d_scores, d_dists, d_nfound, d_nrange, mask, n_live));
    }
    return MX_OK;
}

// one range batch (B <= 512) with queries and outputs on the device; dlim: the B dist bounds (host memory).  The top-k pipeline minus
// the sample and theta launches: theta follows from the caller's threshold (launch_range_theta), one collect launch over every tile with
// the geometry of the shared plan (plan_batch: what search_batch runs for B), range_finish_kernel.  No retry pass; its overflows and
// everything search_batch sends to the EXACT path (but k > 256) take the EXACT range path.  The filter copy's heuristics are left alone.
int range_batch(mx_index *idx, const float *d_q, int B, int cap, const uint32_t *dlim, uint64_t *d_ids, float *d_scores, float *d_dists,
                int32_t *d_nfound, uint64_t *d_nrange) {
    int rc = ensure_scratch(idx);
    if (rc != MX_OK) return rc;
    Scratch &s = idx->s;
    hipStream_t st = idx->stream;
    const uint64_t n_live = idx->n - idx->n_dead;
    const bool trivial = idx->n == 0 || n_live == 0;
    if (idx->compressed && idx->kc > kMaxKC16 && !trivial)
        return fail(MX_EUNSUPPORTED, "a compressed corpus supports dim <= %d", kMaxKC16 * kChunkFloats);
    const BatchPlan pl = plan_batch(idx, B, cap, BatchKind::kRange, trivial);
    if (pl.split) {
        rc = range_batch(idx, d_q, pl.split, cap, dlim, d_ids, d_scores, d_dists, d_nfound, d_nrange);
        if (rc != MX_OK) return rc;
        const size_t o = (size_t)pl.split * cap;
        return range_batch(idx, d_q + (size_t)pl.split * idx->dim, B - pl.split, cap, dlim + pl.split, d_ids + o, d_scores + o,
                           d_dists ? d_dists + o : nullptr, d_nfound + pl.split, d_nrange + pl.split);
    }
    const uint32_t *h_ovf = s.host_flags, *h_qfl = s.host_flags + 3 * kMaxBatch;
    const uint64_t *mask = idx->n_dead ? idx->dead : nullptr;
    LaneLease lease;
    if (pl.fast && (rc = lease.take(idx, pl.lanes)) != MX_OK) return rc;
    MX_HIP(hipMemcpyAsync(s.rlim, dlim, (size_t)B * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if ((rc = prep_queries(idx, pl, d_q, B)) != MX_OK) return rc;
    std::vector<int> exact;
    if (pl.fast) {
        MX_HIP(launch_range_theta(st, B, s.rlim, kRangeEps, s.qa, s.theta));
        const uint64_t tiles = (idx->n + pl.trows - 1) / pl.trows;
        ScanParams p;
        fill_scan_params(p, idx, pl, B, mask);
        p.tile_begin = 0;
        p.tile_end = (uint32_t)tiles;
        p.tile_stride = 1;
        MX_HIP(launch_scan_for(idx, pl, true, p));
        idx->stats.scan_launches += 1;
        idx->stats.scan_bytes += tiles * pl.trows * idx->ds * (uint64_t)pl.bytes_per_elem;

        RangeParams rp;
        FinishParams &fp = rp.f;
        fill_finish_params(fp, idx, pl, B, cap, mask, n_live, d_ids, d_scores, d_dists, d_nfound);
        fp.seq = ++s.flag_seq;
        rp.dlim = s.rlim;
        rp.eps = kRangeEps;
        rp.n_in_range = d_nrange;
        MX_HIP(launch_range_finish(st, B, rp));
        if ((rc = await_finish(idx, B, fp.seq)) != MX_OK) return rc;
        if (s.host_sum[2]) return fail(MX_EINVAL, "a query contains non-finite values");
        idx->stats.candidates += s.host_sum[1];
        if (s.host_sum[0]) {
            if ((rc = fetch_flags(idx)) != MX_OK) return rc;
            for (int b = 0; b < B; ++b)
                if (h_ovf[b] != 0) exact.push_back(b);
        }
        idx->stats.fallback_queries += exact.size();
    } else {
        if ((rc = fetch_flags(idx)) != MX_OK) return rc;
        for (int b = 0; b < B; ++b)
            if (h_qfl[b]) return fail(MX_EINVAL, "a query contains non-finite values");
        for (int b = 0; b < B && !trivial; ++b) exact.push_back(b);
        if (trivial) {  // nothing in range: empty lists, zero counts
            MX_HIP(hipMemsetAsync(s.rlim, 0, (size_t)B * sizeof(uint32_t), st));
            RangeParams rp{};
            rp.f.k = cap;
            rp.f.ds = std::min(idx->ds, kMaxKC16 * kChunkFloats);  // (the blanks alone: the query is never staged, as in search_batch)
            rp.f.x = idx->x;
            rp.f.ids = d_ids;
            rp.f.scores = d_scores;
            rp.f.dists = d_dists;
            rp.f.n_found = d_nfound;
            rp.f.cand_cnt = s.cand_cnt;
            rp.dlim = s.rlim;
            rp.n_in_range = d_nrange;
            MX_HIP(launch_range_finish(st, B, rp));
        }
    }
    if (!exact.empty() || trivial) {
        rc = run_exact_range(idx, exact, cap, d_ids, d_scores, d_dists, d_nfound, d_nrange, mask, n_live);
        if (rc != MX_OK) return rc;
        MX_HIP(hipStreamSynchronize(st));
        drop_large_exact_scratch(idx);
    }
    idx->stats.searches += 1;
    idx->stats.queries += (uint64_t)B;
    return MX_OK;
}

// ---------------------------------------------------------------------------------------------
// composite: rows dealt block-cyclically to shard indexes (one per device), local top-k per shard,
// exchange of the packed [ids | dists] blocks (RCCL all-gather over xGMI, or peer copies), merge
// ---------------------------------------------------------------------------------------------
void sync_shard_streams(mx_index *idx) {
    for (mx_index *sh : idx->shards) {
        DeviceGuard dg(sh->device);
        if (sh->stream) (void)hipStreamSynchronize(sh->stream);
    }
}

// the same with a deadline (after a failed collective part of it may sit on some shard's stream and never complete):
// polls hipStreamQuery; false = a stream did not drain in time
bool sync_shard_streams_within(mx_index *idx, double seconds) {
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::duration<double>(seconds);
    for (mx_index *sh : idx->shards) {
        DeviceGuard dg(sh->device);
        if (!sh->stream) continue;
        for (;;) {
            const hipError_t e = hipStreamQuery(sh->stream);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) {
                (void)hipGetLastError();
                return false;
            }
            if (std::chrono::steady_clock::now() > t_end) return false;
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    }
    return true;
}

int ensure_composite_buffers(mx_index *idx, int k) {
    if (k <= idx->sh_kcap) return MX_OK;
    sync_shard_streams(idx);  // the last batch's all-gather may still be running on shards >= 1
    free_composite_buffers(idx);
    const int kc = std::max(k, 16);
    const size_t G = idx->shards.size();
    const size_t blk = (size_t)kMaxBatch * kc * 12 + kMaxBatch * sizeof(uint64_t);  // [ids | dists] (+ the counts of a range pass)
    idx->sh_block.resize(G); idx->sh_gather.resize(G); idx->sh_q.resize(G);
    idx->sh_scores.resize(G); idx->sh_nf.resize(G);
    for (size_t g = 0; g < G; ++g) {
        DeviceGuard dg(idx->shards[g]->device);
        MX_HIP(idx->sh_block[g].alloc_bytes(blk));
        if (g == 0 || idx->use_rccl) MX_HIP(idx->sh_gather[g].alloc_bytes(blk * G));
        MX_HIP(idx->sh_q[g].alloc((size_t)kMaxBatch * idx->dim));
        MX_HIP(idx->sh_scores[g].alloc((size_t)kMaxBatch * kc));
        MX_HIP(idx->sh_nf[g].alloc(kMaxBatch));
    }
    idx->sh_kcap = kc;
    return MX_OK;
}

// local row count of shard g when the composite holds `total` rows
uint64_t shard_rows(uint64_t total, uint64_t R, uint64_t G, uint64_t g) {
    const uint64_t full_blocks = total / R, tail = total % R;
    uint64_t rows = (full_blocks / G) * R + (g < full_blocks % G ? R : 0);
    if (full_blocks % G == g) rows += tail;
    return rows;
}

// peer copies between the shards' devices and shards[0]'s
void enable_peer_access(mx_index *idx) {
    for (size_t g = 1; g < idx->shards.size(); ++g) {
        if (idx->shards[g]->device == idx->shards[0]->device) continue;
        int can = 0;
        (void)hipDeviceCanAccessPeer(&can, idx->shards[0]->device, idx->shards[g]->device);
        if (can) {
            DeviceGuard dg(idx->shards[0]->device);
            (void)hipDeviceEnablePeerAccess(idx->shards[g]->device, 0);
            (void)hipGetLastError();
            DeviceGuard d2(idx->shards[g]->device);
            (void)hipDeviceEnablePeerAccess(idx->shards[0]->device, 0);
            (void)hipGetLastError();
        }
    }
}

// One tiny all-gather on throw-away streams, bounded by a deadline: a communicator that initialises but whose first
// collective fails or never completes (a first run on a new node) must cost a sharded index its RCCL exchange, not its
// searches.  false: do not use the communicators (a hung collective's streams and buffers are abandoned, not destroyed).
bool rccl_selftest(mx_index *idx, double seconds) {
    const int G = (int)idx->shards.size();
    std::vector<hipStream_t> st(G, nullptr);
    std::vector<Dev<unsigned char>> snd(G), rcv(G);
    bool ok = true;
    for (int g = 0; g < G && ok; ++g) {
        DeviceGuard dg(idx->shards[g]->device);
        ok = hipStreamCreateWithFlags(&st[g], hipStreamNonBlocking) == hipSuccess && snd[g].alloc(64) == hipSuccess &&
             rcv[g].alloc(64 * (size_t)G) == hipSuccess && hipMemsetAsync(snd[g], g + 1, 64, st[g]) == hipSuccess &&
             hipMemsetAsync(rcv[g], 0, 64 * (size_t)G, st[g]) == hipSuccess;
    }
    bool hung = false;
    if (ok) {
        int e = g_rccl.GroupStart();
        for (int g = 0; g < G && e == 0; ++g) e = g_rccl.AllGather(snd[g], rcv[g], 64, 1 /*ncclUint8*/, idx->comms[g], st[g]);
        const int e2 = g_rccl.GroupEnd();
        ok = e == 0 && e2 == 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < G && ok && !hung; ++g) {
            DeviceGuard dg(idx->shards[g]->device);
            for (;;) {
                const hipError_t q = hipStreamQuery(st[g]);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) {
                    ok = false;
                    break;
                }
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) {
                    hung = true;
                    break;
                }
                struct timespec ts = {0, 200 * 1000};
                (void)clock_nanosleep(CLOCK_MONOTONIC, 0, &ts, nullptr);
            }
        }
        if (ok && !hung) {
            std::vector<unsigned char> h(64 * (size_t)G);
            DeviceGuard dg(idx->shards[0]->device);
            ok = hipMemcpy(h.data(), rcv[0], h.size(), hipMemcpyDeviceToHost) == hipSuccess;
            for (int g = 0; g < G && ok; ++g) ok = h[64 * (size_t)g] == (unsigned char)(g + 1) && h[64 * (size_t)g + 63] == (unsigned char)(g + 1);
        }
    }
    if (hung) {
        fprintf(stderr, "memex-hip: the RCCL self-test did not complete within %.0f s; exchanging by peer copies\n", seconds);
        // the collective may still own the streams and buffers: leave them (the buffers move to a holder that is never freed)
        new std::pair<std::vector<Dev<unsigned char>>, std::vector<Dev<unsigned char>>>(std::move(snd), std::move(rcv));
        return false;
    }
    for (int g = 0; g < G; ++g) {
        DeviceGuard dg(idx->shards[g]->device);
        snd[g].reset();
        rcv[g].reset();
        if (st[g]) (void)hipStreamDestroy(st[g]);
    }
    (void)hipGetLastError();
    if (!ok) fprintf(stderr, "memex-hip: the RCCL self-test failed; exchanging by peer copies\n");
    return ok;
}

#ifdef MEMEX_TESTING
// libmemex_hip_testing.so only: the first all-gather of the process reports an error (one flag for every kind of search: not a static
// of the template below, which would have one per instantiation)
bool inject_all_gather_failure() {
    static std::atomic<bool> injected{false};
    return !injected.exchange(true);
}
#endif

// The part of a batch on a composite that does not depend on the kind of search.  Every shard takes the queries (d_q, on shards[0]'s
// device) and answers into its packed block -- local(g, shard, its queries, its block): ids [B, k] | dists [B, k] | whatever the caller
// keeps behind the lists, blk bytes in all -- the blocks meet in the gather area on shards[0]'s device (ONE RCCL all-gather over xGMI,
// or peer copies) and the lists are merged by (dist, id) into the caller's outputs; tail(stream) queues what the caller adds behind the
// merge.  Returns host-synchronised.  exchange = false: the blocks are empty, the shards run and nothing travels.
template <class Local, class Tail>
int exchange_and_merge(mx_index *idx, const float *d_q, int B, int k, size_t blk, bool exchange, uint64_t *d_ids, float *d_scores,
                       float *d_dists, Local &&local, Tail &&tail) {
    const int G = (int)idx->shards.size();
    const size_t ids_bytes = (size_t)B * k * sizeof(uint64_t);
    std::vector<int> rcs(G, MX_OK);
    std::vector<std::string> errs(G);
    auto shard = [&](int g) {
        mx_index *sh = idx->shards[g];
        std::lock_guard<std::mutex> lk(sh->mu);
        DeviceGuard dg(sh->device);
        auto run = [&]() -> int {
            MX_HIP(hipMemcpyAsync(idx->sh_q[g], d_q, (size_t)B * idx->dim * sizeof(float), hipMemcpyDefault, sh->stream));
            char *blkp = static_cast<char *>(idx->sh_block[g].get());
            int r = local(g, sh, idx->sh_q[g], blkp);
            if (r != MX_OK) return r;
            if (!idx->use_rccl && exchange) {  // peer copy into slot g of the gather area on shards[0]'s device
                MX_HIP(hipMemcpyAsync(static_cast<char *>(idx->sh_gather[0].get()) + (size_t)g * blk, blkp, blk, hipMemcpyDefault, sh->stream));
                MX_HIP(hipStreamSynchronize(sh->stream));
            }
            return MX_OK;
        };
        try {  // (a helper thread of the pool: an exception must not leave it)
            rcs[g] = run();
        } catch (...) {
            rcs[g] = guard_exception();
        }
        if (rcs[g] != MX_OK) errs[g] = last_error_slot();
    };
    // the query batch must be complete on shards[0]'s stream before other devices read it
    {
        DeviceGuard dg(idx->shards[0]->device);
        MX_HIP(hipStreamSynchronize(idx->shards[0]->stream));
    }
    if (idx->pool) {  // one persistent helper thread per shard >= 1 (shard_pool.h); shard 0 on this thread
        idx->pool->run(shard);
    } else {          // logical shards on one device: their streams would only take turns on the GPU anyway
        for (int g = 0; g < G; ++g) shard(g);
    }
    for (int g = 0; g < G; ++g)
        if (rcs[g] != MX_OK) {
            last_error_slot() = errs[g];
            return rcs[g];
        }
    mx_index *s0 = idx->shards[0];
    DeviceGuard dg(s0->device);
    const auto t_tail = std::chrono::steady_clock::now();  // every shard has answered: what follows is the step's serial tail
    if (exchange) {
        if (idx->use_rccl) {
            // ONE all-gather of blk bytes per shard over xGMI; every device receives all blocks, device 0 merges
            int e = 0, e2 = 0;
#ifdef MEMEX_TESTING
            if (inject_all_gather_failure()) {
                e = 1;
            } else
#endif
            {
                e = g_rccl.GroupStart();
                for (int g = 0; g < G && e == 0; ++g)
                    e = g_rccl.AllGather(idx->sh_block[g], idx->sh_gather[g], blk, 1 /*ncclUint8*/, idx->comms[g], idx->shards[g]->stream);
                e2 = g_rccl.GroupEnd();
            }
            if (e != 0 || e2 != 0) {
                // The collective could not be queued: this batch and every later one exchange by copies into the slots
                // of the gather area on shards[0]'s device (what an index without RCCL does from the start).  Every shard
                // is host-synchronised at this point (its batch returned), so the blocks are complete.
                fprintf(stderr, "memex-hip: RCCL all-gather failed (%s); the sharded index continues on peer copies\n",
                        g_rccl.GetErrorString && (e > 1 || e2) ? g_rccl.GetErrorString(e ? e : e2) : "error");
                // (part of the group may have been queued on some shard streams before the failure: wait with a deadline, and
                // give the batch up rather than hang the caller if a stream never drains)
                if (!sync_shard_streams_within(idx, 10.0))
                    return fail(MX_EDEVICE, "RCCL all-gather failed and a shard stream did not drain within 10 s");
                idx->use_rccl = false;
                idx->stats.exchange_fallbacks += 1;
                enable_peer_access(idx);
                for (int g = 0; g < G; ++g)  // (the shards left their blocks in place for the all-gather)
                    MX_HIP(hipMemcpyAsync(static_cast<char *>(idx->sh_gather[0].get()) + (size_t)g * blk, idx->sh_block[g], blk, hipMemcpyDefault, s0->stream));
            }
            // no host wait on shards >= 1: their part of the collective is ordered on their own streams (the
            // next batch's kernels queue behind it), and the merge below follows shard 0's part in stream order
        }
        const char *gat = static_cast<const char *>(idx->sh_gather[0].get());
        MX_HIP(launch_merge(s0->stream, gat, blk, gat + ids_bytes, blk, G, B, k, d_ids,
                            d_dists ? d_dists : reinterpret_cast<float *>(static_cast<char *>(idx->sh_block[0].get()) + ids_bytes), d_scores));
    }
    MX_HIP(tail(s0->stream));
    MX_HIP(hipStreamSynchronize(s0->stream));
    idx->stats.exchange_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tail).count();
    idx->stats.searches += 1;
    idx->stats.queries += (uint64_t)B;
    return MX_OK;
}

// one batch on a composite: d_q and the outputs live on shards[0]'s device
// filt: the global rows a filtered search allows (normalised): every shard searches its share of them (shard_ranges); or a
// resident filter: every shard searches with its own bitmap
int composite_batch(mx_index *idx, const float *d_q, int B, int k, uint64_t *d_ids, float *d_scores, float *d_dists,
                    int32_t *d_nfound, const FilterArg *filt = nullptr) {
    const int G = (int)idx->shards.size();
    int rc = ensure_composite_buffers(idx, std::max(k, 1));
    if (rc != MX_OK) return rc;
    std::vector<Ranges> loc(filt && !filt->res ? G : 0);
    std::vector<FilterArg> fa(filt ? G : 0);  // what shard g searches with
    std::vector<char> offers(filt ? G : 0, 0);  // shard g has allowed rows
    uint64_t n_allow = 0;  // allowed rows that are not removed, over the shards
    for (int g = 0; g < (int)loc.size(); ++g) {
        mx_index *sh = idx->shards[g];
        Ranges clipped;
        for (const auto &x : shard_ranges(*filt->ranges, idx->block_rows, (uint64_t)G, (uint64_t)g))
            if (x.first < std::min(x.second, sh->n)) clipped.emplace_back(x.first, std::min(x.second, sh->n));
        n_allow += count_allowed(sh, clipped);
        loc[g] = std::move(clipped);
        fa[g].ranges = &loc[g];
        offers[g] = !loc[g].empty();
    }
    for (int g = 0; filt && filt->res && g < G; ++g) {
        FilterShard &fs = filt->res->sh[(size_t)g];
        refresh_filter_shard(idx->shards[g], fs);
        n_allow += fs.n_live;
        fa[g].res = filt->res;
        fa[g].shard = g;
        offers[g] = fs.n_allowed != 0;
    }
    const size_t ids_bytes = (size_t)B * k * sizeof(uint64_t), blk = ids_bytes + (size_t)B * k * sizeof(float);
    auto local = [&](int g, mx_index *sh, const float *q, char *blkp) {
        return search_batch(sh, q, B, k, reinterpret_cast<uint64_t *>(blkp), idx->sh_scores[g], reinterpret_cast<float *>(blkp + ids_bytes),
                            idx->sh_nf[g], filt ? &fa[g] : nullptr);
    };
    // every shard found min(k, its live rows): the merged lists hold min(k, live rows of the handle) entries
    auto tail = [&](hipStream_t st) {
        return launch_fill_nfound(st, d_nfound, B, (int32_t)std::min<uint64_t>((uint64_t)k, filt ? n_allow : idx->total - idx->n_dead));
    };
    // (k = 0: the blocks are empty, nothing is exchanged or merged)
    if ((rc = exchange_and_merge(idx, d_q, B, k, blk, k > 0, d_ids, d_scores, d_dists, local, tail)) != MX_OK) return rc;
    if (filt) {
        // a query of the handle counts as answered by the subset kernel when every shard that had rows to offer used it
        bool any = false, all = true;
        for (int g = 0; g < G; ++g) {
            if (!offers[g]) continue;
            any = any || idx->shards[g]->last_subset;
            all = all && idx->shards[g]->last_subset;
        }
        idx->stats.filtered_queries += (uint64_t)B;
        if (any && all) idx->stats.subset_queries += (uint64_t)B;
    }
    return MX_OK;
}

// filt: the global rows a filtered search allows (normalised) or a resident filter, or null
int any_batch(mx_index *idx, const float *d_q, int B, int k, uint64_t *d_ids, float *d_scores, float *d_dists,
              int32_t *d_nfound, const FilterArg *filt = nullptr) {
    return idx->composite() ? composite_batch(idx, d_q, B, k, d_ids, d_scores, d_dists, d_nfound, filt)
                            : search_batch(idx, d_q, B, k, d_ids, d_scores, d_dists, d_nfound, filt);
}

// one range batch on a composite: every shard answers its rows with range_batch; the per-shard counts travel behind the packed
// [ids | dists] block (RCCL all-gather or peer copy), are summed, and the lists merged by (dist, id) at k = cap
int composite_range_batch(mx_index *idx, const float *d_q, int B, int cap, const uint32_t *dlim, uint64_t *d_ids, float *d_scores,
                          float *d_dists, int32_t *d_nfound, uint64_t *d_nrange) {
    const int G = (int)idx->shards.size();
    int rc = ensure_composite_buffers(idx, cap);
    if (rc != MX_OK) return rc;
    const size_t ids_bytes = (size_t)B * cap * sizeof(uint64_t), lists = ids_bytes + (size_t)B * cap * sizeof(float);
    const size_t blk = lists + (size_t)B * sizeof(uint64_t);  // ... | counts [B]
    auto local = [&](int g, mx_index *sh, const float *q, char *blkp) {
        return range_batch(sh, q, B, cap, dlim, reinterpret_cast<uint64_t *>(blkp), idx->sh_scores[g], reinterpret_cast<float *>(blkp + ids_bytes),
                           idx->sh_nf[g], reinterpret_cast<uint64_t *>(blkp + lists));
    };
    auto tail = [&](hipStream_t st) {
        return launch_range_sum(st, static_cast<const char *>(idx->sh_gather[0].get()) + lists, blk, G, B, cap, d_nrange, d_nfound);
    };
    return exchange_and_merge(idx, d_q, B, cap, blk, true, d_ids, d_scores, d_dists, local, tail);
}

int any_range_batch(mx_index *idx, const float *d_q, int B, int cap, const uint32_t *dlim, uint64_t *d_ids, float *d_scores, float *d_dists,
                    int32_t *d_nfound, uint64_t *d_nrange) {
    return idx->composite() ? composite_range_batch(idx, d_q, B, cap, dlim, d_ids, d_scores, d_dists, d_nfound, d_nrange)
                            : range_batch(idx, d_q, B, cap, dlim, d_ids, d_scores, d_dists, d_nfound, d_nrange);
}

// The row an id names, as (shard, row of that shard): global row r = id - id_offset - 1 lies in block r / R, which was dealt to shard
// block % G (composite_add); a plain index is its own shard 0.  false: the id names no row of the handle.
bool locate_row(const mx_index *idx, uint64_t id, size_t *shard, uint64_t *local) {
    const uint64_t off = idx->idmap.id_offset, total_rows = idx->composite() ? idx->total : idx->n;
    if (id <= off || id - off - 1 >= total_rows) return false;
    const uint64_t r = id - off - 1, R = idx->composite() ? idx->block_rows : 0, G = idx->shards.size();
    *shard = R ? (size_t)((r / R) % G) : 0;
    *local = R ? (r / R / G) * R + r % R : r;
    return true;
}

// ---- diversified search (mx_index_search_mmr) ------------------------------------------------------
// the candidate stage's lists on the index that owns the stream (the current device is its device)
int ensure_mmr_lists(mx_index *t, int fetch) {
    if (fetch <= t->mmr_fcap) return MX_OK;
    MX_HIP(hipStreamSynchronize(t->stream));
    t->mmr_fcap = 0;
    const size_t fc = (size_t)std::max(fetch, 64);
    MX_HIP(t->mmr_ids.alloc((size_t)kMaxBatch * fc));
    MX_HIP(t->mmr_scores.alloc((size_t)kMaxBatch * fc));
    MX_HIP(t->mmr_dists.alloc((size_t)kMaxBatch * fc));
    MX_HIP(t->mmr_nf.alloc(kMaxBatch));
    MX_HIP(t->mmr_pos.alloc((size_t)kMaxBatch * fc));
    MX_HIP(t->mmr_h_ids.alloc((size_t)kMaxBatch * fc, hipHostMallocDefault));
    MX_HIP(t->mmr_h_nf.alloc(kMaxBatch, hipHostMallocDefault));
    t->mmr_fcap = (int)fc;
    return MX_OK;
}

// the row list of a gather launch on sh, and a block of `bytes` for the gathered rows (0: sh gathers into another index's block); the
// current device is sh's
int ensure_mmr_stage(mx_index *sh, size_t bytes) {
    if (!sh->mmr_rows)
        MX_HIP(sh->mmr_rows.alloc(kMmrStageBytes / (kChunkFloats * sizeof(float))));
    if (bytes <= sh->mmr_stage_bytes) return MX_OK;
    MX_HIP(hipStreamSynchronize(sh->stream));
    sh->mmr_stage_bytes = 0;
    const size_t want = std::min(kMmrStageBytes, (bytes + ((size_t)1 << 20) - 1) >> 20 << 20);
    MX_HIP(sh->mmr_stage.alloc_bytes(want));
    sh->mmr_stage_bytes = want;
    return MX_OK;
}

// One batch (B <= kMaxBatch) of a diversified search, queries and outputs on the device of the index that owns the stream, the caller
// holding idx->mu across both stages: a plain search pass at k = fetch into that index's lists, then per chunk of queries (gathered rows
// <= kMmrStageBytes) every shard copies the stored rows of the candidates it owns into the block and mmr_select_kernel picks.
int mmr_batch(mx_index *idx, const float *d_q, int B, int k, int fetch, float lambda, uint64_t *d_ids, float *d_scores, float *d_dists,
              int32_t *d_nfound) {
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    const int ds = t->ds;
    if (ds > kMmrMaxDs) return fail(MX_EUNSUPPORTED, "diversified search supports dim <= %d", kMmrMaxDs);
    int rc = ensure_mmr_lists(t, fetch);
    if (rc != MX_OK) return rc;
    if ((rc = any_batch(idx, d_q, B, fetch, t->mmr_ids, t->mmr_scores, t->mmr_dists, t->mmr_nf)) != MX_OK) return rc;
    hipStream_t st = t->stream;
    MX_HIP(hipMemcpyAsync(t->mmr_h_ids, t->mmr_ids, (size_t)B * fetch * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MX_HIP(hipMemcpyAsync(t->mmr_h_nf, t->mmr_nf, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    const size_t G = idx->composite() ? idx->shards.size() : 1;
    const size_t row_bytes = (size_t)ds * sizeof(float);
    const int qc = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, kMmrStageBytes / ((size_t)fetch * row_bytes)));
    std::vector<std::vector<uint32_t>> rows(G);  // (alive until the chunk is host-synchronised: sources of async uploads)
    std::vector<uint32_t> pos, owner;
    std::vector<size_t> first(G + 1);
    for (int q0 = 0; q0 < B; q0 += qc) {
        const int nq = std::min(qc, B - q0);
        for (auto &r : rows) r.clear();
        pos.assign((size_t)nq * fetch, 0u);
        owner.assign((size_t)nq * fetch, 0u);
        for (int q = 0; q < nq; ++q) {
            const int m = std::min(std::max(t->mmr_h_nf[q0 + q], 0), fetch);
            for (int i = 0; i < m; ++i) {
                const uint64_t id = t->mmr_h_ids[(size_t)(q0 + q) * fetch + i];
                size_t g;
                uint64_t local;
                if (!locate_row(idx, id, &g, &local)) return fail(MX_ESEARCH, "candidate id %llu names no row", (unsigned long long)id);
                const mx_index *sh = idx->composite() ? idx->shards[g] : idx;
                if (local >= sh->n) return fail(MX_ESEARCH, "candidate id %llu names no row of its shard", (unsigned long long)id);
                const size_t s = (size_t)q * fetch + i;
                owner[s] = (uint32_t)g;
                pos[s] = (uint32_t)rows[g].size();
                rows[g].push_back((uint32_t)local);
            }
        }
        first[0] = 0;
        for (size_t g = 0; g < G; ++g) first[g + 1] = first[g] + rows[g].size();
        for (int q = 0; q < nq; ++q) {
            const int m = std::min(std::max(t->mmr_h_nf[q0 + q], 0), fetch);
            for (int i = 0; i < m; ++i) pos[(size_t)q * fetch + i] += (uint32_t)first[owner[(size_t)q * fetch + i]];
        }
        {
            DeviceGuard dg(t->device);
            if ((rc = ensure_mmr_stage(t, first[G] * row_bytes)) != MX_OK) return rc;
        }
        for (size_t g = 0; g < G; ++g) {
            if (rows[g].empty()) continue;
            mx_index *sh = idx->composite() ? idx->shards[g] : idx;
            std::unique_lock<std::mutex> lk(sh->mu, std::defer_lock);
            if (idx->composite()) lk.lock();  // (a plain index: the caller holds it)
            DeviceGuard dg(sh->device);
            const bool same = sh->device == t->device;
            const size_t bytes = rows[g].size() * row_bytes;
            if (sh != t && (rc = ensure_mmr_stage(sh, same ? 0 : bytes)) != MX_OK) return rc;
            MX_HIP(hipMemcpyAsync(sh->mmr_rows, rows[g].data(), rows[g].size() * sizeof(uint32_t), hipMemcpyHostToDevice, sh->stream));
            float *slot = t->mmr_stage + first[g] * (size_t)ds;
            MX_HIP(launch_mmr_gather(sh->stream, ds, sh->compressed ? nullptr : sh->x, sh->xh, sh->mmr_rows, (uint32_t)rows[g].size(),
                                     same ? slot : sh->mmr_stage));
            if (!same) MX_HIP(hipMemcpyAsync(slot, sh->mmr_stage, bytes, hipMemcpyDefault, sh->stream));  // peer copy to shards[0]'s device
            if (sh != t) MX_HIP(hipStreamSynchronize(sh->stream));
        }
        DeviceGuard dg(t->device);
        MX_HIP(hipMemcpyAsync(t->mmr_pos, pos.data(), pos.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        const size_t c0 = (size_t)q0 * fetch, o0 = (size_t)q0 * k;
        MX_HIP(launch_mmr_select(st, nq, k, fetch, ds, lambda, t->mmr_stage, t->mmr_pos, t->mmr_ids + c0, t->mmr_scores + c0, t->mmr_dists + c0,
                                 t->mmr_nf + q0, d_ids + o0, d_scores + o0, d_dists ? d_dists + o0 : nullptr, d_nfound + q0));
        MX_HIP(hipStreamSynchronize(st));
    }
    return MX_OK;
}

// ---- fused search (mx_index_search_fused) -----------------------------------------------------------
// One chunk of a fused search: nreq requests of m sub-queries each (nreq * m <= kMaxBatch), queries and outputs on the device of the
// index that owns the stream, the caller holding idx->mu across both stages.  A plain search pass over the nreq * m queries at
// k = fetch into that index's lists (the diversified search's: a sharded handle has them merged on devices[0] already, no rows are
// gathered), the chunk's weights (host memory, [nreq, m]; null: all ones) uploaded, one fuse_kernel launch; host-synchronised.
int fused_batch(mx_index *idx, const float *d_q, int nreq, int m, const float *weights, int mode, int k, int fetch, float rrf_c,
                uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_best, double *d_fused, int32_t *d_nfound) {
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    int rc = ensure_mmr_lists(t, fetch);
    if (rc != MX_OK) return rc;
    if (!t->fuse_w) MX_HIP(t->fuse_w.alloc(kMaxBatch));
    const int B = nreq * m;
    if ((rc = any_batch(idx, d_q, B, fetch, t->mmr_ids, t->mmr_scores, t->mmr_dists, t->mmr_nf)) != MX_OK) return rc;
    hipStream_t st = t->stream;
    std::vector<float> w(weights ? weights : nullptr, weights ? weights + B : nullptr);  // (alive until the stream is synchronised)
    if (!weights) w.assign((size_t)B, 1.0f);
    MX_HIP(hipMemcpyAsync(t->fuse_w, w.data(), (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
    FuseArgs p{nreq, m, fetch, k, mode, (double)rrf_c, t->fuse_w, t->mmr_ids, t->mmr_scores, t->mmr_dists, t->mmr_nf,
               d_ids, d_scores, d_dists, d_best, d_fused, d_nfound};
    MX_HIP(launch_fuse(st, p));
    MX_HIP(hipStreamSynchronize(st));
    return MX_OK;
}

// ---- search by stored row (mx_index_search_by_id / mx_index_search_range_by_id) ----------------------------
bool row_removed(const mx_index *t, uint64_t r);

// the pass's own lists, kk wide, and the per-query words on the index that owns the stream (the current device is its device)
int ensure_byid_lists(mx_index *t, int kk) {
    if (!t->byid_q) {
        MX_HIP(t->byid_q.alloc((size_t)kMaxBatch * t->dim));
        MX_HIP(t->byid_nf.alloc(kMaxBatch));
        MX_HIP(t->byid_nr.alloc(kMaxBatch));
        MX_HIP(t->byid_own.alloc(kMaxBatch));
        MX_HIP(t->byid_src.alloc(kMaxBatch));
        MX_HIP(t->byid_dlim.alloc(kMaxBatch));
    }
    if (kk <= t->byid_cap) return MX_OK;
    MX_HIP(hipStreamSynchronize(t->stream));
    t->byid_cap = 0;
    const size_t c = (size_t)std::max(kk, 64);
    MX_HIP(t->byid_ids.alloc((size_t)kMaxBatch * c));
    MX_HIP(t->byid_scores.alloc((size_t)kMaxBatch * c));
    MX_HIP(t->byid_dists.alloc((size_t)kMaxBatch * c));
    t->byid_cap = (int)c;
    return MX_OK;
}

// One batch (B <= kMaxBatch) of a search whose queries are the stored rows qids names (host memory), outputs [B, k] on the device of
// the index that owns the stream, the caller holding idx->mu from here to the end: ids -> (shard, local row) while nothing can move
// them, every shard gathers its rows into its slice of one query block (queries that name no live row are left out of the pass), one
// plain pass at k + exclude -- any_batch, or any_range_batch when dlim (the B dist bounds, host memory) is given, k being the cap --
// into this index's own lists, and byid_drop_self_kernel writes the caller's.
int byid_batch(mx_index *idx, const uint64_t *qids, int B, int k, int exclude, const uint32_t *dlim, uint64_t *d_ids, float *d_scores,
               float *d_dists, int32_t *d_nfound, uint64_t *d_nrange) {
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    const int kk = k + exclude, dim = idx->dim;
    int rc = ensure_byid_lists(t, kk);
    if (rc != MX_OK) return rc;
    hipStream_t st = t->stream;
    const size_t G = idx->composite() ? idx->shards.size() : 1;
    std::vector<std::vector<uint32_t>> rows(G);  // (alive until the batch is host-synchronised: sources of async uploads)
    std::vector<uint32_t> src((size_t)B, kByIdNone), owner((size_t)B, 0u), pd((size_t)B, 0u);
    for (int b = 0; b < B; ++b) {
        const uint64_t id = qids[b];
        size_t g;
        uint64_t local;
        if (!locate_row(idx, id, &g, &local)) continue;  // names no row
        const mx_index *sh = idx->composite() ? idx->shards[g] : idx;
        if (local >= sh->n) return fail(MX_ESEARCH, "id %llu names no row of its shard", (unsigned long long)id);
        if (row_removed(sh, local)) continue;
        owner[b] = (uint32_t)g;
        src[b] = (uint32_t)rows[g].size();
        rows[g].push_back((uint32_t)local);
    }
    std::vector<size_t> first(G + 1, 0);
    for (size_t g = 0; g < G; ++g) first[g + 1] = first[g] + rows[g].size();
    const int live = (int)first[G];
    for (int b = 0; b < B; ++b)
        if (src[b] != kByIdNone) {
            src[b] += (uint32_t)first[owner[b]];
            if (dlim) pd[src[b]] = dlim[b];
        }
    for (size_t g = 0; g < G; ++g) {
        if (rows[g].empty()) continue;
        mx_index *sh = idx->composite() ? idx->shards[g] : idx;
        std::unique_lock<std::mutex> lk(sh->mu, std::defer_lock);
        if (idx->composite()) lk.lock();  // (a plain index: the caller holds it)
        DeviceGuard dg(sh->device);
        const bool same = sh->device == t->device;
        if (!sh->byid_rows) MX_HIP(sh->byid_rows.alloc(kMaxBatch));
        if (!same && !sh->byid_stage) MX_HIP(sh->byid_stage.alloc((size_t)kMaxBatch * dim));
        MX_HIP(hipMemcpyAsync(sh->byid_rows, rows[g].data(), rows[g].size() * sizeof(uint32_t), hipMemcpyHostToDevice, sh->stream));
        float *slot = t->byid_q + first[g] * (size_t)dim;
        MX_HIP(launch_byid_gather(sh->stream, dim, sh->ds, sh->compressed ? nullptr : sh->x, sh->xh, sh->byid_rows, (uint32_t)rows[g].size(),
                                  same ? slot : sh->byid_stage));
        if (!same)  // peer copy to shards[0]'s device
            MX_HIP(hipMemcpyAsync(slot, sh->byid_stage, rows[g].size() * (size_t)dim * sizeof(float), hipMemcpyDefault, sh->stream));
        if (sh != t) MX_HIP(hipStreamSynchronize(sh->stream));
    }
    DeviceGuard dg(t->device);
    if (live > 0) {
        rc = dlim ? any_range_batch(idx, t->byid_q, live, kk, pd.data(), t->byid_ids, t->byid_scores, t->byid_dists, t->byid_nf, t->byid_nr)
                  : any_batch(idx, t->byid_q, live, kk, t->byid_ids, t->byid_scores, t->byid_dists, t->byid_nf);
        if (rc != MX_OK) return rc;
    }
    MX_HIP(hipMemcpyAsync(t->byid_src, src.data(), (size_t)B * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    MX_HIP(hipMemcpyAsync(t->byid_own, qids, (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (dlim) MX_HIP(hipMemcpyAsync(t->byid_dlim, pd.data(), (size_t)B * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ByIdDrop p{};
    p.B = B;
    p.k = k;
    p.kk = kk;
    p.exclude = exclude;
    p.dim = dim;
    p.src = t->byid_src;
    p.own = t->byid_own;
    p.in_ids = t->byid_ids;
    p.in_scores = t->byid_scores;
    p.in_dists = t->byid_dists;
    p.in_nfound = t->byid_nf;
    p.in_nrange = dlim ? t->byid_nr : nullptr;
    p.dlim = t->byid_dlim;
    p.q = t->byid_q;
    p.ids = d_ids;
    p.scores = d_scores;
    p.dists = d_dists;
    p.n_found = d_nfound;
    p.n_in_range = dlim ? d_nrange : nullptr;
    MX_HIP(launch_byid_drop_self(st, p));
    MX_HIP(hipStreamSynchronize(st));
    return MX_OK;
}

// ---- search by examples (mx_index_search_like) ---------------------------------------------------------------
// the pass's own lists, kk wide, and the per-pass words on the index that owns the stream (the current device is its device)
int ensure_like_lists(mx_index *t, int kk) {
    if (!t->like_q) {
        MX_HIP(t->like_rows.alloc((size_t)kMaxBatch * t->dim));
        MX_HIP(t->like_q.alloc((size_t)kMaxBatch * t->dim));
        MX_HIP(t->like_own.alloc(kMaxBatch));
        MX_HIP(t->like_w.alloc(kMaxBatch));
        MX_HIP(t->like_wq.alloc(kMaxBatch));
        MX_HIP(t->like_nf.alloc(kMaxBatch));
        MX_HIP(t->like_nused.alloc(kMaxBatch));
        MX_HIP(t->like_src.alloc(kMaxBatch));
        MX_HIP(t->like_used.alloc(kMaxBatch));
    }
    if (kk <= t->like_cap) return MX_OK;
    MX_HIP(hipStreamSynchronize(t->stream));
    t->like_cap = 0;
    const size_t c = (size_t)std::max(kk, 64);
    MX_HIP(t->like_ids.alloc((size_t)kMaxBatch * c));
    MX_HIP(t->like_scores.alloc((size_t)kMaxBatch * c));
    MX_HIP(t->like_dists.alloc((size_t)kMaxBatch * c));
    t->like_cap = (int)c;
    return MX_OK;
}

// One pass of a search by examples: nreq requests of m example slots each (nreq * m <= kMaxBatch), example ids and weights in host
// memory ([nreq, m]; weights null: all ones), the caller vectors d_q [nreq, dim] (null: none) and the outputs on the device of the
// index that owns the stream, wq their weights (host, [nreq]; null: all ones), the caller holding idx->mu from here to the end.  Ids ->
// (shard, local row) while nothing can move them; slots of weight 0 and ids that name no live row are left out; every shard gathers
// its rows into its slice of one block; like_combine_kernel blends each request's terms into one query; one plain pass at k + (exclude
// ? m : 0) over the nreq queries into this index's own lists; like_drop_examples_kernel writes the caller's.  d_nused, d_combined: null
// = not wanted there (the combined queries stay in t->like_q, the counts go to t->like_nused).  Host-synchronised.
int like_batch(mx_index *idx, const float *d_q, const float *wq, const uint64_t *ex_ids, const float *w, int nreq, int m, int k, int exclude,
               uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_nfound, int32_t *d_nused, float *d_combined) {
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    const int kk = k + (exclude ? m : 0), dim = idx->dim, S = nreq * m;
    int rc = ensure_like_lists(t, kk);
    if (rc != MX_OK) return rc;
    hipStream_t st = t->stream;
    const size_t G = idx->composite() ? idx->shards.size() : 1;
    std::vector<std::vector<uint32_t>> rows(G);  // (alive until the pass is host-synchronised: sources of async uploads)
    std::vector<uint32_t> src((size_t)S, kLikeNone), owner((size_t)S, 0u);
    std::vector<float> hw(w ? w : nullptr, w ? w + S : nullptr), hwq(wq ? wq : nullptr, wq ? wq + nreq : nullptr);
    if (!w) hw.assign((size_t)S, 1.0f);
    if (!wq) hwq.assign((size_t)nreq, 1.0f);
    for (int i = 0; i < S; ++i) {
        if (hw[i] == 0.0f) continue;  // an absent slot
        const uint64_t id = ex_ids[i];
        size_t g;
        uint64_t local;
        if (!locate_row(idx, id, &g, &local)) continue;  // names no row
        const mx_index *sh = idx->composite() ? idx->shards[g] : idx;
        if (local >= sh->n) return fail(MX_ESEARCH, "id %llu names no row of its shard", (unsigned long long)id);
        if (row_removed(sh, local)) continue;
        owner[i] = (uint32_t)g;
        src[i] = (uint32_t)rows[g].size();
        rows[g].push_back((uint32_t)local);
    }
    std::vector<size_t> first(G + 1, 0);
    for (size_t g = 0; g < G; ++g) first[g + 1] = first[g] + rows[g].size();
    for (int i = 0; i < S; ++i)
        if (src[i] != kLikeNone) src[i] += (uint32_t)first[owner[i]];
    for (size_t g = 0; g < G; ++g) {
        if (rows[g].empty()) continue;
        mx_index *sh = idx->composite() ? idx->shards[g] : idx;
        std::unique_lock<std::mutex> lk(sh->mu, std::defer_lock);
        if (idx->composite()) lk.lock();  // (a plain index: the caller holds it)
        DeviceGuard dg(sh->device);
        const bool same = sh->device == t->device;
        if (!sh->byid_rows) MX_HIP(sh->byid_rows.alloc(kMaxBatch));
        if (!same && !sh->byid_stage) MX_HIP(sh->byid_stage.alloc((size_t)kMaxBatch * dim));
        MX_HIP(hipMemcpyAsync(sh->byid_rows, rows[g].data(), rows[g].size() * sizeof(uint32_t), hipMemcpyHostToDevice, sh->stream));
        float *slot = t->like_rows + first[g] * (size_t)dim;
        MX_HIP(launch_byid_gather(sh->stream, dim, sh->ds, sh->compressed ? nullptr : sh->x, sh->xh, sh->byid_rows, (uint32_t)rows[g].size(),
                                  same ? slot : sh->byid_stage));
        if (!same)  // peer copy to shards[0]'s device
            MX_HIP(hipMemcpyAsync(slot, sh->byid_stage, rows[g].size() * (size_t)dim * sizeof(float), hipMemcpyDefault, sh->stream));
        if (sh != t) MX_HIP(hipStreamSynchronize(sh->stream));
    }
    DeviceGuard dg(t->device);
    MX_HIP(hipMemcpyAsync(t->like_src, src.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    MX_HIP(hipMemcpyAsync(t->like_w, hw.data(), (size_t)S * sizeof(float), hipMemcpyHostToDevice, st));
    MX_HIP(hipMemcpyAsync(t->like_own, ex_ids, (size_t)S * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (d_q) MX_HIP(hipMemcpyAsync(t->like_wq, hwq.data(), (size_t)nreq * sizeof(float), hipMemcpyHostToDevice, st));
    LikeCombine c{};
    c.R = nreq;
    c.m = m;
    c.dim = dim;
    c.rows = t->like_rows;
    c.src = t->like_src;
    c.w = t->like_w;
    c.q = d_q;
    c.wq = t->like_wq;
    c.out = t->like_q;
    c.combined = d_combined;
    c.used = t->like_used;
    c.n_used = d_nused ? d_nused : t->like_nused.get();
    MX_HIP(launch_like_combine(st, c));
    if ((rc = any_batch(idx, t->like_q, nreq, kk, t->like_ids, t->like_scores, t->like_dists, t->like_nf)) != MX_OK) {
        (void)hipStreamSynchronize(st);  // (the uploads above read this function's vectors)
        return rc;
    }
    LikeDrop p{};
    p.R = nreq;
    p.m = m;
    p.k = k;
    p.kk = kk;
    p.exclude = exclude;
    p.dim = dim;
    p.own = t->like_own;
    p.used = t->like_used;
    p.q = t->like_q;
    p.in_ids = t->like_ids;
    p.in_scores = t->like_scores;
    p.in_dists = t->like_dists;
    p.in_nfound = t->like_nf;
    p.ids = d_ids;
    p.scores = d_scores;
    p.dists = d_dists;
    p.n_found = d_nfound;
    MX_HIP(launch_like_drop_examples(st, p));
    MX_HIP(hipStreamSynchronize(st));
    return MX_OK;
}

// ---- scoring of named rows (mx_index_score_ids) ------------------------------------------------------------
// The buffers of the call on sh (the current device is its device), each kMaxBatch x m: the id block always; outs: the outputs of the
// host-pointer variant (the index that owns the stream); part: a shard's own dist block (a shard on another device than shards[0]);
// gather > 0: the gather area of that many dist blocks (shards[0] of a composite)
int ensure_score_bufs(mx_index *sh, int m, bool outs, bool part, size_t gather) {
    if (m <= sh->score_cap && (!outs || m <= sh->score_out_cap) && (!part || m <= sh->score_part_cap) && (!gather || m <= sh->score_gather_cap))
        return MX_OK;
    MX_HIP(hipStreamSynchronize(sh->stream));
    const size_t c = (size_t)std::max(m, 64), n = (size_t)kMaxBatch * c;
    if (m > sh->score_cap) {
        sh->score_cap = 0;
        MX_HIP(sh->score_cand.alloc(n));
        sh->score_cap = (int)c;
    }
    if (outs && m > sh->score_out_cap) {
        sh->score_out_cap = 0;
        MX_HIP(sh->score_scores.alloc(n));
        MX_HIP(sh->score_dists.alloc(n));
        MX_HIP(sh->score_order.alloc(n));
        MX_HIP(sh->score_nf.alloc(kMaxBatch));
        sh->score_out_cap = (int)c;
    }
    if (part && m > sh->score_part_cap) {
        sh->score_part_cap = 0;
        MX_HIP(sh->score_part.alloc(n));
        sh->score_part_cap = (int)c;
    }
    if (gather && m > sh->score_gather_cap) {
        sh->score_gather_cap = 0;
        MX_HIP(sh->score_gather.alloc(n * gather));
        sh->score_gather_cap = (int)c;
    }
    return MX_OK;
}

// the query block and the id block (host memory, [B, m]) of a batch on sh, whose device is current: qpad / qnorm2 and the non-finite
// flags as launch_prep_queries leaves them (no filter copy is consulted), and the score kernel's arguments but its outputs
int score_prepare(mx_index *sh, const float *d_q, int B, const uint64_t *cand, int m, uint64_t total, ScoreIds *p) {
    Scratch &s = sh->s;
    MX_HIP(hipMemcpyAsync(sh->score_cand, cand, (size_t)B * m * sizeof(uint64_t), hipMemcpyHostToDevice, sh->stream));
    MX_HIP(launch_prep_queries(sh->stream, d_q, B, sh->dim, sh->ds, s.qfrag, s.qpad, s.qnorm2, s.theta, s.e1, nullptr, s.overflow, s.qflags,
                               s.qa, s.qb));
    *p = ScoreIds{};
    p->B = B;
    p->m = m;
    p->ds = sh->ds;
    p->x = sh->compressed ? nullptr : sh->x.get();
    p->xh = sh->xh;
    p->dead = sh->n_dead ? sh->dead.get() : nullptr;
    p->n_rows = sh->n;
    p->total = total;
    p->idmap = sh->idmap;
    p->qpad = s.qpad;
    p->qnorm2 = s.qnorm2;
    p->cand = sh->score_cand;
    return MX_OK;
}

// One batch (B <= kMaxBatch) of a scoring call: the queries d_q [B, dim] and the outputs [B, m] on the device of the index that owns
// the stream, the ids cand [B, m] in host memory, the caller holding idx->mu from here to the end of the last kernel.  A plain index:
// one score_ids_kernel launch.  A composite: every shard gets the query block and the id block and scores the pairs whose rows it
// owns into its dist block (a shard on shards[0]'s device: straight into its slot of the gather area; another: peer-copied there),
// and score_merge_kernel on shards[0]'s device combines and ranks.  No filter copy, no scan, no counters.  Host-synchronised.
int score_batch(mx_index *idx, const float *d_q, int B, const uint64_t *cand, int m, float *d_scores, float *d_dists, int32_t *d_order,
                int32_t *d_nfound) {
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    hipStream_t st = t->stream;
    const size_t cells = (size_t)B * m;
    int rc;
    ScoreIds p;
    if ((rc = ensure_scratch(t)) != MX_OK) return rc;
    if (!idx->composite()) {
        if ((rc = ensure_score_bufs(t, m, false, false, 0)) != MX_OK) return rc;
        if ((rc = score_prepare(t, d_q, B, cand, m, t->n, &p)) != MX_OK) return rc;
        p.scores = d_scores;
        p.dists = d_dists;
        p.order = d_order;
        p.n_found = d_nfound;
        MX_HIP(launch_score_ids(st, p));
    } else {
        const size_t G = idx->shards.size();
        if ((rc = ensure_score_bufs(t, m, false, false, G)) != MX_OK) return rc;
        MX_HIP(hipStreamSynchronize(st));  // the query block must be complete before other devices read it
        for (size_t g = 0; g < G; ++g) {
            mx_index *sh = idx->shards[g];
            std::lock_guard<std::mutex> lk(sh->mu);
            DeviceGuard dg(sh->device);
            const bool same = sh->device == t->device;
            if ((rc = ensure_scratch(sh)) != MX_OK) return rc;
            if ((rc = ensure_score_bufs(sh, m, false, !same, sh == t ? G : 0)) != MX_OK) return rc;
            const float *q = d_q;
            if (sh != t) {
                MX_HIP(hipMemcpyAsync(sh->s.qstage, d_q, (size_t)B * idx->dim * sizeof(float), hipMemcpyDefault, sh->stream));
                q = sh->s.qstage;
            }
            if ((rc = score_prepare(sh, q, B, cand, m, idx->total, &p)) != MX_OK) return rc;
            uint32_t *slot = t->score_gather + g * cells;
            p.part = same ? slot : sh->score_part.get();
            MX_HIP(launch_score_ids(sh->stream, p));
            if (!same) MX_HIP(hipMemcpyAsync(slot, sh->score_part, cells * sizeof(uint32_t), hipMemcpyDefault, sh->stream));  // peer copy
            if (sh != t) MX_HIP(hipStreamSynchronize(sh->stream));
        }
        DeviceGuard dg(t->device);
        ScoreMerge mg{B, m, (int)G, t->score_gather, cells, t->score_cand, d_scores, d_dists, d_order, d_nfound};
        MX_HIP(launch_score_merge(st, mg));
    }
    if ((rc = fetch_flags(t)) != MX_OK) return rc;  // (host-synchronised)
    const uint32_t *h_qfl = t->s.host_flags + 3 * kMaxBatch;
    for (int b = 0; b < B; ++b)
        if (h_qfl[b]) return fail(MX_EINVAL, "a query contains non-finite values");
    return MX_OK;
}

// what an append can change in a plain index, and how to undo it: an insert is all-or-nothing, also when it
// spans several shards or several staging chunks and a later part fails (non-finite device rows, HBM)
struct RowMark {
    uint64_t n, n_zero, wild_rows, n_wild;
};
RowMark mark_rows(const mx_index *idx) { return RowMark{idx->n, idx->n_zero, idx->wild_rows, idx->n_wild}; }
void rollback_rows(mx_index *idx, const RowMark &m) {
    if (idx->n == m.n) return;
    const std::string keep = last_error_slot();
    DeviceGuard dg(idx->device);
    idx->n = m.n;  // rows past n are never read by a search (finish_kernel drops them); the next append overwrites them
    idx->n_zero = m.n_zero;
    idx->wild_rows = m.wild_rows;
    idx->n_wild = m.n_wild;
    const uint32_t zc[2] = {(uint32_t)m.n_zero, (uint32_t)m.n_wild};  // the device-side list counts: entries past them are dead
    (void)hipMemcpyAsync(idx->flags + 3, zc, sizeof(zc), hipMemcpyHostToDevice, idx->stream);
    (void)hipStreamSynchronize(idx->stream);
    idx->disk_dir.clear();
    last_error_slot() = keep;
}

// append host rows to a composite: global row r -> block b = r / R, shard b % G
int composite_add(mx_index *idx, const float *rows, uint64_t n, uint64_t *first_id, bool on_device) {
    const uint64_t R = idx->block_rows, G = idx->shards.size();
    if (first_id) *first_id = idx->idmap.id_offset + idx->total + 1;  // the id a search reports for the row, as on a plain index
    if (n == 0) return MX_OK;
    const size_t rowf = (size_t)idx->dim;
    // per shard: the (contiguous in the source) segments it receives, in order
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> seg(G);  // (source row, count)
    for (uint64_t r = idx->total, done = 0; done < n;) {
        const uint64_t b = r / R, take = std::min(n - done, R - r % R);
        seg[b % G].push_back({done, take});
        r += take;
        done += take;
    }
    // all-or-nothing: validate host rows up front (device rows are validated per shard by the ingest kernel)
    if (!on_device) {
        const size_t totalf = (size_t)n * rowf;
        for (size_t i = 0; i < totalf; ++i)
            if (!std::isfinite(rows[i])) return fail(MX_EINVAL, "row %zu contains a non-finite value; nothing inserted", i / rowf);
    }
    std::vector<RowMark> marks;
    for (mx_index *sh : idx->shards) marks.push_back(mark_rows(sh));
    auto append_to = [&](uint64_t g) -> int {
        mx_index *sh = idx->shards[g];
        std::lock_guard<std::mutex> lk(sh->mu);
        DeviceGuard dg(sh->device);
        uint64_t cnt = 0;
        for (auto &sgm : seg[g]) cnt += sgm.second;
        Dev<float> stage;
        MX_HIP(stage.alloc((size_t)cnt * rowf));
        uint64_t at = 0;
        for (auto &sgm : seg[g]) {
            MX_HIP(hipMemcpyAsync(stage + (size_t)at * rowf, rows + (size_t)sgm.first * rowf, (size_t)sgm.second * rowf * sizeof(float),
                                  on_device ? hipMemcpyDefault : hipMemcpyHostToDevice, sh->stream));
            at += sgm.second;
        }
        return add_device_locked(sh, stage, cnt, nullptr);
    };
    for (uint64_t g = 0; g < G; ++g) {
        if (seg[g].empty()) continue;
        const int rc = append_to(g);
        if (rc != MX_OK) {  // a non-finite device row or an allocation on shard g: take back what shards < g got
            for (uint64_t h = 0; h < g; ++h) {
                std::lock_guard<std::mutex> lk(idx->shards[h]->mu);
                rollback_rows(idx->shards[h], marks[h]);
            }
            return rc;
        }
    }
    idx->total += n;
    return MX_OK;
}

const char kMagic[8] = {'M', 'X', 'F', 'L', 'A', 'T', '0', '1'};
constexpr long kHeaderBytes = 24;
// a compacted index's store (mx_index_compact): the 01 header + u64 compaction generation
const char kMagic2[8] = {'M', 'X', 'F', 'L', 'A', 'T', '0', '2'};
constexpr long kHeader2Bytes = 32;
long header_bytes(uint64_t gen) { return gen ? kHeader2Bytes : kHeaderBytes; }

// header of vectors.mxflat (either version) -> dim, flags word, rows, generation (0 for MXFLAT01); false: not a store header
bool read_store_header(FILE *f, uint32_t (&hdr)[2], uint64_t *n, uint64_t *gen) {
    char magic[8];
    *gen = 0;
    if (fread(magic, 1, 8, f) != 8 || fread(hdr, sizeof(hdr), 1, f) != 1 || fread(n, sizeof(*n), 1, f) != 1) return false;
    if (memcmp(magic, kMagic, 8) == 0) return true;
    return memcmp(magic, kMagic2, 8) == 0 && fread(gen, sizeof(*gen), 1, f) == 1 && *gen != 0;
}
std::string store_file(const char *dir) { return std::string(dir) + "/vectors.mxflat"; }

int mkdir_p(const std::string &dir) {  // create_dir_all (local.rs:144)
    struct stat sb;
    if (stat(dir.c_str(), &sb) == 0) return S_ISDIR(sb.st_mode) ? 0 : -1;
    const size_t slash = dir.find_last_of('/');
    if (slash != std::string::npos && slash > 0 && mkdir_p(dir.substr(0, slash)) != 0) return -1;
    return (mkdir(dir.c_str(), 0755) == 0 || errno == EEXIST) ? 0 : -1;
}

void remember_disk(mx_index *idx, const char *dir, uint64_t rows) {
    struct stat sb;
    idx->disk_dir.clear();
    if (stat(store_file(dir).c_str(), &sb) != 0) return;
    idx->disk_dir = dir;
    idx->disk_rows = rows;
    idx->disk_size = sb.st_size;
    idx->disk_mtime = sb.st_mtim;
}

bool disk_in_sync(mx_index *idx, const char *dir) {  // vectors.mxflat in dir is what this handle last wrote / read
    if (idx->disk_dir.empty() || idx->disk_dir != dir) return false;
    struct stat sb;
    if (stat(store_file(dir).c_str(), &sb) != 0) return false;
    return sb.st_size == idx->disk_size && sb.st_mtim.tv_sec == idx->disk_mtime.tv_sec &&
           sb.st_mtim.tv_nsec == idx->disk_mtime.tv_nsec;
}

// local rows [r0, r0 + m) of a plain index -> host buffer [m, dim].  A compressed corpus hands out its stored
// (bf16, near-unit) rows widened to f32.
int fetch_local(mx_index *idx, uint64_t r0, uint64_t m, float *out) {
    DeviceGuard dg(idx->device);
    if (!idx->compressed) {
        MX_HIP(hipMemcpy2D(out, (size_t)idx->dim * 4, idx->x + (size_t)r0 * idx->ds, (size_t)idx->ds * 4, (size_t)idx->dim * 4, m,
                           hipMemcpyDeviceToHost));
        return MX_OK;
    }
    const uint64_t chunk = std::max<uint64_t>(1, (idx->xs_rows ? idx->xs_rows : 1) * (uint64_t)idx->ds / (uint64_t)idx->dim);
    if (!idx->xs) return fail(MX_EINVAL, "empty compressed index");
    for (uint64_t done = 0; done < m; done += chunk) {
        const uint64_t c = std::min(chunk, m - done);
        MX_HIP(launch_unshadow(idx->stream, idx->xh, idx->ds, idx->dim, r0 + done, c, idx->xs));
        MX_HIP(hipMemcpyAsync(out + (size_t)done * idx->dim, idx->xs, (size_t)c * idx->dim * 4, hipMemcpyDeviceToHost, idx->stream));
        MX_HIP(hipStreamSynchronize(idx->stream));
    }
    return MX_OK;
}

// rows [r0, r0 + m) of the index in global order -> host buffer [m, dim]
int fetch_rows(mx_index *idx, uint64_t r0, uint64_t m, float *out, std::vector<float> &tmp) {
    (void)tmp;
    if (!idx->composite()) return fetch_local(idx, r0, m, out);
    const uint64_t R = idx->block_rows, G = idx->shards.size();
    for (uint64_t r = r0, done = 0; done < m;) {
        const uint64_t b = r / R, take = std::min(m - done, R - r % R);
        mx_index *sh = idx->shards[b % G];
        const uint64_t lrow = (b / G) * R + r % R;
        int rc = fetch_local(sh, lrow, take, out + (size_t)done * idx->dim);
        if (rc != MX_OK) return rc;
        r += take;
        done += take;
    }
    return MX_OK;
}

uint64_t rows_of(mx_index *idx) { return idx->composite() ? idx->total : idx->n; }
bool is_compressed(mx_index *idx) { return idx->composite() ? idx->shards[0]->compressed : idx->compressed; }
void set_raw_ingest(mx_index *idx, bool on) {
    idx->raw_ingest = on;
    for (mx_index *sh : idx->shards) sh->raw_ingest = on;
}

// ---- removal (tombstones) --------------------------------------------------------------------------------------
// Sets the dead bits of local rows `rows` (all < n) of a plain index or shard and copies the changed words to the device on the
// index's stream -- host-synchronised before it returns, so a search that starts afterwards runs with them.  fresh[i] = 1 when
// rows[i] was not removed before (a row named twice counts once); *newly = how many.
int mark_dead_local(mx_index *idx, const std::vector<uint64_t> &rows, std::vector<uint8_t> &fresh, uint64_t *newly) {
    *newly = 0;
    fresh.assign(rows.size(), 0);
    if (rows.empty()) return MX_OK;
    DeviceGuard dg(idx->device);
    if (!idx->dead) {
        const size_t words = (size_t)(idx->cap / kTile8Rows);
        MX_HIP(idx->dead.alloc(words));
        MX_HIP(hipMemsetAsync(idx->dead, 0, words * sizeof(uint64_t), idx->stream));
        idx->dead_h.assign(words, 0);
    }
    size_t w0 = SIZE_MAX, w1 = 0;
    for (size_t i = 0; i < rows.size(); ++i) {
        const uint64_t r = rows[i];
        uint64_t &w = idx->dead_h[r >> 6];
        const uint64_t bit = 1ull << (r & 63);
        if (w & bit) continue;
        w |= bit;
        fresh[i] = 1;
        *newly += 1;
        w0 = std::min<size_t>(w0, r >> 6);
        w1 = std::max<size_t>(w1, r >> 6);
    }
    if (*newly) {
        MX_HIP(hipMemcpyAsync(idx->dead + w0, idx->dead_h.data() + w0, (w1 - w0 + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, idx->stream));
        idx->n_dead += *newly;
        idx->dead_ver += 1;
        // The side lists (zero-norm rows, rows with an out-of-range norm) keep live rows only, so that the kZeroCap / kWildCap
        // decisions and later appends count live rows.  A list that overflowed its cap is incomplete (rows past the cap were never
        // listed) and stays as it is: such an index answers on the EXACT path either way.
        auto compact = [&](uint32_t *list, uint64_t &cnt, uint64_t cap, int word) -> int {
            if (cnt == 0 || cnt > cap) return MX_OK;
            std::vector<uint32_t> z((size_t)cnt);
            MX_HIP(hipMemcpyAsync(z.data(), list, z.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, idx->stream));
            MX_HIP(hipStreamSynchronize(idx->stream));
            size_t m = 0;
            for (uint32_t r : z)
                if (!((idx->dead_h[r >> 6] >> (r & 63)) & 1ull)) z[m++] = r;  // (ascending order kept)
            if (m == z.size()) return MX_OK;
            if (m) MX_HIP(hipMemcpyAsync(list, z.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, idx->stream));
            const uint32_t c = (uint32_t)m;  // the device count the ingest kernel appends behind
            MX_HIP(hipMemcpyAsync(idx->flags + word, &c, sizeof(c), hipMemcpyHostToDevice, idx->stream));
            MX_HIP(hipStreamSynchronize(idx->stream));
            cnt = m;
            return MX_OK;
        };
        if (int rc = compact(idx->zero_rows, idx->n_zero, kZeroCap, 3); rc != MX_OK) return rc;
        if (int rc = compact(idx->wild_list, idx->n_wild, kWildCap, 4); rc != MX_OK) return rc;
    }
    MX_HIP(hipStreamSynchronize(idx->stream));
    return MX_OK;
}

// global rows (0-based, no id offset) of a plain or composite index -> removed.  The rows are < rows_of(idx) (the caller checked).
// A composite routes row r to the shard that owns its block: block b = r / R, shard b % G, local row (b / G) R + r % R.
// The rows newly removed join dead_log (what the next save appends to vectors.mxdead).
int mark_dead(mx_index *idx, const std::vector<uint64_t> &rows, uint64_t *newly) {
    *newly = 0;
    std::vector<uint8_t> fresh;
    if (!idx->composite()) {
        int rc = mark_dead_local(idx, rows, fresh, newly);
        for (size_t i = 0; i < rows.size(); ++i)
            if (fresh[i]) idx->dead_log.push_back(rows[i]);
        return rc;
    }
    const uint64_t R = idx->block_rows, G = idx->shards.size();
    std::vector<std::vector<uint64_t>> per(G), glob(G);
    for (uint64_t r : rows) {
        const uint64_t b = r / R;
        per[b % G].push_back((b / G) * R + r % R);
        glob[b % G].push_back(r);
    }
    int rc = MX_OK;
    for (uint64_t g = 0; g < G && rc == MX_OK; ++g) {
        mx_index *sh = idx->shards[g];
        std::lock_guard<std::mutex> lk(sh->mu);
        uint64_t m = 0;
        rc = mark_dead_local(sh, per[g], fresh, &m);
        *newly += m;
        for (size_t i = 0; i < glob[g].size(); ++i)
            if (fresh[i]) idx->dead_log.push_back(glob[g][i]);
    }
    idx->n_dead += *newly;
    return rc;
}

// forget every removal (the rows stay): the state mx_index_load starts from before it applies vectors.mxdead
int reset_dead(mx_index *idx) {
    for (mx_index *t : idx->composite() ? idx->shards : std::vector<mx_index *>{idx}) {
        std::unique_lock<std::mutex> lk(t->mu, std::defer_lock);
        if (t != idx) lk.lock();
        if (t->dead) {
            DeviceGuard dg(t->device);
            std::fill(t->dead_h.begin(), t->dead_h.end(), 0);
            MX_HIP(hipMemsetAsync(t->dead, 0, t->dead_h.size() * sizeof(uint64_t), t->stream));
            MX_HIP(hipStreamSynchronize(t->stream));
        }
        t->n_dead = 0;
        t->dead_ver += 1;
    }
    idx->n_dead = 0;
    idx->dead_log.clear();
    return MX_OK;
}

// vectors.mxdead: magic[8] | u64 count | count x u64 removed rows (global, without id offset), in the order they were removed.
// Entries are appended and the count is patched last (the rule of vectors.mxflat); no file = nothing removed.
// MXDEAD02 (a compacted index) has the compaction generation behind the count: it belongs to the MXFLAT02 of that generation only.
const char kDeadMagic[8] = {'M', 'X', 'D', 'E', 'A', 'D', '0', '1'};
constexpr long kDeadHeaderBytes = 16;
const char kDeadMagic2[8] = {'M', 'X', 'D', 'E', 'A', 'D', '0', '2'};
constexpr long kDeadHeader2Bytes = 24;
long dead_header_bytes(uint64_t gen) { return gen ? kDeadHeader2Bytes : kDeadHeaderBytes; }
constexpr uint64_t kDeadStale = ~0ull;  // disk_dead: the removal file in disk_dir belongs to another generation (rewrite it)
std::string dead_file(const char *dir) { return std::string(dir) + "/vectors.mxdead"; }

// reads and validates vectors.mxdead of a store of n_rows rows and compaction generation gen; *present = false when there is
// none, or when it is stale (*stale: it carries another generation -- a crash between the two files of a save)
int read_dead_file(const char *dir, uint64_t n_rows, uint64_t gen, std::vector<uint64_t> *rows, bool *present, bool *stale) {
    rows->clear();
    *present = false;
    *stale = false;
    const std::string path = dead_file(dir);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) {
        if (errno == ENOENT) return MX_OK;
        return fail(MX_EIO, "cannot open %s", path.c_str());
    }
    *present = true;
    char magic[8];
    uint64_t cnt = 0, fgen = 0;
    struct stat sb;
    int rc = MX_OK;
    const bool v1 = fread(magic, 1, 8, f) == 8 && memcmp(magic, kDeadMagic, 8) == 0;
    const bool v2 = !v1 && memcmp(magic, kDeadMagic2, 8) == 0;
    if ((!v1 && !v2) || fread(&cnt, sizeof(cnt), 1, f) != 1 || (v2 && (fread(&fgen, sizeof(fgen), 1, f) != 1 || fgen == 0)) ||
        fstat(fileno(f), &sb) != 0 || (uint64_t)sb.st_size < (uint64_t)dead_header_bytes(fgen))
        rc = fail(MX_EIO, "%s: bad header", path.c_str());
    else if (fgen != gen) {  // another generation's removals: they name rows of another vectors.mxflat
        fclose(f);
        *present = false;
        *stale = true;
        return MX_OK;
    } else if (cnt > ((uint64_t)sb.st_size - dead_header_bytes(fgen)) / 8)
        rc = fail(MX_EIO, "%s: truncated (%lld bytes for %llu entries)", path.c_str(), (long long)sb.st_size, (unsigned long long)cnt);
    if (rc == MX_OK) {
        rows->resize((size_t)cnt);
        if (cnt && fread(rows->data(), sizeof(uint64_t), (size_t)cnt, f) != (size_t)cnt) rc = fail(MX_EIO, "%s: read failed", path.c_str());
    }
    fclose(f);
    for (size_t i = 0; rc == MX_OK && i < rows->size(); ++i)
        if ((*rows)[i] >= n_rows)
            rc = fail(MX_EIO, "%s: entry %zu names row %llu of a store of %llu rows", path.c_str(), i, (unsigned long long)(*rows)[i],
                      (unsigned long long)n_rows);
    if (rc != MX_OK) rows->clear();
    return rc;
}

// brings vectors.mxdead in dir up to the handle's removals: appends the ones made since the last save when the file holds exactly
// the first disk_dead of them, otherwise writes it afresh (temporary file + rename); no removals: no file
int save_dead_file(mx_index *idx, const char *dir, bool in_sync) {
    const std::string path = dead_file(dir);
    const uint64_t total = idx->dead_log.size();
    struct stat sb;
    const bool exists = stat(path.c_str(), &sb) == 0;
    if (total == 0) {
        if (exists && unlink(path.c_str()) != 0) return fail(MX_EIO, "cannot remove %s", path.c_str());
        idx->disk_dead = 0;
        return MX_OK;
    }
    const long hb = dead_header_bytes(idx->gen);
    if (in_sync && exists && idx->disk_dead <= total && (uint64_t)sb.st_size == (uint64_t)hb + 8 * idx->disk_dead) {
        if (idx->disk_dead == total) return MX_OK;
        FILE *f = fopen(path.c_str(), "r+b");
        if (!f) return fail(MX_EIO, "cannot open %s for appending", path.c_str());
        const size_t m = (size_t)(total - idx->disk_dead);
        int rc = fseek(f, hb + (long)(8 * idx->disk_dead), SEEK_SET) == 0 &&
                         fwrite(idx->dead_log.data() + idx->disk_dead, sizeof(uint64_t), m, f) == m
                     ? MX_OK : fail(MX_EIO, "write to %s failed", path.c_str());
        // the count is patched last: a crash before this point leaves the old, consistent file
        if (rc == MX_OK && (fflush(f) != 0 || fseek(f, 8, SEEK_SET) != 0 || fwrite(&total, sizeof(total), 1, f) != 1))
            rc = fail(MX_EIO, "write to %s failed", path.c_str());
        if (fclose(f) != 0 && rc == MX_OK) rc = fail(MX_EIO, "write to %s failed", path.c_str());
        if (rc == MX_OK) idx->disk_dead = total;
        return rc;
    }
    const std::string tmp = path + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(MX_EIO, "cannot open %s for writing", tmp.c_str());
    int rc = fwrite(idx->gen ? kDeadMagic2 : kDeadMagic, 1, 8, f) == 8 && fwrite(&total, sizeof(total), 1, f) == 1 &&
                     (!idx->gen || fwrite(&idx->gen, sizeof(idx->gen), 1, f) == 1) &&
                     fwrite(idx->dead_log.data(), sizeof(uint64_t), (size_t)total, f) == (size_t)total
                 ? MX_OK : fail(MX_EIO, "write to %s failed", tmp.c_str());
    if (fclose(f) != 0 && rc == MX_OK) rc = fail(MX_EIO, "write to %s failed", tmp.c_str());
    if (rc == MX_OK && rename(tmp.c_str(), path.c_str()) != 0) rc = fail(MX_EIO, "cannot rename %s", tmp.c_str());
    if (rc != MX_OK) {
        unlink(tmp.c_str());
        return rc;
    }
    idx->disk_dead = total;
    return MX_OK;
}

int clear_locked(mx_index *idx) {
    if (idx->composite()) {
        for (mx_index *sh : idx->shards) {
            std::lock_guard<std::mutex> lk(sh->mu);
            clear_locked(sh);
        }
        idx->total = 0;
    } else {
        idx->n = 0;  // ids restart at 1 (local.rs:50,63); HBM is kept for reuse
        idx->centred = false;  // (the centre belonged to the rows that are gone: appends refill the copy uncentred)
        idx->plain_bf16_rows = 0;
        idx->wild_rows = 0;
        idx->n_zero = 0;
        idx->n_wild = 0;
        if (idx->dead) {
            DeviceGuard dg(idx->device);
            (void)hipMemsetAsync(idx->dead, 0, idx->dead_h.size() * sizeof(uint64_t), idx->stream);
            std::fill(idx->dead_h.begin(), idx->dead_h.end(), 0);
        }
        for (double &w : idx->wait_ema_us) w = 0.0;
        if (idx->flags) {
            DeviceGuard dg(idx->device);
            (void)hipMemsetAsync(idx->flags + 2, 0, 4 * sizeof(uint32_t), idx->stream);  // ec_max, zero-row count, listed-row count, rc_max
        }
    }
    idx->n_dead = 0;
    idx->dead_ver += 1;
    idx->row_epoch += 1;  // (every resident filter of the handle is stale: the rows it named are gone)
    idx->dead_log.clear();
    idx->disk_dead = 0;
    idx->disk_dir.clear();
    idx->failed = false;
    return MX_OK;
}

int add_host_locked(mx_index *idx, const float *rows, uint64_t n, uint64_t *first_id) {
    if (idx->composite()) return composite_add(idx, rows, n, first_id, false);
    DeviceGuard g(idx->device);
    if (n == 0) return add_device_locked(idx, nullptr, 0, first_id);
    // validate on the host first so that a rejected call leaves the index untouched
    const size_t total = (size_t)n * idx->dim;
    for (size_t i = 0; i < total; ++i)
        if (!std::isfinite(rows[i])) return fail(MX_EINVAL, "row %zu contains a non-finite value; nothing inserted", i / idx->dim);
    const uint64_t chunk_rows = std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)idx->dim * 4));
    Dev<float> stage;  // (add_device_locked returns host-synchronised)
    MX_HIP(stage.alloc((size_t)std::min(chunk_rows, n) * idx->dim));
    int rc = MX_OK;
    uint64_t first = 0;
    const RowMark mark = mark_rows(idx);
    for (uint64_t done = 0; done < n && rc == MX_OK; done += chunk_rows) {
        const uint64_t m = std::min(chunk_rows, n - done);
        hipError_t e = hipMemcpyAsync(stage, rows + (size_t)done * idx->dim, (size_t)m * idx->dim * sizeof(float),
                                      hipMemcpyHostToDevice, idx->stream);
        if (e != hipSuccess) {
            rc = fail(MX_EDEVICE, "hipMemcpy H2D: %s", hipGetErrorString(e));
            break;
        }
        uint64_t f = 0;
        rc = add_device_locked(idx, stage, m, &f);
        if (done == 0) first = f;
    }
    if (rc != MX_OK) rollback_rows(idx, mark);  // a later chunk failed: the earlier ones go too
    if (rc == MX_OK && first_id) *first_id = first;
    return rc;
}

int open_plain(const std::string &k, int dim, int device, mx_index **out) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(MX_EDEVICE, "no HIP device available (%s)", e == hipSuccess ? "count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(MX_EDEVICE, "device %d out of range (have %d)", device, ndev);
    if (device >= kMaxDevices) return fail(MX_EUNSUPPORTED, "device %d: at most %d devices per process", device, kMaxDevices);
    DeviceGuard g(device);
    if (!g.ok) return fail(MX_EDEVICE, "hipSetDevice(%d) failed", device);
    std::call_once(g_scan_once, [] {
        g_scan_setup_err = scan_setup();
        if (g_scan_setup_err == hipSuccess) g_scan_setup_err = scan16_setup();
        if (g_scan_setup_err == hipSuccess) g_scan_setup_err = scan16w_setup();
        if (g_scan_setup_err == hipSuccess) g_scan_setup_err = scan8_setup();
        if (g_scan_setup_err == hipSuccess) g_scan_setup_err = finish_setup();
        if (g_scan_setup_err == hipSuccess) g_scan_setup_err = subset_setup();
        if (g_scan_setup_err == hipSuccess) g_scan_setup_err = range_setup();
    });
    if (g_scan_setup_err != hipSuccess)
        return fail(MX_EDEVICE, "scan kernel setup failed: %s (is this a gfx950 device?)", hipGetErrorString(g_scan_setup_err));
    std::unique_ptr<mx_index> idx(new mx_index());
    idx->key = k;
    idx->dim = dim;
    // stored row width: a multiple of 128 dims (one scan slot); wide rows (> 768) of 256, so that the two waves
    // that share a row's k-steps in scan16w_kernel get whole slots each
    idx->ds = (int)round_up((uint64_t)dim, dim > kMaxKC * kChunkFloats ? 2 * kChunkFloats : kChunkFloats);
    idx->kc = idx->ds / kChunkFloats;
    {   // which filter copy an f32 corpus keeps (mx_index_set_filter_copy overrides): MEMEX_HIP_FILTER=bf16|i8
        const char *fk = getenv("MEMEX_HIP_FILTER");
        idx->filter_auto = !(fk && fk[0]);
        idx->filter_i8 = idx->filter_auto ? idx->ds <= kAutoI8MaxDim : (fk[0] == 'i' || fk[0] == '8');
    }
    idx->device = device;
    hipDeviceProp_t prop;
    MX_HIP(hipGetDeviceProperties(&prop, device));
    idx->n_cu = prop.multiProcessorCount;
    idx->nwg = std::max(1, std::min(idx->n_cu, kMaxScanCUs));
    {   // MEMEX_HIP_SCAN8_PAIR=0: the int8 scan keeps one 8-wave workgroup per CU for 129-256 queries (A/B runs)
        const char *pv = getenv("MEMEX_HIP_SCAN8_PAIR");
        idx->scan8_pair = !(pv && pv[0] == '0');
    }
    {   // MEMEX_HIP_EXACT_THETA=0: the int8 collect threshold from the lane maxima alone, and the sample size that goes with it (A/B runs)
        const char *pv = getenv("MEMEX_HIP_EXACT_THETA");
        idx->exact_theta = !(pv && pv[0] == '0');
    }
    idx->serial = debug_flag("serial", kSerialAll) & kSerialAll;
    idx->sample_div = debug_flag("sample_div", 0);  // read here, not per batch: debug_flag costs a getenv, a mutex and a string compare
    idx->print_records = debug_flag("records", 0) != 0;
    MX_HIP(hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking));
    MX_HIP(hipEventCreate(&idx->ev0));
    MX_HIP(hipEventCreate(&idx->ev1));
    MX_HIP(hipEventCreateWithFlags(&idx->ev_wait, hipEventDisableTiming));
    MX_HIP(idx->flags.alloc(6));
    MX_HIP(hipMemset(idx->flags, 0, 6 * sizeof(uint32_t)));
    MX_HIP(idx->zero_rows.alloc(kZeroCap));
    MX_HIP(idx->wild_list.alloc(kWildCap));
    if (device < kMaxDevices) {
        std::lock_guard<std::mutex> lk(g_lanes[device].mu);
        g_lanes[device].open_indexes += 1;
        idx->pooled = true;
    }
    *out = idx.release();
    return MX_OK;
}

// ---- compaction (mx_index_compact) ----------------------------------------------------------------------
bool row_removed(const mx_index *t, uint64_t r) {
    return t->dead && (r >> 6) < t->dead_h.size() && ((t->dead_h[r >> 6] >> (r & 63)) & 1ull);
}
// global row r of a plain or composite index is removed
bool global_removed(const mx_index *idx, uint64_t r) {
    if (!idx->composite()) return row_removed(idx, r);
    const uint64_t R = idx->block_rows, G = idx->shards.size(), b = r / R;
    return row_removed(idx->shards[b % G], (b / G) * R + r % R);
}

// After a compaction: the capacity a fresh index of the same rows would have, round_up(max(n, 1024), 64), through the
// reallocate-and-copy ensure_capacity grows with.  Old and new storage coexist for the copy; without HBM for the new one the
// larger capacity stays (not an error).
int release_capacity(mx_index *idx) {
    const uint64_t want = round_up(std::max<uint64_t>(idx->n, 1024), kTile8Rows);
    if (want >= idx->cap) return MX_OK;
    const size_t ds = (size_t)idx->ds;
    const size_t eb = idx->compressed ? 2 : idx->filter_i8 ? 1 : 2;  // bytes per element of the bf16 / int8 copy
    Dev<float> nx, nsc, nts, nam;
    Dev<void> nh;
    auto get = [](auto &b, size_t bytes) {
        if (b.alloc_bytes(bytes) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    };
    bool ok = idx->compressed || (get(nx, want * ds * 4) && get(nsc, want * sizeof(float)));
    if (ok && idx->xh) ok = get(nh, want * ds * eb);
    if (ok && idx->tsc) ok = get(nts, (want / kTile8Rows) * kTscaleFloats * sizeof(float));
    if (ok && idx->amean) ok = get(nam, want * sizeof(float));
    if (!ok) return MX_OK;
    const uint64_t used = round_up(idx->n, kTile8Rows);  // rows [n, used) were zeroed by the compaction
    hipStream_t st = idx->stream;
    auto move = [&](void *b, const void *old, size_t used_bytes, size_t all_bytes) -> hipError_t {
        hipError_t e = used_bytes ? hipMemcpyAsync(b, old, used_bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
        if (e == hipSuccess && all_bytes > used_bytes) e = hipMemsetAsync(static_cast<char *>(b) + used_bytes, 0, all_bytes - used_bytes, st);
        return e;
    };
    if (!idx->compressed) {
        MX_HIP(move(nx, idx->x, used * ds * 4, want * ds * 4));
        MX_HIP(move(nsc, idx->scale, used * sizeof(float), want * sizeof(float)));
    }
    if (nh) MX_HIP(move(nh, idx->xh, used * ds * eb, want * ds * eb));
    if (nts) MX_HIP(move(nts, idx->tsc, (used / kTile8Rows) * kTscaleFloats * sizeof(float), (want / kTile8Rows) * kTscaleFloats * sizeof(float)));
    if (nam) MX_HIP(move(nam, idx->amean, used * sizeof(float), want * sizeof(float)));
    MX_HIP(hipStreamSynchronize(st));
    if (nx) idx->x = std::move(nx);
    if (nsc) idx->scale = std::move(nsc);
    if (nh) idx->xh = std::move(nh);
    if (nts) idx->tsc = std::move(nts);
    if (nam) idx->amean = std::move(nam);
    idx->cap = want;
    return MX_OK;
}

// Compacts a plain index (or one shard) in place.  Everything that can fail without harm -- the plan, every allocation, the
// device prefix checked against the host's count -- comes first; *moved turns true before the first row moves.
int compact_plain(mx_index *idx, bool *moved) {
    *moved = false;
    DeviceGuard dg(idx->device);
    hipStream_t st = idx->stream;
    const uint64_t n = idx->n, tiles = (n + kTile8Rows - 1) / kTile8Rows, ds = (uint64_t)idx->ds;
    if (!idx->dead || idx->dead_h.size() < tiles) return fail(MX_EDEVICE, "removal mask smaller than the index");
    // live rows before every tile, on the host (the chunk plan) and on the device (the gather's destinations)
    std::vector<uint64_t> hp((size_t)tiles + 1, 0);
    uint64_t t_first = tiles;
    for (uint64_t t = 0; t < tiles; ++t) {
        const uint64_t r0 = t * kTile8Rows;
        const uint64_t valid = n - r0 >= (uint64_t)kTile8Rows ? ~0ull : (1ull << (n - r0)) - 1ull;
        const uint64_t live = ~idx->dead_h[t] & valid;
        if (live != valid && t_first == tiles) t_first = t;
        hp[t + 1] = hp[t] + (uint64_t)__builtin_popcountll(live);
    }
    const uint64_t n_live = hp[tiles];
    if (n_live != n - idx->n_dead) return fail(MX_EDEVICE, "removal bookkeeping out of step (%llu live rows counted, %llu expected)",
                                               (unsigned long long)n_live, (unsigned long long)(n - idx->n_dead));
    if (idx->compressed) t_first = 0;  // the bf16 rows are re-ingested from the first: the zero-norm list is rebuilt whole
    const uint32_t nb = compact_count_blocks(tiles);
    Dev<uint32_t> tile_base, blk_off;
    Dev<float> stage, wa, wb;
    MX_HIP(tile_base.alloc(std::max<uint64_t>(tiles, 1)));
    MX_HIP(blk_off.alloc((size_t)nb + 1));
    // staging of a chunk whose destination overlaps its source: 64 MiB of rows, a multiple of 64 rows
    const uint64_t stage_tiles = std::max<uint64_t>(1, (64ull << 20) / (kTile8Rows * ds * 4));
    constexpr uint64_t kWinTiles = 16384 / kTile8Rows;  // compressed corpus: rows widened per chunk (the append path's window holds 65536)
    if (idx->compressed) {
        MX_HIP(wa.alloc((size_t)kWinTiles * kTile8Rows * idx->dim));
        MX_HIP(wb.alloc((size_t)kWinTiles * kTile8Rows * idx->dim));
        if (!idx->xs) {
            MX_HIP(idx->xs.alloc((size_t)(65536 + kTileRows) * idx->ds));
            MX_HIP(idx->ss.alloc((size_t)(65536 + kTileRows)));
            idx->xs_rows = 65536 + kTileRows;
        }
    } else {
        MX_HIP(stage.alloc((size_t)stage_tiles * kTile8Rows * (ds + 1)));
    }
    MX_HIP(launch_compact_prefix(st, idx->dead, n, tile_base, blk_off));
    uint32_t dev_live = 0;
    MX_HIP(hipMemcpyAsync(&dev_live, blk_off + nb, sizeof(dev_live), hipMemcpyDeviceToHost, st));
    MX_HIP(hipStreamSynchronize(st));
    if (dev_live != n_live) return fail(MX_EDEVICE, "device removal mask out of step (%u live rows, %llu expected)", dev_live,
                                        (unsigned long long)n_live);

    *moved = true;  // ---- from here on rows move: an error leaves the index failed
    if (!idx->compressed) {
        float *sx = stage, *ss = sx + stage_tiles * kTile8Rows * ds;
        for (uint64_t t = t_first; t < tiles;) {
            const uint64_t lag = t * kTile8Rows - hp[t];  // rows removed before tile t
            uint64_t c;
            if (lag >= stage_tiles * kTile8Rows) {
                // every destination of the next lag / 64 tiles lies below their first source row: gather straight into place
                c = std::min(tiles - t, lag / kTile8Rows);
                MX_HIP(launch_compact_gather(st, idx->dead, n, t, c, tile_base, blk_off, idx->x + t * kTile8Rows * ds, idx->scale + t * kTile8Rows,
                                             (int)ds, 0, idx->x, idx->scale));
            } else {
                c = std::min(tiles - t, stage_tiles);
                MX_HIP(launch_compact_gather(st, idx->dead, n, t, c, tile_base, blk_off, idx->x + t * kTile8Rows * ds, idx->scale + t * kTile8Rows,
                                             (int)ds, hp[t], sx, ss));
                const uint64_t m = hp[t + c] - hp[t];
                if (m) {
                    MX_HIP(hipMemcpyAsync(idx->x + hp[t] * ds, sx, m * ds * sizeof(float), hipMemcpyDeviceToDevice, st));
                    MX_HIP(hipMemcpyAsync(idx->scale + hp[t], ss, m * sizeof(float), hipMemcpyDeviceToDevice, st));
                }
            }
            t += c;
        }
        // rows past the new end read as a fresh append leaves them: zeros
        const uint64_t z1 = std::min<uint64_t>(round_up(n, kTile8Rows), idx->cap);
        MX_HIP(hipMemsetAsync(idx->x + n_live * ds, 0, (z1 - n_live) * ds * sizeof(float), st));
        MX_HIP(hipMemsetAsync(idx->scale + n_live, 0, (z1 - n_live) * sizeof(float), st));
        // the side lists afresh in the new numbering: a list that had overflowed is complete again when the live rows fit
        MX_HIP(hipMemsetAsync(idx->flags, 0, 2 * sizeof(uint32_t), st));
        MX_HIP(hipMemsetAsync(idx->flags + 3, 0, 2 * sizeof(uint32_t), st));
        MX_HIP(launch_relist(st, idx->x, idx->scale, n_live, idx->ds, idx->flags, idx->zero_rows, idx->wild_list));
        idx->n = n_live;
        idx->n_zero = 0;
        idx->n_wild = 0;
        uint32_t fl[5] = {0, 0, 0, 0, 0};
        if (int rc = commit_ingest(idx, fl); rc != MX_OK) return rc;
        // the filter copy over the compacted rows, of the kind and centring it had (a centred copy: around the live rows' mean)
        if (idx->xh) {
            MX_HIP(hipMemsetAsync(idx->flags + 2, 0, sizeof(uint32_t), st));
            MX_HIP(hipMemsetAsync(idx->flags + 5, 0, sizeof(uint32_t), st));
            const bool ctr = idx->centred && idx->amean && idx->mean && idx->msum;
            if (ctr && n_live) MX_HIP(launch_mean_dir(st, idx->x, idx->scale, n_live, idx->ds, idx->msum, idx->mean));
            const uint32_t t1 = (uint32_t)((n_live + kTileRows - 1) / kTileRows);
            if (n_live) {
                if (idx->filter_i8)
                    MX_HIP(launch_shadow8(st, idx->x, idx->scale, idx->ds, 0, (uint32_t)round_up(t1, 2), n_live, idx->xh, idx->tsc, idx->flags + 2,
                                          ctr ? idx->mean : nullptr, ctr ? idx->amean : nullptr, ctr ? idx->flags + 5 : nullptr));
                else
                    MX_HIP(launch_shadow(st, idx->x, idx->scale, idx->ds, 0, t1, idx->xh, idx->flags + 2, 0, 0, ~0ull, ctr ? idx->mean : nullptr,
                                         ctr ? idx->amean : nullptr));
            }
        }
    } else {
        // the bf16 fragments are the only copy of the rows: per window, widen them (launch_unshadow), keep the live ones, and
        // append those through the raw-ingest path behind the rows already moved -- how mx_index_load reproduces stored rows
        float *wa_f = wa, *wb_f = wb;
        MX_HIP(hipMemsetAsync(idx->flags + 2, 0, 3 * sizeof(uint32_t), st));
        idx->n = 0;
        idx->n_zero = 0;
        idx->n_wild = 0;
        idx->wild_rows = 0;
        idx->raw_ingest = true;
        int rc = MX_OK;
        for (uint64_t t = 0; t < tiles && rc == MX_OK; t += kWinTiles) {
            const uint64_t c = std::min(kWinTiles, tiles - t), r0 = t * kTile8Rows, rows = std::min(c * kTile8Rows, n - r0);
            hipError_t e = launch_unshadow(st, idx->xh, idx->ds, idx->dim, r0, rows, wa_f);
            if (e == hipSuccess) e = launch_compact_gather(st, idx->dead, n, t, c, tile_base, blk_off, wa_f, nullptr, idx->dim, hp[t], wb_f, nullptr);
            if (e != hipSuccess) rc = fail(MX_EDEVICE, "compaction of the bf16 rows: %s", hipGetErrorString(e));
            else rc = add_device_locked(idx, wb_f, hp[t + c] - hp[t], nullptr);
        }
        idx->raw_ingest = false;
        if (rc != MX_OK) return rc;
        // rows past the new end of its 32-row tile hold zeros, as a fresh append leaves them
        const uint64_t z1 = round_up(n_live, kTileRows);
        if (z1 > n_live) {
            MX_HIP(hipMemsetAsync(idx->xs, 0, (size_t)kTileRows * ds * sizeof(float), st));
            MX_HIP(hipMemsetAsync(idx->ss, 0, (size_t)kTileRows * sizeof(float), st));
            const uint32_t tl = (uint32_t)(n_live / kTileRows);
            MX_HIP(launch_shadow(st, idx->xs, idx->ss, idx->ds, tl, tl + 1, idx->xh, idx->flags + 2, tl, n_live, z1));
        }
    }
    MX_HIP(hipStreamSynchronize(st));
    // no row is removed any more: the launchers pass a null mask and run the unmasked kernels again
    idx->dead.reset();
    idx->dead_h.clear();
    idx->dead_h.shrink_to_fit();
    idx->n_dead = 0;
    // the doubling thresholds of the filter copy's promotion rules follow the rows they were set on
    auto rescale = [&](uint64_t &v) {
        if (v) v = std::max<uint64_t>(1, (uint64_t)((double)v * (double)n_live / (double)std::max<uint64_t>(n, 1)));
    };
    rescale(idx->demoted_at_rows);
    rescale(idx->plain_bf16_rows);
    return release_capacity(idx);
}

// Compacts a sharded handle: global row r lives on shard (r / R) % G, so compaction re-deals rows between shards.  New shards
// (same devices and settings) take the live rows through the fetch and append paths in bounded chunks; they replace the old ones
// only once complete, so a failure leaves the handle as it was.  Costs HBM for both sets of shards and a trip through host memory.
int compact_composite(mx_index *idx) {
    const uint64_t R = idx->block_rows, G = idx->shards.size(), total = idx->total;
    std::unique_ptr<mx_index, IndexCloser> fresh(new mx_index());  // a composite shell that composite_add fills; frees the shards it ends up with
    fresh->dim = idx->dim;
    fresh->block_rows = R;
    for (uint64_t g = 0; g < G; ++g) {
        mx_index *old = idx->shards[g], *sh = nullptr;
        int rc = open_plain("", idx->dim, old->device, &sh);
        if (rc != MX_OK) return rc;
        sh->idmap = old->idmap;
        sh->mode = old->mode;
        sh->profiling = old->profiling;
        sh->scan8_pair = old->scan8_pair;
        sh->exact_theta = old->exact_theta;
        sh->sample_div = old->sample_div;
        sh->serial = old->serial;
        sh->print_records = old->print_records;
        sh->want_filter = old->want_filter;
        sh->filter_i8 = old->filter_i8;
        sh->filter_auto = old->filter_auto;
        sh->compressed = old->compressed;
        sh->raw_ingest = old->compressed;  // stored values of a compressed corpus go back in unchanged
        fresh->shards.push_back(sh);
    }
    const uint64_t chunk = std::max<uint64_t>(kTile8Rows, (32ull << 20) / ((uint64_t)idx->dim * 4));
    std::vector<float> buf((size_t)std::min<uint64_t>(chunk, std::max<uint64_t>(total, 1)) * idx->dim), tmpv;
    int rc = MX_OK;
    for (uint64_t r0 = 0; r0 < total && rc == MX_OK; r0 += chunk) {
        const uint64_t m = std::min(chunk, total - r0);
        rc = fetch_rows(idx, r0, m, buf.data(), tmpv);
        uint64_t k = 0;  // live rows of the chunk, packed to the front
        for (uint64_t i = 0; i < m && rc == MX_OK; ++i) {
            if (global_removed(idx, r0 + i)) continue;
            if (k != i) memmove(buf.data() + k * idx->dim, buf.data() + i * idx->dim, (size_t)idx->dim * sizeof(float));
            ++k;
        }
        if (rc == MX_OK && k) rc = composite_add(fresh.get(), buf.data(), k, nullptr, false);
    }
    for (mx_index *sh : fresh->shards) sh->raw_ingest = false;
    if (rc != MX_OK) return rc;
    std::swap(idx->shards, fresh->shards);  // (the old shards go with `fresh`)
    idx->total = fresh->total;
    idx->n_dead = 0;
    return MX_OK;
}

int usable(mx_index *idx) {
    if (!idx->failed) return MX_OK;
    return fail(MX_EDEVICE, "this index is unusable: a compaction failed after rows had moved (mx_index_clear or mx_index_load resets it)");
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char *mx_last_error(void) { return last_error_slot().c_str(); }
const char *mx_version(void) { return "memex-hip 0.6.0 (gfx950)"; }
size_t mx_index_stats_size(void) { return sizeof(mx_index_stats); }

int mx_device_count(int *n) try {
    if (!n) return fail(MX_EINVAL, "null argument");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        return fail(MX_EDEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *n = c;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_open(const char *key, int dim, int device, mx_index **out) try {
    if (!out) return fail(MX_EINVAL, "out is null");
    *out = nullptr;
    if (dim < 1 || dim > (1 << 16)) return fail(MX_EINVAL, "dim %d out of range: 1 <= dim <= %d", dim, 1 << 16);
    const std::string k = key ? key : "";
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (!k.empty()) {
        auto it = g_registry.find(k);
        if (it != g_registry.end()) {
            mx_index *idx = it->second;
            if (idx->dim != dim) return fail(MX_EINVAL, "index '%s' is open with dim %d, not %d", k.c_str(), idx->dim, dim);
            if (!idx->composite() && idx->device != device)
                return fail(MX_EINVAL, "index '%s' lives on device %d, not %d", k.c_str(), idx->device, device);
            idx->refs += 1;
            *out = idx;
            return MX_OK;
        }
    }
    mx_index *raw = nullptr;
    int rc = open_plain(k, dim, device, &raw);
    if (rc != MX_OK) return rc;
    if (!k.empty()) g_registry[k] = raw;
    *out = raw;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_open_sharded(const char *key, int dim, int n_dev, const int *devices, uint64_t block_rows, mx_index **out) try {
    if (!out) return fail(MX_EINVAL, "out is null");
    *out = nullptr;
    if (dim < 1 || dim > (1 << 16)) return fail(MX_EINVAL, "dim %d out of range: 1 <= dim <= %d", dim, 1 << 16);
    if (n_dev < 1 || n_dev > 64) return fail(MX_EINVAL, "n_dev %d out of range", n_dev);
    const std::string k = key ? key : "";
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (!k.empty()) {
        auto it = g_registry.find(k);
        if (it != g_registry.end()) {
            mx_index *idx = it->second;
            if (idx->dim != dim) return fail(MX_EINVAL, "index '%s' is open with dim %d, not %d", k.c_str(), idx->dim, dim);
            if ((int)idx->shards.size() != n_dev) return fail(MX_EINVAL, "index '%s' is open with %zu shards, not %d", k.c_str(), idx->shards.size(), n_dev);
            idx->refs += 1;
            *out = idx;
            return MX_OK;
        }
    }
    std::unique_ptr<mx_index, IndexCloser> idx(new mx_index());  // (shards already opened are freed on any failure, an exception too)
    idx->key = k;
    idx->dim = dim;
    idx->block_rows = round_up(block_rows ? block_rows : 65536, kTileRows);
    bool distinct = n_dev > 1;
    for (int g = 0; g < n_dev; ++g) {
        const int dev = devices ? devices[g] : g;
        mx_index *sh = nullptr;
        int rc = open_plain("", dim, dev, &sh);
        if (rc != MX_OK) return rc;
        sh->idmap = IdMap{0, (uint32_t)idx->block_rows, (uint32_t)n_dev, (uint32_t)g};
        idx->shards.push_back(sh);
        for (int h = 0; h < g; ++h) distinct = distinct && idx->shards[h]->device != dev;
    }
    idx->device = idx->shards[0]->device;
    // exchange: RCCL all-gather when every shard has its own device (MEMEX_HIP_EXCHANGE=p2p forces
    // peer copies, =rccl insists on RCCL and fails without it); logical shards on one device use copies
    const char *ex = getenv("MEMEX_HIP_EXCHANGE");
    const bool want_rccl = ex ? strcmp(ex, "rccl") == 0 : distinct;
    const bool forbid_rccl = ex && strcmp(ex, "p2p") == 0;
    if (want_rccl && !forbid_rccl && (distinct || n_dev == 1)) {
        std::string why;
        if (g_rccl_broken) {
            why = "an earlier RCCL initialisation of this process hung";
        } else if (!load_rccl()) {
            why = "librccl.so.1 cannot be loaded";
        } else {
            // ncclCommInitAll under a watchdog (MEMEX_HIP_RCCL_TIMEOUT seconds, default 30): on a node where it never
            // returns, the thread is abandoned and this process exchanges by peer copies from here on
            struct Init {
                std::mutex mu;
                std::condition_variable cv;
                bool done = false;
                int rc = -1;
                std::vector<void *> comms;
                std::vector<int> devs;
            };
            auto init = std::make_shared<Init>();
            for (mx_index *sh : idx->shards) init->devs.push_back(sh->device);
            init->comms.assign(n_dev, nullptr);
            std::thread([init, n_dev] {
                const int rc = g_rccl.CommInitAll(init->comms.data(), n_dev, init->devs.data());
                std::lock_guard<std::mutex> l2(init->mu);
                init->rc = rc;
                init->done = true;
                init->cv.notify_all();
            }).detach();
            const char *tv = getenv("MEMEX_HIP_RCCL_TIMEOUT");
            const double secs = tv && atof(tv) > 0.0 ? atof(tv) : 30.0;
            std::unique_lock<std::mutex> l2(init->mu);
            if (!init->cv.wait_for(l2, std::chrono::duration<double>(secs), [&] { return init->done; })) {
                g_rccl_broken = true;
                why = "ncclCommInitAll did not return in time";
            } else if (init->rc != 0) {
                why = std::string("ncclCommInitAll failed: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(init->rc) : "?");
            } else {
                idx->comms = init->comms;
                if (rccl_selftest(idx.get(), secs)) {
                    idx->use_rccl = true;
                } else {
                    why = "the first all-gather failed or did not complete";
                    idx->comms.clear();  // (not destroyed: a communicator with a collective in an unknown state)
                }
            }
        }
        if (!idx->use_rccl) {
            if (ex)  // MEMEX_HIP_EXCHANGE=rccl insists
                return fail(MX_EDEVICE, "MEMEX_HIP_EXCHANGE=rccl: %s", why.c_str());
            fprintf(stderr, "memex-hip: sharded index '%s' exchanges by peer copies (%s)\n", k.c_str(), why.c_str());
        }
    }
    if (!idx->use_rccl && distinct) enable_peer_access(idx.get());
    {   // helper threads: one per shard >= 1 when every shard has its own device.  MEMEX_HIP_SHARD_THREADS=1
        // forces them for logical shards on one device too (how the hand-off is tested on a 1-GPU box), =0 never
        const char *tv = getenv("MEMEX_HIP_SHARD_THREADS");
        const bool threads = tv ? tv[0] == '1' : distinct;
        if (threads && n_dev > 1) idx->pool.reset(new ShardPool(n_dev - 1));
    }
    mx_index *raw = idx.release();
    if (!k.empty()) g_registry[k] = raw;
    *out = raw;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

// how the shards of `idx` exchange their top-k blocks: 0 = not sharded, 1 = copies into a slot per shard on
// devices[0] (peer-to-peer between devices), 2 = RCCL all-gather
int mx_index_exchange(mx_index *idx, int *kind) try {
    if (!idx || !kind) return fail(MX_EINVAL, "null argument");
    *kind = !idx->composite() ? 0 : (idx->use_rccl ? 2 : 1);
    return MX_OK;
} catch (...) {
    return guard_exception();
}

void mx_index_close(mx_index *idx) {
    if (!idx) return;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        if (--idx->refs > 0) return;
        if (!idx->key.empty()) g_registry.erase(idx->key);
    }
    free_index(idx);
}

int mx_index_dim(mx_index *idx, int *dim) try {
    if (!idx || !dim) return fail(MX_EINVAL, "null argument");
    *dim = idx->dim;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_n_shards(mx_index *idx, int *n) try {
    if (!idx || !n) return fail(MX_EINVAL, "null argument");
    *n = idx->composite() ? (int)idx->shards.size() : 1;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_size(mx_index *idx, uint64_t *n) try {
    if (!idx || !n) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    *n = rows_of(idx);
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_remove(mx_index *idx, const uint64_t *ids, uint64_t n, uint64_t *n_removed) try {
    if (n_removed) *n_removed = 0;
    if (!idx || (!ids && n)) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    const uint64_t size = rows_of(idx), off = idx->idmap.id_offset;
    std::vector<uint64_t> rows((size_t)n);
    for (uint64_t i = 0; i < n; ++i) {  // all ids are checked before anything changes
        if (ids[i] <= off || ids[i] - off > size)
            return fail(MX_EINVAL, "id %llu is outside [%llu, %llu]; nothing removed", (unsigned long long)ids[i], (unsigned long long)(off + 1),
                        (unsigned long long)(off + size));
        rows[i] = ids[i] - off - 1;
    }
    uint64_t m = 0;
    const int rc = mark_dead(idx, rows, &m);
    if (n_removed) *n_removed = m;
    return rc;
} catch (...) {
    return guard_exception();
}

int mx_index_removed(mx_index *idx, uint64_t *n) try {
    if (!idx || !n) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    *n = idx->n_dead;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_compact(mx_index *idx, uint64_t *kept_ids, uint64_t kept_cap, uint64_t *n_live) try {
    if (n_live) *n_live = 0;
    if (!idx) return fail(MX_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(idx->mu);  // the lock a combined search pass holds: searches see the old rows or the new ones
    if (int rc = usable(idx); rc != MX_OK) return rc;
    const uint64_t size = rows_of(idx), live = size - idx->n_dead, off = idx->idmap.id_offset;
    if (kept_ids && kept_cap < live)
        return fail(MX_EINVAL, "kept_ids holds %llu entries, %llu live rows; nothing changed", (unsigned long long)kept_cap, (unsigned long long)live);
    if (kept_ids) {  // the id every new id had before, from the host copy of the removal masks
        uint64_t k = 0;
        for (uint64_t r = 0; r < size; ++r)
            if (!idx->n_dead || !global_removed(idx, r)) kept_ids[k++] = off + r + 1;
    }
    if (idx->n_dead == 0) {  // nothing removed: the identity, the index and its disk state untouched
        if (n_live) *n_live = size;
        return MX_OK;
    }
    bool moved = false;
    int rc;
    if (idx->composite()) {
        rc = compact_composite(idx);
    } else {
        rc = compact_plain(idx, &moved);
        if (rc != MX_OK && moved) {
            const std::string why = last_error_slot();
            idx->failed = true;
            idx->row_epoch += 1;
            return fail(MX_EDEVICE, "compaction failed after rows had moved (%s); the index is unusable until mx_index_clear or mx_index_load",
                        why.c_str());
        }
    }
    if (rc != MX_OK) return rc;
    // the store on disk no longer matches: the next save rewrites it whole, in the next generation's formats
    idx->gen += 1;
    idx->row_epoch += 1;  // the rows were renumbered: resident filters of the old numbering are stale
    idx->n_dead = 0;
    idx->dead_log.clear();
    idx->disk_dead = 0;
    idx->disk_dir.clear();
    if (n_live) *n_live = rows_of(idx);
    return MX_OK;
} catch (...) {
    return guard_exception();
}

static int reserve_locked(mx_index *idx, uint64_t rows) {
    if (idx->composite()) {
        const uint64_t G = idx->shards.size();
        for (uint64_t g = 0; g < G; ++g) {
            mx_index *sh = idx->shards[g];
            std::lock_guard<std::mutex> l2(sh->mu);
            DeviceGuard dg(sh->device);
            int rc = ensure_capacity(sh, shard_rows(rows, idx->block_rows, G, g));
            if (rc != MX_OK) return rc;
        }
        return MX_OK;
    }
    DeviceGuard g(idx->device);
    return ensure_capacity(idx, rows);
}

int mx_index_reserve(mx_index *idx, uint64_t rows) try {
    if (!idx) return fail(MX_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    return reserve_locked(idx, rows);
} catch (...) {
    return guard_exception();
}

int mx_index_set_id_offset(mx_index *idx, uint64_t off) try {
    if (!idx) return fail(MX_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->idmap.id_offset = off;
    for (mx_index *sh : idx->shards) sh->idmap.id_offset = off;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_wait_stream(mx_index *idx, void *stream) try {
    if (!idx) return fail(MX_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(idx->mu);
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    DeviceGuard g(t->device);
    // nothing pending on the caller's stream (the usual case between two searches): no event, no dependency to process --
    // one query call instead of a record + wait pair in front of every batch
    if (hipStreamQuery(static_cast<hipStream_t>(stream)) == hipSuccess) return MX_OK;
    (void)hipGetLastError();
    MX_HIP(hipEventRecord(t->ev_wait, static_cast<hipStream_t>(stream)));
    MX_HIP(hipStreamWaitEvent(t->stream, t->ev_wait, 0));
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_add_device(mx_index *idx, const float *d_rows, uint64_t n, uint64_t *first_id) try {
    if (!idx || (!d_rows && n)) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (idx->composite()) {
        {   // rows must be complete on shards[0]'s stream before other devices copy them
            DeviceGuard dg(idx->shards[0]->device);
            MX_HIP(hipStreamSynchronize(idx->shards[0]->stream));
        }
        return composite_add(idx, d_rows, n, first_id, true);
    }
    DeviceGuard g(idx->device);
    return add_device_locked(idx, d_rows, n, first_id);
} catch (...) {
    return guard_exception();
}

int mx_index_add(mx_index *idx, const float *rows, uint64_t n, uint64_t *first_id) try {
    if (!idx || (!rows && n)) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    return add_host_locked(idx, rows, n, first_id);
} catch (...) {
    return guard_exception();
}

int mx_index_clear(mx_index *idx) try {
    if (!idx) return fail(MX_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(idx->mu);
    return clear_locked(idx);
} catch (...) {
    return guard_exception();
}

int mx_index_set_search_mode(mx_index *idx, int mode) try {
    if (!idx) return fail(MX_EINVAL, "null index");
    if (mode != MX_SEARCH_AUTO && mode != MX_SEARCH_EXACT) return fail(MX_EINVAL, "unknown search mode %d", mode);
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->mode = mode;
    for (mx_index *sh : idx->shards) sh->mode = mode;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

namespace {

// the ranges argument of the filtered entry points -> normalised id ranges; MX_EINVAL for a null array or a pair with lo > hi
int read_id_ranges(const uint64_t *ranges, uint64_t n_ranges, Ranges *out) {
    if (!ranges && n_ranges) return fail(MX_EINVAL, "null ranges with n_ranges = %llu", (unsigned long long)n_ranges);
    out->clear();
    out->reserve((size_t)n_ranges);
    for (uint64_t i = 0; i < n_ranges; ++i) {
        if (ranges[2 * i] > ranges[2 * i + 1])
            return fail(MX_EINVAL, "range %llu is [%llu, %llu): lo > hi; nothing searched", (unsigned long long)i,
                        (unsigned long long)ranges[2 * i], (unsigned long long)ranges[2 * i + 1]);
        out->emplace_back(ranges[2 * i], ranges[2 * i + 1]);
    }
    normalise_ranges(*out);
    return MX_OK;
}

// a resident filter named in a call on idx (under idx->mu): made for this handle, and not older than its rows
int check_filter(const mx_index *idx, const mx_filter *f) {
    if (f->idx != idx) return fail(MX_EINVAL, "the filter was made for another index");
    if (f->epoch != idx->row_epoch)
        return fail(MX_EINVAL, "the filter is stale: the index was cleared, loaded or compacted after it was made (destroy it and make a new one)");
    return MX_OK;
}

// mx_index_search_device and its filtered forms (id_filt: normalised id ranges, res: a resident filter; at most one of them)
int search_device(mx_index *idx, const float *d_q, int B, int k, uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_nfound,
                  const Ranges *id_filt, mx_filter *res = nullptr) {
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (B < 0 || k < 0) return fail(MX_EINVAL, "negative batch or k");
    if (B == 0) return MX_OK;
    if (!d_q || !d_nfound || (k > 0 && (!d_ids || !d_scores))) return fail(MX_EINVAL, "null argument");
    if (k > 4096) return fail(MX_EUNSUPPORTED, "k = %d > 4096", k);
    std::lock_guard<std::mutex> lk(idx->mu);
    DeviceGuard g(idx->device);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (res)
        if (int rc = check_filter(idx, res); rc != MX_OK) return rc;
    Ranges rows;
    if (id_filt) rows = rows_of_ids(*id_filt, idx->idmap.id_offset, rows_of(idx));  // (under idx->mu)
    const FilterArg fa{id_filt ? &rows : nullptr, res, 0};
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, B - b0);
        int rc = any_batch(idx, d_q + (size_t)b0 * idx->dim, nb, k, d_ids + (size_t)b0 * k,
                           d_scores + (size_t)b0 * k, d_dists ? d_dists + (size_t)b0 * k : nullptr, d_nfound + b0,
                           id_filt || res ? &fa : nullptr);
        if (rc != MX_OK) return rc;
    }
    return MX_OK;
}

}  // namespace

int mx_index_search_device(mx_index *idx, const float *d_q, int B, int k, uint64_t *d_ids, float *d_scores,
                           float *d_dists, int32_t *d_nfound) try {
    return search_device(idx, d_q, B, k, d_ids, d_scores, d_dists, d_nfound, nullptr);
} catch (...) {
    return guard_exception();
}

int mx_index_search_filtered_device(mx_index *idx, const float *d_q, int B, int k, const uint64_t *ranges, uint64_t n_ranges,
                                    uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_nfound) try {
    Ranges ids;
    if (int rc = read_id_ranges(ranges, n_ranges, &ids); rc != MX_OK) return rc;
    return search_device(idx, d_q, B, k, d_ids, d_scores, d_dists, d_nfound, &ids);
} catch (...) {
    return guard_exception();
}

namespace {

// the results of a batch of nb queries, `width` wide, from the index's device outputs into its pinned staging buffers: one D2H per
// output array, host-synchronised (width = 0, a top-k search at k = 0: the counts alone).  static, like scatter_to_caller: a function
// of an unnamed namespace inside extern "C" is exported under its plain name
static int copy_out_to_host(mx_index *t, int nb, int width, bool want_nrange) {
    Scratch &s = t->s;
    if (width > 0) {
        MX_HIP(hipMemcpyAsync(s.h_ids, s.out_ids, (size_t)nb * width * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
        MX_HIP(hipMemcpyAsync(s.h_scores, s.out_scores, (size_t)nb * width * sizeof(float), hipMemcpyDeviceToHost, t->stream));
        MX_HIP(hipMemcpyAsync(s.h_dists, s.out_dists, (size_t)nb * width * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    }
    MX_HIP(hipMemcpyAsync(s.h_nf, s.out_nfound, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    if (want_nrange) MX_HIP(hipMemcpyAsync(s.h_nr, s.out_nrange, (size_t)nb * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
    MX_HIP(hipStreamSynchronize(t->stream));
    return MX_OK;
}

// queries [b0, b0 + n) of the staged results to a caller's arrays (dists, n_in_range: null = not wanted)
static void scatter_to_caller(const Scratch &s, int b0, int n, int width, uint64_t *ids, float *scores, float *dists, int32_t *n_found,
                              uint64_t *n_in_range) {
    if (width > 0) {
        memcpy(ids, s.h_ids + (size_t)b0 * width, (size_t)n * width * sizeof(uint64_t));
        memcpy(scores, s.h_scores + (size_t)b0 * width, (size_t)n * width * sizeof(float));
        if (dists) memcpy(dists, s.h_dists + (size_t)b0 * width, (size_t)n * width * sizeof(float));
    }
    memcpy(n_found, s.h_nf + b0, (size_t)n * sizeof(int32_t));
    if (n_in_range) memcpy(n_in_range, s.h_nr + b0, (size_t)n * sizeof(uint64_t));
}

// one GPU batch (sum of B <= 256, same k) for a group of host requests: queries are packed into
// pinned memory, one H2D, the search pipeline, one D2H per output array, results scattered to the callers.
// A range pass (every request of it has the same cap, k): the requests' dist bounds side by side, and the n_in_range staging
int run_combined(mx_index *idx, const std::vector<SearchReq *> &batch) {
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;  // owner of the staging buffers and the stream
    DeviceGuard g(t->device);
    const int k = batch[0]->k;
    const bool range = batch[0]->dlim != nullptr;
    Ranges rows;  // a filtered pass: every request of it has the same ranges, or names the same resident filter
    if (batch[0]->filt) rows = rows_of_ids(*batch[0]->filt, idx->idmap.id_offset, rows_of(idx));
    if (batch[0]->res)
        if (int rc = check_filter(idx, batch[0]->res); rc != MX_OK) return rc;
    const FilterArg fa{batch[0]->filt ? &rows : nullptr, batch[0]->res, 0};
    const FilterArg *filt = batch[0]->filt || batch[0]->res ? &fa : nullptr;
    int rc = ensure_scratch(t);
    if (rc != MX_OK) return rc;
    rc = ensure_out(t, k);
    if (rc != MX_OK) return rc;
    Scratch &s = t->s;
    const size_t dim = (size_t)idx->dim;
    int nb = 0;
    std::vector<uint32_t> dl;
    for (const SearchReq *r : batch) {
        memcpy(s.h_q + (size_t)nb * dim, r->q, (size_t)r->B * dim * sizeof(float));
        if (range) dl.insert(dl.end(), r->dlim, r->dlim + r->B);
        nb += r->B;
    }
    // A plain index reads the queries from, and writes the answers into, the pinned staging buffers themselves (they are mapped
    // into the device's address space): prep_queries_kernel is the only reader of the raw queries, finish_kernel (or the EXACT
    // kernels) the only writers of the outputs, and every exit of search_batch is host-synchronised -- through the completion
    // word, behind a system-scope fence per workgroup, on the fast path.  That is one H2D copy, four D2H copies and a stream
    // synchronise less per call: 25-30 us of a single query's 95-115 us on a small collection (profiles/r5_small_corpus_latency.txt).
    // A sharded index merges on the device and copies as before.
    if (!idx->composite()) {
        s.out_on_host = true;
        rc = range ? any_range_batch(idx, s.h_q, nb, k, dl.data(), s.h_ids, s.h_scores, s.h_dists, s.h_nf, s.h_nr)
                   : any_batch(idx, s.h_q, nb, k, s.h_ids, s.h_scores, s.h_dists, s.h_nf, filt);
        s.out_on_host = false;
        if (rc != MX_OK) return rc;
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        MX_HIP(hipMemcpyAsync(s.qstage, s.h_q, (size_t)nb * dim * sizeof(float), hipMemcpyHostToDevice, t->stream));
        rc = range ? any_range_batch(idx, s.qstage, nb, k, dl.data(), s.out_ids, s.out_scores, s.out_dists, s.out_nfound, s.out_nrange)
                   : any_batch(idx, s.qstage, nb, k, s.out_ids, s.out_scores, s.out_dists, s.out_nfound, filt);
        if (rc != MX_OK) return rc;
        if ((rc = copy_out_to_host(t, nb, k, range)) != MX_OK) return rc;
    }
    int b0 = 0;
    for (SearchReq *r : batch) {
        scatter_to_caller(s, b0, r->B, k, r->ids, r->scores, r->dists, r->n_found, range ? r->n_in_range : nullptr);
        b0 += r->B;
    }
    return MX_OK;
}

}  // namespace

// The reference serves one query per HTTP request on a multi-threaded runtime (handlers.rs:55-109):
// calls arrive concurrently, each with B = 1.  A GPU pass over the corpus costs the same for 1 and for
// 256 queries, so concurrent callers are COMBINED: every call queues its request; whoever finds no
// leader becomes the leader and serves batches (up to 256 queries with the same k, FIFO) until its
// own request is done, then hands over.  A lone caller runs immediately (no timer, no added
// latency); under load the batch is whatever queued up while the previous pass was on the GPU.
namespace {

bool same_filter(const Ranges *a, const Ranges *b) { return a == b || (a && b && *a == *b); }

// queues one host request and waits for its answer; the caller that finds no leader serves batches until its own request is done
int serve(mx_index *idx, SearchReq &req) {
    std::unique_lock<std::mutex> ql(idx->cmu);
    idx->pending.push_back(&req);
    idx->ccv.wait(ql, [&] { return req.done || !idx->leader; });
    if (!req.done) {
        idx->leader = true;
        while (!req.done) {
            // FIFO batch: the oldest request decides k and the filter; later requests with the same k and the same filter (or none
            // like it) join while they fit
            std::vector<SearchReq *> batch;
            int total = 0;
            const int bk = idx->pending.front()->k;
            const Ranges *bf = idx->pending.front()->filt;
            const mx_filter *br = idx->pending.front()->res;  // a resident filter: by handle
            const bool brange = idx->pending.front()->dlim != nullptr;  // range requests combine only with range requests
            for (auto it = idx->pending.begin(); it != idx->pending.end();) {
                SearchReq *r = *it;
                if (r->k == bk && same_filter(r->filt, bf) && r->res == br && (r->dlim != nullptr) == brange && total + r->B <= kMaxBatch) {
                    batch.push_back(r);
                    total += r->B;
                    it = idx->pending.erase(it);
                } else {
                    ++it;
                }
            }
            ql.unlock();
            int rc;
            try {  // the leader answers for the others: an exception must reach them as an error code, not leave them waiting
                rc = run_combined(idx, batch);
            } catch (...) {
                rc = guard_exception();
            }
            const std::string err = rc == MX_OK ? std::string() : last_error_slot();
            ql.lock();
            for (SearchReq *r : batch) {
                r->rc = rc;
                r->err = err;
                r->done = true;
            }
            idx->ccv.notify_all();
        }
        idx->leader = false;
        idx->ccv.notify_all();  // a waiter (if any) takes over
    }
    ql.unlock();
    if (req.rc != MX_OK) last_error_slot() = req.err;  // the leader's message, in the caller's thread
    return req.rc;
}

// mx_index_search and its filtered forms (filt: normalised id ranges, res: a resident filter; at most one of them)
int search_host(mx_index *idx, const float *q, int B, int k, uint64_t *ids, float *scores, float *dists, int32_t *n_found,
                const Ranges *filt, mx_filter *res = nullptr) {
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (B < 0 || k < 0) return fail(MX_EINVAL, "negative batch or k");
    if (B == 0) return MX_OK;
    if (!q || !n_found || (k > 0 && (!ids || !scores))) return fail(MX_EINVAL, "null argument");
    if (k > 4096) return fail(MX_EUNSUPPORTED, "k = %d > 4096", k);
    {   // reject non-finite queries here, per caller: inside a combined batch they would fail everyone
        const size_t total = (size_t)B * idx->dim;
        for (size_t i = 0; i < total; ++i)
            if (!std::isfinite(q[i])) return fail(MX_EINVAL, "query %zu contains a non-finite value", i / idx->dim);
    }
    if (B > kMaxBatch) {  // large requests are their own batches: split and recurse
        for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
            const int nb = std::min(kMaxBatch, B - b0);
            int rc = search_host(idx, q + (size_t)b0 * idx->dim, nb, k, ids ? ids + (size_t)b0 * k : nullptr,
                                 scores ? scores + (size_t)b0 * k : nullptr,
                                 dists ? dists + (size_t)b0 * k : nullptr, n_found + b0, filt, res);
            if (rc != MX_OK) return rc;
        }
        return MX_OK;
    }
    SearchReq req{q, B, k, ids, scores, dists, n_found, filt, res};
    return serve(idx, req);
}

}  // namespace

int mx_index_search(mx_index *idx, const float *q, int B, int k, uint64_t *ids, float *scores, float *dists,
                    int32_t *n_found) try {
    return search_host(idx, q, B, k, ids, scores, dists, n_found, nullptr);
} catch (...) {
    return guard_exception();
}

int mx_index_search_filtered(mx_index *idx, const float *q, int B, int k, const uint64_t *ranges, uint64_t n_ranges, uint64_t *ids,
                             float *scores, float *dists, int32_t *n_found) try {
    Ranges id_ranges;
    if (int rc = read_id_ranges(ranges, n_ranges, &id_ranges); rc != MX_OK) return rc;
    return search_host(idx, q, B, k, ids, scores, dists, n_found, &id_ranges);
} catch (...) {
    return guard_exception();
}

// ---- resident filters (mx_filter) ---------------------------------------------------------------------------------
namespace {

// the plain index or shard that holds shard g of a filter's rows
mx_index *filter_target(mx_index *idx, size_t g) { return idx->composite() ? idx->shards[g] : idx; }

// the index that owns the stream, the candidate lists and the per-row columns of a handle
mx_index *group_owner(mx_index *idx) { return idx->composite() ? idx->shards[0] : idx; }

// For the scope, inside a call that holds idx->mu: t (idx itself, or the shard of it named; the owner by default) locked unless it is
// idx, and its device current.
struct OwnerLock {
    mx_index *t;
    std::unique_lock<std::mutex> lk;
    DeviceGuard dg;
    OwnerLock(mx_index *idx, mx_index *target) : t(target), lk(take(idx, target)), dg(target->device) {}
    explicit OwnerLock(mx_index *idx) : OwnerLock(idx, group_owner(idx)) {}

  private:
    static std::unique_lock<std::mutex> take(const mx_index *idx, mx_index *t) {
        std::unique_lock<std::mutex> l(t->mu, std::defer_lock);
        if (t != idx) l.lock();
        return l;
    }
};

extern "C++" {  // (templates: the file's functions are declared inside extern "C")
// The frame of mx_filter_create, mx_grouping_create and mx_prior_create.  The handle takes a reference of its own (the rows stay while
// it lives, whoever closes the index), build(h) allocates under idx->mu; a failure frees what it allocated, gives the reference back
// and keeps the error text.
template <class H, class Build>
int create_handle(mx_index *idx, H **out, Build build) {
    if (!out) return fail(MX_EINVAL, "out is null");
    *out = nullptr;
    if (!idx) return fail(MX_EINVAL, "null index");
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        idx->refs += 1;
    }
    std::unique_ptr<H> h(new H());
    int rc = MX_OK;
    {
        std::lock_guard<std::mutex> lk(idx->mu);
        rc = usable(idx);
        if (rc == MX_OK && (rc = build(h.get())) != MX_OK) free_buffers(h.get());
    }
    if (rc != MX_OK) {
        const std::string keep = last_error_slot();
        mx_index_close(idx);
        last_error_slot() = keep;
        return rc;
    }
    *out = h.release();
    return MX_OK;
}

// mx_filter_destroy, mx_grouping_destroy, mx_prior_destroy (no search that names the handle is inside the library)
template <class H>
void destroy_handle(H *h, mx_index *idx) {
    try {
        std::lock_guard<std::mutex> lk(idx->mu);
        free_buffers(h);
    } catch (...) {
    }
    delete h;
    mx_index_close(idx);
}

}  // extern "C++"

// the bitmap of one shard covers the shard's capacity: new words hold no row of the set (t's device is current)
int ensure_filter_bits(mx_index *t, FilterShard &fs) {
    const size_t words = (size_t)(t->cap / kTile8Rows);
    if (fs.words >= words) return MX_OK;
    Dev<uint64_t> nb;
    MX_HIP(nb.alloc(words));
    MX_HIP(hipMemsetAsync(nb, 0, words * sizeof(uint64_t), t->stream));
    if (fs.words) MX_HIP(hipMemcpyAsync(nb, fs.bits, fs.words * sizeof(uint64_t), hipMemcpyDeviceToDevice, t->stream));
    MX_HIP(hipStreamSynchronize(t->stream));
    fs.bits = std::move(nb);
    fs.words = words;
    fs.bits_h.resize(words, 0);
    return MX_OK;
}

int ensure_filter_stage(FilterShard &fs, size_t words) {
    if (fs.stage_words >= words) return MX_OK;
    fs.stage_words = 0;
    const size_t want = std::max<size_t>(words + words / 2, 128);
    MX_HIP(fs.stage.alloc(want));  // (every edit is host-synchronised before it returns)
    fs.stage_words = want;
    return MX_OK;
}

// set_ranges on the handle's global rows (normalised, clipped to the rows); under idx->mu
int filter_edit_ranges(mx_filter *f, const Ranges &rows, bool allow) {
    mx_index *idx = f->idx;
    const size_t G = f->sh.size();
    std::vector<Ranges> loc(G);
    // every allocation first: a call that fails leaves the set as it was
    for (size_t g = 0; g < G; ++g) {
        mx_index *t = filter_target(idx, g);
        OwnerLock own(idx, t);
        if (idx->composite()) {
            for (const auto &x : shard_ranges(rows, idx->block_rows, (uint64_t)G, (uint64_t)g))
                if (x.first < std::min(x.second, t->n)) loc[g].emplace_back(x.first, std::min(x.second, t->n));
        } else {
            loc[g] = rows;
        }
        if (loc[g].size() > 0x7fffffffull) return fail(MX_EINVAL, "too many ranges");
        if (int rc = ensure_filter_bits(t, f->sh[g]); rc != MX_OK) return rc;
        if (int rc = ensure_filter_stage(f->sh[g], 2 * loc[g].size()); rc != MX_OK) return rc;
        if (!loc[g].empty() && ((loc[g].back().second + 63) >> 6) > f->sh[g].words)
            return fail(MX_EDEVICE, "filter bitmap shorter than the rows");
    }
    std::vector<uint64_t> flat;
    for (size_t g = 0; g < G; ++g) {
        if (loc[g].empty()) continue;
        mx_index *t = filter_target(idx, g);
        FilterShard &fs = f->sh[g];
        OwnerLock own(idx, t);
        flat.clear();
        for (const auto &x : loc[g]) {
            flat.push_back(x.first);
            flat.push_back(x.second);
        }
        fs.cached = false;
        MX_HIP(hipMemcpyAsync(fs.stage, flat.data(), flat.size() * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream));
        MX_HIP(launch_filter_range_edit(t->stream, fs.stage, (uint32_t)loc[g].size(), loc[g].front().first >> 6,
                                        (loc[g].back().second + 63) >> 6, allow, fs.bits));
        for (const auto &x : loc[g]) edit_mirror(fs.bits_h, x.first, x.second, allow);
        MX_HIP(hipStreamSynchronize(t->stream));
    }
    return MX_OK;
}

// set_ids; under idx->mu.  Every shard gets the caller's ids as they are: the kernel maps them to its own rows.
int filter_edit_ids(mx_filter *f, const uint64_t *ids, uint64_t n_ids, bool allow) {
    mx_index *idx = f->idx;
    const size_t G = f->sh.size();
    const uint64_t total = rows_of(idx), off = idx->idmap.id_offset, R = idx->block_rows;
    for (size_t g = 0; g < G; ++g) {
        mx_index *t = filter_target(idx, g);
        OwnerLock own(idx, t);
        if (int rc = ensure_filter_bits(t, f->sh[g]); rc != MX_OK) return rc;
        if (int rc = ensure_filter_stage(f->sh[g], (size_t)n_ids); rc != MX_OK) return rc;
    }
    if (n_ids == 0 || total == 0) return MX_OK;
    for (size_t g = 0; g < G; ++g) {
        mx_index *t = filter_target(idx, g);
        FilterShard &fs = f->sh[g];
        OwnerLock own(idx, t);
        fs.cached = false;
        MX_HIP(hipMemcpyAsync(fs.stage, ids, (size_t)n_ids * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream));
        MX_HIP(launch_filter_id_edit(t->stream, fs.stage, n_ids, total, t->idmap, allow, fs.bits, fs.words));
        MX_HIP(hipStreamSynchronize(t->stream));
    }
    for (uint64_t i = 0; i < n_ids; ++i) {  // the mirrors, by the kernel's mapping
        if (ids[i] <= off || ids[i] - off > total) continue;
        uint64_t r = ids[i] - off - 1;
        size_t g = 0;
        if (idx->composite()) {
            const uint64_t b = r / R;
            g = (size_t)(b % G);
            r = (b / G) * R + r % R;
        }
        std::vector<uint64_t> &bits = f->sh[g].bits_h;
        if ((r >> 6) >= bits.size()) continue;
        if (allow) bits[r >> 6] |= 1ull << (r & 63);
        else bits[r >> 6] &= ~(1ull << (r & 63));
    }
    return MX_OK;
}

// the set as normalised global row ranges, from the mirrors; under idx->mu
void filter_rows(mx_filter *f, Ranges &out) {
    mx_index *idx = f->idx;
    out.clear();
    if (!idx->composite()) {
        append_runs(f->sh[0].bits_h, 0, idx->n, 0, out);
        return;
    }
    const uint64_t R = idx->block_rows, G = f->sh.size();
    for (uint64_t b = 0; b * R < idx->total; ++b) {  // global block b: local block b / G of shard b % G
        const mx_index *t = idx->shards[(size_t)(b % G)];
        const uint64_t lo = (b / G) * R;
        append_runs(f->sh[(size_t)(b % G)].bits_h, lo, std::min<uint64_t>(lo + R, t->n), b * R, out);
    }
}

}  // namespace

int mx_filter_create(mx_index *idx, mx_filter **out) try {
    return create_handle(idx, out, [idx](mx_filter *f) {
        f->idx = idx;
        f->epoch = idx->row_epoch;
        f->sh.resize(idx->composite() ? idx->shards.size() : 1);
        for (size_t g = 0; g < f->sh.size(); ++g) {
            mx_index *t = filter_target(idx, g);
            OwnerLock own(idx, t);
            f->sh[g].device = t->device;
            if (int rc = ensure_filter_bits(t, f->sh[g]); rc != MX_OK) return rc;
        }
        return (int)MX_OK;
    });
} catch (...) {
    return guard_exception();
}

void mx_filter_destroy(mx_filter *f) {
    if (f) destroy_handle(f, f->idx);
}

int mx_filter_set_ranges(mx_filter *f, const uint64_t *ranges, uint64_t n_ranges, int allow) try {
    if (!f) return fail(MX_EINVAL, "null filter");
    if (allow != 0 && allow != 1) return fail(MX_EINVAL, "allow = %d: 1 adds the ids to the set, 0 takes them away", allow);
    Ranges ids;
    if (int rc = read_id_ranges(ranges, n_ranges, &ids); rc != MX_OK) return rc;
    mx_index *idx = f->idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (int rc = check_filter(idx, f); rc != MX_OK) return rc;
    return filter_edit_ranges(f, rows_of_ids(ids, idx->idmap.id_offset, rows_of(idx)), allow == 1);
} catch (...) {
    return guard_exception();
}

int mx_filter_set_ids(mx_filter *f, const uint64_t *ids, uint64_t n_ids, int allow) try {
    if (!f) return fail(MX_EINVAL, "null filter");
    if (allow != 0 && allow != 1) return fail(MX_EINVAL, "allow = %d: 1 adds the ids to the set, 0 takes them away", allow);
    if (!ids && n_ids) return fail(MX_EINVAL, "null ids with n_ids = %llu", (unsigned long long)n_ids);
    mx_index *idx = f->idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (int rc = check_filter(idx, f); rc != MX_OK) return rc;
    return filter_edit_ids(f, ids, n_ids, allow == 1);
} catch (...) {
    return guard_exception();
}

int mx_filter_count(mx_filter *f, uint64_t *n_allowed, uint64_t *n_live) try {
    if (!f) return fail(MX_EINVAL, "null filter");
    mx_index *idx = f->idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (int rc = check_filter(idx, f); rc != MX_OK) return rc;
    uint64_t a = 0, l = 0;
    for (size_t g = 0; g < f->sh.size(); ++g) {
        refresh_filter_shard(filter_target(idx, g), f->sh[g]);
        a += f->sh[g].n_allowed;
        l += f->sh[g].n_live;
    }
    if (n_allowed) *n_allowed = a;
    if (n_live) *n_live = l;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_filter_get_ranges(mx_filter *f, uint64_t *ranges, uint64_t cap_pairs, uint64_t *n_ranges) try {
    if (!f || !n_ranges) return fail(MX_EINVAL, "null argument");
    *n_ranges = 0;
    if (!ranges && cap_pairs) return fail(MX_EINVAL, "null ranges with cap_pairs = %llu", (unsigned long long)cap_pairs);
    mx_index *idx = f->idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (int rc = check_filter(idx, f); rc != MX_OK) return rc;
    Ranges rows;
    filter_rows(f, rows);
    *n_ranges = rows.size();
    if (rows.size() > cap_pairs) return MX_OK;  // the caller asks again with room for *n_ranges pairs
    const uint64_t off = idx->idmap.id_offset;
    for (size_t i = 0; i < rows.size(); ++i) {
        ranges[2 * i] = off + rows[i].first + 1;
        ranges[2 * i + 1] = off + rows[i].second + 1;
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_search_with_filter(mx_index *idx, mx_filter *f, const float *q, int B, int k, uint64_t *ids, float *scores, float *dists,
                                int32_t *n_found) try {
    if (!f) return fail(MX_EINVAL, "null filter");
    return search_host(idx, q, B, k, ids, scores, dists, n_found, nullptr, f);
} catch (...) {
    return guard_exception();
}

int mx_index_search_with_filter_device(mx_index *idx, mx_filter *f, const float *d_q, int B, int k, uint64_t *d_ids, float *d_scores,
                                       float *d_dists, int32_t *d_nfound) try {
    if (!f) return fail(MX_EINVAL, "null filter");
    return search_device(idx, d_q, B, k, d_ids, d_scores, d_dists, d_nfound, nullptr, f);
} catch (...) {
    return guard_exception();
}

namespace {

// arguments of the range entry points, checked before the index is looked at; dlim: the thresholds as dist bounds
int read_range_args(int B, const float *min_scores, int cap, std::vector<uint32_t> *dlim) {
    if (B < 0) return fail(MX_EINVAL, "negative batch");
    if (cap < 1) return fail(MX_EINVAL, "cap = %d < 1", cap);
    if (cap > 4096) return fail(MX_EUNSUPPORTED, "cap = %d > 4096", cap);
    if (B > 0 && !min_scores) return fail(MX_EINVAL, "null min_scores");
    dlim->resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (std::isnan(min_scores[b])) return fail(MX_EINVAL, "min_scores[%d] is NaN", b);
        (*dlim)[b] = range_dist_limit(min_scores[b]);
    }
    return MX_OK;
}

}  // namespace

int mx_index_search_range(mx_index *idx, const float *q, int B, const float *min_scores, int cap, uint64_t *ids, float *scores, float *dists,
                          int32_t *n_found, uint64_t *n_in_range) try {
    std::vector<uint32_t> dlim;
    if (int rc = read_range_args(B, min_scores, cap, &dlim); rc != MX_OK) return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (B == 0) return MX_OK;
    if (!q || !ids || !scores || !n_found || !n_in_range) return fail(MX_EINVAL, "null argument");
    const size_t total = (size_t)B * idx->dim;
    for (size_t i = 0; i < total; ++i)
        if (!std::isfinite(q[i])) return fail(MX_EINVAL, "query %zu contains a non-finite value", i / idx->dim);
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {  // large requests are their own batches
        const int nb = std::min(kMaxBatch, B - b0);
        const size_t o = (size_t)b0 * cap;
        SearchReq req{q + (size_t)b0 * idx->dim, nb, cap, ids + o, scores + o, dists ? dists + o : nullptr, n_found + b0, nullptr};
        req.dlim = dlim.data() + b0;
        req.n_in_range = n_in_range + b0;
        if (int rc = serve(idx, req); rc != MX_OK) return rc;
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_search_range_device(mx_index *idx, const float *d_q, int B, const float *min_scores, int cap, uint64_t *d_ids,
                                 float *d_scores, float *d_dists, int32_t *d_nfound, uint64_t *d_n_in_range) try {
    std::vector<uint32_t> dlim;
    if (int rc = read_range_args(B, min_scores, cap, &dlim); rc != MX_OK) return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (B == 0) return MX_OK;
    if (!d_q || !d_ids || !d_scores || !d_nfound || !d_n_in_range) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    DeviceGuard g(idx->device);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, B - b0);
        const size_t o = (size_t)b0 * cap;
        int rc = any_range_batch(idx, d_q + (size_t)b0 * idx->dim, nb, cap, dlim.data() + b0, d_ids + o, d_scores + o,
                                 d_dists ? d_dists + o : nullptr, d_nfound + b0, d_n_in_range + b0);
        if (rc != MX_OK) return rc;
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

namespace {

// arguments of the diversified-search entry points, checked before the index is looked at
int read_mmr_args(int B, int k, int fetch, float lambda) {
    if (B < 0) return fail(MX_EINVAL, "negative batch");
    if (k < 1) return fail(MX_EINVAL, "k = %d < 1", k);
    if (fetch < k) return fail(MX_EINVAL, "fetch = %d < k = %d", fetch, k);
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return fail(MX_EINVAL, "lambda = %g is not in [0, 1]", (double)lambda);
    if (fetch > kMmrMaxFetch) return fail(MX_EUNSUPPORTED, "fetch = %d > %d", fetch, kMmrMaxFetch);
    return MX_OK;
}

}  // namespace

int mx_index_search_mmr(mx_index *idx, const float *q, int B, int k, int fetch, float lambda, uint64_t *ids, float *scores, float *dists,
                        int32_t *n_found) try {
    if (int rc = read_mmr_args(B, k, fetch, lambda); rc != MX_OK) return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (B == 0) return MX_OK;
    if (!q || !ids || !scores || !n_found) return fail(MX_EINVAL, "null argument");
    const size_t dim = (size_t)idx->dim;
    for (size_t i = 0; i < (size_t)B * dim; ++i)
        if (!std::isfinite(q[i])) return fail(MX_EINVAL, "query %zu contains a non-finite value", i / dim);
    // not combined with other callers: the call holds the index across the candidate stage and the selection, like a device-pointer call
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;  // owner of the staging buffers and the stream
    DeviceGuard g(t->device);
    int rc = ensure_scratch(t);
    if (rc != MX_OK) return rc;
    if ((rc = ensure_out(t, k)) != MX_OK) return rc;
    Scratch &s = t->s;
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, B - b0);
        const size_t o = (size_t)b0 * k;
        memcpy(s.h_q, q + (size_t)b0 * dim, (size_t)nb * dim * sizeof(float));
        MX_HIP(hipMemcpyAsync(s.qstage, s.h_q, (size_t)nb * dim * sizeof(float), hipMemcpyHostToDevice, t->stream));
        if ((rc = mmr_batch(idx, s.qstage, nb, k, fetch, lambda, s.out_ids, s.out_scores, s.out_dists, s.out_nfound)) != MX_OK) return rc;
        if ((rc = copy_out_to_host(t, nb, k, false)) != MX_OK) return rc;
        scatter_to_caller(s, 0, nb, k, ids + o, scores + o, dists ? dists + o : nullptr, n_found + b0, nullptr);
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_search_mmr_device(mx_index *idx, const float *d_q, int B, int k, int fetch, float lambda, uint64_t *d_ids, float *d_scores,
                               float *d_dists, int32_t *d_nfound) try {
    if (int rc = read_mmr_args(B, k, fetch, lambda); rc != MX_OK) return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (B == 0) return MX_OK;
    if (!d_q || !d_ids || !d_scores || !d_nfound) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    DeviceGuard g(t->device);
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, B - b0);
        const size_t o = (size_t)b0 * k;
        int rc = mmr_batch(idx, d_q + (size_t)b0 * idx->dim, nb, k, fetch, lambda, d_ids + o, d_scores + o, d_dists ? d_dists + o : nullptr,
                           d_nfound + b0);
        if (rc != MX_OK) return rc;
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

namespace {

// arguments of the fused-search entry points, checked before the index is looked at (weights: host memory [R, m] or null)
int read_fused_args(const void *q, int R, int m, const float *weights, int mode, int k, int fetch, float rrf_c, const void *ids,
                    const void *scores, const void *n_found) {
    if (R < 0) return fail(MX_EINVAL, "negative batch");
    if (m < 1) return fail(MX_EINVAL, "m = %d < 1", m);
    if (k < 1) return fail(MX_EINVAL, "k = %d < 1", k);
    if (fetch < k) return fail(MX_EINVAL, "fetch = %d < k = %d", fetch, k);
    if (mode != MX_FUSE_MAX && mode != MX_FUSE_RRF) return fail(MX_EINVAL, "mode = %d is neither MX_FUSE_MAX nor MX_FUSE_RRF", mode);
    if (weights)
        for (size_t i = 0; i < (size_t)R * (size_t)m; ++i)
            if (!(weights[i] >= 0.0f) || std::isinf(weights[i]))
                return fail(MX_EINVAL, "weights[%zu] = %g is not a finite value >= 0", i, (double)weights[i]);
    if (mode == MX_FUSE_RRF && (!(rrf_c >= 0.0f) || std::isinf(rrf_c)))
        return fail(MX_EINVAL, "rrf_c = %g is not a finite value >= 0", (double)rrf_c);
    if (R > 0 && (!q || !ids || !scores || !n_found)) return fail(MX_EINVAL, "null argument");
    if (m > kFuseMaxSub) return fail(MX_EUNSUPPORTED, "m = %d > %d", m, kFuseMaxSub);
    if (fetch > kFuseMaxFetch) return fail(MX_EUNSUPPORTED, "fetch = %d > %d", fetch, kFuseMaxFetch);
    return MX_OK;
}

}  // namespace

int mx_index_search_fused(mx_index *idx, const float *q, int R, int m, const float *weights, int mode, int k, int fetch, float rrf_c,
                          uint64_t *ids, float *scores, float *dists, int32_t *best_sub, double *fused, int32_t *n_found) try {
    if (int rc = read_fused_args(q, R, m, weights, mode, k, fetch, rrf_c, ids, scores, n_found); rc != MX_OK) return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (R == 0) return MX_OK;
    const size_t dim = (size_t)idx->dim;
    for (size_t i = 0; i < (size_t)R * m * dim; ++i)
        if (!std::isfinite(q[i])) return fail(MX_EINVAL, "query %zu contains a non-finite value", i / dim);
    // not combined with other callers: the call holds the index across the candidate stage and the fusion, like a device-pointer call
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;  // owner of the staging buffers and the stream
    DeviceGuard g(t->device);
    int rc = ensure_scratch(t);
    if (rc != MX_OK) return rc;
    if ((rc = ensure_out(t, k)) != MX_OK) return rc;
    if (best_sub && !t->fuse_best)
        MX_HIP(t->fuse_best.alloc((size_t)kMaxBatch * kFuseMaxFetch));
    if (fused && !t->fuse_val) MX_HIP(t->fuse_val.alloc((size_t)kMaxBatch * kFuseMaxFetch));
    Scratch &s = t->s;
    const int per = kMaxBatch / m;  // whole requests per pass
    for (int r0 = 0; r0 < R; r0 += per) {
        const int nr = std::min(per, R - r0);
        const size_t o = (size_t)r0 * k, nq = (size_t)nr * m;
        memcpy(s.h_q, q + (size_t)r0 * m * dim, nq * dim * sizeof(float));
        MX_HIP(hipMemcpyAsync(s.qstage, s.h_q, nq * dim * sizeof(float), hipMemcpyHostToDevice, t->stream));
        if ((rc = fused_batch(idx, s.qstage, nr, m, weights ? weights + (size_t)r0 * m : nullptr, mode, k, fetch, rrf_c, s.out_ids, s.out_scores,
                              s.out_dists, best_sub ? t->fuse_best : nullptr, fused ? t->fuse_val : nullptr, s.out_nfound)) != MX_OK)
            return rc;
        if (best_sub) MX_HIP(hipMemcpyAsync(best_sub + o, t->fuse_best, (size_t)nr * k * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        if (fused) MX_HIP(hipMemcpyAsync(fused + o, t->fuse_val, (size_t)nr * k * sizeof(double), hipMemcpyDeviceToHost, t->stream));
        if ((rc = copy_out_to_host(t, nr, k, false)) != MX_OK) return rc;
        scatter_to_caller(s, 0, nr, k, ids + o, scores + o, dists ? dists + o : nullptr, n_found + r0, nullptr);
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_search_fused_device(mx_index *idx, const float *d_q, int R, int m, const float *weights, int mode, int k, int fetch,
                                 float rrf_c, uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_best_sub, double *d_fused,
                                 int32_t *d_nfound) try {
    if (int rc = read_fused_args(d_q, R, m, weights, mode, k, fetch, rrf_c, d_ids, d_scores, d_nfound); rc != MX_OK) return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (R == 0) return MX_OK;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    DeviceGuard g(t->device);
    const int per = kMaxBatch / m;
    for (int r0 = 0; r0 < R; r0 += per) {
        const int nr = std::min(per, R - r0);
        const size_t o = (size_t)r0 * k;
        int rc = fused_batch(idx, d_q + (size_t)r0 * m * idx->dim, nr, m, weights ? weights + (size_t)r0 * m : nullptr, mode, k, fetch, rrf_c,
                             d_ids + o, d_scores + o, d_dists ? d_dists + o : nullptr, d_best_sub ? d_best_sub + o : nullptr,
                             d_fused ? d_fused + o : nullptr, d_nfound + r0);
        if (rc != MX_OK) return rc;
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

// ---- per-row columns and grouped search (RowColumn, mx_grouping, mx_index_search_grouped) ---------------------------
namespace {

// a column named in a call on idx (under idx->mu): made for this handle, and not older than its rows
int check_column(const mx_index *idx, const RowColumn &c) {
    if (c.idx != idx) return fail(MX_EINVAL, "the %s was made for another index", c.noun);
    if (c.epoch != idx->row_epoch)
        return fail(MX_EINVAL, "the %s is stale: the index was cleared, loaded or compacted after it was made (destroy it and make a new one)",
                    c.noun);
    return MX_OK;
}

// the head of every mx_grouping_* and mx_prior_* call but create and destroy; the caller holds idx->mu
int column_ready(const RowColumn &c) {
    if (int rc = usable(c.idx); rc != MX_OK) return rc;
    return check_column(c.idx, c);
}

// the words cover `rows` rows: a new block, the old words copied, the rest zero (the owner's device is current)
int ensure_column_rows(RowColumn &c, mx_index *t, uint64_t rows) {
    if (rows <= c.len) return MX_OK;
    const uint64_t want = (rows + 1023) / 1024 * 1024;
    Dev<uint32_t> nb;
    MX_HIP(nb.alloc((size_t)want));
    if (c.len) MX_HIP(hipMemcpyAsync(nb, c.words, (size_t)c.len * sizeof(uint32_t), hipMemcpyDeviceToDevice, t->stream));
    MX_HIP(hipMemsetAsync(nb.get() + c.len, 0, (size_t)(want - c.len) * sizeof(uint32_t), t->stream));
    MX_HIP(hipStreamSynchronize(t->stream));
    c.words = std::move(nb);
    c.len = want;
    return MX_OK;
}

int ensure_column_stage(RowColumn &c, size_t bytes) {
    if (c.stage_bytes >= bytes) return MX_OK;
    c.stage_bytes = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 2, 4096);
    MX_HIP(c.stage.alloc_bytes(want));  // (every call is host-synchronised before it returns)
    c.stage_bytes = want;
    return MX_OK;
}

// what mx_grouping_create and mx_prior_create build (under idx->mu): a column over the rows of the moment, all zero
int make_column(RowColumn &c, mx_index *idx) {
    OwnerLock own(idx);
    c.idx = idx;
    c.epoch = idx->row_epoch;
    c.device = own.t->device;
    return ensure_column_rows(c, own.t, rows_of(idx));
}

// ---- host checks of the per-row edits (a grouping's keys, a prior's values: 32-bit words either way) -----------------------------------
struct WordSpan {
    uint64_t lo, hi;
    uint32_t word;
};

// the non-empty ranges of a set_ranges call sorted by lo, each with its word; lo > hi in a pair or an overlap: MX_EINVAL
int read_word_spans(const uint64_t *ranges, const uint32_t *words, uint64_t n_ranges, std::vector<WordSpan> *out) {
    if (n_ranges > 0x7fffffffull) return fail(MX_EINVAL, "too many ranges");
    std::vector<WordSpan> &sp = *out;
    sp.clear();
    sp.reserve((size_t)n_ranges);
    for (uint64_t i = 0; i < n_ranges; ++i) {
        if (ranges[2 * i] > ranges[2 * i + 1])
            return fail(MX_EINVAL, "range %llu is [%llu, %llu): lo > hi; nothing changed", (unsigned long long)i,
                        (unsigned long long)ranges[2 * i], (unsigned long long)ranges[2 * i + 1]);
        if (ranges[2 * i] < ranges[2 * i + 1]) sp.push_back({ranges[2 * i], ranges[2 * i + 1], words[i]});  // (an empty range covers nothing)
    }
    std::sort(sp.begin(), sp.end(), [](const WordSpan &a, const WordSpan &b) { return a.lo < b.lo; });
    for (size_t i = 1; i < sp.size(); ++i)
        if (sp[i - 1].hi > sp[i].lo)
            return fail(MX_EINVAL, "ranges [%llu, %llu) and [%llu, %llu) overlap: the ranges of one call must be disjoint; nothing changed",
                        (unsigned long long)sp[i - 1].lo, (unsigned long long)sp[i - 1].hi, (unsigned long long)sp[i].lo,
                        (unsigned long long)sp[i].hi);
    return MX_OK;
}

// the spans as pairs of rows clipped to the `total` rows of the moment, and the word of each span that is left
void spans_to_rows(const std::vector<WordSpan> &sp, uint64_t off, uint64_t total, std::vector<uint64_t> *rows, std::vector<uint32_t> *words) {
    for (const WordSpan &s : sp) {
        const uint64_t lo = s.lo > off ? s.lo - off - 1 : 0, hi = std::min(s.hi > off ? s.hi - off - 1 : 0, total);
        if (lo >= hi) continue;
        rows->push_back(lo);
        rows->push_back(hi);
        words->push_back(s.word);
    }
}

// an id with two different words in one set_ids call would make the result depend on which store lands last
int check_id_words(const uint64_t *ids, const uint32_t *words, uint64_t n_ids, const char *what) {
    std::vector<std::pair<uint64_t, uint32_t>> pr((size_t)n_ids);
    for (uint64_t i = 0; i < n_ids; ++i) pr[i] = {ids[i], words[i]};
    std::sort(pr.begin(), pr.end());
    for (size_t i = 1; i < pr.size(); ++i)
        if (pr[i - 1].first == pr[i].first && pr[i - 1].second != pr[i].second)
            return fail(MX_EINVAL, "id %llu is named with the %s 0x%08x and 0x%08x; nothing changed", (unsigned long long)pr[i].first, what,
                        pr[i - 1].second, pr[i].second);
    return MX_OK;
}

// one past the last row a set_ids call names; 0: it names none
uint64_t top_row_named(const uint64_t *ids, uint64_t n_ids, uint64_t off, uint64_t total) {
    uint64_t top = 0;
    for (uint64_t i = 0; i < n_ids; ++i)
        if (ids[i] > off && ids[i] - off <= total) top = std::max(top, ids[i] - off);
    return top;
}

// a sharded handle's removal mask by global row, rows [0, n), from the shards' host copies (under idx->mu); empty: a plain index, or
// nothing removed
void composite_dead_mask(mx_index *idx, uint64_t n, std::vector<uint64_t> *out) {
    std::vector<uint64_t> &mask = *out;
    mask.clear();
    if (!idx->composite() || !idx->n_dead) return;
    mask.assign((size_t)((n + 63) >> 6), 0);
    const uint64_t R = idx->block_rows, G = idx->shards.size();
    for (uint64_t s = 0; s < G; ++s) {
        mx_index *sh = idx->shards[(size_t)s];
        std::lock_guard<std::mutex> ls(sh->mu);
        if (!sh->dead) continue;
        for (size_t w = 0; w < sh->dead_h.size(); ++w) {
            for (uint64_t bits = sh->dead_h[w]; bits; bits &= bits - 1) {
                const uint64_t loc = (uint64_t)w * 64 + (uint64_t)__builtin_ctzll(bits);
                const uint64_t r = ((loc / R) * G + s) * R + loc % R;
                if (r < n) mask[(size_t)(r >> 6)] |= 1ull << (r & 63);
            }
        }
    }
}

// *d_dead = the removal mask by global row that a reduction over the rows of idx is taken against on t's device (current, t->mu
// held): `mask` copied into buf on t's stream, a plain index's own mask, or null when nothing is removed
int dead_mask_on_device(mx_index *idx, mx_index *t, const std::vector<uint64_t> &mask, Dev<uint64_t> &buf, size_t &buf_words,
                        const uint64_t **d_dead) {
    *d_dead = nullptr;
    if (!mask.empty()) {
        if (buf_words < mask.size()) {
            buf_words = 0;
            MX_HIP(buf.alloc(mask.size()));
            buf_words = mask.size();
        }
        MX_HIP(hipMemcpyAsync(buf, mask.data(), mask.size() * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream));
        *d_dead = buf;
    } else if (!idx->composite() && idx->n_dead && idx->dead) {
        *d_dead = idx->dead;  // a plain index: its own mask, one word per 64 rows of its capacity
    }
    return MX_OK;
}

extern "C++" {  // (templates: the file's functions are declared inside extern "C")
// The edits and the read of a column, after the entry point's own checks of its arguments.  Each takes the handle's mutex, and the
// owner's for the device work.  Every allocation comes first, the rows before the stage: a call that fails leaves the words as they
// were.  commit() runs once in an edit that gets as far as storing (before the store is queued), or that has no row to store to.

// set_ranges: the spans of read_word_spans
template <class Commit>
int column_set_ranges(RowColumn &c, const std::vector<WordSpan> &sp, Commit commit) {
    mx_index *idx = c.idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = column_ready(c); rc != MX_OK) return rc;
    std::vector<uint64_t> rows;
    std::vector<uint32_t> rw;
    spans_to_rows(sp, idx->idmap.id_offset, rows_of(idx), &rows, &rw);
    if (rw.empty()) {
        commit();
        return MX_OK;
    }
    OwnerLock own(idx);
    mx_index *t = own.t;
    const size_t rb = rows.size() * sizeof(uint64_t), wb = rw.size() * sizeof(uint32_t);
    if (int rc = ensure_column_rows(c, t, rows.back()); rc != MX_OK) return rc;
    if (int rc = ensure_column_stage(c, rb + wb); rc != MX_OK) return rc;
    char *st = static_cast<char *>(c.stage.get());
    MX_HIP(hipMemcpyAsync(st, rows.data(), rb, hipMemcpyHostToDevice, t->stream));
    MX_HIP(hipMemcpyAsync(st + rb, rw.data(), wb, hipMemcpyHostToDevice, t->stream));
    commit();
    MX_HIP(launch_grouping_range_edit(t->stream, reinterpret_cast<const uint64_t *>(st), reinterpret_cast<const uint32_t *>(st + rb),
                                      (uint32_t)rw.size(), rows.front(), rows.back(), c.words));
    MX_HIP(hipStreamSynchronize(t->stream));
    return MX_OK;
}

// set_ids: words[i] for the row of ids[i]; an id that names no row is passed over
template <class Commit>
int column_set_ids(RowColumn &c, const uint64_t *ids, const uint32_t *words, uint64_t n_ids, Commit commit) {
    mx_index *idx = c.idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = column_ready(c); rc != MX_OK) return rc;
    const uint64_t off = idx->idmap.id_offset, total = rows_of(idx);
    const uint64_t top = top_row_named(ids, n_ids, off, total);
    if (top == 0) {
        commit();
        return MX_OK;
    }
    OwnerLock own(idx);
    mx_index *t = own.t;
    const size_t ib = (size_t)n_ids * sizeof(uint64_t), wb = (size_t)n_ids * sizeof(uint32_t);
    if (int rc = ensure_column_rows(c, t, top); rc != MX_OK) return rc;
    if (int rc = ensure_column_stage(c, ib + wb); rc != MX_OK) return rc;
    char *st = static_cast<char *>(c.stage.get());
    MX_HIP(hipMemcpyAsync(st, ids, ib, hipMemcpyHostToDevice, t->stream));
    MX_HIP(hipMemcpyAsync(st + ib, words, wb, hipMemcpyHostToDevice, t->stream));
    commit();
    MX_HIP(launch_grouping_id_edit(t->stream, reinterpret_cast<const uint64_t *>(st), reinterpret_cast<const uint32_t *>(st + ib), n_ids, off,
                                   std::min(total, c.len), c.words));
    MX_HIP(hipStreamSynchronize(t->stream));
    return MX_OK;
}

// words[i] = the word of the row of ids[i]; 0 for an id that names no row (as a prior's value: +0.0f)
int column_get(RowColumn &c, const uint64_t *ids, uint64_t n_ids, void *words) {
    mx_index *idx = c.idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = column_ready(c); rc != MX_OK) return rc;
    if (n_ids == 0) return MX_OK;
    OwnerLock own(idx);
    mx_index *t = own.t;
    const size_t ib = (size_t)n_ids * sizeof(uint64_t), wb = (size_t)n_ids * sizeof(uint32_t);
    if (int rc = ensure_column_stage(c, ib + wb); rc != MX_OK) return rc;
    char *st = static_cast<char *>(c.stage.get());
    MX_HIP(hipMemcpyAsync(st, ids, ib, hipMemcpyHostToDevice, t->stream));
    MX_HIP(launch_grouping_get(t->stream, reinterpret_cast<const uint64_t *>(st), n_ids, idx->idmap.id_offset, std::min(rows_of(idx), c.len),
                               c.words, reinterpret_cast<uint32_t *>(st + ib)));
    MX_HIP(hipMemcpyAsync(words, st + ib, wb, hipMemcpyDeviceToHost, t->stream));
    MX_HIP(hipStreamSynchronize(t->stream));
    return MX_OK;
}

// ---- the call path of the searches that re-rank the top-fetch rows by a column: grouped, group-rows, capped, boosted ------------------
constexpr int kRerankExtras = 5;

// one output of such a search beyond ids, scores, dists and n_found
struct RerankOut {
    void *dev;     // device: [kMaxBatch, per] the handle's buffer a host-pointer call stages the output in
    void *user;    // the caller's array, host or device memory as the call's other arrays; null: not wanted
    size_t elem;   // bytes per element
    size_t per;    // elements per query
};

// where one batch leaves its results, all on the owner's device; x[i]: output i, null where the caller wants none
struct RerankDst {
    uint64_t *ids;
    float *scores, *dists;
    int32_t *nfound;
    void *x[kRerankExtras];
};

// handles named in such a search (under idx->mu)
int check_rerank_handles(mx_index *idx, const RowColumn &c, mx_filter *f) {
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (int rc = check_column(idx, c); rc != MX_OK) return rc;
    return f ? check_filter(idx, f) : MX_OK;
}

// One batch (B <= kMaxBatch), queries and outputs on the device of the index that owns the stream, the caller holding idx->mu across
// both stages: a plain (or resident-filtered) search pass at k = fetch into that index's lists (the diversified search's: a sharded
// handle has them merged on devices[0] already, which is where the column is), then rank(t, b0, B, dst), which queues the feature's
// one kernel; host-synchronised.
template <class Rank>
int rerank_batch(mx_index *idx, mx_filter *f, const float *d_q, int b0, int B, int fetch, const RerankDst &dst, Rank rank) {
    mx_index *t = group_owner(idx);
    int rc = ensure_mmr_lists(t, fetch);
    if (rc != MX_OK) return rc;
    const FilterArg fa{nullptr, f, 0};
    if ((rc = any_batch(idx, d_q, B, fetch, t->mmr_ids, t->mmr_scores, t->mmr_dists, t->mmr_nf, f ? &fa : nullptr)) != MX_OK) return rc;
    if ((rc = rank(t, b0, B, dst)) != MX_OK) return rc;
    MX_HIP(hipStreamSynchronize(t->stream));
    return MX_OK;
}

// The host-pointer variants: queries staged per batch of kMaxBatch, ids, scores, dists (width per query) and n_found through the
// owner's staging block, the nx outputs of x through the handle's buffers, which size_outputs() allocates and enters into x as dev.  Not
// combined with other callers: the call holds the index across the candidate stage and the re-ranking, like a device-pointer call.
template <class Size, class Rank>
int rerank_host(mx_index *idx, const RowColumn &c, mx_filter *f, const float *q, int B, int width, int fetch, RerankOut *x, int nx,
                Size size_outputs, Rank rank, uint64_t *ids, float *scores, float *dists, int32_t *n_found) {
    if (!idx) return fail(MX_ESEARCH, "null index");
    const size_t dim = (size_t)idx->dim;
    for (size_t i = 0; i < (size_t)B * dim; ++i)
        if (!std::isfinite(q[i])) return fail(MX_EINVAL, "query %zu contains a non-finite value", i / dim);
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = check_rerank_handles(idx, c, f); rc != MX_OK) return rc;
    if (B == 0) return MX_OK;
    mx_index *t = group_owner(idx);  // owner of the staging buffers and the stream
    DeviceGuard dg(t->device);
    int rc = ensure_scratch(t);
    if (rc != MX_OK) return rc;
    if ((rc = ensure_out(t, width)) != MX_OK) return rc;
    if ((rc = size_outputs()) != MX_OK) return rc;
    Scratch &s = t->s;
    RerankDst dst{s.out_ids, s.out_scores, s.out_dists, s.out_nfound, {}};
    for (int i = 0; i < nx; ++i) dst.x[i] = x[i].dev;
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, B - b0);
        const size_t o = (size_t)b0 * width;
        memcpy(s.h_q, q + (size_t)b0 * dim, (size_t)nb * dim * sizeof(float));
        MX_HIP(hipMemcpyAsync(s.qstage, s.h_q, (size_t)nb * dim * sizeof(float), hipMemcpyHostToDevice, t->stream));
        if ((rc = rerank_batch(idx, f, s.qstage, b0, nb, fetch, dst, rank)) != MX_OK) return rc;
        for (int i = 0; i < nx; ++i)
            if (x[i].user)
                MX_HIP(hipMemcpyAsync(static_cast<char *>(x[i].user) + (size_t)b0 * x[i].per * x[i].elem, x[i].dev,
                                      (size_t)nb * x[i].per * x[i].elem, hipMemcpyDeviceToHost, t->stream));
        if ((rc = copy_out_to_host(t, nb, width, false)) != MX_OK) return rc;
        scatter_to_caller(s, 0, nb, width, ids + o, scores + o, dists ? dists + o : nullptr, n_found + b0, nullptr);
    }
    return MX_OK;
}

// the device-pointer variants: every batch writes straight into the caller's arrays; prepare() allocates what rank needs besides
template <class Prepare, class Rank>
int rerank_device(mx_index *idx, const RowColumn &c, mx_filter *f, const float *d_q, int B, int width, int fetch, const RerankOut *x, int nx,
                  Prepare prepare, Rank rank, uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_nfound) {
    if (!idx) return fail(MX_ESEARCH, "null index");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = check_rerank_handles(idx, c, f); rc != MX_OK) return rc;
    if (B == 0) return MX_OK;
    mx_index *t = group_owner(idx);
    DeviceGuard dg(t->device);
    if (int rc = prepare(); rc != MX_OK) return rc;
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, B - b0);
        const size_t o = (size_t)b0 * width;
        RerankDst dst{d_ids + o, d_scores + o, d_dists ? d_dists + o : nullptr, d_nfound + b0, {}};
        for (int i = 0; i < nx; ++i) dst.x[i] = x[i].user ? static_cast<char *>(x[i].user) + (size_t)b0 * x[i].per * x[i].elem : nullptr;
        if (int rc = rerank_batch(idx, f, d_q + (size_t)b0 * idx->dim, b0, nb, fetch, dst, rank); rc != MX_OK) return rc;
    }
    return MX_OK;
}

}  // extern "C++"

// arguments of the grouped-search entry points, checked before the index is looked at
int read_grouped_args(int B, int k, int fetch, const mx_grouping *g, const void *q, const void *ids, const void *scores, const void *n_found) {
    if (B < 0) return fail(MX_EINVAL, "negative batch");
    if (k < 1) return fail(MX_EINVAL, "k = %d < 1", k);
    if (fetch < k) return fail(MX_EINVAL, "fetch = %d < k = %d", fetch, k);
    if (!g) return fail(MX_EINVAL, "null grouping");
    if (B > 0 && (!q || !ids || !scores || !n_found)) return fail(MX_EINVAL, "null argument");
    if (fetch > kGroupMaxFetch) return fail(MX_EUNSUPPORTED, "fetch = %d > %d", fetch, kGroupMaxFetch);
    return MX_OK;
}

// the per-head staging of the host-pointer variants covers k heads per query (the owner's device is current); members: also the
// group-rows form's
int ensure_group_out(mx_grouping *g, int k, bool members) {
    const size_t kc = (size_t)std::max(k, 16);
    if (k > g->out_cap) {
        g->out_cap = 0;
        MX_HIP(g->out_keys.alloc((size_t)kMaxBatch * kc));
        MX_HIP(g->out_rows.alloc((size_t)kMaxBatch * kc));
        MX_HIP(g->out_complete.alloc(kMaxBatch));
        g->out_cap = (int)kc;
    }
    if (members && k > g->members_cap) {
        g->members_cap = 0;
        MX_HIP(g->out_members.alloc((size_t)kMaxBatch * kc));
        MX_HIP(g->out_members_complete.alloc((size_t)kMaxBatch * kc));
        g->members_cap = (int)kc;
    }
    return MX_OK;
}

// both variants of the grouped search: one group_heads_kernel launch per batch
int grouped_search(bool host, mx_index *idx, mx_grouping *g, mx_filter *f, const float *q, int B, int k, int fetch, uint64_t *ids, float *scores,
                   float *dists, uint32_t *keys, int32_t *group_rows, int32_t *n_found, uint8_t *complete) {
    RerankOut x[] = {{nullptr, keys, sizeof(uint32_t), (size_t)k}, {nullptr, group_rows, sizeof(int32_t), (size_t)k}, {nullptr, complete, 1, 1}};
    auto rank = [&](mx_index *t, int, int nb, const RerankDst &d) {
        GroupHeads p{nb, k, fetch, idx->idmap.id_offset, g->col.len, g->col.words, t->mmr_ids, t->mmr_scores, t->mmr_dists, t->mmr_nf,
                     d.ids, d.scores, d.dists, (uint32_t *)d.x[0], (int32_t *)d.x[1], d.nfound, (uint8_t *)d.x[2]};
        MX_HIP(launch_group_heads(t->stream, p));
        return (int)MX_OK;
    };
    auto size_outputs = [&] {
        if (int rc = ensure_group_out(g, k, false); rc != MX_OK) return rc;
        x[0].dev = g->out_keys, x[1].dev = g->out_rows, x[2].dev = g->out_complete;
        return (int)MX_OK;
    };
    if (host) return rerank_host(idx, g->col, f, q, B, k, fetch, x, 3, size_outputs, rank, ids, scores, dists, n_found);
    return rerank_device(idx, g->col, f, q, B, k, fetch, x, 3, [] { return (int)MX_OK; }, rank, ids, scores, dists, n_found);
}

}  // namespace

int mx_grouping_create(mx_index *idx, mx_grouping **out) try {
    return create_handle(idx, out, [idx](mx_grouping *g) { return make_column(g->col, idx); });
} catch (...) {
    return guard_exception();
}

void mx_grouping_destroy(mx_grouping *g) {
    if (g) destroy_handle(g, g->col.idx);
}

int mx_grouping_set_ranges(mx_grouping *g, const uint64_t *ranges, const uint32_t *keys, uint64_t n_ranges) try {
    if (!g) return fail(MX_EINVAL, "null grouping");
    if ((!ranges || !keys) && n_ranges) return fail(MX_EINVAL, "null ranges or keys with n_ranges = %llu", (unsigned long long)n_ranges);
    std::vector<WordSpan> sp;
    if (int rc = read_word_spans(ranges, keys, n_ranges, &sp); rc != MX_OK) return rc;
    return column_set_ranges(g->col, sp, [] {});
} catch (...) {
    return guard_exception();
}

int mx_grouping_set_ids(mx_grouping *g, const uint64_t *ids, const uint32_t *keys, uint64_t n_ids) try {
    if (!g) return fail(MX_EINVAL, "null grouping");
    if ((!ids || !keys) && n_ids) return fail(MX_EINVAL, "null ids or keys with n_ids = %llu", (unsigned long long)n_ids);
    if (int rc = check_id_words(ids, keys, n_ids, "keys"); rc != MX_OK) return rc;
    return column_set_ids(g->col, ids, keys, n_ids, [] {});
} catch (...) {
    return guard_exception();
}

int mx_grouping_get_keys(mx_grouping *g, const uint64_t *ids, uint64_t n_ids, uint32_t *keys) try {
    if (!g) return fail(MX_EINVAL, "null grouping");
    if ((!ids || !keys) && n_ids) return fail(MX_EINVAL, "null ids or keys with n_ids = %llu", (unsigned long long)n_ids);
    return column_get(g->col, ids, n_ids, keys);
} catch (...) {
    return guard_exception();
}

int mx_grouping_count(mx_grouping *g, uint64_t *n_keyed, uint64_t *n_live_keyed) try {
    if (!g) return fail(MX_EINVAL, "null grouping");
    RowColumn &c = g->col;
    mx_index *idx = c.idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = column_ready(c); rc != MX_OK) return rc;
    const uint64_t n = std::min(rows_of(idx), c.len);
    uint64_t a = 0, l = 0;
    if (n) {
        std::vector<uint64_t> mask;
        composite_dead_mask(idx, n, &mask);
        OwnerLock own(idx);
        mx_index *t = own.t;
        if (!g->part) MX_HIP(g->part.alloc(2 * kGroupCountBlocks));
        const uint64_t *d_dead = nullptr;
        if (int rc = dead_mask_on_device(idx, t, mask, c.dead, c.dead_words, &d_dead); rc != MX_OK) return rc;
        uint64_t part[2 * kGroupCountBlocks];
        MX_HIP(launch_grouping_count(t->stream, c.words, n, d_dead, g->part));
        MX_HIP(hipMemcpyAsync(part, g->part, sizeof(part), hipMemcpyDeviceToHost, t->stream));
        MX_HIP(hipStreamSynchronize(t->stream));
        for (int w = 0; w < kGroupCountBlocks; ++w) {
            a += part[2 * w];
            l += part[2 * w + 1];
        }
    }
    if (n_keyed) *n_keyed = a;
    if (n_live_keyed) *n_live_keyed = l;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_search_grouped(mx_index *idx, mx_grouping *g, mx_filter *f, const float *q, int B, int k, int fetch, uint64_t *ids,
                            float *scores, float *dists, uint32_t *keys, int32_t *group_rows, int32_t *n_found, uint8_t *complete) try {
    if (int rc = read_grouped_args(B, k, fetch, g, q, ids, scores, n_found); rc != MX_OK) return rc;
    return grouped_search(true, idx, g, f, q, B, k, fetch, ids, scores, dists, keys, group_rows, n_found, complete);
} catch (...) {
    return guard_exception();
}

int mx_index_search_grouped_device(mx_index *idx, mx_grouping *g, mx_filter *f, const float *d_q, int B, int k, int fetch, uint64_t *d_ids,
                                   float *d_scores, float *d_dists, uint32_t *d_keys, int32_t *d_group_rows, int32_t *d_nfound,
                                   uint8_t *d_complete) try {
    if (int rc = read_grouped_args(B, k, fetch, g, d_q, d_ids, d_scores, d_nfound); rc != MX_OK) return rc;
    return grouped_search(false, idx, g, f, d_q, B, k, fetch, d_ids, d_scores, d_dists, d_keys, d_group_rows, d_nfound, d_complete);
} catch (...) {
    return guard_exception();
}

// ---- grouped search with members (mx_index_search_group_rows, mx_index_search_capped, mx_grouping_key_counts) -------
namespace {

// arguments of the group-rows and capped entry points, checked before the index is looked at; per: n or per_key, `what` its name,
// per_cap: the most the kernel takes (0: no cap)
int read_group_rows_args(int B, int k, int per, const char *what, int per_cap, int fetch, const mx_grouping *g, const void *q, const void *ids,
                         const void *scores, const void *n_found) {
    if (B < 0) return fail(MX_EINVAL, "negative batch");
    if (k < 1) return fail(MX_EINVAL, "k = %d < 1", k);
    if (per < 1) return fail(MX_EINVAL, "%s = %d < 1", what, per);
    if (fetch < k) return fail(MX_EINVAL, "fetch = %d < k = %d", fetch, k);
    if (!g) return fail(MX_EINVAL, "null grouping");
    if (B > 0 && (!q || !ids || !scores || !n_found)) return fail(MX_EINVAL, "null argument");
    if (fetch > kGroupMaxFetch) return fail(MX_EUNSUPPORTED, "fetch = %d > %d", fetch, kGroupMaxFetch);
    if (per_cap && per > per_cap) return fail(MX_EUNSUPPORTED, "%s = %d > %d", what, per, per_cap);
    if (per_cap && (long long)k * per > kGroupMaxFetch) return fail(MX_EUNSUPPORTED, "k * %s = %lld > %d", what, (long long)k * per, kGroupMaxFetch);
    return MX_OK;
}

// both variants of the group-rows form at n (per_key == 0) and of the capped form (n = 1): results of width k * n, one
// group_rows_kernel launch per batch
int group_rows_search(bool host, mx_index *idx, mx_grouping *g, mx_filter *f, const float *q, int B, int k, int n, int per_key, int fetch,
                      uint64_t *ids, float *scores, float *dists, uint32_t *keys, int32_t *group_rows, int32_t *n_members,
                      uint8_t *members_complete, int32_t *n_found, uint8_t *complete) {
    const size_t kk = (size_t)k;
    RerankOut x[] = {{nullptr, keys, sizeof(uint32_t), kk}, {nullptr, group_rows, sizeof(int32_t), kk}, {nullptr, n_members, sizeof(int32_t), kk},
                     {nullptr, members_complete, 1, kk}, {nullptr, complete, 1, 1}};
    auto rank = [&](mx_index *t, int, int nb, const RerankDst &d) {
        GroupRows p{nb, k, n, per_key, fetch, idx->idmap.id_offset, g->col.len, g->col.words, t->mmr_ids, t->mmr_scores, t->mmr_dists,
                    t->mmr_nf, d.ids, d.scores, d.dists, (uint32_t *)d.x[0], (int32_t *)d.x[1], (int32_t *)d.x[2], (uint8_t *)d.x[3],
                    d.nfound, (uint8_t *)d.x[4]};
        MX_HIP(launch_group_rows(t->stream, p));
        return (int)MX_OK;
    };
    auto size_outputs = [&] {
        if (int rc = ensure_group_out(g, k, true); rc != MX_OK) return rc;
        x[0].dev = g->out_keys, x[1].dev = g->out_rows, x[2].dev = g->out_members, x[3].dev = g->out_members_complete;
        x[4].dev = g->out_complete;
        return (int)MX_OK;
    };
    if (host) return rerank_host(idx, g->col, f, q, B, k * n, fetch, x, 5, size_outputs, rank, ids, scores, dists, n_found);
    return rerank_device(idx, g->col, f, q, B, k * n, fetch, x, 5, [] { return (int)MX_OK; }, rank, ids, scores, dists, n_found);
}

}  // namespace

int mx_index_search_group_rows(mx_index *idx, mx_grouping *g, mx_filter *f, const float *q, int B, int k, int n, int fetch, uint64_t *ids,
                               float *scores, float *dists, uint32_t *keys, int32_t *group_rows, int32_t *n_members,
                               uint8_t *members_complete, int32_t *n_found, uint8_t *complete) try {
    if (int rc = read_group_rows_args(B, k, n, "n", kGroupMaxMembers, fetch, g, q, ids, scores, n_found); rc != MX_OK) return rc;
    return group_rows_search(true, idx, g, f, q, B, k, n, 0, fetch, ids, scores, dists, keys, group_rows, n_members, members_complete, n_found, complete);
} catch (...) {
    return guard_exception();
}

int mx_index_search_group_rows_device(mx_index *idx, mx_grouping *g, mx_filter *f, const float *d_q, int B, int k, int n, int fetch,
                                      uint64_t *d_ids, float *d_scores, float *d_dists, uint32_t *d_keys, int32_t *d_group_rows,
                                      int32_t *d_n_members, uint8_t *d_members_complete, int32_t *d_nfound, uint8_t *d_complete) try {
    if (int rc = read_group_rows_args(B, k, n, "n", kGroupMaxMembers, fetch, g, d_q, d_ids, d_scores, d_nfound); rc != MX_OK) return rc;
    return group_rows_search(false, idx, g, f, d_q, B, k, n, 0, fetch, d_ids, d_scores, d_dists, d_keys, d_group_rows, d_n_members,
                             d_members_complete, d_nfound, d_complete);
} catch (...) {
    return guard_exception();
}

int mx_index_search_capped(mx_index *idx, mx_grouping *g, mx_filter *f, const float *q, int B, int k, int per_key, int fetch, uint64_t *ids,
                           float *scores, float *dists, uint32_t *keys, int32_t *n_found, uint8_t *complete) try {
    if (int rc = read_group_rows_args(B, k, per_key, "per_key", 0, fetch, g, q, ids, scores, n_found); rc != MX_OK) return rc;
    return group_rows_search(true, idx, g, f, q, B, k, 1, per_key, fetch, ids, scores, dists, keys, nullptr, nullptr, nullptr, n_found, complete);
} catch (...) {
    return guard_exception();
}

int mx_index_search_capped_device(mx_index *idx, mx_grouping *g, mx_filter *f, const float *d_q, int B, int k, int per_key, int fetch,
                                  uint64_t *d_ids, float *d_scores, float *d_dists, uint32_t *d_keys, int32_t *d_nfound,
                                  uint8_t *d_complete) try {
    if (int rc = read_group_rows_args(B, k, per_key, "per_key", 0, fetch, g, d_q, d_ids, d_scores, d_nfound); rc != MX_OK) return rc;
    return group_rows_search(false, idx, g, f, d_q, B, k, 1, per_key, fetch, d_ids, d_scores, d_dists, d_keys, nullptr, nullptr, nullptr, d_nfound,
                             d_complete);
} catch (...) {
    return guard_exception();
}

int mx_grouping_key_counts(mx_grouping *g, const uint32_t *keys, uint64_t n_keys, uint64_t *n_rows, uint64_t *n_live) try {
    if (!g) return fail(MX_EINVAL, "null grouping");
    if (!keys && n_keys) return fail(MX_EINVAL, "null keys with n_keys = %llu", (unsigned long long)n_keys);
    if (n_keys > kGroupMaxCountKeys)
        return fail(MX_EUNSUPPORTED, "n_keys = %llu > %llu", (unsigned long long)n_keys, (unsigned long long)kGroupMaxCountKeys);
    std::vector<uint32_t> sorted(keys, keys + n_keys);
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    RowColumn &c = g->col;
    mx_index *idx = c.idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = column_ready(c); rc != MX_OK) return rc;
    if (n_keys == 0) return MX_OK;
    const uint64_t rows = rows_of(idx);
    std::vector<uint64_t> counts(2 * sorted.size(), 0);
    if (rows) {
        std::vector<uint64_t> mask;
        composite_dead_mask(idx, rows, &mask);
        OwnerLock own(idx);
        mx_index *t = own.t;
        const uint64_t *d_dead = nullptr;
        if (int rc = dead_mask_on_device(idx, t, mask, c.dead, c.dead_words, &d_dead); rc != MX_OK) return rc;
        const size_t cb = counts.size() * sizeof(uint64_t), kb = sorted.size() * sizeof(uint32_t);  // the counters first: 8-byte aligned
        if (int rc = ensure_column_stage(c, cb + kb); rc != MX_OK) return rc;
        char *st = static_cast<char *>(c.stage.get());
        MX_HIP(hipMemsetAsync(st, 0, cb, t->stream));
        MX_HIP(hipMemcpyAsync(st + cb, sorted.data(), kb, hipMemcpyHostToDevice, t->stream));
        MX_HIP(launch_grouping_key_counts(t->stream, c.words, c.len, rows, d_dead, reinterpret_cast<const uint32_t *>(st + cb),
                                          (uint32_t)sorted.size(), reinterpret_cast<uint64_t *>(st)));
        MX_HIP(hipMemcpyAsync(counts.data(), st, cb, hipMemcpyDeviceToHost, t->stream));
        MX_HIP(hipStreamSynchronize(t->stream));
    }
    for (uint64_t i = 0; i < n_keys; ++i) {
        const size_t at = (size_t)(std::lower_bound(sorted.begin(), sorted.end(), keys[i]) - sorted.begin());
        if (n_rows) n_rows[i] = counts[2 * at];
        if (n_live) n_live[i] = counts[2 * at + 1];
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

// ---- boosted search (mx_prior, mx_index_search_boosted) -------------------------------------------------------------
namespace {

// the values of an edit as the words the edit kernels store; *top = the largest of them.  A value that is not finite: MX_EINVAL
int read_prior_values(const float *values, uint64_t n, std::vector<uint32_t> *words, float *top) {
    words->resize((size_t)n);
    *top = -INFINITY;
    for (uint64_t i = 0; i < n; ++i) {
        if (!std::isfinite(values[i])) return fail(MX_EINVAL, "value %llu is not finite; nothing changed", (unsigned long long)i);
        *top = std::max(*top, values[i]);
    }
    if (n) memcpy(words->data(), values, (size_t)n * sizeof(uint32_t));
    return MX_OK;
}

// arguments of the boosted-search entry points, checked before the index is looked at
int read_boosted_args(int B, int k, int fetch, const mx_prior *p, const float *weights, const void *q, const void *ids, const void *scores,
                      const void *n_found) {
    if (B < 0) return fail(MX_EINVAL, "negative batch");
    if (k < 1) return fail(MX_EINVAL, "k = %d < 1", k);
    if (fetch < k) return fail(MX_EINVAL, "fetch = %d < k = %d", fetch, k);
    if (!p) return fail(MX_EINVAL, "null prior");
    if (B > 0 && (!q || !ids || !scores || !n_found)) return fail(MX_EINVAL, "null argument");
    for (int b = 0; weights && b < B; ++b)
        if (!std::isfinite(weights[b]) || weights[b] < 0.0f)
            return fail(MX_EINVAL, "weights[%d] = %g: a weight is finite and not negative", b, (double)weights[b]);
    if (fetch > kBoostMaxFetch) return fail(MX_EUNSUPPORTED, "fetch = %d > %d", fetch, kBoostMaxFetch);
    return MX_OK;
}

// both variants of the boosted search: one boost_rank_kernel launch per batch.  weights: host memory [B] or null.
int boosted_search(bool host, mx_index *idx, mx_prior *p, mx_filter *f, const float *q, const float *weights, int B, int k, int fetch,
                   uint64_t *ids, float *scores, float *dists, float *priors, double *combined, int32_t *n_found, uint8_t *complete) {
    RerankOut x[] = {{nullptr, priors, sizeof(float), (size_t)k}, {nullptr, combined, sizeof(double), (size_t)k}, {nullptr, complete, 1, 1}};
    auto rank = [&](mx_index *t, int b0, int nb, const RerankDst &d) {
        if (weights) MX_HIP(hipMemcpyAsync(p->weights, weights + b0, (size_t)nb * sizeof(float), hipMemcpyHostToDevice, t->stream));
        BoostRank a{nb, k, fetch, idx->idmap.id_offset, p->col.len, p->col.floats(), weights ? p->weights.get() : nullptr, p->hi, t->mmr_ids,
                    t->mmr_scores, t->mmr_dists, t->mmr_nf, d.ids, d.scores, d.dists, (float *)d.x[0], (double *)d.x[1], d.nfound,
                    (uint8_t *)d.x[2]};
        MX_HIP(launch_boost_rank(t->stream, a));
        return (int)MX_OK;
    };
    auto size_weights = [&] {
        if (weights && !p->weights) MX_HIP(p->weights.alloc(kMaxBatch));
        return (int)MX_OK;
    };
    auto size_outputs = [&] {
        if (int rc = size_weights(); rc != MX_OK) return rc;
        if (k > p->out_cap) {
            p->out_cap = 0;
            const size_t kc = (size_t)std::max(k, 16);
            MX_HIP(p->out_priors.alloc((size_t)kMaxBatch * kc));
            MX_HIP(p->out_combined.alloc((size_t)kMaxBatch * kc));
            MX_HIP(p->out_complete.alloc(kMaxBatch));
            p->out_cap = (int)kc;
        }
        x[0].dev = p->out_priors, x[1].dev = p->out_combined, x[2].dev = p->out_complete;
        return (int)MX_OK;
    };
    if (host) return rerank_host(idx, p->col, f, q, B, k, fetch, x, 3, size_outputs, rank, ids, scores, dists, n_found);
    return rerank_device(idx, p->col, f, q, B, k, fetch, x, 3, size_weights, rank, ids, scores, dists, n_found);
}

}  // namespace

int mx_prior_create(mx_index *idx, mx_prior **out) try {
    return create_handle(idx, out, [idx](mx_prior *p) { return make_column(p->col, idx); });
} catch (...) {
    return guard_exception();
}

void mx_prior_destroy(mx_prior *p) {
    if (p) destroy_handle(p, p->col.idx);
}

int mx_prior_set_ranges(mx_prior *p, const uint64_t *ranges, const float *values, uint64_t n_ranges) try {
    if (!p) return fail(MX_EINVAL, "null prior");
    if ((!ranges || !values) && n_ranges) return fail(MX_EINVAL, "null ranges or values with n_ranges = %llu", (unsigned long long)n_ranges);
    std::vector<uint32_t> words;
    float top = 0.0f;
    if (int rc = read_prior_values(values, n_ranges, &words, &top); rc != MX_OK) return rc;
    std::vector<WordSpan> sp;
    if (int rc = read_word_spans(ranges, words.data(), n_ranges, &sp); rc != MX_OK) return rc;
    // (hi follows what the call was handed, whether or not a row took it, and is never below a value of the column)
    return column_set_ranges(p->col, sp, [p, top] { p->hi = std::max(p->hi, top); });
} catch (...) {
    return guard_exception();
}

int mx_prior_set_ids(mx_prior *p, const uint64_t *ids, const float *values, uint64_t n_ids) try {
    if (!p) return fail(MX_EINVAL, "null prior");
    if ((!ids || !values) && n_ids) return fail(MX_EINVAL, "null ids or values with n_ids = %llu", (unsigned long long)n_ids);
    std::vector<uint32_t> words;
    float top = 0.0f;
    if (int rc = read_prior_values(values, n_ids, &words, &top); rc != MX_OK) return rc;
    if (int rc = check_id_words(ids, words.data(), n_ids, "value bits"); rc != MX_OK) return rc;
    return column_set_ids(p->col, ids, words.data(), n_ids, [p, top] { p->hi = std::max(p->hi, top); });
} catch (...) {
    return guard_exception();
}

int mx_prior_get(mx_prior *p, const uint64_t *ids, uint64_t n_ids, float *values) try {
    if (!p) return fail(MX_EINVAL, "null prior");
    if ((!ids || !values) && n_ids) return fail(MX_EINVAL, "null ids or values with n_ids = %llu", (unsigned long long)n_ids);
    return column_get(p->col, ids, n_ids, values);
} catch (...) {
    return guard_exception();
}

int mx_prior_bound(mx_prior *p, int refresh, float *hi) try {
    if (!p) return fail(MX_EINVAL, "null prior");
    if (refresh != 0 && refresh != 1) return fail(MX_EINVAL, "refresh = %d is neither 0 nor 1", refresh);
    RowColumn &c = p->col;
    mx_index *idx = c.idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = column_ready(c); rc != MX_OK) return rc;
    if (refresh) {
        const uint64_t n = std::min(rows_of(idx), c.len);
        float top = 0.0f;
        if (n) {
            std::vector<uint64_t> mask;
            composite_dead_mask(idx, n, &mask);
            OwnerLock own(idx);
            mx_index *t = own.t;
            if (!p->part) MX_HIP(p->part.alloc(kBoostMaxBlocks));
            const uint64_t *d_dead = nullptr;
            if (int rc = dead_mask_on_device(idx, t, mask, c.dead, c.dead_words, &d_dead); rc != MX_OK) return rc;
            float part[kBoostMaxBlocks];
            MX_HIP(launch_prior_max(t->stream, c.floats(), n, d_dead, p->part));
            MX_HIP(hipMemcpyAsync(part, p->part, sizeof(part), hipMemcpyDeviceToHost, t->stream));
            MX_HIP(hipStreamSynchronize(t->stream));
            for (int w = 0; w < kBoostMaxBlocks; ++w) top = std::max(top, part[w]);
        }
        p->hi = top;
    }
    if (hi) *hi = p->hi;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_search_boosted(mx_index *idx, mx_prior *p, mx_filter *f, const float *q, const float *weights, int B, int k, int fetch,
                            uint64_t *ids, float *scores, float *dists, float *priors, double *combined, int32_t *n_found,
                            uint8_t *complete) try {
    if (int rc = read_boosted_args(B, k, fetch, p, weights, q, ids, scores, n_found); rc != MX_OK) return rc;
    return boosted_search(true, idx, p, f, q, weights, B, k, fetch, ids, scores, dists, priors, combined, n_found, complete);
} catch (...) {
    return guard_exception();
}

int mx_index_search_boosted_device(mx_index *idx, mx_prior *p, mx_filter *f, const float *d_q, const float *weights, int B, int k, int fetch,
                                   uint64_t *d_ids, float *d_scores, float *d_dists, float *d_priors, double *d_combined,
                                   int32_t *d_nfound, uint8_t *d_complete) try {
    if (int rc = read_boosted_args(B, k, fetch, p, weights, d_q, d_ids, d_scores, d_nfound); rc != MX_OK) return rc;
    return boosted_search(false, idx, p, f, d_q, weights, B, k, fetch, d_ids, d_scores, d_dists, d_priors, d_combined, d_nfound, d_complete);
} catch (...) {
    return guard_exception();
}

// ---- filters from row attributes (mx_filter_set_where / set_keys / combine / invert) ---------------------------------
namespace {

constexpr uint64_t kWhereMaxKeys = 1ull << 20;

extern "C++" {  // (templates: the file's functions are declared inside extern "C")
// An edit by predicate, under idx->mu.  The predicate kernel (launch(stream, rows, d_sel, d_extra)) runs on the device of the column
// c it reads, the owner's, and leaves a selection bitmap over the handle's GLOBAL rows at the head of the column's staging buffer;
// `extra` (extra_bytes of host memory, the sorted keys) is uploaded behind it.  The selection comes to the host, where it is
// counted and folded into the mirrors, and goes into every shard's words by filter_words_kernel: a plain index reads
// it where it lies (global rows are its local rows), a shard gets its own rows of it, dealt as filter_edit_ids deals ids (global block
// b: local block b / G of shard b % G), through its stage.  Every allocation comes first: a call that fails leaves the set as it was.
template <class Launch>
int filter_edit_selected(mx_filter *f, RowColumn &c, const void *extra, size_t extra_bytes, Launch launch, bool allow, uint64_t *n_selected) {
    mx_index *idx = f->idx;
    const size_t G = f->sh.size();
    const uint64_t rows = rows_of(idx), R = idx->block_rows;
    const size_t sw = (size_t)((rows + 63) >> 6), sb = sw * sizeof(uint64_t);
    std::vector<size_t> lw(G);  // the words of shard g that hold its rows
    for (size_t g = 0; g < G; ++g) {
        mx_index *t = filter_target(idx, g);
        OwnerLock own(idx, t);
        FilterShard &fs = f->sh[g];
        if (int rc = ensure_filter_bits(t, fs); rc != MX_OK) return rc;
        lw[g] = (size_t)((t->n + 63) >> 6);
        if (lw[g] > fs.words) return fail(MX_EDEVICE, "filter bitmap shorter than the rows");
        if (idx->composite())
            if (int rc = ensure_filter_stage(fs, lw[g]); rc != MX_OK) return rc;
    }
    if (rows == 0) {
        if (n_selected) *n_selected = 0;
        return MX_OK;
    }
    std::vector<uint64_t> sel_h(sw);
    const uint64_t *d_sel = nullptr;
    {
        OwnerLock own(idx);
        mx_index *t = own.t;
        if (int rc = ensure_column_stage(c, sb + extra_bytes); rc != MX_OK) return rc;
        char *st = static_cast<char *>(c.stage.get());
        if (extra_bytes) MX_HIP(hipMemcpyAsync(st + sb, extra, extra_bytes, hipMemcpyHostToDevice, t->stream));
        MX_HIP(launch(t->stream, rows, reinterpret_cast<uint64_t *>(st), st + sb));
        MX_HIP(hipMemcpyAsync(sel_h.data(), st, sb, hipMemcpyDeviceToHost, t->stream));
        MX_HIP(hipStreamSynchronize(t->stream));
        d_sel = reinterpret_cast<const uint64_t *>(st);
    }
    uint64_t count = 0;
    for (uint64_t w : sel_h) count += (uint64_t)__builtin_popcountll(w);
    const int op = allow ? kFilterOr : kFilterAndNot;
    std::vector<uint64_t> loc;
    for (size_t g = 0; g < G && count; ++g) {
        mx_index *t = filter_target(idx, g);
        FilterShard &fs = f->sh[g];
        if (lw[g] == 0) continue;
        OwnerLock own(idx, t);
        const std::vector<uint64_t> *src = &sel_h;
        if (idx->composite()) {
            loc.assign(lw[g], 0);
            for (uint64_t b = g; b * R < rows; b += G) {
                const uint64_t n = std::min(R, rows - b * R), lo = (b / G) * R;
                if (lo + n > (uint64_t)lw[g] * 64) return fail(MX_EDEVICE, "shard %zu holds fewer rows than its blocks", g);
                copy_bits(loc, lo, sel_h, b * R, n);
            }
            MX_HIP(hipMemcpyAsync(fs.stage, loc.data(), lw[g] * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream));
            src = &loc;
        }
        fs.cached = false;
        fs.list_ok = false;
        MX_HIP(launch_filter_words(t->stream, fs.bits, fs.bits, idx->composite() ? fs.stage.get() : d_sel, lw[g], op, 0));
        for (size_t w = 0; w < lw[g]; ++w) fs.bits_h[w] = combine_word(op, fs.bits_h[w], (*src)[w]);
        MX_HIP(hipStreamSynchronize(t->stream));
    }
    if (n_selected) *n_selected = count;
    return MX_OK;
}

}  // extern "C++"

// the handles of a predicate edit or a combination (under idx->mu, idx the filter's own index)
int where_ready(mx_filter *f) {
    if (int rc = usable(f->idx); rc != MX_OK) return rc;
    return check_filter(f->idx, f);
}

}  // namespace

int mx_filter_set_where(mx_filter *f, mx_prior *p, float lo, float hi, int allow, uint64_t *n_selected) try {
    if (!f) return fail(MX_EINVAL, "null filter");
    if (!p) return fail(MX_EINVAL, "null prior");
    if (allow != 0 && allow != 1) return fail(MX_EINVAL, "allow = %d: 1 adds the selected rows to the set, 0 takes them away", allow);
    if (std::isnan(lo) || std::isnan(hi)) return fail(MX_EINVAL, "a bound is NaN; nothing changed");
    mx_index *idx = f->idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = where_ready(f); rc != MX_OK) return rc;
    RowColumn &c = p->col;
    if (int rc = check_column(idx, c); rc != MX_OK) return rc;
    return filter_edit_selected(
        f, c, nullptr, 0,
        [&](hipStream_t s, uint64_t rows, uint64_t *sel, const char *) { return launch_where_range(s, c.floats(), c.len, rows, lo, hi, sel); },
        allow == 1, n_selected);
} catch (...) {
    return guard_exception();
}

int mx_filter_set_keys(mx_filter *f, mx_grouping *g, const uint32_t *keys, uint64_t n_keys, int allow, uint64_t *n_selected) try {
    if (!f) return fail(MX_EINVAL, "null filter");
    if (!g) return fail(MX_EINVAL, "null grouping");
    if (allow != 0 && allow != 1) return fail(MX_EINVAL, "allow = %d: 1 adds the selected rows to the set, 0 takes them away", allow);
    if (!keys && n_keys) return fail(MX_EINVAL, "null keys with n_keys = %llu", (unsigned long long)n_keys);
    if (n_keys > kWhereMaxKeys)
        return fail(MX_EUNSUPPORTED, "n_keys = %llu > %llu", (unsigned long long)n_keys, (unsigned long long)kWhereMaxKeys);
    std::vector<uint32_t> sorted(keys, keys + n_keys);
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    mx_index *idx = f->idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = where_ready(f); rc != MX_OK) return rc;
    RowColumn &c = g->col;
    if (int rc = check_column(idx, c); rc != MX_OK) return rc;
    if (sorted.empty()) {
        if (n_selected) *n_selected = 0;
        return MX_OK;
    }
    return filter_edit_selected(
        f, c, sorted.data(), sorted.size() * sizeof(uint32_t),
        [&](hipStream_t s, uint64_t rows, uint64_t *sel, const char *extra) {
            return launch_where_keys(s, c.words, c.len, rows, reinterpret_cast<const uint32_t *>(extra), (uint32_t)sorted.size(), sel);
        },
        allow == 1, n_selected);
} catch (...) {
    return guard_exception();
}

int mx_filter_combine(mx_filter *dst, mx_filter *a, mx_filter *b, int op) try {
    if (!dst || !a || !b) return fail(MX_EINVAL, "null filter");
    if (op != MX_FILTER_AND && op != MX_FILTER_OR && op != MX_FILTER_ANDNOT && op != MX_FILTER_XOR)
        return fail(MX_EINVAL, "op = %d is none of MX_FILTER_AND, MX_FILTER_OR, MX_FILTER_ANDNOT, MX_FILTER_XOR", op);
    mx_index *idx = dst->idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = where_ready(dst); rc != MX_OK) return rc;
    if (int rc = check_filter(idx, a); rc != MX_OK) return rc;
    if (int rc = check_filter(idx, b); rc != MX_OK) return rc;
    const size_t G = dst->sh.size();
    for (size_t g = 0; g < G; ++g) {  // every allocation first: the three bitmaps cover the shard's capacity, missing words are zeros
        mx_index *t = filter_target(idx, g);
        OwnerLock own(idx, t);
        for (mx_filter *x : {dst, a, b})
            if (int rc = ensure_filter_bits(t, x->sh[g]); rc != MX_OK) return rc;
    }
    for (size_t g = 0; g < G; ++g) {
        mx_index *t = filter_target(idx, g);
        FilterShard &d = dst->sh[g];
        const FilterShard &x = a->sh[g], &y = b->sh[g];
        OwnerLock own(idx, t);
        const size_t words = std::min(d.words, std::min(x.words, y.words));  // (equal: the capacity's)
        d.cached = false;
        d.list_ok = false;
        MX_HIP(launch_filter_words(t->stream, d.bits, x.bits, y.bits, words, op, 0));
        for (size_t w = 0; w < words; ++w) d.bits_h[w] = combine_word(op, x.bits_h[w], y.bits_h[w]);
        MX_HIP(hipStreamSynchronize(t->stream));
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_filter_invert(mx_filter *f) try {
    if (!f) return fail(MX_EINVAL, "null filter");
    mx_index *idx = f->idx;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = where_ready(f); rc != MX_OK) return rc;
    const size_t G = f->sh.size();
    for (size_t g = 0; g < G; ++g) {
        mx_index *t = filter_target(idx, g);
        OwnerLock own(idx, t);
        if (int rc = ensure_filter_bits(t, f->sh[g]); rc != MX_OK) return rc;
    }
    for (size_t g = 0; g < G; ++g) {  // a shard's rows are [0, n) of its own: the complement within the handle's rows, shard by shard
        mx_index *t = filter_target(idx, g);
        FilterShard &fs = f->sh[g];
        OwnerLock own(idx, t);
        const size_t words = std::min(fs.words, (size_t)((t->n + 63) >> 6));
        fs.cached = false;
        fs.list_ok = false;
        MX_HIP(launch_filter_words(t->stream, fs.bits, fs.bits, nullptr, words, kFilterXor, t->n));
        for (size_t w = 0; w < words; ++w) fs.bits_h[w] ^= rows_below_word(t->n, w);
        MX_HIP(hipStreamSynchronize(t->stream));
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

namespace {

// arguments of the by-id entry points, checked before the index is looked at; k is the cap of a range call, whose thresholds become
// dist bounds in dlim
int read_by_id_args(int B, int k, int exclude_self, bool range, const float *min_scores, std::vector<uint32_t> *dlim) {
    const char *what = range ? "cap" : "k";
    if (B < 0) return fail(MX_EINVAL, "negative batch");
    if (k < 1) return fail(MX_EINVAL, "%s = %d < 1", what, k);
    if (exclude_self != 0 && exclude_self != 1) return fail(MX_EINVAL, "exclude_self = %d is neither 0 nor 1", exclude_self);
    if (range) {
        if (B > 0 && !min_scores) return fail(MX_EINVAL, "null min_scores");
        dlim->resize((size_t)B);
        for (int b = 0; b < B; ++b) {
            if (std::isnan(min_scores[b])) return fail(MX_EINVAL, "min_scores[%d] is NaN", b);
            (*dlim)[b] = range_dist_limit(min_scores[b]);
        }
    }
    if (k > 4096 - exclude_self)
        return fail(MX_EUNSUPPORTED, "%s = %d%s > 4096", what, k, exclude_self ? " + 1 (the own row)" : "");
    return MX_OK;
}

// the four by-id entry points: dlim null = top-k; on_host: outputs are host memory and pass through the staging buffers
int search_by_id(mx_index *idx, const uint64_t *qids, int B, int k, int exclude_self, const std::vector<uint32_t> *dlim, bool on_host,
                 uint64_t *ids, float *scores, float *dists, int32_t *n_found, uint64_t *n_in_range) {
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (B == 0) return MX_OK;
    if (!qids || !ids || !scores || !n_found || (dlim && !n_in_range)) return fail(MX_EINVAL, "null argument");
    // not combined with other callers: the call holds the index from the id translation to the end of the drop kernel
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;  // owner of the staging buffers and the stream
    DeviceGuard g(t->device);
    int rc;
    if (on_host) {
        if ((rc = ensure_scratch(t)) != MX_OK) return rc;
        if ((rc = ensure_out(t, k)) != MX_OK) return rc;
    }
    Scratch &s = t->s;
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, B - b0);
        const size_t o = (size_t)b0 * k;
        const uint32_t *dl = dlim ? dlim->data() + b0 : nullptr;
        if (!on_host) {
            rc = byid_batch(idx, qids + b0, nb, k, exclude_self, dl, ids + o, scores + o, dists ? dists + o : nullptr, n_found + b0,
                            dlim ? n_in_range + b0 : nullptr);
            if (rc != MX_OK) return rc;
            continue;
        }
        if ((rc = byid_batch(idx, qids + b0, nb, k, exclude_self, dl, s.out_ids, s.out_scores, s.out_dists, s.out_nfound, s.out_nrange)) != MX_OK)
            return rc;
        if ((rc = copy_out_to_host(t, nb, k, dlim != nullptr)) != MX_OK) return rc;
        scatter_to_caller(s, 0, nb, k, ids + o, scores + o, dists ? dists + o : nullptr, n_found + b0, dlim ? n_in_range + b0 : nullptr);
    }
    return MX_OK;
}

}  // namespace

int mx_index_search_by_id(mx_index *idx, const uint64_t *query_ids, int B, int k, int exclude_self, uint64_t *ids, float *scores,
                          float *dists, int32_t *n_found) try {
    if (int rc = read_by_id_args(B, k, exclude_self, false, nullptr, nullptr); rc != MX_OK) return rc;
    return search_by_id(idx, query_ids, B, k, exclude_self, nullptr, true, ids, scores, dists, n_found, nullptr);
} catch (...) {
    return guard_exception();
}

int mx_index_search_by_id_device(mx_index *idx, const uint64_t *query_ids, int B, int k, int exclude_self, uint64_t *d_ids, float *d_scores,
                                 float *d_dists, int32_t *d_nfound) try {
    if (int rc = read_by_id_args(B, k, exclude_self, false, nullptr, nullptr); rc != MX_OK) return rc;
    return search_by_id(idx, query_ids, B, k, exclude_self, nullptr, false, d_ids, d_scores, d_dists, d_nfound, nullptr);
} catch (...) {
    return guard_exception();
}

int mx_index_search_range_by_id(mx_index *idx, const uint64_t *query_ids, int B, const float *min_scores, int cap, int exclude_self,
                                uint64_t *ids, float *scores, float *dists, int32_t *n_found, uint64_t *n_in_range) try {
    std::vector<uint32_t> dlim;
    if (int rc = read_by_id_args(B, cap, exclude_self, true, min_scores, &dlim); rc != MX_OK) return rc;
    return search_by_id(idx, query_ids, B, cap, exclude_self, &dlim, true, ids, scores, dists, n_found, n_in_range);
} catch (...) {
    return guard_exception();
}

int mx_index_search_range_by_id_device(mx_index *idx, const uint64_t *query_ids, int B, const float *min_scores, int cap, int exclude_self,
                                       uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_nfound, uint64_t *d_n_in_range) try {
    std::vector<uint32_t> dlim;
    if (int rc = read_by_id_args(B, cap, exclude_self, true, min_scores, &dlim); rc != MX_OK) return rc;
    return search_by_id(idx, query_ids, B, cap, exclude_self, &dlim, false, d_ids, d_scores, d_dists, d_nfound, d_n_in_range);
} catch (...) {
    return guard_exception();
}

namespace {

// a weight of the search by examples: 0 (absent), or finite with a magnitude in [1e-6, 1e6]
static bool like_weight_ok(float w) { return w == 0.0f || (std::fabs(w) >= 1e-6f && std::fabs(w) <= 1e6f); }  // (NaN, inf: false)

// arguments of the search-by-examples entry points, checked before the index is looked at (ids and weights: host memory)
static int read_like_args(const void *q, const float *qw, const uint64_t *ex_ids, const float *ew, int R, int m, int k, int exclude,
                   const void *ids, const void *scores, const void *n_found) {
    if (R < 0) return fail(MX_EINVAL, "negative batch");
    if (m < 1) return fail(MX_EINVAL, "m = %d < 1", m);
    if (k < 1) return fail(MX_EINVAL, "k = %d < 1", k);
    if (exclude != 0 && exclude != 1) return fail(MX_EINVAL, "exclude_examples = %d is neither 0 nor 1", exclude);
    if (qw && !q) return fail(MX_EINVAL, "query_weights without queries");
    if (ew)
        for (size_t i = 0; i < (size_t)R * (size_t)m; ++i)
            if (!like_weight_ok(ew[i]))
                return fail(MX_EINVAL, "example_weights[%zu] = %g is neither 0 nor a finite value of magnitude 1e-6 .. 1e6", i, (double)ew[i]);
    if (qw)
        for (int r = 0; r < R; ++r)
            if (!like_weight_ok(qw[r]))
                return fail(MX_EINVAL, "query_weights[%d] = %g is neither 0 nor a finite value of magnitude 1e-6 .. 1e6", r, (double)qw[r]);
    if (R > 0 && (!ex_ids || !ids || !scores || !n_found)) return fail(MX_EINVAL, "null argument");
    if (m > kLikeMaxExamples) return fail(MX_EUNSUPPORTED, "m = %d > %d", m, kLikeMaxExamples);
    if ((long long)k + (exclude ? m : 0) > 4096)
        return fail(MX_EUNSUPPORTED, "k = %d%s > 4096", k, exclude ? " + m (the examples)" : "");
    return MX_OK;
}

}  // namespace

int mx_index_search_like(mx_index *idx, const float *queries, const float *query_weights, const uint64_t *example_ids,
                         const float *example_weights, int R, int m, int k, int exclude_examples, uint64_t *ids, float *scores, float *dists,
                         int32_t *n_found, int32_t *n_used, float *combined) try {
    if (int rc = read_like_args(queries, query_weights, example_ids, example_weights, R, m, k, exclude_examples, ids, scores, n_found);
        rc != MX_OK)
        return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (R == 0) return MX_OK;
    const size_t dim = (size_t)idx->dim;
    if (queries)
        for (size_t i = 0; i < (size_t)R * dim; ++i)
            if (!std::isfinite(queries[i])) return fail(MX_EINVAL, "query %zu contains a non-finite value", i / dim);
    // not combined with other callers: the call holds the index from the id translation to the end of the drop kernel
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;  // owner of the staging buffers and the stream
    DeviceGuard g(t->device);
    int rc = ensure_scratch(t);
    if (rc != MX_OK) return rc;
    if ((rc = ensure_out(t, k)) != MX_OK) return rc;
    Scratch &s = t->s;
    const int per = kMaxBatch / m;  // whole requests per pass
    for (int r0 = 0; r0 < R; r0 += per) {
        const int nr = std::min(per, R - r0);
        const size_t o = (size_t)r0 * k, e0 = (size_t)r0 * m;
        if (queries) {
            memcpy(s.h_q, queries + (size_t)r0 * dim, (size_t)nr * dim * sizeof(float));
            MX_HIP(hipMemcpyAsync(s.qstage, s.h_q, (size_t)nr * dim * sizeof(float), hipMemcpyHostToDevice, t->stream));
        }
        if ((rc = like_batch(idx, queries ? s.qstage.get() : nullptr, query_weights ? query_weights + r0 : nullptr, example_ids + e0,
                             example_weights ? example_weights + e0 : nullptr, nr, m, k, exclude_examples, s.out_ids, s.out_scores,
                             s.out_dists, s.out_nfound, nullptr, nullptr)) != MX_OK)
            return rc;
        if (n_used) MX_HIP(hipMemcpyAsync(n_used + r0, t->like_nused, (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        if (combined)
            MX_HIP(hipMemcpyAsync(combined + (size_t)r0 * dim, t->like_q, (size_t)nr * dim * sizeof(float), hipMemcpyDeviceToHost, t->stream));
        if ((rc = copy_out_to_host(t, nr, k, false)) != MX_OK) return rc;
        scatter_to_caller(s, 0, nr, k, ids + o, scores + o, dists ? dists + o : nullptr, n_found + r0, nullptr);
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_search_like_device(mx_index *idx, const float *d_queries, const float *query_weights, const uint64_t *example_ids,
                                const float *example_weights, int R, int m, int k, int exclude_examples, uint64_t *d_ids, float *d_scores,
                                float *d_dists, int32_t *d_n_found, int32_t *d_n_used, float *d_combined) try {
    if (int rc = read_like_args(d_queries, query_weights, example_ids, example_weights, R, m, k, exclude_examples, d_ids, d_scores, d_n_found);
        rc != MX_OK)
        return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (R == 0) return MX_OK;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    DeviceGuard g(t->device);
    const size_t dim = (size_t)idx->dim;
    const int per = kMaxBatch / m;
    for (int r0 = 0; r0 < R; r0 += per) {
        const int nr = std::min(per, R - r0);
        const size_t o = (size_t)r0 * k, e0 = (size_t)r0 * m;
        int rc = like_batch(idx, d_queries ? d_queries + (size_t)r0 * dim : nullptr, query_weights ? query_weights + r0 : nullptr,
                            example_ids + e0, example_weights ? example_weights + e0 : nullptr, nr, m, k, exclude_examples, d_ids + o,
                            d_scores + o, d_dists ? d_dists + o : nullptr, d_n_found + r0, d_n_used ? d_n_used + r0 : nullptr,
                            d_combined ? d_combined + (size_t)r0 * dim : nullptr);
        if (rc != MX_OK) return rc;
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

namespace {

// arguments of the scoring entry points, checked before the index is looked at
static int read_score_args(const void *q, int B, const uint64_t *cand_ids, int m, const void *scores) {
    if (B < 0) return fail(MX_EINVAL, "negative batch");
    if (m < 1) return fail(MX_EINVAL, "m = %d < 1", m);
    if (B > 0 && (!q || !cand_ids || !scores)) return fail(MX_EINVAL, "null argument");
    if (m > kScoreMaxIds) return fail(MX_EUNSUPPORTED, "m = %d > %d", m, kScoreMaxIds);
    return MX_OK;
}

}  // namespace

int mx_index_score_ids(mx_index *idx, const float *queries, int B, const uint64_t *cand_ids, int m, float *scores, float *dists,
                       int32_t *order, int32_t *n_found) try {
    if (int rc = read_score_args(queries, B, cand_ids, m, scores); rc != MX_OK) return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (B == 0) return MX_OK;
    const size_t dim = (size_t)idx->dim;
    for (size_t i = 0; i < (size_t)B * dim; ++i)
        if (!std::isfinite(queries[i])) return fail(MX_EINVAL, "query %zu contains a non-finite value", i / dim);
    // not combined with other callers: the call holds the index from the first upload to the end of its last kernel
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;  // owner of the staging buffers and the stream
    if (t->ds > kMmrMaxDs) return fail(MX_EUNSUPPORTED, "scoring of named rows supports dim <= %d", kMmrMaxDs);
    DeviceGuard g(t->device);
    int rc = ensure_scratch(t);
    if (rc != MX_OK) return rc;
    if ((rc = ensure_score_bufs(t, m, true, false, 0)) != MX_OK) return rc;
    Scratch &s = t->s;
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, B - b0);
        const size_t o = (size_t)b0 * m, cells = (size_t)nb * m;
        memcpy(s.h_q, queries + (size_t)b0 * dim, (size_t)nb * dim * sizeof(float));
        MX_HIP(hipMemcpyAsync(s.qstage, s.h_q, (size_t)nb * dim * sizeof(float), hipMemcpyHostToDevice, t->stream));
        if ((rc = score_batch(idx, s.qstage, nb, cand_ids + o, m, t->score_scores, dists ? t->score_dists.get() : nullptr,
                              order ? t->score_order.get() : nullptr, n_found ? t->score_nf.get() : nullptr)) != MX_OK)
            return rc;
        MX_HIP(hipMemcpyAsync(scores + o, t->score_scores, cells * sizeof(float), hipMemcpyDeviceToHost, t->stream));
        if (dists) MX_HIP(hipMemcpyAsync(dists + o, t->score_dists, cells * sizeof(float), hipMemcpyDeviceToHost, t->stream));
        if (order) MX_HIP(hipMemcpyAsync(order + o, t->score_order, cells * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        if (n_found) MX_HIP(hipMemcpyAsync(n_found + b0, t->score_nf, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        MX_HIP(hipStreamSynchronize(t->stream));
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_score_ids_device(mx_index *idx, const float *d_queries, int B, const uint64_t *cand_ids, int m, float *d_scores,
                              float *d_dists, int32_t *d_order, int32_t *d_n_found) try {
    if (int rc = read_score_args(d_queries, B, cand_ids, m, d_scores); rc != MX_OK) return rc;
    if (!idx) return fail(MX_ESEARCH, "null index");
    if (B == 0) return MX_OK;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    mx_index *t = idx->composite() ? idx->shards[0] : idx;
    if (t->ds > kMmrMaxDs) return fail(MX_EUNSUPPORTED, "scoring of named rows supports dim <= %d", kMmrMaxDs);
    DeviceGuard g(t->device);
    const size_t dim = (size_t)idx->dim;
    for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, B - b0);
        const size_t o = (size_t)b0 * m;
        int rc = score_batch(idx, d_queries + (size_t)b0 * dim, nb, cand_ids + o, m, d_scores + o, d_dists ? d_dists + o : nullptr,
                             d_order ? d_order + o : nullptr, d_n_found ? d_n_found + b0 : nullptr);
        if (rc != MX_OK) return rc;
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_set_filter_copy(mx_index *idx, int on) try {
    if (!idx) return fail(MX_EINVAL, "null index");
    if (on < 0 || on > 3) return fail(MX_EINVAL, "filter copy: 0 = none, 1 = kind chosen by the library, 2 = int8, 3 = bf16 (got %d)", on);
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (idx->composite()) {
        for (mx_index *sh : idx->shards) {
            int rc = mx_index_set_filter_copy(sh, on);
            if (rc != MX_OK) return rc;
        }
        return MX_OK;
    }
    DeviceGuard g(idx->device);
    if (idx->compressed) return on ? MX_OK : fail(MX_EINVAL, "a compressed corpus has no f32 rows to fall back to");
    const bool i8 = on == 2 || (on == 1 && idx->ds <= kAutoI8MaxDim);
    auto drop = [&]() -> int {
        if (idx->xh) {
            MX_HIP(hipStreamSynchronize(idx->stream));
            idx->xh.reset();
            idx->tsc.reset();
            idx->amean.reset();
            idx->centred = false;
        }
        return MX_OK;
    };
    idx->want_filter = on != 0;
    if (!on) return drop();
    if (idx->xh && idx->filter_i8 != i8) {  // the other kind is resident: replace it
        int rc = drop();
        if (rc != MX_OK) return rc;
    }
    idx->filter_i8 = i8;
    idx->filter_auto = on == 1;
    idx->i8_batches = idx->i8_retry_batches = 0;
    idx->demoted_at_rows = 0;
    for (double &w : idx->wait_ema_us) w = 0.0;
    if (idx->xh || idx->cap == 0 || idx->kc > kMaxKC16) return MX_OK;  // present, or built with the first rows
    return build_filter_copy(idx, i8);
} catch (...) {
    return guard_exception();
}

int mx_index_set_corpus_mode(mx_index *idx, int mode) try {
    if (!idx) return fail(MX_EINVAL, "null index");
    if (mode != MX_CORPUS_F32 && mode != MX_CORPUS_BF16) return fail(MX_EINVAL, "unknown corpus mode %d", mode);
    std::lock_guard<std::mutex> lk(idx->mu);
    if (rows_of(idx) != 0) return fail(MX_EINVAL, "the corpus mode can only be chosen while the index is empty");
    if (idx->composite()) {
        for (mx_index *sh : idx->shards) {
            int rc = mx_index_set_corpus_mode(sh, mode);
            if (rc != MX_OK) return rc;
        }
        return MX_OK;
    }
    if (mode == MX_CORPUS_BF16 && idx->kc > kMaxKC16)
        return fail(MX_EUNSUPPORTED, "a compressed corpus supports dim <= %d", kMaxKC16 * kChunkFloats);
    DeviceGuard g(idx->device);
    MX_HIP(hipStreamSynchronize(idx->stream));
    idx->x.reset(); idx->scale.reset(); idx->xh.reset(); idx->tsc.reset(); idx->amean.reset();
    idx->centred = false;
    idx->cap = 0;
    idx->compressed = mode == MX_CORPUS_BF16;
    idx->want_filter = true;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_get_rows(mx_index *idx, uint64_t first_row, uint64_t n, float *out) try {
    if (!idx || (!out && n)) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (first_row + n > rows_of(idx)) return fail(MX_EINVAL, "rows [%llu, %llu) outside the index", (unsigned long long)first_row,
                                                 (unsigned long long)(first_row + n));
    if (n == 0) return MX_OK;
    std::vector<float> tmp;
    return fetch_rows(idx, first_row, n, out, tmp);
} catch (...) {
    return guard_exception();
}

int mx_index_set_profiling(mx_index *idx, int on) try {
    if (!idx) return fail(MX_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->profiling = on != 0;
    for (mx_index *sh : idx->shards) sh->profiling = on != 0;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_get_stats(mx_index *idx, mx_index_stats *out) try {
    if (!idx || !out) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (idx->composite()) {
        mx_index_stats acc = idx->stats;  // searches / queries are counted on the composite
        for (mx_index *sh : idx->shards) {
            mx_index_stats s1;
            int rc = mx_index_get_stats(sh, &s1);
            if (rc != MX_OK) return rc;
            acc.fallback_queries += s1.fallback_queries;
            acc.retry_queries += s1.retry_queries;
            acc.scan_launches += s1.scan_launches;
            acc.scan_bytes += s1.scan_bytes;
            acc.scan_ms += s1.scan_ms;
            acc.candidates += s1.candidates;
            acc.max_abs_err = std::max(acc.max_abs_err, s1.max_abs_err);
            acc.approx_err_bound = std::max(acc.approx_err_bound, s1.approx_err_bound);
            acc.filter_copy_bytes += s1.filter_copy_bytes;
            acc.filter_kind = std::max(acc.filter_kind, s1.filter_kind);  // shards choose alike; a demoted one shows as bf16
            acc.filter_demotions += s1.filter_demotions;
            acc.filter_promotions += s1.filter_promotions;
            acc.listed_rows += s1.listed_rows;
            acc.filter_centred = std::max(acc.filter_centred, s1.filter_centred);
            // (exchange_ms is counted on the composite)
        }
        *out = acc;
        return MX_OK;
    }
    if (idx->s.max_err) {  // device-side running maximum (profiling mode); fetched on demand
        DeviceGuard g(idx->device);
        float e = 0.f;
        MX_HIP(hipMemcpy(&e, idx->s.max_err, sizeof(float), hipMemcpyDeviceToHost));
        idx->stats.max_abs_err = std::max(idx->stats.max_abs_err, (double)e);
    }
    if (idx->s.host_sum) {  // largest e1 of the last batch (all queries share Ec; Eq is the query's own)
        float e1 = 0.f;
        memcpy(&e1, idx->s.host_sum + 3, sizeof(float));
        idx->stats.approx_err_bound = e1;
    }
    idx->stats.filter_kind = !idx->xh ? 0u : (idx->filter_i8 && !idx->compressed ? 2u : 3u);
    idx->stats.filter_copy_bytes = idx->xh ? (uint64_t)idx->cap * idx->ds * (idx->filter_i8 && !idx->compressed ? 1ull : 2ull) : 0;
    idx->stats.listed_rows = idx->n_zero + idx->n_wild;
    idx->stats.filter_centred = idx->centred && idx->xh ? 1u : 0u;
    *out = idx->stats;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_reset_stats(mx_index *idx) try {
    if (!idx) return fail(MX_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->stats = mx_index_stats{};
    for (mx_index *sh : idx->shards) (void)mx_index_reset_stats(sh);
    if (idx->s.max_err) {
        DeviceGuard g(idx->device);
        (void)hipMemset(idx->s.max_err, 0, sizeof(float));
    }
    return MX_OK;
} catch (...) {
    return guard_exception();
}

// ---- persistence (replaces hnsw file_dump / load_hnsw, local.rs:115-165) ----------------------
// vectors.mxflat: magic[8] | u32 dim | u32 0 | u64 n_rows | n_rows * dim f32 (row-major, global id
// order: the file does not depend on how many devices hold the index).  The reference saves after
// EVERY insert (local.rs:67); to make that affordable a save into the directory this handle last
// saved to / loaded from APPENDS the new rows and patches the header instead of rewriting the file.
int mx_index_save(mx_index *idx, const char *dir) try {
    if (!idx || !dir) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (int rc = usable(idx); rc != MX_OK) return rc;
    if (mkdir_p(dir) != 0) return fail(MX_EIO, "cannot create directory %s", dir);
    const uint64_t n = rows_of(idx);
    const std::string path = store_file(dir);
    const uint64_t chunk = std::max<uint64_t>(1, (32ull << 20) / ((uint64_t)idx->dim * 4));
    std::vector<float> host((size_t)std::min<uint64_t>(chunk, std::max<uint64_t>(n, 1)) * idx->dim), tmpv;
    auto write_rows = [&](FILE *f, uint64_t r0) -> int {
        for (uint64_t r = r0; r < n; r += chunk) {
            const uint64_t m = std::min(chunk, n - r);
            int rc = fetch_rows(idx, r, m, host.data(), tmpv);
            if (rc != MX_OK) return rc;
            if (fwrite(host.data(), sizeof(float), (size_t)m * idx->dim, f) != (size_t)m * idx->dim)
                return fail(MX_EIO, "write to %s failed", path.c_str());
        }
        return MX_OK;
    };
    if (disk_in_sync(idx, dir) && idx->disk_rows <= n) {
        if (idx->disk_rows == n) return save_dead_file(idx, dir, true);  // no new rows; removals made since the last save, if any
        FILE *f = fopen(path.c_str(), "r+b");
        if (!f) return fail(MX_EIO, "cannot open %s for appending", path.c_str());
        int rc = fseek(f, header_bytes(idx->gen) + (long)(idx->disk_rows * (uint64_t)idx->dim * 4), SEEK_SET) == 0 ? MX_OK : fail(MX_EIO, "seek in %s failed", path.c_str());
        if (rc == MX_OK) rc = write_rows(f, idx->disk_rows);
        // the header is patched last: a crash before this point leaves the old, consistent store
        if (rc == MX_OK && (fflush(f) != 0 || fseek(f, 16, SEEK_SET) != 0 || fwrite(&n, sizeof(n), 1, f) != 1))
            rc = fail(MX_EIO, "write to %s failed", path.c_str());
        if (fclose(f) != 0 && rc == MX_OK) rc = fail(MX_EIO, "write to %s failed", path.c_str());
        if (rc == MX_OK) remember_disk(idx, dir, n);
        else idx->disk_dir.clear();
        if (rc == MX_OK) rc = save_dead_file(idx, dir, true);
        return rc;
    }
    const std::string tmp = path + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(MX_EIO, "cannot open %s for writing", tmp.c_str());
    uint32_t hdr[2] = {(uint32_t)idx->dim, is_compressed(idx) ? 1u : 0u};  // [1] = rows are the stored values of a compressed corpus
    // a compacted index writes MXFLAT02 with its generation: removal files of other generations beside it are stale
    int rc = (fwrite(idx->gen ? kMagic2 : kMagic, 1, 8, f) == 8 && fwrite(hdr, sizeof(hdr), 1, f) == 1 && fwrite(&n, sizeof(n), 1, f) == 1 &&
              (!idx->gen || fwrite(&idx->gen, sizeof(idx->gen), 1, f) == 1))
                 ? MX_OK : fail(MX_EIO, "write to %s failed", tmp.c_str());
    if (rc == MX_OK) rc = write_rows(f, 0);
    if (fclose(f) != 0 && rc == MX_OK) rc = fail(MX_EIO, "write to %s failed", tmp.c_str());
    if (rc == MX_OK && rename(tmp.c_str(), path.c_str()) != 0) rc = fail(MX_EIO, "cannot rename %s", tmp.c_str());
    if (rc != MX_OK) {
        unlink(tmp.c_str());
        return rc;
    }
    remember_disk(idx, dir, n);
    return save_dead_file(idx, dir, false);
} catch (...) {
    return guard_exception();
}

int mx_index_load(mx_index *idx, const char *dir) try {
    if (!idx || !dir) return fail(MX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    const std::string path = store_file(dir);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return fail(MX_EIO, "cannot open %s", path.c_str());
    uint32_t hdr[2];
    uint64_t n = 0, gen = 0;
    struct stat sb;
    if (!read_store_header(f, hdr, &n, &gen) || fstat(fileno(f), &sb) != 0) {
        fclose(f);
        return fail(MX_EIO, "%s: bad header", path.c_str());
    }
    const long hbytes = header_bytes(gen);
    if ((int)hdr[0] != idx->dim) {
        fclose(f);
        return fail(MX_EIO, "%s holds dim %u, index has dim %d", path.c_str(), hdr[0], idx->dim);
    }
    // validate BEFORE touching the live contents: a truncated file must not destroy them
    if (n > (UINT64_MAX - (uint64_t)hbytes) / ((uint64_t)idx->dim * 4) ||  // (a damaged row count must not wrap the product)
        (uint64_t)sb.st_size < (uint64_t)hbytes + n * (uint64_t)idx->dim * 4) {
        fclose(f);
        return fail(MX_EIO, "%s: truncated (%lld bytes for %llu rows)", path.c_str(), (long long)sb.st_size, (unsigned long long)n);
    }
    // the removals beside it (vectors.mxdead), validated before anything changes as well
    std::vector<uint64_t> file_dead;
    bool dead_present = false, dead_stale = false;
    if (int drc = read_dead_file(dir, n, gen, &file_dead, &dead_present, &dead_stale); drc != MX_OK) {
        fclose(f);
        return drc;
    }
    // get_vector_storage loads the store on every request (storage/mod.rs:115-116): when the resident
    // rows are exactly what this file holds, attaching is O(1) -- the removals are taken from the file unless they are its own
    if (disk_in_sync(idx, dir) && idx->disk_rows == n && rows_of(idx) == n && idx->gen == gen && !idx->failed) {
        fclose(f);
        idx->row_epoch += 1;  // (a load stands for new rows whether or not they had to be read: resident filters are stale either way)
        if (file_dead != idx->dead_log) {
            uint64_t m = 0;
            int rc = reset_dead(idx);
            if (rc == MX_OK) rc = mark_dead(idx, file_dead, &m);
            if (rc != MX_OK) return rc;
            idx->dead_log = file_dead;
        }
        idx->disk_dead = dead_stale ? kDeadStale : dead_present ? file_dead.size() : 0;
        return MX_OK;
    }
    clear_locked(idx);
    idx->gen = gen;
    set_raw_ingest(idx, hdr[1] == 1);  // stored values of a compressed corpus go back in unchanged
    // Cold start (a collection after a restart): the file is read in 32 MB pieces into two PINNED buffers; a piece
    // goes to the device on a copy stream while the next one is being read and the previous one is ingested
    // (validated on the device like any device-row append): the load runs at the speed of the read, not at the
    // sum of read + pageable copy + host validation + ingest (round 2).  A sharded index takes its pieces
    // through composite_add (each shard validates its part).
    const uint64_t chunk = std::max<uint64_t>(1, (32ull << 20) / ((uint64_t)idx->dim * 4));
    const size_t chunk_bytes = (size_t)chunk * idx->dim * sizeof(float);
    mx_index *t0 = idx->composite() ? idx->shards[0] : idx;
    DeviceGuard dg(t0->device);
    Pin<float> pin[2];
    Dev<float> dev[2];
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t cs = nullptr;
    int rc = MX_OK;
    auto release = [&] {
        for (int i = 0; i < 2; ++i) {
            pin[i].reset();
            dev[i].reset();
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
        if (cs) (void)hipStreamDestroy(cs);
    };
    for (int i = 0; i < 2 && rc == MX_OK; ++i) {
        if (pin[i].alloc_bytes(chunk_bytes, hipHostMallocDefault) != hipSuccess ||
            (!idx->composite() && dev[i].alloc_bytes(chunk_bytes) != hipSuccess) ||
            hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess)
            rc = fail(MX_ENOMEM, "staging buffers for %s", path.c_str());
    }
    if (rc == MX_OK && hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) rc = fail(MX_EDEVICE, "stream creation failed");
    if (rc == MX_OK && n > 0) rc = reserve_locked(idx, n);
    uint64_t pending_rows = 0;  // rows of the piece that is on its way to dev[pending_buf]
    int pending_buf = 0;
    auto ingest_pending = [&]() -> int {
        if (!pending_rows) return MX_OK;
        MX_HIP(hipStreamWaitEvent(idx->stream, ev[pending_buf], 0));
        const int r = add_device_locked(idx, dev[pending_buf], pending_rows, nullptr);
        pending_rows = 0;
        return r;
    };
    int buf = 0;
    for (uint64_t r = 0; r < n && rc == MX_OK; r += chunk, buf ^= 1) {
        const uint64_t m = std::min(chunk, n - r);
        if (fread(pin[buf], sizeof(float), (size_t)m * idx->dim, f) != (size_t)m * idx->dim) {
            rc = fail(MX_EIO, "%s: read failed", path.c_str());
            break;
        }
        if (idx->composite()) {
            rc = composite_add(idx, pin[buf], m, nullptr, false);
            continue;
        }
        // dev[buf] was last read by the ingest of the piece before the previous one: that call returned synchronised
        hipError_t e = hipMemcpyAsync(dev[buf], pin[buf], (size_t)m * idx->dim * sizeof(float), hipMemcpyHostToDevice, cs);
        if (e == hipSuccess) e = hipEventRecord(ev[buf], cs);
        if (e != hipSuccess) {
            rc = fail(MX_EDEVICE, "hipMemcpy H2D: %s", hipGetErrorString(e));
            break;
        }
        rc = ingest_pending();  // the previous piece, while this one is in flight
        pending_rows = m;
        pending_buf = buf;
    }
    if (rc == MX_OK) rc = ingest_pending();
    if (cs) (void)hipStreamSynchronize(cs);
    release();
    fclose(f);
    set_raw_ingest(idx, false);
    if (rc != MX_OK) {
        const std::string keep = last_error_slot();
        clear_locked(idx);
        last_error_slot() = keep;
        return rc;
    }
    if (!file_dead.empty()) {
        uint64_t m = 0;
        rc = mark_dead(idx, file_dead, &m);
        if (rc != MX_OK) {
            const std::string keep = last_error_slot();
            clear_locked(idx);
            last_error_slot() = keep;
            return rc;
        }
    }
    idx->dead_log = file_dead;  // the file's entries as they stand (the next save appends behind them)
    idx->disk_dead = dead_stale ? kDeadStale : file_dead.size();
    remember_disk(idx, dir, n);
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_has_store(const char *dir, int *exists) try {
    if (!dir || !exists) return fail(MX_EINVAL, "null argument");
    struct stat sb;
    *exists = stat(store_file(dir).c_str(), &sb) == 0 ? 1 : 0;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_store_info(const char *dir, int *dim, uint64_t *n_rows) try {
    if (!dir || !dim || !n_rows) return fail(MX_EINVAL, "null argument");
    FILE *f = fopen(store_file(dir).c_str(), "rb");
    if (!f) return fail(MX_EIO, "cannot open %s", store_file(dir).c_str());
    uint32_t hdr[2];
    uint64_t n = 0, gen = 0;
    const bool ok = read_store_header(f, hdr, &n, &gen);  // MXFLAT01 or MXFLAT02
    fclose(f);
    if (!ok) return fail(MX_EIO, "%s: bad header", store_file(dir).c_str());
    *dim = (int)hdr[0];
    *n_rows = n;
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_index_remove_files(const char *dir) try {
    if (!dir) return fail(MX_EINVAL, "null argument");
    const std::string p = store_file(dir);
    struct stat sb;
    if (stat(p.c_str(), &sb) == 0 && unlink(p.c_str()) != 0) return fail(MX_EIO, "cannot remove %s", p.c_str());
    const std::string d = dead_file(dir);  // the removals beside it
    if (stat(d.c_str(), &sb) == 0 && unlink(d.c_str()) != 0) return fail(MX_EIO, "cannot remove %s", d.c_str());
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_topk_merge_device(int device, const uint64_t *d_ids, const float *d_dists, int G, int B, int k,
                         uint64_t *d_out_ids, float *d_out_dists, float *d_out_scores) try {
    if (G < 1 || B < 0 || k < 0) return fail(MX_EINVAL, "bad merge shape");
    if (B == 0 || k == 0) return MX_OK;
    if (!d_ids || !d_dists || !d_out_ids || !d_out_dists) return fail(MX_EINVAL, "null argument");
    DeviceGuard g(device);
    if (!g.ok) return fail(MX_EDEVICE, "hipSetDevice(%d) failed", device);
    MX_HIP(launch_merge(hipStreamPerThread, d_ids, (size_t)B * k * sizeof(uint64_t), d_dists, (size_t)B * k * sizeof(float),
                        G, B, k, d_out_ids, d_out_dists, d_out_scores));
    MX_HIP(hipStreamSynchronize(hipStreamPerThread));
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_topk_merge_packed_device(int device, const void *d_packed, int G, int B, int k, uint64_t *d_out_ids,
                                float *d_out_dists, float *d_out_scores) try {
    if (G < 1 || B < 0 || k < 0) return fail(MX_EINVAL, "bad merge shape");
    if (B == 0 || k == 0) return MX_OK;
    if (!d_packed || !d_out_ids || !d_out_dists) return fail(MX_EINVAL, "null argument");
    DeviceGuard g(device);
    if (!g.ok) return fail(MX_EDEVICE, "hipSetDevice(%d) failed", device);
    const size_t ids_bytes = (size_t)B * k * sizeof(uint64_t), blk = ids_bytes + (size_t)B * k * sizeof(float);
    MX_HIP(launch_merge(hipStreamPerThread, d_packed, blk, static_cast<const char *>(d_packed) + ids_bytes, blk, G, B, k,
                        d_out_ids, d_out_dists, d_out_scores));
    MX_HIP(hipStreamSynchronize(hipStreamPerThread));
    return MX_OK;
} catch (...) {
    return guard_exception();
}

int mx_topk_merge_packed_async(int device, void *hip_stream, const void *d_packed, int G, int B, int k, uint64_t *d_out_ids,
                               float *d_out_dists, float *d_out_scores) try {
    if (G < 1 || B < 0 || k < 0) return fail(MX_EINVAL, "bad merge shape");
    if (B == 0 || k == 0) return MX_OK;
    if (!d_packed || !d_out_ids || !d_out_dists) return fail(MX_EINVAL, "null argument");
    DeviceGuard g(device);
    if (!g.ok) return fail(MX_EDEVICE, "hipSetDevice(%d) failed", device);
    const size_t ids_bytes = (size_t)B * k * sizeof(uint64_t), blk = ids_bytes + (size_t)B * k * sizeof(float);
    MX_HIP(launch_merge(static_cast<hipStream_t>(hip_stream), d_packed, blk, static_cast<const char *>(d_packed) + ids_bytes, blk, G,
                        B, k, d_out_ids, d_out_dists, d_out_scores));
    return MX_OK;
} catch (...) {
    return guard_exception();
}

#ifdef MEMEX_TESTING
// libmemex_hip_testing.so only (mx_owned.h): how many device and pinned buffers of this file are alive; fail the n-th next
// allocation with hipErrorOutOfMemory (0: none) -- returns how many allocations were asked for since the previous call
long mx_testing_live_buffers(void) { return g_owned_live.load(); }
long mx_testing_fail_alloc(long n) {
    g_owned_fail_at.store(n);
    return g_owned_allocs.exchange(0);
}
#endif

}  // extern "C"
