/*
 * memex_hip.h -- C ABI of libmemex_hip.so: the MI355X (gfx950) embedding + vector-search path
 * that drops in under memex's `VectorStore` trait and `SentenceEmbedder` actor.
 *
 * The reference (spyglass-search/memex, Rust) has no FFI layer; the seam is the Rust surface of
 * lib/libmemex.  Every entry point below names the reference item it replaces (paths relative to
 * the reference root).  INTEGRATION.md shows the ~100-line Rust shim (`extern "C"` block +
 * `impl VectorStore for HipFlatStore`) a maintainer would add.
 *
 * Conventions
 *   - every function returns MX_OK (0) or a negative mx_status; mx_last_error() is thread-local.
 *   - nothing aborts or throws across this boundary (contrast: the reference panics at
 *     storage/local.rs:83 and :31): every entry point is a function-try-block, a C++ exception inside
 *     the library (std::bad_alloc -> MX_ENOMEM, anything else -> MX_EDEVICE "internal error: ...")
 *     comes back as a status code; helper threads and the leader of a combined search hand their
 *     exceptions to the callers they serve the same way.
 *   - the caller owns every input buffer (copied/consumed before return) and every output buffer.
 *   - handles are safe to use from several threads; calls on one handle are serialised inside.
 *   - "_device" variants take pointers into the HBM of the handle's device (for callers that keep
 *     data resident: the encoder output feeding mx_index_add_device, benchmarks, multi-GPU merge).
 *
 * Environment (everything the library reads; there is no fault-injection switch -- the two hooks the
 * tests need exist only in libmemex_hip_testing.so, built with -DMEMEX_TESTING):
 *   MEMEX_HIP_SPIN=1            host waits poll the completion word from the start (a benchmark owns its
 *                               core); default: sleep for most of the expected batch time, then poll
 *   MEMEX_HIP_EXCHANGE=rccl|p2p sharded index: insist on the RCCL all-gather / force peer copies
 *                               (default: RCCL when every shard has its own device)
 *   MEMEX_HIP_RCCL_TIMEOUT=s    deadline of ncclCommInitAll and of the communicator self-test (30)
 *   MEMEX_HIP_SHARD_THREADS=0|1 per-shard helper threads never / also for logical shards on one device
 *   MEMEX_HIP_FILTER=i8|bf16    pins the filter copy of every index opened afterwards (mx_index_set_filter_copy)
 *   MEMEX_HIP_EXACT_THETA=0     indexes opened afterwards keep the int8 scan's collect threshold from the sample's lane maxima
 *                               alone, without rescoring the sample's best rows, and the larger sample that goes with it (A/B
 *                               runs; results do not depend on it)
 *   MEMEX_HIP_DEBUG=key=v,...   which of two equivalent kernel forms runs (parity tests; keys in
 *                               memex_amd/csrc/mx_debug.h).  Results do not depend on it beyond the bounds
 *                               stated there (bit-identical forms, or different f32 summation orders).
 */
#ifndef MEMEX_HIP_H
#define MEMEX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: map 1:1 onto VectorStoreError (lib/libmemex/src/storage/mod.rs:31-48) and
 *      EmbeddingError (lib/libmemex/src/llm/embedding.rs:11-16) in the Rust shim ------------- */
typedef enum mx_status {
    MX_OK = 0,
    MX_EINVAL = -1,       /* bad argument                    -> InsertionError / SearchError      */
    MX_EDEVICE = -2,      /* HIP runtime / no device         -> ConnectionError / SetupError      */
    MX_EINSERT = -3,      /* insert failed                   -> InsertionError                    */
    MX_ESEARCH = -4,      /* search failed                   -> SearchError / EncodingFailure     */
    MX_EIO = -5,          /* save / load / delete files      -> FileIOError / SaveError           */
    MX_EUNSUPPORTED = -6, /* unsupported config              -> Unsupported / SetupError          */
    MX_ENOMEM = -7        /* host or device allocation       -> InsertionError / SetupError       */
} mx_status;

const char *mx_last_error(void); /* thread-local message of the last failing call on this thread */
const char *mx_version(void);
int mx_device_count(int *n_devices);

/* =====================================================================================
 * Flat cosine index  (replaces HnswStore, lib/libmemex/src/storage/local.rs:21-166)
 * ===================================================================================== */
typedef struct mx_index mx_index;

/*
 * Open (or attach to) the GPU-resident index registered under `key`.
 * Replaces HnswStore::new / the per-request construction in get_vector_storage
 * (storage/mod.rs:95-121, storage/local.rs:95-108): callers there build a store per request, so
 * a second open of the same key returns the SAME resident index (ref-counted, O(1)).
 * key == NULL or "" creates a private, unregistered index.  device = HIP device ordinal.
 * 1 <= dim <= 65536, else MX_EINVAL (also mx_index_open_sharded).  Every accepted dim can be added to, searched by every form below but
 * the two named here, removed from, compacted, saved and loaded, and answers bit-exactly.  Rows are padded internally to a multiple
 * of 128 dims up to 768 and of 256 above; the padded width decides what runs:
 *   padded dim <= 768    every filter copy (int8, bf16) and the f32 scan
 *   padded dim <= 1536   the int8 and bf16 filter copies (chosen automatically: int8 up to 1024, bf16 above); no f32 scan: without
 *                        a copy every search is answered on the EXACT path
 *   padded dim >  1536   no filter copy (mx_index_set_filter_copy returns MX_OK and keeps none): every form is answered on the
 *                        EXACT path; mx_index_set_corpus_mode(MX_CORPUS_BF16) is MX_EUNSUPPORTED
 *   padded dim >  8192   mx_index_search_mmr and mx_index_score_ids (and their _device forms) are MX_EUNSUPPORTED; nothing is
 *                        written to their outputs
 */
int mx_index_open(const char *key, int dim, int device, mx_index **out);
void mx_index_close(mx_index *idx); /* drops one reference; frees HBM when the last one goes */

/*
 * Multi-GPU index inside ONE process (SURVEY.md section 8b `n_dev`, 8e): the Rust host is a single
 * process (bin/memex/src/main.rs spawns api + worker as tasks), so the 8-way shard of BASELINE
 * configs[3] has to live behind this handle.  Rows are dealt to the n_dev shards in blocks of
 * block_rows consecutive rows (0 = 65536; rounded up to 32): global row r lives on shard
 * (r / block_rows) % n_dev, so an append-only collection stays balanced without knowing its final
 * size.  devices[g] = HIP ordinal of shard g (NULL = 0 .. n_dev-1); ordinals may repeat (logical
 * shards on one GPU: how the sharded path is tested on a 1-GPU box).
 * A search runs the local scan of every shard concurrently (one host thread + one stream per
 * device), exchanges the per-shard top-k blocks ([ids | dists], B*k*12 bytes each) with ONE RCCL
 * all-gather over xGMI (librccl is dlopen'ed on first use; peer copies into a slot per shard when the
 * shards share a device or MEMEX_HIP_EXCHANGE=p2p) and merges by (dist, id) on devices[0].
 * Results are bit-identical to the unsharded index for every n_dev.
 * Every mx_index_* function accepts the returned handle; *_device pointers refer to devices[0];
 * vectors.mxflat written by mx_index_save does not depend on n_dev.
 */
int mx_index_open_sharded(const char *key, int dim, int n_dev, const int *devices, uint64_t block_rows,
                          mx_index **out);
int mx_index_n_shards(mx_index *idx, int *n_shards); /* 1 for a plain index */
/* How the shards exchange their per-shard top-k blocks: 0 = plain index (nothing to exchange), 1 = copies into
 * a slot per shard on devices[0] (peer-to-peer between devices), 2 = one RCCL all-gather. */
int mx_index_exchange(mx_index *idx, int *kind);

/*
 * Stream contract of the *_device entry points.  The index works on its own HIP stream and every
 * call returns only after its results are complete in HBM (host-synchronous), so the caller may read
 * outputs from any stream afterwards.  INPUTS (and zero-fills of output buffers) enqueued on a
 * caller stream are NOT ordered against the index's stream by themselves: either synchronise that
 * stream first, or call mx_index_wait_stream(idx, stream) -- the next operation on the index then
 * starts after everything enqueued on `stream` (a hipStream_t; NULL = the default stream) so far.
 * "Non-finite queries rejected" means, for a *_device variant, that the pipeline notices them where it reads the queries (MX_EINVAL,
 * the outputs unspecified); a top-k form with nothing to find -- an empty index, a filter that allows no live row -- writes
 * the blank lists without looking and returns MX_OK, on plain and sharded handles alike, while the range forms look on every path.
 */
int mx_index_wait_stream(mx_index *idx, void *hip_stream);

int mx_index_dim(mx_index *idx, int *dim);
int mx_index_size(mx_index *idx, uint64_t *n_rows); /* = _id_map.len(), storage/local.rs:63 */
int mx_index_reserve(mx_index *idx, uint64_t n_rows); /* pre-size HBM (optional)             */

/*
 * Row-sharding support: ids returned by search are
 * `id_offset + local_row + 1`.  Default 0 = the reference's dense 1-based ids.
 */
int mx_index_set_id_offset(mx_index *idx, uint64_t id_offset);

/*
 * Append n rows ([n, dim] row-major f32).  Replaces HnswStore::insert / bulk_insert
 * (storage/local.rs:55-69): ids are dense, 1-based, in insertion order; *first_id receives the id
 * of rows[0] (later rows follow consecutively).  Non-finite values are rejected (MX_EINVAL) and
 * nothing is inserted.  (Finite values whose f32 products overflow -- elements beyond ~1.8e19 in a row or
 * a query -- take DistCosine into inf / inf = NaN, where hnsw_rs asserts, i.e. the reference panics;
 * here such a call returns, rows at a NaN distance are left out, everything that has a defined distance
 * is ranked by it: tests/test_centred_gpu.py.)  Unlike the reference there is no save-per-insert (local.rs:67); call
 * mx_index_save.
 */
int mx_index_add(mx_index *idx, const float *rows, uint64_t n, uint64_t *first_id);
int mx_index_add_device(mx_index *idx, const float *d_rows, uint64_t n, uint64_t *first_id);

/* Replaces HnswStore::delete_all (storage/local.rs:34-53): drops every row, ids restart at 1.
 * (Removing the persisted files is mx_index_remove_files; the shim calls both.) */
int mx_index_clear(mx_index *idx);

/*
 * Remove single rows (HnswStore::delete, storage/local.rs:29-32, which the reference leaves unimplemented).
 * Tombstones: a removed row keeps its storage and its id and never appears in a search result again; ids
 * are never reused or renumbered until mx_index_compact, so mx_index_size still counts every row ever added and
 * mx_index_get_rows still returns a removed row's stored values.  `ids` are the ids search returns
 * (id_offset applied).  Every id is checked first: one outside [id_offset + 1, id_offset + size] gives
 * MX_EINVAL and nothing is removed.  An id already removed, or named twice, is not an error;
 * *n_removed (may be NULL) counts the rows newly removed.  A search that starts after this call returns
 * never returns them.  mx_index_clear forgets every removal; mx_index_load replaces them with the ones
 * saved beside the store (vectors.mxdead); mx_index_save appends the ones made since the last save.
 */
int mx_index_remove(mx_index *idx, const uint64_t *ids, uint64_t n, uint64_t *n_removed);
int mx_index_removed(mx_index *idx, uint64_t *n_removed); /* rows removed so far */

/* Drop removed rows for good.  Live rows keep their order and get dense ids again:
 * the i-th live row (0-based) gets id id_offset + i + 1.  kept_ids (may be NULL) receives, for
 * each new id in order, the id the row had before (it must hold size - removed entries, checked
 * with kept_cap BEFORE anything changes: MX_EINVAL).  Afterwards size == live rows, removed == 0.
 * Nothing removed: a no-op that returns the identity, with the index and its disk state untouched.
 * Holds the index like a search does: a search sees either the old rows and ids or the new ones.
 * Ids a caller holds from before the call no longer name the same rows.  The move is in place: a device
 * error after the first row moved marks the index failed (every later call: MX_EDEVICE) until
 * mx_index_clear or mx_index_load.  The next mx_index_save rewrites the store whole. */
int mx_index_compact(mx_index *idx, uint64_t *kept_ids, uint64_t kept_cap, uint64_t *n_live);

/*
 * Top-k cosine search.  Replaces HnswStore::search (storage/local.rs:71-91) + hnsw_rs DistCosine:
 *   dist  = max(0, 1 - sum_f64(fl32(q_i*c_i)) / sqrt(sum_f64(fl32(q_i^2)) * sum_f64(fl32(c_i^2)))) as f32
 *           (0 when either norm is 0)
 *   score = 1.0f - (1.0f / (1.0f / dist))                                  (local.rs:86)
 * Results per query are ordered by (dist ascending, id ascending) -- exact brute force, so recall
 * is 1 by construction.  Outputs are row-major [B, k]; n_found[b] = min(k, size); unused slots
 * hold id 0 / score 0 / dist +inf.  `dists` may be NULL.  B > 1 is an extension (the trait is
 * single-query); B is processed in batches of up to 512.  Thread-safe, and concurrent calls are COMBINED:
 * requests that arrive while a pass is on the GPU are served together (up to 512 queries with the
 * same k per pass, FIFO), which is what turns the reference's one-query-per-HTTP-request pattern
 * (api/handlers.rs:55-109) into full batches without touching the trait.  k <= 4096 (MX_EUNSUPPORTED above; the
 * reference's callers pass limit = 10, api/handlers.rs search default).
 */
int mx_index_search(mx_index *idx, const float *queries, int B, int k, uint64_t *ids, float *scores,
                    float *dists, int32_t *n_found);
int mx_index_search_device(mx_index *idx, const float *d_queries, int B, int k, uint64_t *d_ids,
                           float *d_scores, float *d_dists, int32_t *d_n_found);

/*
 * Filtered search: the exact top-k among the rows whose ids lie in caller-given ranges (searching within one document, one
 * tenant, one ingest window: process_embeddings inserts a document's segments in one call, so each document is one run of ids).
 * `ranges` holds n_ranges pairs [lo, hi) of ids as search returns them (id_offset applied), in any order, overlapping or
 * repeated; on the _device variant it is HOST memory, like every other argument but the queries and the outputs.  Ids outside
 * [id_offset + 1, id_offset + size] select nothing (a filter is a predicate, not an id list to check).  n_ranges = 0 is the empty
 * set: n_found = 0 for every query ("no filter" is mx_index_search).  lo > hi in any pair, or ranges == NULL with n_ranges > 0:
 * MX_EINVAL and nothing is searched (checked before the other arguments; then the codes of mx_index_search).
 * The answer is bit-identical to mx_index_search on an index holding only the allowed rows that have not been removed, reported
 * under their own ids: ordered by (dist, id), n_found[b] = min(k, allowed live rows), unused slots id 0 / score 0 / dist +inf,
 * k <= 4096, non-finite queries rejected, B split as there.  A filter covering every id gives what mx_index_search gives.
 * Concurrent host-pointer calls are combined like mx_index_search's, but a pass takes requests only when k and the normalised
 * (sorted, merged) ranges are equal, and never mixes filtered with unfiltered requests.  Filtered passes do not count towards the
 * filter copy's demotion / promotion.  Few allowed rows (at most 16384) are scored directly by a subset kernel, more by the
 * masked scan over the span of tiles the ranges touch.
 */
int mx_index_search_filtered(mx_index *idx, const float *queries, int B, int k, const uint64_t *ranges, uint64_t n_ranges,
                             uint64_t *ids, float *scores, float *dists, int32_t *n_found);
int mx_index_search_filtered_device(mx_index *idx, const float *d_queries, int B, int k, const uint64_t *ranges, uint64_t n_ranges,
                                    uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_n_found);

/*
 * Resident filters: an allow-set that is an object (one tenant's, one ACL group's, one tag's documents).  It is built once from id
 * ranges or a plain id list, kept as one bit per row next to the rows on every shard, edited when the tenant gains or loses a
 * document, and named by handle in a search; a search with it uploads nothing and does no host work that grows with the ranges or
 * ids it was built from.
 *   mx_filter_create       the empty set of rows of `idx`.  The filter holds a reference on the index: mx_index_close by the owner
 *                          does not pull the rows from under it; mx_filter_destroy drops the reference.
 *   mx_filter_set_ranges   allow = 1 adds the ids of the ranges to the set, allow = 0 takes them away (any other value: MX_EINVAL).
 *                          Ranges as in mx_index_search_filtered: pairs [lo, hi), any order, overlapping, repeated; lo > hi in any
 *                          pair, or ranges == NULL with n_ranges > 0: MX_EINVAL.
 *   mx_filter_set_ids      the same for a plain list of ids; they may repeat and come in any order.
 * Ids are the ids search returns, id_offset applied at the time of the call; an id outside [id_offset + 1, id_offset + size] at
 * that time is ignored (a filter is a predicate, not an id list to check), so rows appended later are not in the set until a later
 * call names them.  The stored bits are per row: a later mx_index_set_id_offset moves the ids the filter stands for with the rows.
 * A failing call changes nothing.
 *   mx_filter_count        n_allowed: rows in the set; n_live: those of them that are not removed (either may be NULL).  Removed
 *                          rows stay in the set and are never returned.
 *   mx_filter_get_ranges   the set as normalised id ranges (sorted, merged, current id_offset).  *n_ranges is always the number
 *                          of pairs needed; nothing is written when cap_pairs is smaller (MX_OK all the same: ask again).
 *   mx_index_search_with_filter[_device]
 *                          bit-identical to mx_index_search_filtered[_device] called at the same moment with what
 *                          mx_filter_get_ranges returns: ids, scores, dists, n_found, empty slots, k <= 4096, the codes, the split
 *                          of B, both search modes, every filter copy and corpus mode, the same counters.  The empty filter finds
 *                          nothing (n_found = 0, MX_OK).  Concurrent host-pointer calls that name the same filter and the same k
 *                          share passes; they never share one with plain, per-call-filtered or range requests.
 * mx_index_clear, mx_index_load and an mx_index_compact that dropped at least one row renumber or replace the rows: every filter
 * of the index is STALE afterwards, and every call with it except mx_filter_destroy returns MX_EINVAL with a message that says so.
 * A filter named together with an index it was not made for: MX_EINVAL.  A null filter, or a null pointer where a result is
 * required, is MX_EINVAL before anything else; a null index on the search calls is then MX_ESEARCH.  Filter calls are thread-safe
 * beside every other call on the index, and a search sees a filter before or after a whole set_* call, never half of one; a
 * filter must not be destroyed while a call that names it is running.
 */
typedef struct mx_filter mx_filter;
int mx_filter_create(mx_index *idx, mx_filter **out);
void mx_filter_destroy(mx_filter *f);
int mx_filter_set_ranges(mx_filter *f, const uint64_t *ranges, uint64_t n_ranges, int allow);
int mx_filter_set_ids(mx_filter *f, const uint64_t *ids, uint64_t n_ids, int allow);
int mx_filter_count(mx_filter *f, uint64_t *n_allowed, uint64_t *n_live);
int mx_filter_get_ranges(mx_filter *f, uint64_t *ranges, uint64_t cap_pairs, uint64_t *n_ranges);
int mx_index_search_with_filter(mx_index *idx, mx_filter *f, const float *queries, int B, int k, uint64_t *ids, float *scores,
                                float *dists, int32_t *n_found);
int mx_index_search_with_filter_device(mx_index *idx, mx_filter *f, const float *d_queries, int B, int k, uint64_t *d_ids,
                                       float *d_scores, float *d_dists, int32_t *d_n_found);

/*
 * Range search: every row whose score reaches a per-query threshold, exactly ("which rows are at least this similar?").
 * Row r is in range for query b iff score(q_b, r) >= min_scores[b], score being exactly the f32 value mx_index_search reports for that
 * pair (1 - 1/(1/dist), dist the f64 DistCosine rounded to f32).  min_scores holds B floats and is HOST memory on both variants.
 * Per query the in-range live rows are written best-first in (dist, id) order, at most cap of them; n_found[b] = min(cap, n_in_range[b])
 * is the number written and n_in_range[b] the EXACT number of in-range live rows, which may exceed cap.  Unused slots hold id 0,
 * score 0, dist +inf; dists may be NULL.  Removed rows are never in range; a threshold above 1 selects nothing, one <= -1 every live row;
 * a zero-norm query has score 1 against every row (the first cap live rows by id).  The first n_found[b] entries equal, bit for bit,
 * those of mx_index_search with k = cap.
 * Arguments are checked first: B < 0, cap < 1, min_scores == NULL (B > 0) or a NaN threshold: MX_EINVAL; cap > 4096: MX_EUNSUPPORTED;
 * then a null index: MX_ESEARCH.  Non-finite queries are rejected, B is split into batches of 512, id_offset applies, sharded handles
 * sum n_in_range over their shards.  Concurrent host-pointer calls are combined like mx_index_search's, a pass taking only range
 * requests with the same cap (thresholds may differ).  Range passes never change the filter copy and do not count towards its
 * demotion / promotion.  The collect scan runs with the pass threshold the caller's score implies (no sample launch); a query whose
 * candidates overflow, and everything mx_index_search answers on the EXACT path but k > 256, takes the EXACT range path.
 */
int mx_index_search_range(mx_index *idx, const float *queries, int B, const float *min_scores, int cap, uint64_t *ids, float *scores,
                          float *dists, int32_t *n_found, uint64_t *n_in_range);
int mx_index_search_range_device(mx_index *idx, const float *d_queries, int B, const float *min_scores, int cap, uint64_t *d_ids,
                                 float *d_scores, float *d_dists, int32_t *d_n_found, uint64_t *d_n_in_range);

/*
 * Diversified search: the k most relevant rows that do not repeat each other -- exact maximal-marginal-relevance (MMR) re-ranking of the
 * top-`fetch` rows.  Overlapping windows of one document are near-copies of each other; a plain top-k returns them side by side.
 * Per query:
 *   candidates  the exact top-fetch live rows in (dist, id) order: what mx_index_search gives with k = fetch, bit for bit (removed rows,
 *               id_offset, the AUTO path up to fetch = 256 and the EXACT path above, B split into batches of 512); m = min(fetch, live rows).
 *               The candidate stage IS a plain search pass: it counts as one in mx_index_stats and in the filter copy's heuristics.
 *   selection   greedy, n_found = min(k, m) picks.  The first pick is candidate 0; every later pick maximises, over the candidates not
 *               picked yet,   v_i = (double)lambda * (double)rel_i - (1.0 - (double)lambda) * (double)pen_i   (plain IEEE f64 operations,
 *               not contracted), rel_i the f32 score the search reports for candidate i, pen_i the largest sim(i, j) over the rows j
 *               picked so far (f32), sim(i, j) = score(DistCosine(row_j, row_i)) on the rows AS STORED (a bf16 corpus: its values widened,
 *               what mx_index_get_rows returns) with the arithmetic of mx_index_search: f32 products summed sequentially in f64 in element
 *               order.  A sim that is NaN (two rows whose element products overflow f32) counts as 1, a v that is NaN as -inf.  Ties in v go
 *               to the earlier candidate, i.e. the smaller (dist, id).
 *   output      ids / scores / dists [B, k] in SELECTION order, each entry with the id, score (= rel) and dist of its candidate, unchanged;
 *               unused slots id 0 / score 0 / dist +inf; dists may be NULL.
 * lambda = 1 returns the first k entries of mx_index_search; fetch = k a permutation of the plain top-k that starts with its first entry.
 * Arguments are checked first: B < 0, k < 1, fetch < k, lambda NaN or outside [0, 1]: MX_EINVAL; fetch > 1024: MX_EUNSUPPORTED (the
 * selection costs O(k * fetch * dim) per query: k - 1 rounds of one f64 chain of dim terms per remaining candidate); then a null index:
 * MX_ESEARCH.  Non-finite queries are rejected; dim <= 8192.  Thread-safe beside every other call.  Concurrent callers are NOT combined
 * into shared passes: each call holds the index across its candidate stage and its selection (both see one snapshot of the rows; no
 * append, removal or compaction slips between them) and never rides in a plain, filtered or range pass.  A sharded handle merges the
 * candidates on devices[0] as a search does; then every shard copies the stored rows of the candidates it owns, widened to f32, to
 * devices[0] (peer copies), where one kernel selects -- the answer equals the plain index's bit for bit.  Extra HBM, allocated at the
 * first call: the candidate lists and at most 64 MiB of gathered rows per device (a batch is processed in chunks of queries that fit).
 */
int mx_index_search_mmr(mx_index *idx, const float *queries, int B, int k, int fetch, float lambda, uint64_t *ids, float *scores,
                        float *dists, int32_t *n_found);
int mx_index_search_mmr_device(mx_index *idx, const float *d_queries, int B, int k, int fetch, float lambda, uint64_t *d_ids,
                               float *d_scores, float *d_dists, int32_t *d_n_found);

/*
 * Search by stored row: the queries are rows of the index, named by the ids search returns ("more like this segment", "which rows
 * repeat this one").  The rows never leave HBM: every shard gathers the rows it owns into one query block on devices[0], one plain pass
 * runs over it, and a last kernel takes the own row out of each list.  query_ids holds B ids and is HOST memory on both variants.
 * Let v_b be what mx_index_get_rows returns for the row query_ids[b] names (a bf16 corpus: its values widened) and e = exclude_self.
 *   mx_index_search_by_id        per query: the entries of mx_index_search(v_b, k + e) in their (dist, id) order, the entry whose id is
 *                                query_ids[b] dropped if it is among them, cut to k; n_found follows.  With e = 1 that is the EXACT
 *                                top-k of the live rows other than the own row -- also when k + 1 or more exact copies with smaller ids
 *                                come before it: then the own row is not among the k + 1 listed, nothing is dropped, and the first k
 *                                are the answer (stripping "the first entry" of a k + 1 search by hand is wrong exactly there).
 *   mx_index_search_range_by_id  per query: the same procedure on mx_index_search_range(v_b, min_scores[b], cap + e).  n_in_range is the
 *                                plain call's count, minus one (e = 1) if the own row is itself in range by the plain call's own
 *                                membership test -- usually dist 0, but a row whose norm leaves [1e-15, 1e15] is judged by the dist
 *                                the plain path computes for it; n_found = min(cap, n_in_range).
 * Unused slots hold id 0, score 0, dist +inf; dists may be NULL.  An id that names no row, or a removed row, finds nothing: n_found 0,
 * n_in_range 0, blank slots, and the call still returns MX_OK (a batch over "all ids" does not fail on a tombstone).  id_offset applies
 * to query ids exactly as to result ids.
 * Arguments are checked first: B < 0, k < 1 / cap < 1, exclude_self not 0 or 1, min_scores == NULL (B > 0) or a NaN threshold:
 * MX_EINVAL; k + e > 4096 / cap + e > 4096: MX_EUNSUPPORTED; then a null index: MX_ESEARCH.  Everything else is the plain pass's:
 * removed rows, the AUTO and EXACT paths, B split into batches of 512, statistics; a range pass never changes the filter copy.
 * Thread-safe beside every other call.  Concurrent callers are NOT combined into shared passes: each call holds the index from the
 * translation of its ids to the end of its last kernel, so no append, removal or compaction slips between the stages.  Extra HBM,
 * allocated at the first call: a query block of 512 rows and lists of 512 x max(k + e, 64) entries on devices[0].
 */
int mx_index_search_by_id(mx_index *idx, const uint64_t *query_ids, int B, int k, int exclude_self, uint64_t *ids, float *scores,
                          float *dists, int32_t *n_found);
int mx_index_search_by_id_device(mx_index *idx, const uint64_t *query_ids, int B, int k, int exclude_self, uint64_t *d_ids,
                                 float *d_scores, float *d_dists, int32_t *d_n_found);
int mx_index_search_range_by_id(mx_index *idx, const uint64_t *query_ids, int B, const float *min_scores, int cap, int exclude_self,
                                uint64_t *ids, float *scores, float *dists, int32_t *n_found, uint64_t *n_in_range);
int mx_index_search_range_by_id_device(mx_index *idx, const uint64_t *query_ids, int B, const float *min_scores, int cap, int exclude_self,
                                       uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_n_found, uint64_t *d_n_in_range);

/*
 * Fused search: ONE ranked list from several query vectors -- the phrasings of a question, a question and a hypothetical answer, the
 * last turns of a conversation.  queries is [R, m, dim] row-major, R requests of m sub-queries each; the outputs are [R, k].  weights
 * is [R, m] in HOST memory on both variants (NULL: all ones); a weight of exactly 0 marks the sub-query ABSENT for that request (the
 * padding of ragged requests): its vector is still checked and still rides in the pass, but its list is never consulted.
 * Per request:
 *   candidates  for every sub-query i with weight > 0, list i = what mx_index_search gives for it with k = fetch, bit for bit: (dist, id)
 *               order, removed rows, id_offset, the AUTO and EXACT modes.  The candidate stage IS a plain search pass over the R * m
 *               queries (split into passes of floor(512 / m) whole requests): it counts as one in mx_index_stats and in the filter
 *               copy's heuristics.
 *   best list   a row of the union of the consulted lists is reported ONCE, with the entry of its best sub-query: the consulted list that
 *               holds it with the smallest (dist, sub-query index).  scores / dists are that entry's, unchanged; best_sub is that index.
 *   MX_FUSE_MAX ("any of these phrasings") the rows ordered by (best dist ascending, id ascending), cut to k; weights matter only as
 *               present or absent; fused = (double)score.  This is the EXACT global top-k by min_i dist_i(row) over ALL live rows, for
 *               any fetch >= k, not only among the listed rows (DESIGN.md 3.13 has the proof: a row outside list i has fetch >= k rows
 *               ahead of it there, each with a fused key no larger than its own).  Hence n_found = min(k, live rows) whenever a
 *               weight is > 0, and fetch = k is enough.
 *   MX_FUSE_RRF reciprocal-rank fusion of the top-fetch lists:  fused(row) = sum over the consulted lists i that hold the row, in
 *               ASCENDING i, of  (double)w_i / ((double)rrf_c + (double)rank_i(row)),  rank_i the row's 1-based position in list i;
 *               plain IEEE f64 operations, not contracted, a true division (no reciprocal approximation).  The rows are ordered by
 *               (fused descending, id ascending) and cut to k.  Exact with respect to the top-fetch lists (a row outside every list
 *               has no rank), the framing of mx_index_search_mmr.  n_found = min(k, size of the union).
 * Unused slots hold id 0, score 0, dist +inf, best_sub -1, fused 0; dists, best_sub and fused may be NULL.  A request whose weights are
 * all 0 finds nothing, and the call still returns MX_OK.
 * Arguments are checked first: R < 0, m < 1, k < 1, fetch < k, a mode that is neither of the two, a weight that is NaN, infinite or
 * negative, (MX_FUSE_RRF) an rrf_c that is NaN, infinite or < 0, a NULL queries / ids / scores / n_found with R > 0: MX_EINVAL;
 * m > 16 or fetch > 256: MX_EUNSUPPORTED (one workgroup fuses one request from LDS, at most 16 x 256 = 4096 entries; fetch <= 256 keeps
 * the candidate stage on the AUTO path); then a null index: MX_ESEARCH.  Non-finite queries are rejected as by mx_index_search.
 * Thread-safe beside every other call.  Concurrent callers are NOT combined into shared passes: each call holds the index across its
 * candidate stage and its fusion (both see one snapshot of the rows) and never rides in a plain, filtered or range pass.  A sharded
 * handle merges the candidate lists on devices[0] as a search does and fuses there: no rows are gathered, and the answer equals the
 * plain index's bit for bit.  The fusion costs O(m * fetch * log^2(m * fetch)) per request, independent of dim and of the row count.
 * Extra HBM, allocated at the first call: the candidate lists (shared with mx_index_search_mmr) and 1.5 MiB of outputs on devices[0].
 */
enum { MX_FUSE_MAX = 0, MX_FUSE_RRF = 1 };
int mx_index_search_fused(mx_index *idx, const float *queries, int R, int m, const float *weights, int mode, int k, int fetch,
                          float rrf_c, uint64_t *ids, float *scores, float *dists, int32_t *best_sub, double *fused, int32_t *n_found);
int mx_index_search_fused_device(mx_index *idx, const float *d_queries, int R, int m, const float *weights, int mode, int k, int fetch,
                                 float rrf_c, uint64_t *d_ids, float *d_scores, float *d_dists, int32_t *d_best_sub, double *d_fused,
                                 int32_t *d_n_found);

/*
 * Search by examples: the exact top-k for a BLEND of stored rows -- "more like these segments, less like those" (relevance feedback,
 * pinned passages, more-like-this for a document of several segments), optionally together with a caller vector.  The example rows
 * never leave HBM: every shard gathers the rows it owns to devices[0], one kernel blends each request's terms into ONE f32 query in
 * stated arithmetic, one plain pass runs over those queries, and a last kernel takes the used examples out of each list.
 * R requests of m example slots each.  example_ids [R, m], example_weights [R, m] (NULL: all 1) and query_weights [R] (NULL: all 1)
 * are HOST memory on both variants; queries [R, dim] is optional (NULL: no caller term) and is host memory on the first variant,
 * device memory on the second.  Outputs: ids / scores / dists [R, k], n_found / n_used [R], combined [R, dim]; dists, n_used and
 * combined may be NULL.
 *   terms       Let v_i be what mx_index_get_rows returns for the row example_ids[r, i] names (a bf16 corpus: its values widened), id_offset
 *               applied as for results, and na_i = sum_j (double)fl32(v_ij * v_ij) in ascending j.  Example i is USED when its weight is not
 *               0, its id names a live (not removed) row and na_i > 0.  A weight of exactly 0 marks an absent slot (the padding of ragged
 *               requests); a removed row, an id that names no row and a zero row are skipped without error.  The caller vector q =
 *               queries[r] is a term under the same rule, with weight w_q = query_weights[r]: it is skipped when w_q is 0 or na_q is 0
 *               (a non-finite vector has a non-finite na_q and is not skipped).
 *   combined    c_j = +0.0, then c_j += (double)w_q * ((double)q_j / sqrt(na_q)) if the caller term is used, then
 *               c_j += (double)w_i * ((double)v_ij / sqrt(na_i)) for the used examples in ASCENDING i: IEEE f64 operations, round to nearest,
 *               a true square root and division, nothing contracted.  combined_j = (float)c_j, round to nearest even.  Results below f32's
 *               normal range are unspecified.  The value depends on nothing else: not on the shard count, the copy kind or the pass split.
 *   result      Let E = m when exclude_examples = 1, else 0.  The entries of mx_index_search(combined, k + E) in their (dist, id) order;
 *               with exclude_examples = 1 every entry whose id is a used example's id of that request is dropped; the list is cut to k and
 *               n_found follows.  With exclude_examples = 1 that is the EXACT top-k of the live rows other than the used examples: at most
 *               E entries leave a sorted prefix of k + E, so at least the first k of the others are in it (exact copies of an example are
 *               other rows and stay).  An id named twice contributes twice and is dropped once.  n_used counts the used examples, the
 *               caller term not included.
 *   blank       A request without a used term, or whose combined is all zeros (a row used as positive and negative with equal weight),
 *               finds nothing: n_found 0, combined zeros, and the call still returns MX_OK.
 * Unused slots hold id 0, score 0, dist +inf.
 * Arguments are checked first: R < 0, m < 1, k < 1, exclude_examples not 0 or 1, a weight that is NaN or infinite or whose magnitude is
 * non-zero and outside [1e-6, 1e6] (the message names it, e.g. example_weights[3]), a NULL example_ids / ids / scores / n_found with
 * R > 0, query_weights without queries: MX_EINVAL; m > 16 or k + E > 4096: MX_EUNSUPPORTED; then a null index: MX_ESEARCH.  A non-finite
 * caller vector is rejected as by mx_index_search (MX_EINVAL).  Everything else is the plain pass's: removed rows, the AUTO path and -- for
 * k + E > 256, like any such k -- the EXACT path, statistics.  Requests go in passes of floor(512 / m) whole requests (at most 512 gathered
 * rows).  Thread-safe beside every other call.  Concurrent callers are NOT combined into shared passes: each call holds the index from
 * the translation of its ids to the end of its last kernel, so no append, removal or compaction slips between the stages.  A sharded
 * handle answers bit for bit what the plain index answers.  Extra HBM, allocated at the first call: two blocks of 512 rows and lists of
 * 512 x max(k + E, 64) entries on devices[0].
 */
int mx_index_search_like(mx_index *idx, const float *queries, const float *query_weights, const uint64_t *example_ids,
                         const float *example_weights, int R, int m, int k, int exclude_examples, uint64_t *ids, float *scores,
                         float *dists, int32_t *n_found, int32_t *n_used, float *combined);
int mx_index_search_like_device(mx_index *idx, const float *d_queries, const float *query_weights, const uint64_t *example_ids,
                                const float *example_weights, int R, int m, int k, int exclude_examples, uint64_t *d_ids,
                                float *d_scores, float *d_dists, int32_t *d_n_found, int32_t *d_n_used, float *d_combined);

/*
 * Score named rows: what does this query score against THESE rows?  The exact scores of a candidate list per query -- the hits of a
 * keyword backend before the two lists are fused, a cached result page after the query changed, a user's own documents, the gold
 * passage of an evaluation -- and the ranking of each list.  Nothing is scanned and no row leaves HBM: one workgroup per query
 * translates its ids to rows on the device and runs the exact arithmetic on them.
 * queries is [B, dim]; cand_ids is [B, m] and is HOST memory on both variants, ids as search returns them (id_offset applied).
 * Outputs: scores / dists / order [B, m], n_found [B]; dists, order and n_found may be NULL.
 *   found       Entry (b, j) is FOUND iff mx_index_search(queries[b], k = every live row) would list cand_ids[b, j]: the id names a live
 *               (not removed) row whose dist is defined (not NaN).  scores[b, j] and dists[b, j] are then bit for bit that list's
 *               entry for the id: f32 products, sequential f64 sums in element order, then the dist and the score of the plain search,
 *               on the rows as stored (a bf16 corpus: its values widened).
 *   blank       An entry that is not found holds score 0 and dist +inf: id 0 (the padding of ragged lists), an id that names no row, a
 *               removed row, a NaN dist.  The call still returns MX_OK.
 *   repeats     An id named twice in a list is scored twice.
 *   n_found     n_found[b] = the found entries of query b.
 *   order       order[b, r], r < n_found[b], is the position j of the r-th best found entry by (dist ascending, id ascending, position
 *               j ascending); the slots from n_found[b] on hold -1.  For distinct ids that is the order in which the plain search lists
 *               them: cand_ids[b, order[b, :k]] is the exact top-k of the list.
 *   zero query  A zero-norm query has dist 0 against every row, as in mx_index_search.
 * Arguments are checked first: B < 0, m < 1, a NULL queries / cand_ids / scores with B > 0: MX_EINVAL; m > 4096 (the cap on k):
 * MX_EUNSUPPORTED; then a null index: MX_ESEARCH; B = 0 is MX_OK.  Non-finite queries are rejected as by mx_index_search.  Rows wider
 * than 8192 padded dims: MX_EUNSUPPORTED, as for mx_index_search_mmr.  B is split into batches of 512.
 * Thread-safe beside every other call.  Concurrent callers are NOT combined into shared passes: each call holds the index from its
 * first upload to the end of its last kernel, so no append, removal or compaction slips in between.  The call touches neither
 * mx_index_stats nor the filter copy (its kind, its demotion and promotion counts) and does not depend on the search mode.  A sharded
 * handle answers bit for bit what the plain index answers: every shard scores the pairs whose rows it owns, the dist blocks meet on
 * devices[0], and the ranking runs once on the combined block.  Extra HBM, allocated at the first call: blocks of 512 x max(m, 64)
 * entries.
 */
int mx_index_score_ids(mx_index *idx, const float *queries, int B, const uint64_t *cand_ids, int m, float *scores, float *dists,
                       int32_t *order, int32_t *n_found);
int mx_index_score_ids_device(mx_index *idx, const float *d_queries, int B, const uint64_t *cand_ids, int m, float *d_scores,
                              float *d_dists, int32_t *d_order, int32_t *d_n_found);

/*
 * Grouped search: the k best DOCUMENTS, each represented by its best segment.  A row is one window of a document, and a document is
 * stored as a run of overlapping windows: a plain top-10 for a question one long document answers well is ten windows of it.
 *
 * A GROUPING says which rows belong together: one u32 key per row, kept in HBM on devices[0] and named by handle, like a resident
 * filter.  Key 0 means "ungrouped": such a row is a group of its own.  A new grouping has key 0 everywhere, and rows appended after
 * the last edit have key 0 until a call names them.  Nothing is written to the store files and nothing is dealt to shards: the host
 * that owns the segment -> document mapping builds the grouping, and builds it again after a restart.  4 bytes of HBM per row.
 *   mx_grouping_create     the all-zero grouping of the rows of `idx`.  The grouping holds a reference on the index, as a filter does;
 *                          mx_grouping_destroy drops it.
 *   mx_grouping_set_ranges range i, the ids [ranges[2 i], ranges[2 i + 1]), gets the key keys[i]; a key of 0 un-groups.  The ranges
 *                          of ONE call must be pairwise disjoint (empty ranges aside): an overlap, lo > hi in any pair, or a NULL
 *                          ranges / keys with n_ranges > 0 is MX_EINVAL.  They may come in any order.
 *   mx_grouping_set_ids    ids[i] gets the key keys[i].  Ids may repeat and come in any order; an id named twice in one call with
 *                          DIFFERENT keys is MX_EINVAL (the same key twice is fine).
 *   mx_grouping_get_keys   keys[i] = the key of the row ids[i] names; 0 for an id that names no row.
 *   mx_grouping_count      n_keyed: rows with a non-zero key; n_live_keyed: those of them that are not removed (either may be NULL).
 * Ids are the ids search returns, id_offset applied at the time of the call; an id outside [id_offset + 1, id_offset + size] at that
 * time is ignored.  The keys are stored per row: a later mx_index_set_id_offset moves the ids along with the rows.  Removed rows keep
 * their key and are never listed.  A failing call changes nothing.  mx_index_clear, mx_index_load and an mx_index_compact that dropped
 * at least one row make every grouping of the index STALE: every call with it except mx_grouping_destroy returns MX_EINVAL with a
 * message that says so.  A grouping named together with an index it was not made for: MX_EINVAL.  Grouping calls are thread-safe
 * beside every other call on the index; a search sees a grouping before or after a whole set_* call, never half of one; a grouping
 * must not be destroyed while a call that names it is running.
 *
 *   mx_index_search_grouped[_device]   queries [B, dim]; outputs ids / scores / dists / keys / group_rows [B, k], n_found / complete
 *                          [B]; dists, keys, group_rows and complete may be NULL.  f may be NULL.  Per query:
 *   candidates  the list L = what mx_index_search gives with k = fetch, bit for bit -- with f, what mx_index_search_with_filter
 *               gives: (dist, id) order, removed rows, id_offset, the AUTO path up to fetch = 256 and the EXACT path above, B split
 *               into batches of 512.  The candidate stage IS a plain search pass: it counts as one in mx_index_stats and in the
 *               filter copy's heuristics.
 *   heads       walking L in its order, an entry is a HEAD if its key is 0 or no earlier entry of L has its key.  The first k heads
 *               are reported, in that order: ids / scores / dists are the entry's, unchanged; keys is its key; group_rows the number
 *               of entries of L with that key (1 for key 0).  n_found = min(k, heads in L).  Unused slots hold id 0, score 0,
 *               dist +inf, key 0, group_rows 0.
 *   complete    complete[b] = 1 iff n_found[b] == k or L holds fewer than fetch entries.
 * complete = 1 promises the EXACT top-k groups over ALL live rows (all allowed live rows, with f), each with its exact best row and
 * score; complete = 0 promises the exact grouping of the top-fetch list only, and a larger fetch may find more groups.  (L is a prefix of
 * all rows in (dist, id) order: with k heads in it, nothing ahead of a head is missing, and every group without a row in L lies behind
 * its last entry; a list shorter than fetch holds every row.  DESIGN.md 3.16.)  group_rows is always with respect to L.
 * Arguments are checked first: B < 0, k < 1, fetch < k, a NULL grouping, a NULL queries / ids / scores / n_found with B > 0:
 * MX_EINVAL; fetch > 4096 (the cap on k): MX_EUNSUPPORTED; then a null index: MX_ESEARCH; then a stale or foreign grouping or filter:
 * MX_EINVAL.  Non-finite queries are rejected as by mx_index_search.  Thread-safe beside every other call.  Concurrent callers are
 * NOT combined into shared passes: each call holds the index across its candidate stage and its grouping (both see one snapshot of
 * the rows and of the keys) and never rides in a plain, filtered or range pass.  A sharded handle merges the candidate lists on
 * devices[0] as a search does and groups there: the answer equals the plain index's bit for bit.  The grouping step costs
 * O(fetch^2) key compares per query, independent of dim and of the row count.  Extra HBM, allocated at the first call: the candidate
 * lists (shared with mx_index_search_mmr) and, for the host-pointer variant, 512 x max(k, 16) keys and counts.
 */
typedef struct mx_grouping mx_grouping;
int mx_grouping_create(mx_index *idx, mx_grouping **out);
void mx_grouping_destroy(mx_grouping *g);
int mx_grouping_set_ranges(mx_grouping *g, const uint64_t *ranges, const uint32_t *keys, uint64_t n_ranges);
int mx_grouping_set_ids(mx_grouping *g, const uint64_t *ids, const uint32_t *keys, uint64_t n_ids);
int mx_grouping_get_keys(mx_grouping *g, const uint64_t *ids, uint64_t n_ids, uint32_t *keys);
int mx_grouping_count(mx_grouping *g, uint64_t *n_keyed, uint64_t *n_live_keyed);
int mx_index_search_grouped(mx_index *idx, mx_grouping *g, mx_filter *f, const float *queries, int B, int k, int fetch, uint64_t *ids,
                            float *scores, float *dists, uint32_t *keys, int32_t *group_rows, int32_t *n_found, uint8_t *complete);
int mx_index_search_grouped_device(mx_index *idx, mx_grouping *g, mx_filter *f, const float *d_queries, int B, int k, int fetch,
                                   uint64_t *d_ids, float *d_scores, float *d_dists, uint32_t *d_keys, int32_t *d_group_rows,
                                   int32_t *d_n_found, uint8_t *d_complete);

/*
 * Grouped search with members: the k best documents, each with its n best segments -- or a flat top-k in which no document supplies
 * more than per_key segments.  Both forms read the candidate list L of mx_index_search_grouped (same candidates, same heads, same
 * path choice, statistics and batches of 512) and a grouping; key 0 is "ungrouped", a group of its own.
 *
 *   mx_index_search_group_rows[_device]   queries [B, dim]; outputs ids / scores / dists [B, k, n]; keys / group_rows / n_members /
 *                          members_complete [B, k]; n_found / complete [B].  dists, keys, group_rows, n_members, members_complete
 *                          and complete may be NULL.  f may be NULL.  Per query:
 *   heads       as in mx_index_search_grouped: the first k heads of L in list order; n_found = min(k, heads in L).
 *   members     for head j with key K != 0, slot [j, r] holds the r-th entry of L with key K, in list order, r < n: the entry's id,
 *               score and dist unchanged.  Slot [j, 0] is the head itself.  A key-0 head has itself as its only member.
 *               group_rows[j] = the entries of L under K (1 for key 0); n_members[j] = min(n, group_rows[j]).  Unused slots hold id 0,
 *               score 0, dist +inf; behind the heads found keys, group_rows, n_members and members_complete are 0.
 *   complete    complete[b] = 1 iff n_found[b] == k or L holds fewer than fetch entries: the heads are the exact top-k groups.
 *   members_complete   [j] = 1 iff n_members[j] == n, or L holds fewer than fetch entries, or the key is 0.
 * The listed members of a group are ALWAYS its exact best n_members live (with f: allowed live) rows over all rows, in (dist, id)
 * order: L is a prefix of that order, so a row of the group outside L lies behind every listed one.  members_complete = 1 adds that
 * the group has no further member that belongs in its first n.  Where it is 0, mx_grouping_key_counts settles it: a group whose
 * n_members equals its live row count is fully listed (with or without f: the allowed rows are a subset of the live ones).  With
 * n = 1, ids, scores, dists, keys, group_rows, n_found and complete equal those of mx_index_search_grouped bit for bit.
 *
 *   mx_index_search_capped[_device]   outputs ids / scores / dists / keys [B, k]; n_found / complete [B]; dists, keys and complete
 *                          may be NULL.  Walking L in its order, an entry is ACCEPTED if its key is 0 or fewer than per_key earlier
 *                          entries of L have its key.  The first k accepted entries are reported unchanged, with their key; unused
 *                          slots hold id 0, score 0, dist +inf, key 0.  complete[b] = 1 iff n_found[b] == k or L holds fewer than fetch
 *                          entries; then the answer is the exact capped top-k over all rows (acceptance depends only on the entries
 *                          ahead of an entry, so the walk over the prefix equals the walk over everything).  per_key = 1 gives the
 *                          heads of mx_index_search_grouped bit for bit; per_key >= fetch gives mx_index_search at k.
 *
 *   mx_grouping_key_counts for each of keys[0, n_keys): n_rows[i] = the rows of the index under that key, n_live[i] = those of them not
 *                          removed (either may be NULL).  Key 0 counts the ungrouped rows, those appended after the last edit
 *                          included.  Keys may repeat and come in any order.  A NULL keys with n_keys > 0: MX_EINVAL; n_keys > 2^20:
 *                          MX_EUNSUPPORTED.  One pass over the keys of all rows; a sharded handle counts against the removal masks
 *                          of all shards, as mx_grouping_count does.
 *
 * Arguments are checked first: B < 0, k < 1, n < 1, per_key < 1, fetch < k, a NULL grouping, a NULL queries / ids / scores / n_found
 * with B > 0: MX_EINVAL; fetch > 4096, n > 16 or k * n > 4096: MX_EUNSUPPORTED; then a null index: MX_ESEARCH; then a stale or foreign
 * grouping or filter: MX_EINVAL.  Non-finite queries are rejected as by mx_index_search.  Thread-safe beside every other call; as
 * with mx_index_search_grouped, concurrent callers are NOT combined into shared passes, and a sharded handle merges the lists on
 * devices[0] and answers as the plain index does, bit for bit.  O(fetch^2) key compares per query.  Extra HBM, allocated at the
 * first call: the candidate lists, the result staging at width k * n, and 512 x max(k, 16) per-head words on the grouping.
 */
int mx_index_search_group_rows(mx_index *idx, mx_grouping *g, mx_filter *f, const float *queries, int B, int k, int n, int fetch,
                               uint64_t *ids, float *scores, float *dists, uint32_t *keys, int32_t *group_rows, int32_t *n_members,
                               uint8_t *members_complete, int32_t *n_found, uint8_t *complete);
int mx_index_search_group_rows_device(mx_index *idx, mx_grouping *g, mx_filter *f, const float *d_queries, int B, int k, int n, int fetch,
                                      uint64_t *d_ids, float *d_scores, float *d_dists, uint32_t *d_keys, int32_t *d_group_rows,
                                      int32_t *d_n_members, uint8_t *d_members_complete, int32_t *d_n_found, uint8_t *d_complete);
int mx_index_search_capped(mx_index *idx, mx_grouping *g, mx_filter *f, const float *queries, int B, int k, int per_key, int fetch,
                           uint64_t *ids, float *scores, float *dists, uint32_t *keys, int32_t *n_found, uint8_t *complete);
int mx_index_search_capped_device(mx_index *idx, mx_grouping *g, mx_filter *f, const float *d_queries, int B, int k, int per_key,
                                  int fetch, uint64_t *d_ids, float *d_scores, float *d_dists, uint32_t *d_keys, int32_t *d_n_found,
                                  uint8_t *d_complete);
int mx_grouping_key_counts(mx_grouping *g, const uint32_t *keys, uint64_t n_keys, uint64_t *n_rows, uint64_t *n_live);

/*
 * Boosted search: relevance plus something the vectors do not carry -- how recent a segment is, how important the host has marked it,
 * how trusted its source is.  Rows are ranked by score + weight * prior, exactly, and the answer says whether a row outside the
 * candidates could have won.
 *
 * A PRIOR is one f32 per row, kept in HBM on devices[0] and named by handle, like a grouping.  A new prior is 0 everywhere, and rows
 * appended after the last edit read 0 until a call names them.  Negative values are a penalty.  Nothing is written to the store files
 * and nothing is dealt to shards; there is no host copy of the values.  4 bytes of HBM per row.
 *   mx_prior_create      the all-zero prior of the rows of `idx`.  It holds a reference on the index; mx_prior_destroy drops it.
 *   mx_prior_set_ranges  range i, the ids [ranges[2 i], ranges[2 i + 1]), gets values[i].  The ranges of ONE call must be pairwise
 *                        disjoint (empty ranges aside): an overlap, lo > hi in any pair, or a NULL ranges / values with n_ranges > 0
 *                        is MX_EINVAL.  They may come in any order.
 *   mx_prior_set_ids     ids[i] gets values[i].  Ids may repeat and come in any order; an id named twice in one call with values of
 *                        DIFFERENT bits is MX_EINVAL (the same bits twice are fine).
 *                        Both: a value that is NaN or +-inf is MX_EINVAL, and nothing is written.
 *   mx_prior_get         values[i] = the value of the row ids[i] names; 0 for an id that names no row.
 *   mx_prior_bound       *hi = an upper bound of every value in the array, the one the certificate below uses.  It starts at 0 (rows
 *                        nobody set read 0), every successful edit raises it to the largest value the call was handed, and no edit
 *                        lowers it.  refresh = 1 first replaces it by the exact maximum of 0 and the values of the rows that are not
 *                        removed (one reduction over the array): the remedy after large values were overwritten with small ones.
 *                        refresh other than 0 or 1: MX_EINVAL.  hi may be NULL.
 * Ids, id_offset, removed rows, failing calls, staleness after mx_index_clear / mx_index_load / a compaction that dropped rows
 * (MX_EINVAL, "stale" in the message), a foreign index (MX_EINVAL), threads and destruction: as for a grouping, above.
 *
 *   mx_index_search_boosted[_device]   queries [B, dim]; weights f32 [B] in HOST memory on both variants, NULL = 1.0 for every query;
 *                        outputs ids / scores / dists / priors f32 [B, k], combined f64 [B, k], n_found / complete [B]; dists, priors,
 *                        combined and complete may be NULL.  f may be NULL.  Per query b, with w = weights[b]:
 *   candidates  the list L = what mx_index_search gives with k = fetch, bit for bit -- with f, what mx_index_search_with_filter
 *               gives; m entries.  As for grouped search the candidate stage IS a plain search pass.
 *   combined    c_j = (double)score_j + (double)w * (double)prior_j for entry j: the f32 score L reports, the row's prior.  The product
 *               is exact in f64, so c_j is rounded once: the same bits as that expression anywhere else.
 *   order       by c descending, then by position in L (its (dist, id) order).  The first min(k, m) entries are reported: ids / scores /
 *               dists are the entry's, unchanged; priors and combined are prior_j and c_j.  n_found = min(k, m).  Unused slots hold
 *               id 0, score 0, dist +inf, prior 0, combined 0.
 *   complete    complete[b] = 1 iff m < fetch, or the k-th reported c is strictly greater than
 *               U = (double)score_last + (double)w * (double)hi, score_last the score of L's last entry, hi as mx_prior_bound(p, 0).
 * complete = 1 promises the EXACT top-k of ALL live rows (all allowed live rows, with f) by (c descending, dist, id); complete = 0
 * promises the exact re-ranking of L only, and a larger fetch (or a refreshed bound) may change the answer.  (Every live row outside
 * L scores at most score_last and has a prior of at most hi, so with w >= 0 its c is at most U.  DESIGN.md 3.17.)  The test is
 * sufficient, not necessary: at w = 0 with equal scores at the end of L it reports 0 for an answer that is right.
 * Arguments are checked first: B < 0, k < 1, fetch < k, a NULL prior, a NULL queries / ids / scores / n_found with B > 0, a weight
 * that is negative, NaN or infinite: MX_EINVAL; then fetch > 4096: MX_EUNSUPPORTED; then a null index: MX_ESEARCH; then a stale or
 * foreign prior or filter: MX_EINVAL.  Non-finite queries are rejected as by mx_index_search.  B is split into batches of 512.
 * Thread-safe beside every other call; NOT combined with other callers, as grouped search.  A sharded handle merges the candidate
 * lists on devices[0] as a search does and re-ranks there: the answer equals the plain index's bit for bit.  The re-ranking costs
 * O(fetch^2) f64 compares per query, independent of dim and of the row count.  Extra HBM, allocated at the first call: the candidate
 * lists (shared with mx_index_search_mmr) and, for the host-pointer variant, 512 x max(k, 16) priors and combined values.
 */
typedef struct mx_prior mx_prior;
int mx_prior_create(mx_index *idx, mx_prior **out);
void mx_prior_destroy(mx_prior *p);
int mx_prior_set_ranges(mx_prior *p, const uint64_t *ranges, const float *values, uint64_t n_ranges);
int mx_prior_set_ids(mx_prior *p, const uint64_t *ids, const float *values, uint64_t n_ids);
int mx_prior_get(mx_prior *p, const uint64_t *ids, uint64_t n_ids, float *values);
int mx_prior_bound(mx_prior *p, int refresh, float *hi);
int mx_index_search_boosted(mx_index *idx, mx_prior *p, mx_filter *f, const float *queries, const float *weights, int B, int k, int fetch,
                            uint64_t *ids, float *scores, float *dists, float *priors, double *combined, int32_t *n_found,
                            uint8_t *complete);
int mx_index_search_boosted_device(mx_index *idx, mx_prior *p, mx_filter *f, const float *d_queries, const float *weights, int B, int k,
                                   int fetch, uint64_t *d_ids, float *d_scores, float *d_dists, float *d_priors, double *d_combined,
                                   int32_t *d_n_found, uint8_t *d_complete);

/*
 * Filters from row attributes: a resident filter built from what the rows already carry in HBM -- a predicate on a prior's values
 * ("only segments stamped after T", "only sources trusted >= 0.8"), membership of the row's grouping key in a list ("only these 300
 * documents") -- and the set algebra of filters that exist (tenant AND tag AND NOT already-shown).  No id is enumerated on the host
 * and none is uploaded: the device decides the set in one pass over 4 bytes per row.  The result is an ordinary
 * mx_filter: mx_index_search_with_filter, grouped search and boosted search take it as they take any other, and mx_filter_count,
 * mx_filter_get_ranges and every search behave exactly as after an mx_filter_set_ids with the same rows.
 *   mx_filter_set_where  the selection S is the rows r in [0, size) at the time of the call with lo <= v_r && v_r <= hi, v_r the value
 *                        of row r in `p`: 0 for a row at or past the prior's length, exactly as mx_prior_get reads it.  The comparison
 *                        is plain IEEE f32, so a stored -0.0 matches [0, 0].  allow = 1 adds S to the set, allow = 0 takes S away (any
 *                        other value: MX_EINVAL).  +-inf bounds are allowed and make a one-sided predicate; lo > hi selects nothing
 *                        and returns MX_OK; a NaN bound is MX_EINVAL.  Removed rows are selected like any other row: they stay in the
 *                        set and are never returned.  n_selected may be NULL; it receives |S|, not the change of the set.
 *   mx_filter_set_keys   the same with S = the rows whose key in `g` is one of keys[0 .. n_keys).  Keys may repeat and come in any
 *                        order.  Key 0 may be listed: it names the ungrouped rows, those past the grouping's length included.
 *                        n_keys = 0 is a no-op (S is empty).  NULL keys with n_keys > 0: MX_EINVAL; n_keys > 2^20: MX_EUNSUPPORTED.
 *   mx_filter_combine    dst = a op b, bitwise over the rows; MX_FILTER_ANDNOT is a and not b.  dst may be a or b, and a may be b.  An
 *                        op outside the enum: MX_EINVAL.  The operands hold no row at or past size, so the result holds none either.
 *   mx_filter_invert     the complement within [0, size) at the time of the call; rows appended later are outside the set, as for
 *                        every filter.
 * All four: a NULL handle is MX_EINVAL ("null filter", "null prior", "null grouping") before anything else; objects of different
 * indexes: MX_EINVAL; a stale filter, prior or grouping: MX_EINVAL with "stale" in the message.  A failing call changes nothing.  The
 * calls hold the handle's mutex as mx_filter_set_ids does: a search sees the filter before or after a whole call, never half of one.
 * A sharded handle evaluates the predicate on devices[0], where priors and groupings live, and deals the selected rows to the shards'
 * bitmaps; combine and invert run shard by shard.  Its filters equal a plain index's bit for bit.  One selection bitmap (1 bit per
 * row) crosses to the host per set_where / set_keys call: the host mirror of the filter is taken from the kernel's own output.
 */
enum { MX_FILTER_AND = 0, MX_FILTER_OR = 1, MX_FILTER_ANDNOT = 2, MX_FILTER_XOR = 3 };
int mx_filter_set_where(mx_filter *f, mx_prior *p, float lo, float hi, int allow, uint64_t *n_selected);
int mx_filter_set_keys(mx_filter *f, mx_grouping *g, const uint32_t *keys, uint64_t n_keys, int allow, uint64_t *n_selected);
int mx_filter_combine(mx_filter *dst, mx_filter *a, mx_filter *b, int op);
int mx_filter_invert(mx_filter *f);

/* Search strategy (testing / diagnostics).  AUTO = low-precision MFMA streaming scan (int8 or bf16
 * filter copy, or the f32 rows) that certifies a candidate superset, f32 then exact f64 rescoring of the
 * candidates, per-query fallback to EXACT when a candidate buffer overflows twice.  EXACT = f64 arithmetic on every row (slow, always available). */
enum { MX_SEARCH_AUTO = 0, MX_SEARCH_EXACT = 1 };
int mx_index_set_search_mode(mx_index *idx, int mode);

/* Filter copy.  By default the index keeps, next to the f32 rows, a low-precision copy of them laid out
 * for the MFMA scan; the AUTO scan streams that copy instead of the f32 rows and candidates are rescored
 * from the f32 rows, so results are bit-identical with every kind and without one.
 *   on = 0  no copy (the scan reads the f32 rows: 4 bytes per element streamed)
 *   on = 1  a copy whose kind the library chooses (the default): int8 up to 1024 dims, bf16 above; an int8
 *           copy is rebuilt as bf16 -- once, from the f32 rows -- when the corpus proves too dense for its
 *           certificate (more than 1/16 of a batch overflows the int8 pass, or the retry pass has become
 *           habitual) and built again as int8 once the collection has doubled since (or when this call is
 *           repeated with on = 1); mx_index_stats.filter_kind / filter_demotions / filter_promotions tell
 *   on = 2  int8 copy (+25 % HBM: rows*dim_pad bytes + 16 bytes per 64 rows): one quantisation step and one
 *           measured residual bound per 32 rows, exact integer sums; the certificate is 4-5x wider than
 *           bf16's, so finish_kernel sifts a few hundred candidates per query instead of a few dozen
 *   on = 3  bf16 copy (+50 % HBM: rows*dim_pad*2 bytes)
 * (Re)builds from the resident rows when the kind changes.  If HBM for the copy cannot be allocated while
 * the index grows, it is dropped silently and the index continues on the f32 scan.  Environment:
 * MEMEX_HIP_FILTER=i8|bf16 pins the kind for every index opened afterwards. */
int mx_index_set_filter_copy(mx_index *idx, int on);

/*
 * Corpus mode (compressed corpus).  MX_CORPUS_F32 (default): the f32 rows are
 * kept and results are bit-identical to the reference's arithmetic on them.  MX_CORPUS_BF16: the index
 * keeps ONLY bf16(c / |c|) -- 2 bytes per element instead of 4 (+2 for the filter copy), i.e. a third
 * of the default footprint: 7.7 GB for 10M x 384, ~110M x 384-d rows per 288 GB GPU.  Searches are then
 * EXACT with respect to the stored (rounded) rows: same pipeline, the rescoring stages read the
 * stored rows, and the answer is bit-identical to the reference's arithmetic applied to
 * mx_index_get_rows() -- each cosine is within ~2e-3 of the f32 one, so recall@10 against the f32
 * corpus stays ~0.99 while the scan is unchanged.  Choose the mode while the index is empty.
 * dim <= 1536.  mx_index_save marks such a store in the file header; loading it into an index of
 * either mode reproduces the stored rows exactly.
 */
enum { MX_CORPUS_F32 = 0, MX_CORPUS_BF16 = 1 };
int mx_index_set_corpus_mode(mx_index *idx, int mode);
/* Rows [first_row, first_row + n) (0-based, insertion order) as stored, into out [n, dim] f32: the
 * inserted values (F32 mode) or the stored near-unit bf16 values widened to f32 (BF16 mode; zero-norm
 * rows come back as zeros).  Also how a collection is re-exported / rebuilt elsewhere. */
int mx_index_get_rows(mx_index *idx, uint64_t first_row, uint64_t n, float *out);

/*
 * Persistence.  Replaces HnswStore::save / load / has_store (storage/local.rs:110-165).  Files in
 * `dir`: `vectors.mxflat` (header + raw f32 rows) and, once rows have been removed, `vectors.mxdead`
 * (magic "MXDEAD01" | u64 count | count x u64 removed rows, 0-based without id offset; entries are
 * appended and the count patched last; no file = nothing removed; a damaged one fails the load with
 * MX_EIO and leaves the index as it was).  A compacted index (mx_index_compact) writes "MXFLAT02" and
 * "MXDEAD02", whose headers carry its compaction generation (u64, after the row count); a removal file
 * whose generation is not the vector file's is stale: ignored on load, replaced on the next save.
 * The string-id map `vectors.meta.json`
 * (local.rs:19,156-163) stays on the Rust side unchanged.
 */
int mx_index_save(mx_index *idx, const char *dir);
int mx_index_load(mx_index *idx, const char *dir); /* replaces current contents */
int mx_index_has_store(const char *dir, int *exists);
int mx_index_store_info(const char *dir, int *dim, uint64_t *n_rows); /* header of vectors.mxflat */
int mx_index_remove_files(const char *dir);        /* the file half of delete_all, local.rs:36-46 */

/* Counters for the bench / roofline report (cumulative since open or last reset). */
typedef struct mx_index_stats {
    uint64_t searches;          /* query batches served                                   */
    uint64_t queries;           /* queries served                                          */
    uint64_t fallback_queries;  /* queries answered by the EXACT path (rescan overflowed too) */
    uint64_t scan_launches;     /* launches of the main streaming-scan kernel              */
    uint64_t scan_bytes;        /* bytes those launches streamed: rows*dim_pad*(1 int8 copy, 2 bf16 copy, 4 f32 rows) */
    double scan_ms;             /* HIP-event time of those launches (profiling on)         */
    uint64_t candidates;        /* candidates that passed the filter and were rescored in f32 */
    double max_abs_err;         /* profiling only: max |approx - exact| cosine on candidates */
    uint64_t filter_copy_bytes; /* HBM held by the filter copy (0 = scanning the f32 rows) */
    uint64_t retry_queries;     /* queries rescanned once with a tightened threshold (lane buffer overflow) */
    double approx_err_bound;    /* largest per-query bound e1 on |filter score - cosine| of the last batch */
    uint64_t filter_kind;       /* what the scan streams now: 0 = the f32 rows, 2 = int8 filter copy, 3 = bf16 filter copy */
    uint64_t filter_demotions;  /* times an automatically chosen int8 copy was rebuilt as bf16 (dense corpus)   */
    uint64_t filter_promotions; /* times a demoted index got its int8 copy back (the collection had doubled since)  */
    uint64_t listed_rows;       /* rows on the side list finish_kernel adds to every query: zero norm, or a norm outside [1e-15, 1e15] */
    uint64_t exchange_fallbacks;/* sharded index: times the RCCL exchange failed at run time and peer copies took over  */
    uint64_t filter_centred;    /* 1 = the bf16 copy holds the rows minus their component along the corpus mean direction
                                   (a rebuilt copy of a corpus that sits in a cone: a several times tighter certificate)   */
    double exchange_ms;         /* sharded index: host time from "every shard has answered" to "merged result complete" (the
                                   all-gather or peer copies' tail, merge_kernel, n_found, one synchronise): the serial tail of
                                   a step that the shards' own work does not hide                                           */
    uint64_t filtered_queries;  /* queries served by mx_index_search_filtered[_device]                                          */
    uint64_t subset_queries;    /* ... of them answered by the subset kernel (few allowed rows: no scan)           */
} mx_index_stats;
/* sizeof(mx_index_stats) of the library that is loaded: a shim compares it with its own at start-up (the struct grows
 * at the end from version to version; mx_version() names the release). */
size_t mx_index_stats_size(void);
int mx_index_set_profiling(mx_index *idx, int on); /* record HIP events around the scan kernel */
int mx_index_get_stats(mx_index *idx, mx_index_stats *out);
int mx_index_reset_stats(mx_index *idx);

/*
 * Multi-GPU merge: after an RCCL all-gather of per-shard results
 * ([G, B, k] ids + dists, each shard list ordered), produce the global top-k ordered by
 * (dist, id) and the scores.  Pointers are device pointers on `device`.
 */
int mx_topk_merge_device(int device, const uint64_t *d_ids, const float *d_dists, int G, int B, int k,
                         uint64_t *d_out_ids, float *d_out_dists, float *d_out_scores);
/* Same merge for ONE all-gather: every shard writes its results into one block
 * [ids: B*k u64][dists: B*k f32] (pass `block` and `block + B*k*8` to mx_index_search_device), the
 * collective gathers the G blocks back to back into d_packed. */
int mx_topk_merge_packed_device(int device, const void *d_packed, int G, int B, int k, uint64_t *d_out_ids,
                                float *d_out_dists, float *d_out_scores);
/* The same merge ENQUEUED on the caller's stream (a hipStream_t; NULL = default stream), returning
 * at once: put it on the stream the all-gather was issued on and no host round trip separates the
 * collective from the merge. */
int mx_topk_merge_packed_async(int device, void *hip_stream, const void *d_packed, int G, int B, int k,
                               uint64_t *d_out_ids, float *d_out_dists, float *d_out_scores);

/* =====================================================================================
 * Sentence encoder  (replaces the rust-bert model owned by SentenceEmbedder::runner,
 * lib/libmemex/src/llm/embedding.rs:94-135; `model.encode(&segments)` at :109)
 * ===================================================================================== */
typedef struct mx_encoder mx_encoder;

enum { MX_POOL_MEAN = 0, MX_POOL_CLS = 1 };

typedef struct mx_encoder_cfg {
    int32_t layers;     /* 6  (all-MiniLM-L6-v2) / 12 (all-MiniLM-L12-v2, bge-base-en)      */
    int32_t hidden;     /* 384 / 768: nothing else (see "What mx_encoder_create accepts" below) */
    int32_t heads;      /* 12; hidden/heads must be 32 or 64: 12 or 6 heads at 384, 24 or 12 at 768 */
    int32_t ffn;        /* 1536 / 3072; any multiple of 384                                  */
    int32_t vocab;      /* 30522                                                              */
    int32_t max_pos;    /* rows of the position table: 512 (BERT) / 514 (RoBERTa); sequences <= 512 tokens */
    int32_t type_vocab; /* 2                                                                  */
    float ln_eps;       /* 1e-12                                                              */
    int32_t pooling;    /* MX_POOL_MEAN (MiniLM) | MX_POOL_CLS (bge)                          */
    int32_t normalize;  /* 1 = L2-normalise the pooled vector                                 */
    int32_t pos_offset; /* row of the position table used by a sequence's first token: 0 for BERT
                           (MiniLM, bge); 2 for RoBERTa-style checkpoints such as all-distilroberta-v1
                           (embedding.rs:29,159: position ids start at padding_idx + 1; such models also
                           have max_pos = 514, type_vocab = 1, ln_eps = 1e-5)                  */
    int32_t precision;  /* MX_PREC_BF16 (0, the default: bf16 operands, f32 accumulation -- the ingest path) |
                           MX_PREC_BF16X3: every GEMM operand carried as hi + lo bf16 (three MFMA products per
                           f32 product), f32 hidden state and f32 attention -- scores BETWEEN embeddings within
                           1e-3 of the f64 evaluation of the f32 CPU path (embedding.rs:109) on every draw of
                           checkpoint-like weights tried (2e-5 typical, 6e-4 at worst), where the bf16 path moves
                           them by 1e-2 ... 4e-2; about 3.2x slower.  What the loaders pick
                           for CLS-pooled hidden-768 models |
                           MX_PREC_MIXED (round 6): the attention block (Q, K, V, scores, PV, out-projection) as in
                           MX_PREC_BF16X3, the MLP's two GEMMs as TWO fp16 products per product (fp16 weights x fp16 hi + lo
                           activations): 15-17 % faster than MX_PREC_BF16X3; scores within 5.3e-4 on nine of eleven draws of
                           checkpoint-like weights, 1.1e-3 on the other two, where MX_PREC_BF16X3 has 6e-4
                           (profiles/r6_precision_modes_over_seeds.txt) -- "about 1e-3 at worst", opt-in |
                           MX_PREC_MIXED1 (round 6): MX_PREC_MIXED with the MLP on ONE fp16 product per product (weights, LayerNorm
                           output and GELU output one fp16 value each; residual stream, GEMM results and LayerNorm stay f32) and P
                           as one bf16 value in P.V: 0.39 / 0.48 of the bf16 rate, scores 1.5e-5 ... 2e-2 by draw -- an order
                           of magnitude better than bf16, NOT a mode that holds 1e-3; opt-in                           */
} mx_encoder_cfg;
enum { MX_PREC_BF16 = 0, MX_PREC_BF16X3 = 1, MX_PREC_MIXED = 2, MX_PREC_MIXED1 = 3 };
/* sizeof(mx_encoder_cfg) of the library that is loaded: the struct grew a trailing field (`precision`) and may again; a shim
 * built against an older header compares this with its own sizeof at start-up instead of letting the library read past
 * its struct (same handshake as mx_index_stats_size). */
size_t mx_encoder_cfg_size(void);

/*
 * Weight blob: f32, little-endian, tensors concatenated in this order (HF BertModel names,
 * Linear weights [out, in]):
 *   embeddings.word_embeddings.weight [vocab,H]; embeddings.position_embeddings.weight [max_pos,H];
 *   embeddings.token_type_embeddings.weight [type_vocab,H]; embeddings.LayerNorm.{weight,bias} [H];
 *   then per layer l: attention.self.{query,key,value}.{weight [H,H], bias [H]} (q,k,v in turn);
 *   attention.output.dense.{weight [H,H], bias}; attention.output.LayerNorm.{weight,bias};
 *   intermediate.dense.{weight [F,H], bias [F]}; output.dense.{weight [H,F], bias [H]};
 *   output.LayerNorm.{weight,bias}.
 * mx_encoder_weight_bytes() gives the exact size.  memex_amd/weights.py packs it from a
 * state-dict / safetensors file.
 */
size_t mx_encoder_weight_bytes(const mx_encoder_cfg *cfg);

/*
 * What mx_encoder_create accepts -- and whatever it accepts encodes every batch of B >= 1 sequences of
 * 1 <= S <= min(512, max_pos - pos_offset) tokens, in every precision mode (tests/test_encoder_lattice_gpu.py):
 *   layers    1 ... 48                                              else MX_EUNSUPPORTED
 *   hidden    384 or 768                                            else MX_EUNSUPPORTED
 *   heads     must divide hidden                                    else MX_EINVAL
 *             hidden / heads = 32 or 64: 12 or 6 heads at hidden 384, 24 or 12 at hidden 768   else MX_EUNSUPPORTED
 *             (24 heads are as good as 12: the attention work list is sized by the head count of the configuration)
 *   ffn       any multiple of 384, no upper limit                   else MX_EUNSUPPORTED
 *   vocab, type_vocab >= 1; 1 <= max_pos <= 8192; 0 <= pos_offset < max_pos; ln_eps >= 0; pooling and precision one of
 *   their enumerators                                               else MX_EINVAL
 * Every accepted shape computes the same function; the ffn width decides which kernels do (MX_PREC_BF16 only):
 *   hidden 384, ffn <= 1536 (384, 768, 1152, 1536)   the layer tail as ONE kernel (out-projection, Add&Norm, MLP, Add&Norm) and,
 *                                                    in passes of <= 2048 packed rows, the small-pass kernels (query latency)
 *   hidden 384, ffn > 1536                           neither: GEMM by GEMM at every pass size
 *   hidden 768                                       GEMM by GEMM; passes of <= 4096 packed rows split the two Add&Norm GEMMs
 *                                                    over k, W2 into min(8, ffn / 384) chunks where those are whole k-tiles of 32
 *   passes of >= 32768 packed rows                   the 256 x 256-tile GEMM where N is a multiple of 256 (f32 outputs of the
 *                                                    split-operand modes: also a last half tile), the 64-row GEMM otherwise
 */
/* Replaces SentenceEmbeddingsBuilder::remote(..).create_model() (embedding.rs:99-100). */
int mx_encoder_create(const mx_encoder_cfg *cfg, const void *weights, size_t nbytes, int device,
                      mx_encoder **out);
void mx_encoder_destroy(mx_encoder *enc); /* drops one reference; frees HBM when the last one goes */
/*
 * Keyed, ref-counted form: the reference spawns an embedder -- loads the
 * checkpoint -- for every HTTP search and every ingest task (collections/handlers.rs:61-63,
 * worker/tasks.rs:17).  The first mx_encoder_open(key, ...) uploads the weights; later opens of the
 * same key return the SAME resident encoder in O(1) (weights may then be NULL).  Calls on a shared
 * handle are serialised inside.  key NULL / "" = mx_encoder_create.
 */
int mx_encoder_open(const char *key, const mx_encoder_cfg *cfg, const void *weights, size_t nbytes, int device,
                    mx_encoder **out);
/* Stream contract as for the index (mx_index_wait_stream): order the next *_device call after the
 * work enqueued so far on `hip_stream`. */
int mx_encoder_wait_stream(mx_encoder *enc, void *hip_stream);

/*
 * Replaces model.encode(&segments) (embedding.rs:109) after tokenisation: ids [B, S] row-major
 * ([CLS] .. [SEP] already added, padded with anything past lens[b]); lens[b] in [1, S];
 * out [B, hidden] f32 (pooled, L2-normalised when cfg.normalize).  bf16 MFMA arithmetic with f32
 * accumulation; agrees with the f32 CPU path to |delta cosine| <= 1e-3 (north_star tolerance).
 * A row's embedding does not depend on its neighbours in a call, but it does depend, in its last bits, on
 * how many packed rows share its pass (calls are cut into passes of <= 1024 sequences / 131072 rows): three
 * kernel sets round at the same points and sum in f32 in different orders -- hidden 384: passes of <= 2048
 * rows (query-time and small documents: encoder_small.hip) / larger ones; hidden 768: passes of <= 4096 rows (the two Add & LayerNorm
 * GEMMs split over k) / below / from 32768 rows (the latter round the pre-LayerNorm sum to bf16 once more).  The same text embedded alone and inside a bulk ingest call
 * agrees to 1 - cos ~ 1e-7 .. 1e-5 (tests/test_encoder_gpu.py::test_a_row_across_the_pass_size_regimes),
 * not bit for bit; calls of the same shape are bit-reproducible.  MX_PREC_BF16X3 uses one kernel set.
 * (The attention of a head-dim-32 model comes in three forms chosen per pass from its longest sequence and its size -- one
 * head per work item, two, or a kernel of its own for short sequences: the same arithmetic per head and the same bits, except
 * that in the two-head form a head whose exp2 row sums leave the fast path's range -- logits of several hundred -- takes
 * its pair partner through the running-maximum loop with it.)
 */
int mx_encoder_encode(mx_encoder *enc, const int32_t *ids, const int32_t *lens, int B, int S, float *out);
int mx_encoder_encode_device(mx_encoder *enc, const int32_t *d_ids, const int32_t *d_lens, int B, int S,
                             float *d_out);

typedef struct mx_encoder_stats {
    uint64_t calls;
    uint64_t sequences;
    uint64_t tokens;   /* non-padding tokens processed */
    double flops;      /* algorithmic flops: tokens * L * (8H^2 + 4HF) + attention 4*S_b*H per token */
    double gpu_ms;     /* HIP-event time (profiling on) */
} mx_encoder_stats;
int mx_encoder_set_profiling(mx_encoder *enc, int on);
int mx_encoder_get_stats(mx_encoder *enc, mx_encoder_stats *out);
int mx_encoder_reset_stats(mx_encoder *enc);
int mx_encoder_get_cfg(mx_encoder *enc, mx_encoder_cfg *out); /* precision = the mode the handle runs */

/*
 * Calibrated open: which precision mode holds the score bar is a property of the loaded WEIGHTS, not of the model's shape
 * (profiles/r6_precision_modes_over_seeds.txt: bf16 misses north_star's 1e-3 on several draws of the MiniLM-L6 shape where
 * MX_PREC_MIXED1 reads <= 2.6e-4; on the CLS-pooled bge-base shape only MX_PREC_BF16X3 holds on every draw).  So measure at
 * load time, on the weights that were loaded, and open the cheapest mode that holds.
 *
 * The rule.  The f32 blob is uploaded ONCE; every mode's weight images are built from it in HBM (bit for bit what
 * mx_encoder_create's host routines lay out; only the fused tail's fragment stream is still laid out on the host).  The
 * MX_PREC_BF16X3 encoder is built as the reference and encodes a probe batch.  Then the candidates in order of cost --
 * MX_PREC_BF16, MX_PREC_MIXED1, MX_PREC_MIXED -- are built, encode the same probe, and are compared with the reference on
 * the device, in f64:  pair_dev = max_{i<j} |cos_mode(i, j) - cos_bf16x3(i, j)|,  row_dev = max_i 1 - cos(e_mode_i, e_bf16x3_i).
 * The first candidate with pair_dev <= bar is chosen, MX_PREC_BF16X3 if none is.  cfg->precision on entry is ignored.
 * Without MX_CALIBRATE_ALL the measurement stops at the chosen mode.  A reference that gives non-finite (or zero) embeddings
 * on the probe is an error (MX_EINVAL, text in mx_last_error), not a choice.
 *
 * The bar.  MX_CALIBRATE_BAR = 4e-4 = north_star's 1e-3 minus the 6.0e-4 that MX_PREC_BF16X3 itself is from the f64 oracle at
 * worst (seed 4, profiles/r6_precision_modes_over_seeds.txt section 2).  bar must be finite and > 0, else MX_EINVAL.
 *
 * The probe.  ids NULL = mx_encoder_default_probe: 16 sequences, lengths spread evenly over [n/2, n], n = min(200, max_pos -
 * pos_offset), ids from a counter hash (splitmix64) modulo vocab -- about 2400 packed rows at n = 200, so a hidden-384
 * MX_PREC_BF16 candidate is measured on its bulk kernels (above the 2048-row small pass) and a hidden-768 one in its <= 4096-row
 * form (the pass-size regimes round at the same points, see mx_encoder_encode).  A caller who wants the >= 32768-row regime
 * measured passes a probe of 64 x 512.  A caller's probe needs 2 <= B <= 64, 1 <= S <= min(512, max_pos - pos_offset) and
 * lens[b] in [1, S], else MX_EINVAL.
 */
typedef struct mx_encoder_calibration {
    int32_t chosen;          /* MX_PREC_* */
    int32_t tried;           /* bit (1 << MX_PREC_*) per mode that was run */
    int32_t probe_seqs, probe_tokens;
    double  bar;
    double  pair_dev[4];     /* by MX_PREC_*: max |cos_mode(i,j) - cos_bf16x3(i,j)|; 0 for BF16X3; NaN where not tried */
    double  row_dev[4];      /* by MX_PREC_*: max 1 - cos(e_mode_i, e_bf16x3_i) */
    double  ms;              /* wall time of the calibration */
} mx_encoder_calibration;
size_t mx_encoder_calibration_size(void);                 /* same handshake as mx_encoder_cfg_size */
#define MX_CALIBRATE_BAR 4e-4
enum { MX_CALIBRATE_ALL = 1 };                            /* measure every mode even after one has passed */

/* host only.  ids [16 x S] and lens [16] may both be NULL (B and S only); S <= 200. */
int mx_encoder_default_probe(const mx_encoder_cfg *cfg, int32_t *ids, int32_t *lens, int *B, int *S);
/* the report alone: nothing stays resident */
int mx_encoder_calibrate(const mx_encoder_cfg *cfg, const void *weights, size_t nbytes, int device,
                         const int32_t *ids, const int32_t *lens, int B, int S,   /* NULL ids = the default probe */
                         double bar, int flags, mx_encoder_calibration *out);
/*
 * Calibrates and returns the encoder that was chosen -- the one that was measured, not a rebuilt one; the f32 blob in HBM,
 * the other encoders and the probe buffers are released before return, and the handle's mx_encoder_stats start at zero.
 * report may be NULL.  Keyed form: the first open of `key` calibrates and registers the handle with its report; later opens
 * return the same handle and the stored report in O(1) when every field of cfg except `precision` matches (a resident handle
 * that mx_encoder_open created reports its precision as chosen and tried = 0).  mx_encoder_open(key, cfg ...) on a calibrated
 * resident handle keeps its strict comparison: a caller who names a precision gets that precision or MX_EINVAL.
 */
int mx_encoder_open_calibrated(const char *key, const mx_encoder_cfg *cfg, const void *weights, size_t nbytes, int device,
                               const int32_t *ids, const int32_t *lens, int B, int S, double bar, int flags,
                               mx_encoder **out, mx_encoder_calibration *report);

/* For tests.  The K-blocked image [k'/32][rows][32] of a Linear weight w [rows, k] (k a multiple of 32) in one of the four
 * forms.  form: MX_PREC_*; via_device = 0 host routine, 1 the kernel.  out: rows * k * {1, 3, 2, 1} uint16, sized by the form. */
int mx_encoder_weight_image(const float *w, int rows, int k, int form, int via_device, int device, uint16_t *out);
/* For tests.  d_a, d_b: [B, H] f32 on the current device, complete (the caller's streams synchronised); 2 <= B <= 64, H 384 /
 * 768.  pair / row as in mx_encoder_calibration; both +inf on a non-finite value or a zero row. */
int mx_embeddings_deviation_device(const float *d_a, const float *d_b, int B, int H, double *pair, double *row);

/* =====================================================================================
 * WordPiece / byte-level BPE tokenizer + sliding-window segmenter (host code; replaces the `tokenizers` crate
 * calls of segment_text, lib/libmemex/src/llm/embedding.rs:155-198, and the tokenisation rust-bert
 * performs inside model.encode, embedding.rs:109)
 * ===================================================================================== */
typedef struct mx_tokenizer mx_tokenizer;

/* vocab: BERT vocab.txt (one token per line; needs [PAD] [UNK] [CLS] [SEP]).  lowercase = 1 for
 * the uncased MiniLM / bge models.  Replaces Tokenizer::from_pretrained (embedding.rs:163). */
int mx_tokenizer_create(const char *vocab_path, int lowercase, mx_tokenizer **out);
int mx_tokenizer_create_from_memory(const char *vocab, size_t nbytes, int lowercase, mx_tokenizer **out);
/* Byte-level BPE: the tokenizer of all-distilroberta-v1, the third model segment_text accepts (embedding.rs:159): GPT-2
 * pre-tokenizer regex, bytes -> printable code points, BPE over vocab.json + merges.txt (needs <s> </s> <pad>), <s> .. </s>
 * as the special tokens, ByteLevel decoder.  Every call below works on either kind of handle. */
int mx_tokenizer_create_bpe(const char *vocab_json_path, const char *merges_path, mx_tokenizer **out);
int mx_tokenizer_create_bpe_from_memory(const char *vocab_json, size_t n_vocab, const char *merges, size_t n_merges,
                                        mx_tokenizer **out);
/* tokenizer.json -- the file Tokenizer::from_pretrained itself reads (embedding.rs:163): model.vocab (+ model.merges) and the
 * normalizer's lowercase flag select one of the two kinds above.  The stacks of the reference's three models are accepted
 * (BertNormalizer / BertPreTokenizer / WordPiece "##" / WordPiece decoder; ByteLevel / BPE / ByteLevel decoder); any other
 * component -> MX_EUNSUPPORTED.  The file's truncation / padding blocks are ignored (segment_text overrides the first,
 * embedding.rs:172-176, and decodes with skip_special_tokens, :182,189). */
int mx_tokenizer_create_from_json(const char *tokenizer_json_path, mx_tokenizer **out);
int mx_tokenizer_create_from_json_memory(const char *json, size_t nbytes, mx_tokenizer **out);
void mx_tokenizer_destroy(mx_tokenizer *tok);
int mx_tokenizer_vocab_size(mx_tokenizer *tok, int *n);

/* tokenizer.encode(text, add_special_tokens) (embedding.rs:181).  *n = number of ids produced
 * (may exceed cap: only the first cap are written). */
int mx_tokenizer_encode(mx_tokenizer *tok, const char *text, int add_special_tokens, int32_t *ids, int cap, int *n);
/* tokenizer.decode(ids, skip_special_tokens) (embedding.rs:182,189); *nbytes includes the NUL. */
int mx_tokenizer_decode(mx_tokenizer *tok, const int32_t *ids, int n, int skip_special_tokens, char *out, size_t cap,
                        size_t *nbytes);
/* segment_text (embedding.rs:155-198): windows of max_length tokens starting every
 * max_length - stride tokens, each decoded back to text (first window also gets " ' " -> "'").
 * out receives the segments as consecutive NUL-terminated strings; *nbytes = total bytes. */
int mx_tokenizer_segment(mx_tokenizer *tok, const char *text, int max_length, int stride, char *out, size_t cap,
                         size_t *nbytes, int *n_segments);
/* segment_text for a batch of documents (what the ingest worker's queue holds: tasks.rs:17-19, up to five tasks at a time,
 * worker/lib.rs:36): the documents are dealt to host threads.  out: the windows of text 0, then of text 1, ..., each
 * NUL-terminated; n_segments[i] = windows of text i.  *nbytes is always the size needed; out is filled only when cap covers
 * it (call again with a larger buffer otherwise). */
int mx_tokenizer_segment_batch(mx_tokenizer *tok, const char *const *texts, int n_texts, int max_length, int stride,
                               char *out, size_t cap, size_t *nbytes, int32_t *n_segments);
/* Test hook: the WordPiece encoder stage by stage (normalize -> pre-tokenize -> WordPiece, as embedding.rs:181's encode is
 * usually described) -- mx_tokenizer_encode runs the same steps in one pass; tests hold the two against each other. */
int mx_tokenizer_encode_staged(mx_tokenizer *tok, const char *text, int32_t *ids, int cap, int *n);
/* Batch for mx_encoder_encode: [CLS] .. [SEP], truncated to max_seq_length, padded with [PAD] to
 * row pitch s_cap; lens[b] = tokens incl. specials; *S = longest row (<= s_cap or MX_EINVAL). */
int mx_tokenizer_encode_batch(mx_tokenizer *tok, const char *const *texts, int B, int max_seq_length, int32_t *ids,
                              int s_cap, int32_t *lens, int *S);

#ifdef __cplusplus
}
#endif
#endif /* MEMEX_HIP_H */
