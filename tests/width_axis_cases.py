"""The width axis of the index (tests/WIDTH_AXIS.md) -- TEST INFRASTRUCTURE, not product code: the lattice of row widths either side
of every point where the code that serves a row changes, the route each width is expected to take for each kind of filter copy, and
one builder of small corpora that can still go wrong.  tests/test_width_axis_model.py checks this file on the CPU (every switch has a
width on each side, the route table is total, the edge rows really are among the answers compared); tests/test_width_axis_gpu.py runs
the lattice on the GPU.

The switch points are copies of constants of memex_amd/csrc; each stands beside the constant it comes from.  The GPU test reads the
padded width back from mx_index_stats (filter_copy_bytes, scan_bytes), so a constant that changes there without changing here fails
loudly instead of silently un-testing a regime."""
import functools

import numpy as np

# ---- the constants the switches come from ---------------------------------------------------------------------------------------------
CHUNK = 128             # index_kernels.h  kChunkFloats = 128: rows are padded to whole 128-dim slots ...
MAX_KC = 6              # index_kernels.h  kMaxKC = 6: ... up to 6 slots (768 dims); above, to whole pairs of slots (index.hip, mx_index_open:
                        #                  idx->ds = round_up(dim, dim > kMaxKC * kChunkFloats ? 2 * kChunkFloats : kChunkFloats))
MAX_KC8X2 = 4           # index_kernels.h  kMaxKC8x2 = 4: the int8 scan's pair and 512-query geometries (plan_batch: two_groups)
AUTO_I8_MAX_DIM = 1024  # index.hip        kAutoI8MaxDim = 1024: the automatic copy is int8 up to here, bf16 above
RING_4_MAX_DIM = 1280   # scan8.hip        the int8 scan's register ring: R = 8 up to 1024, 4 up to 1280, 2 up to 1536 padded dims
MAX_KC16 = 12           # index_kernels.h  kMaxKC16 = 12: the last width with a filter copy, a subset / range finish kernel, a compressed corpus
MMR_MAX_DS = 8192       # index_kernels.h  kMmrMaxDs = 8192: mmr_select_kernel / score_ids_kernel stage a padded row in 32 KiB of LDS
PREP_CHUNK = 4096       # prep_wide.hip    kPrepChunk = 4096: the floats of a query one LDS chunk holds above MAX_KC16 slots
PREP_LDS_DIMS = 16384   # the widest query prep_queries_kernel stages whole: 4 * dim bytes of dynamic LDS, and a launch gets 64 KiB without
                        # hipFuncSetAttribute.  Before prep_wide.hip, wider rows (65535, 65536: 256 KiB) could not be searched at all
MAX_DIM = 1 << 16       # index.hip        mx_index_open: dim < 1 || dim > (1 << 16) -> MX_EINVAL
TILE_ROWS = 32          # index_kernels.h  kTileRows = 32 (bf16 / f32 scan tile); kTile8Rows = 64 (int8 scan tile)
TILE8_ROWS = 64
WIDE_BATCH = 128        # index_kernels.h  kWideBatch = 128: queries per pass of scan16w_kernel (768 < padded dim <= 1536, bf16 copy)
EXACT_GROUP = 32        # index_kernels.h  kExactGroup = 32: queries per group of the EXACT path
FIRST_CAPACITY = 1024   # index.hip        ensure_capacity: the row capacity of an index that holds its first 1 .. 1024 rows

# (the last width on the near side of a switch, what switches there): the width itself and the next one must both be in the lattice
SWITCHES = (
    (0, "mx_index_open refuses dim < 1"),
    (3, "byid_gather_kernel / like_combine_kernel / compact_gather_kernel: element stores for dim & 3 != 0 ..."),
    (4, "... 16-byte stores for dim & 3 == 0, and back"),
    (CHUNK - 1, "a row shorter than its one slot"),
    (CHUNK, "one slot exactly; the next width takes a second one"),
    (MAX_KC8X2 * CHUNK, "int8 scan: pair and 512-query geometries up to 4 slots"),
    (MAX_KC * CHUNK, "scan_kernel / scan16_kernel / centred forms up to 6 slots; above: 256-rounding, scan16w_kernel, no f32 scan"),
    (AUTO_I8_MAX_DIM, "automatic copy int8 up to here, bf16 above; int8 ring R = 8 up to here"),
    (RING_4_MAX_DIM, "int8 ring R = 4 up to here, R = 2 above"),
    (MAX_KC16 * CHUNK, "the last width with a filter copy; above: EXACT path for every form, no compressed corpus"),
    (MAX_KC16 * CHUNK + 2 * CHUNK, "1792: the first padded width without a scan, filled exactly; the next width pads to 2048"),
    (MMR_MAX_DS, "MMR and score_ids up to here; two whole chunks of the wide query preparation, then a third of one float"),
    (MAX_DIM, "mx_index_open refuses dim > 65536"),
)

LATTICE = (1, 3, 4, 5, 127, 128, 129, 512, 513, 640, 768, 769, 1024, 1025, 1280, 1281, 1536, 1537, 1792, 1793, 2048, 3072, 4096,
           8191, 8192, 8193, 16384, 65535, 65536)
REFUSED = (0, -1, 65537)
REDUCED = (3, 130, 513, 769, 1025, 1281, 1536, 1537, 2048, 4096, 8192, 8193, 65536)    # every row-touching form
MOVERS = (769, 1536, 1537, 4096, 65536)                                                # get_rows, add_device, compact, save / load, shards
COMPRESSED = (769, 1281, 1536)
LISTS_ONLY = (1537, 4096)                                                              # fused, grouped, group_rows, capped, boosted
KINDS = ("auto", "i8", "bf16", "none", "compressed")
KS = (10, 300)


# a layout of tests/random_walk.py that has no scan (1792 padded dims, the automatic copy: none).  It is not one of random_walk.CASES:
# tests/test_random_walk_model.py asserts every event and every defect for those.  The seed: the clean model walks it against itself
# and meets every event of random_walk.EVENTS -- growth of the row storage under live handles, every form after a compaction, handles
# made stale by a load -- within the 40 steps (tests/test_width_axis_model.py).
WALK = dict(name="wide-d1540", seed=1540, d=1540, copy=None, cone=False, compressed=False, devices=None, block_rows=0)


def ds_of(dim):
    """the padded width of a row (mx_index_open)"""
    step = 2 * CHUNK if dim > MAX_KC * CHUNK else CHUNK
    return (dim + step - 1) // step * step


def batch_sizes(dim):
    """129 splits the 128-query wide pass and takes the pair geometry up to 512 dims; 40 is one full EXACT group and a partial one"""
    return (1, 33, 129) if ds_of(dim) <= MAX_KC16 * CHUNK else (1, 40)


def n_rows(dim):
    """700: ten 64-row tiles and a partial one, and more than the 256 rows several copy decisions wait for; 300 above 8192 dims"""
    return 700 if dim <= MMR_MAX_DS else 300


def route(dim, kind):
    """What mx_index_stats must show for an index of this width that was asked for this kind of copy and holds n_rows(dim) rows.
    -> None when the width does not admit the kind at all (a compressed corpus above 1536 padded dims: MX_EUNSUPPORTED), else a dict:
      filter_kind         0 none, 2 int8, 3 bf16 (mx_index_get_stats)
      elem_bytes          of the copy; filter_copy_bytes == FIRST_CAPACITY * ds * elem_bytes
      scan                a search with k <= 256 in the AUTO mode launches a scan (scan_launches > 0); else the EXACT path answers
      scan_elem_bytes     of what the scan streams (scan_bytes == passes * 704 * ds * scan_elem_bytes: 704 = 700 rows in whole tiles)
      wide                the scan takes 128 queries per pass (scan16w_kernel)
      subset              a small filter is answered by subset_topk_kernel (subset_queries counts it)
    and, for every kind and width, what a plain search must leave at 0: FALLBACK_QUERIES (no query of these corpora overflows a scan
    into the EXACT path: a scan that wrote useless bounds would still answer bit-exactly, through that path) and FILTER_DEMOTIONS
    (no batch makes the automatic int8 copy give way to bf16: that would be another route than the one named here)."""
    if kind not in KINDS:
        raise KeyError(kind)
    ds = ds_of(dim)
    if ds > MAX_KC16 * CHUNK:
        if kind == "compressed":
            return None
        return dict(filter_kind=0, elem_bytes=0, scan=False, scan_elem_bytes=0, wide=False, subset=False)
    if kind == "none":
        f32_scan = ds <= MAX_KC * CHUNK
        return dict(filter_kind=0, elem_bytes=0, scan=f32_scan, scan_elem_bytes=4 if f32_scan else 0, wide=False, subset=True)
    i8 = kind == "i8" or (kind == "auto" and ds <= AUTO_I8_MAX_DIM)
    return dict(filter_kind=2 if i8 else 3, elem_bytes=1 if i8 else 2, scan=True, scan_elem_bytes=1 if i8 else 2,
                wide=not i8 and ds > MAX_KC * CHUNK, subset=True)


FALLBACK_QUERIES = 0
FILTER_DEMOTIONS = 0


def passes(dim, kind, B):
    """scan launches counted for one search of B <= 256 queries on the scan route (the wide pass splits a batch at 128)"""
    return -(-B // WIDE_BATCH) if route(dim, kind)["wide"] else 1


# ---- the corpus ---------------------------------------------------------------------------------------------------------------------
ZERO_ROW = 5                     # a zero row: dist 0 to every query, so it heads every list
TINY_ROW, HUGE_ROW = 40, 41      # norms 1e-22 and 1e18: outside what the f32 stages are certified for (ingest_kernel lists them)
ENDS_ROW = 60                    # non-zero in its first and its last element only: a chain that stops a chunk early, or a padding
                                 # column that leaks, changes its bits
DUP_FIRST, DUP_COUNT = 100, 26   # a run of exact duplicates: 26 equal keys, ordered by row
REMOVED_ROW = 250                # the row the form tests remove before they search
Q_DOUBLE, Q_ZERO, Q_LAST, Q_RANGE = 0, 1, 2, 3     # 2 x a stored row (the duplicated one); zero; non-zero in the last element only;
                                                   # the query the range thresholds are made for (B >= 33)


@functools.lru_cache(maxsize=2)
def corpus(dim):
    """-> (X f32 [n_rows(dim), dim], Q f32 [129, dim]); the arrays are shared: leave them unchanged"""
    rng = np.random.default_rng(7000 + dim)
    n = n_rows(dim)
    X = rng.standard_normal((n, dim), dtype=np.float32)
    X *= rng.uniform(0.1, 10.0, (n, 1)).astype(np.float32)
    X[ZERO_ROW] = 0
    for row, norm in ((TINY_ROW, 1e-22), (HUGE_ROW, 1e18)):
        v = X[row].astype(np.float64)
        X[row] = (v * (norm / np.linalg.norm(v))).astype(np.float32)
    X[ENDS_ROW] = 0
    X[ENDS_ROW, 0] = 0.25
    X[ENDS_ROW, dim - 1] += 3.0                                          # (dim 1: the one element is both)
    X[DUP_FIRST:DUP_FIRST + DUP_COUNT] = X[DUP_FIRST]
    Q = rng.standard_normal((129, dim), dtype=np.float32)
    Q[Q_DOUBLE] = 2.0 * X[DUP_FIRST]
    Q[Q_ZERO] = 0
    Q[Q_LAST] = 0
    Q[Q_LAST, dim - 1] = 1.5
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


@functools.lru_cache(maxsize=2)
def tame_corpus(dim):
    """corpus(dim) with ordinary rows in place of the two whose norms are out of range.  A compressed corpus that holds such a row
    answers every search on the EXACT path (plan_batch); this one lets the scan over the compressed rows run.  -> X, shared"""
    X = corpus(dim)[0].copy()
    rng = np.random.default_rng(9000 + dim)
    X[[TINY_ROW, HUGE_ROW]] = rng.standard_normal((2, dim), dtype=np.float32) * np.float32(1.7)
    X.setflags(write=False)
    return X


def queries(dim, B):
    """the first B queries; a single query is the one that doubles a stored row"""
    return corpus(dim)[1][:B]


def form_queries(dim):
    """the four named queries and one more: what the form tests search with"""
    return corpus(dim)[1][:5]


def range_thresholds(oracle, dim, alive=None):
    """-> (t5, t_all) for query Q_RANGE: min_score values that admit exactly 5 live rows and every live row.  The scores come from the
    oracle's distances; t5 is the 5th best score itself (the 6th must differ: asserted), t_all is -1, the least score there is"""
    X, Q = corpus(dim)
    d = oracle.all_dists(X, Q[Q_RANGE])
    if alive is not None:
        d = d[alive]
    from oracle.search_oracle import score_from_dist
    s = np.sort(score_from_dist(d.astype(np.float32)))[::-1]
    assert s[4] > s[5], "the 5th and 6th best rows tie: the threshold cannot admit exactly 5"
    return np.float32(s[4]), np.float32(-1.0)
