"""Integer records of the int8 scans (scan8.hip, scan_common.h): a collect launch of scan8_kernel stores a passing lane's 16
integer sums as they are (INT_MIN for a removed row), and the two readers -- finish_kernel and range_finish_kernel -- rebuild each
score as ((float)sum * s_h) * s_q from the tile's step and the query's step, the two roundings the scan itself applied to the
maximum it tested.  Bar for every case: the AUTO path's ids, scores, dists and n_found (and a range search's lists and counts) are
bit for bit those of MX_SEARCH_EXACT on the same index, and the batch was answered by the scan pipeline (no query fell back).
One case per form of the kernel and per reader: pair form, 8-wave form with idle waves, two query groups, six slots, removed rows,
the centred copy (the accumulators start from a_q a_c), range search, and lanes that overflow into the retry pass."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

_cache = {}


def _corpus(d):
    """65 536 seeded Gaussian rows of d dims and 300 queries, the first 32 of them near neighbours of rows; built once per module"""
    if d not in _cache:
        rng = np.random.default_rng(1000 + d)
        X = rng.standard_normal((65536, d), dtype=np.float32)
        Q = rng.standard_normal((300, d), dtype=np.float32)
        Q[:32] = X[rng.integers(0, len(X), 32)] + 0.05 * rng.standard_normal((32, d), dtype=np.float32)
        X.setflags(write=False)
        Q.setflags(write=False)
        _cache[d] = (X, Q)
    return _cache[d]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x.dtype == np.float32:
            np.testing.assert_array_equal(bits(x), bits(y))
        else:
            np.testing.assert_array_equal(x, y)


def _auto_and_exact(idx, call):
    """call(idx) on the AUTO path (which must answer every query itself) and on the EXACT path -> (auto, exact, AUTO's stats)"""
    from memex_amd.index import SEARCH_AUTO, SEARCH_EXACT
    idx.reset_stats()
    auto = call(idx)
    st = idx.stats()
    assert st.scan_launches > 0 and st.fallback_queries == 0, (st.scan_launches, st.fallback_queries)
    idx.set_search_mode(SEARCH_EXACT)
    try:
        exact = call(idx)
    finally:
        idx.set_search_mode(SEARCH_AUTO)
    return auto, exact, st


def _i8_index(X, d):
    from memex_amd.index import FlatIndex
    idx = FlatIndex(d)
    idx.add(X)
    idx.set_filter_copy("i8")
    st = idx.stats()
    assert st.filter_kind == 2 and st.filter_centred == 0
    return idx


def test_every_lane_records_every_tile(lib_built):
    """4070 rows: at most two tiles per workgroup, so there is no sample, theta is -inf and every lane of the pair form records
    every tile -- the most records read per row.  40 scattered zero rows, one all-zero half tile (step 0), a cut last tile."""
    rng = np.random.default_rng(1)
    n, d = 4070, 384
    X = rng.standard_normal((n, d), dtype=np.float32)
    X[rng.choice(n, 40, replace=False)] = 0.0
    X[32 * 51: 32 * 52] = 0.0
    Q = rng.standard_normal((200, d), dtype=np.float32)
    Q[:16] = X[1000:1016] + 0.05 * rng.standard_normal((16, d), dtype=np.float32)
    with _i8_index(X, d) as idx:
        auto, exact, st = _auto_and_exact(idx, lambda i: i.search(Q, 10))
        assert st.retry_queries == 0
        _same(auto, exact)


@pytest.mark.parametrize("d,B", [(384, 200), (384, 40), (128, 300)])   # pair form | 8-wave form, idle waves | two-group 512 pass
def test_sample_theta_and_collect(d, B, lib_built):
    X, Q = _corpus(d)
    with _i8_index(X, d) as idx:
        auto, exact, _ = _auto_and_exact(idx, lambda i: i.search(Q[:B], 10))
        _same(auto, exact)


def test_six_slots(lib_built):
    """768 dims: KC = 6, the plain family's 8-wave kernel"""
    X, Q = _corpus(768)
    with _i8_index(X, 768) as idx:
        auto, exact, _ = _auto_and_exact(idx, lambda i: i.search(Q[:64], 10))
        _same(auto, exact)


def test_removed_rows(lib_built):
    """1000 scattered rows and one whole 64-row tile removed: the DEAD instances, INT_MIN in the records"""
    X, Q = _corpus(384)
    rng = np.random.default_rng(4)
    gone = np.unique(np.concatenate([rng.choice(len(X), 1000, replace=False), np.arange(64 * 333, 64 * 334)]))
    Qn = Q[:200].copy()
    Qn[40:48] = X[gone[:8]]                        # queries that are removed rows: their best row must not come back
    Qn[48:52] = X[64 * 333 + 5: 64 * 333 + 9]
    with _i8_index(X, 384) as idx:
        assert idx.remove(gone + 1) == len(gone)   # ids are 1-based
        auto, exact, _ = _auto_and_exact(idx, lambda i: i.search(Qn, 10))
        _same(auto, exact)
        assert not np.isin(auto[0], gone + 1).any()


def test_centred_copy(lib_built):
    """a cone corpus on a centred int8 copy: the stored sums include the accumulators' initial value a_q a_c / (s_h s_q)"""
    from memex_amd.index import FlatIndex
    from test_centred_gpu import cone_rows
    rng = np.random.default_rng(5)
    n, d = 65536, 384
    X = cone_rows(rng, n, d)
    Q = cone_rows(rng, 64, d)
    Q[0] = X[99]
    Q[1] = rng.standard_normal(d).astype(np.float32)   # a query off the cone
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.set_filter_copy("bf16")
        idx.set_filter_copy("i8")                       # rebuilt from the resident rows: centred
        st = idx.stats()
        assert st.filter_centred == 1 and st.filter_kind == 2
        auto, exact, _ = _auto_and_exact(idx, lambda i: i.search(Q, 10))
        _same(auto, exact)
        assert idx.stats().filter_centred == 1 and idx.stats().filter_kind == 2


def test_range_search_reader(lib_built):
    """range_finish_kernel's reader: cosines of Gaussian rows at 384 dims have sigma 0.051, so 0.165 keeps a few dozen of 65 536"""
    X, Q = _corpus(384)
    with _i8_index(X, 384) as idx:
        auto, exact, _ = _auto_and_exact(idx, lambda i: i.search_range(Q[:200], 0.165, 256))
        _same(auto, exact)
        nr = auto[4][32:]                               # (the first 32 queries also have their near neighbour)
        assert 10 <= np.median(nr) <= 100 and (auto[3] == np.minimum(auto[4], 256)).all(), (nr.min(), np.median(nr), nr.max())


def test_lanes_over_their_capacity_take_the_retry_pass(lib_built):
    """8-wave form, 128 dims, 32 queries: the 71 tiles of ONE workgroup's stride (tile % 256 == 7; the sample visits multiples of
    its stride, never an odd tile) hold rows close to query 3, two records per lane and tile against a capacity of 64: the overflow
    bit, the retry pass with its tight threshold, and the readers on the second set of records."""
    from test_search_gpu import _rows_with_cosine
    rng = np.random.default_rng(7)
    n, d = 1_150_000, 128
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((32, d), dtype=np.float32)
    tiles = np.arange(7, n // 64, 256)
    assert len(tiles) >= 70
    rows = (64 * tiles[:, None] + np.arange(64)[None, :]).ravel()
    X[rows] = _rows_with_cosine(rng, Q[3], np.linspace(0.99, 0.79, len(rows)))
    with _i8_index(X, d) as idx:
        auto, exact, st = _auto_and_exact(idx, lambda i: i.search(Q, 10))
        assert st.retry_queries > 0
        _same(auto, exact)
