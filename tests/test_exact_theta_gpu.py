"""The int8 collect threshold from exact scores of the sample's best rows (launch_theta's ThetaExact).

The sample launch of the plain int8 copy leaves, beside every lane maximum, the row that gave it; theta_kernel rescores the rows of
the max(32, 2k + 12) best lanes in f32 and raises the collect threshold to max(today's, L' - qa), L' = the k-th largest s2 - e2.  The
threshold only decides which rows reach finish_kernel, so the bar is the usual one: ids, dists, scores and n_found bit-equal to the
EXACT path (and to the C oracle), with the switch on, with it off (MEMEX_HIP_EXACT_THETA=0), and with a sample in which every
workgroup visits several tiles (MEMEX_HIP_DEBUG=sample_div=2, read when the index is created).

Shapes: the sample path needs more than 2 x CUs scan tiles of 64 rows, so the corpora hold at least 40k rows on a 256-CU part (more
on a larger one: the CU count is read from the device).  Batches 1 and 33 run the 256-query geometry, 200 the two-workgroup form,
300 the 512-query pass.
"""
import functools

import numpy as np
import pytest

from conftest import bits  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = {"48kx128": (48_011, 128), "40kx384": (40_003, 384)}
VARIANTS = {"default": {}, "sample_div2": {"MEMEX_HIP_DEBUG": "sample_div=2"}, "off": {"MEMEX_HIP_EXACT_THETA": "0"}}


def _same(a, b):
    ids, sc, di, nf = a
    ids2, sc2, di2, nf2 = b
    np.testing.assert_array_equal(ids, ids2)
    np.testing.assert_array_equal(bits(di), bits(di2))
    np.testing.assert_array_equal(bits(sc), bits(sc2))
    np.testing.assert_array_equal(nf, nf2)


@functools.lru_cache(maxsize=None)
def _n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rows_for(n):
    """At least n rows, and enough that the scan has more than 2 x CUs tiles (the sample path), not a multiple of the tile."""
    return max(n, 64 * (2 * min(_n_cu(), 256) + 64) + 37)


@functools.lru_cache(maxsize=None)
def _corpus(shape):
    n, d = SHAPES[shape]
    n = _rows_for(n)
    rng = np.random.default_rng(d)
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((300, d), dtype=np.float32)
    Q[:16] = X[rng.integers(0, n, 16)] + 0.05 * rng.standard_normal((16, d), dtype=np.float32)  # near neighbours
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


def _open(X, env=None, setup=None):
    """An index over X with the plain int8 copy pinned, created under the environment `env` (both switches are read at creation)."""
    from memex_amd.index import FlatIndex
    with pytest.MonkeyPatch.context() as mp:
        for key in ("MEMEX_HIP_DEBUG", "MEMEX_HIP_EXACT_THETA"):
            mp.delenv(key, raising=False)
        for key, v in (env or {}).items():
            mp.setenv(key, v)
        idx = FlatIndex(X.shape[1])
    idx.add(X)
    idx.set_filter_copy("i8")
    if setup:
        setup(idx)
    return idx


_indexes = {}


@pytest.fixture(scope="module")
def indexes(lib_built):
    """(shape, variant) -> index, opened on first use and closed with the module"""
    def get(shape, variant):
        if (shape, variant) not in _indexes:
            _indexes[(shape, variant)] = _open(_corpus(shape)[0], VARIANTS[variant])
        return _indexes[(shape, variant)]
    yield get
    for idx in _indexes.values():
        idx.close()
    _indexes.clear()


_exact_cache = {}


def _exact(idx, Q, k, key=None, search=None):
    from memex_amd.index import SEARCH_AUTO, SEARCH_EXACT
    if key is not None and key in _exact_cache:
        return _exact_cache[key]
    idx.set_search_mode(SEARCH_EXACT)
    try:
        out = (search or idx.search)(Q, k)
    finally:
        idx.set_search_mode(SEARCH_AUTO)
    if key is not None:
        _exact_cache[key] = out
    return out


def _fast(idx, Q, k, search=None):
    idx.reset_stats()
    out = (search or idx.search)(Q, k)
    return out, idx.stats()


@gpu
@pytest.mark.parametrize("B", [1, 33, 200, 300])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_main_matrix_bit_equal_to_exact(shape, B, indexes):
    """Every geometry of scan8_kernel, k = 1 / 10 / 100, the three variants: the same outputs as the EXACT path, and no retry or
    fallback with the exact threshold where there is none without it."""
    Q = _corpus(shape)[1][:B]
    for k in (1, 10, 100):
        want = _exact(indexes(shape, "default"), Q, k, key=(shape, B, k))
        stats = {}
        for variant in VARIANTS:
            out, st = _fast(indexes(shape, variant), Q, k)
            _same(out, want)
            stats[variant] = (int(st.retry_queries), int(st.fallback_queries))
            print(f"{shape} B={B} k={k} {variant}: retry={stats[variant][0]} fallback={stats[variant][1]} candidates/query="
                  f"{st.candidates / max(1, st.queries):.0f}")
        for variant in ("default", "sample_div2"):
            for j in range(2):
                if stats["off"][j] == 0:
                    assert stats[variant][j] == 0, (variant, k, stats)


@gpu
def test_bit_equal_to_oracle(oracle, indexes):
    X, Q = _corpus("40kx384")
    Q = Q[:200]
    out, st = _fast(indexes("40kx384", "default"), Q, 10)
    assert st.fallback_queries == 0
    oi, od, os_, onf = oracle.search(X, Q, 10)
    _same(out, (oi, os_, od, onf))


def _adversarial(n, d, seed):
    rng = np.random.default_rng(seed)
    n = _rows_for(n)
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((33, d), dtype=np.float32)
    return rng, X, Q


# tiles 0, 2, 4, 6: block 0's first tile is always sampled, the even ones at every stride the sample of these corpora can take;
# one planted row per tile, so every one of them meets other lanes
PLANT_TILES = (0, 2, 4, 6)


@gpu
@pytest.mark.parametrize("B", [33, 200])
def test_copies_of_a_query_in_sampled_tiles(B, lib_built):
    """Rows that ARE the query (cosine 1) sit in sampled tiles: with k <= their number L' is within e2 of 1, the tightest threshold
    there can be, and the answer (ties broken by id) must still be the EXACT path's; with k above it every other row of the top-k
    must still be found."""
    rng, X, Q = _adversarial(40_003, 128, 1)
    Q = np.concatenate([Q] * 7)[:B]
    rows = [64 * t + 5 + t for t in PLANT_TILES]
    for j, r in enumerate(rows):
        X[r] = (0.5 + j) * Q[2]
    idx = _open(X)
    try:
        for k in (3, 4, 5, 10):
            out, st = _fast(idx, Q, k)
            assert st.fallback_queries == 0
            _same(out, _exact(idx, Q, k))
            assert set(out[0][2][: min(k, 4)]) <= {r + 1 for r in rows}
    finally:
        idx.close()


@gpu
def test_fewer_than_k_valid_lanes_keeps_todays_fallback(monkeypatch, lib_built):
    """A row filter that leaves 5 rows in the sampled span (forced onto the masked scan pipeline): fewer than k lanes see a row, L' is
    -inf and today's fallback threshold must survive the max; with k = 3 the five rows may give a threshold of either kind."""
    rng, X, Q = _adversarial(40_003, 128, 2)
    n = X.shape[0]
    allowed = np.array([3, 64 * 2 + 9, 64 * 4 + 40, n - 200, n - 3], dtype=np.uint64) + 1
    idx = _open(X)
    try:
        monkeypatch.setenv("MEMEX_HIP_DEBUG", "filt_subset=0")
        for k in (10, 3):
            search = lambda q, kk: idx.search_filtered(q, kk, ids=allowed)  # noqa: E731
            out, st = _fast(idx, Q, k, search)
            assert st.subset_queries == 0 and st.fallback_queries == 0
            assert (out[3] == min(k, 5)).all()
            _same(out, _exact(idx, Q, k, search=search))
    finally:
        idx.close()


@gpu
def test_removed_rows_that_were_the_lanes_best(lib_built):
    """Near copies of the queries in sampled tiles, then removed: the masked sample must not name them, and nothing may be rescored
    in their place that is not a live row."""
    from test_search_gpu import _rows_with_cosine
    rng, X, Q = _adversarial(40_003, 128, 3)
    planted = []
    for qi in range(8):
        rows = [64 * t + 8 + qi for t in PLANT_TILES] + [64 * (2 * qi + 8) + j for j in range(12)]
        X[rows] = _rows_with_cosine(rng, Q[qi], np.linspace(0.995, 0.9, len(rows)))
        planted += rows
    idx = _open(X)
    try:
        assert idx.remove(np.asarray(planted, dtype=np.uint64) + 1) == len(planted)
        for k in (1, 10):
            out, st = _fast(idx, Q, k)
            assert st.fallback_queries == 0
            _same(out, _exact(idx, Q, k))
            assert not (set(out[0].ravel().tolist()) & {r + 1 for r in planted})
    finally:
        idx.close()


@gpu
def test_zero_norm_rows_among_the_best(lib_built):
    """Rows and queries on opposite sides of a common direction: every cosine is negative, so the zero-norm rows (filter score 0, exact
    dist 0) are the best of their lanes.  They have no norm to rescore with and are left out of L'; they still lead every answer."""
    rng, X, Q = _adversarial(40_003, 128, 4)
    u = np.zeros(128, dtype=np.float32)
    u[0] = 12.0
    X -= u
    Q += u
    zero = list(range(32)) + [64 * 2 + 3 * j for j in range(8)]
    X[zero] = 0.0
    idx = _open(X)
    try:
        for k in (10, 100):
            out, _ = _fast(idx, Q, k)
            _same(out, _exact(idx, Q, k))
            assert set(out[0][0][: min(k, 40)].tolist()) <= {r + 1 for r in zero}
    finally:
        idx.close()


@gpu
def test_k_256(indexes):
    """The largest k of the scan pipeline: C = min(lanes, 524) rows rescored per query."""
    Q = _corpus("48kx128")[1][:33]
    out, st = _fast(indexes("48kx128", "default"), Q, 256)
    assert st.fallback_queries == 0
    _same(out, _exact(indexes("48kx128", "default"), Q, 256))


@gpu
def test_non_finite_query_is_still_an_error(indexes):
    from memex_amd import _lib
    Q = _corpus("48kx128")[1][:33].copy()
    Q[1, 5] = np.nan
    with pytest.raises(_lib.MemexHipError) as ei:
        indexes("48kx128", "default").search(Q, 10)
    assert ei.value.code == _lib.MX_EINVAL
    Q[1, 5] = np.inf
    with pytest.raises(_lib.MemexHipError) as ei:
        indexes("48kx128", "default").search(Q, 10)
    assert ei.value.code == _lib.MX_EINVAL


def test_threshold_rule_restated_in_numpy():
    """The rule of theta_kernel's exact form on random data, no GPU: lanes hold distinct rows, each lane's maximum is the best LOWER
    bound score - (qa + qb e) of its rows, theta_today = (k-th largest lane maximum) - qa; the rows behind the C best lanes get
    s2 with |s2 - cos| <= e2 and L' = the k-th largest s2 - e2.  Then max(theta_today, L' - qa) <= c_k - qa (c_k: the k-th best
    cosine of the whole corpus), and so every row of the top-k passes the collect test score >= theta - qb e."""
    rng = np.random.default_rng(9)
    e2 = 2.5e-5
    for trial in range(200):
        n, lanes = 4096, int(rng.integers(8, 129))
        k = int(rng.integers(1, 41))
        cos = np.clip(rng.normal(0.0, 0.09, n), -1.0, 1.0)
        if trial % 4 == 0:  # a few rows far above the rest, as copies of the query are
            cos[rng.integers(0, n, 2 * k)] = 1.0 - rng.random(2 * k) * 1e-3
        qa, qb = 0.011 + rng.random() * 0.01, 1.0 + rng.random() * 0.02
        e = 0.012 + 0.01 * rng.random(n)                       # residual bound of each row's half tile
        score = cos + (2.0 * rng.random(n) - 1.0) * (qa + qb * e)  # any filter score the certificate allows
        sampled = rng.permutation(n)[: n // 8]
        lane_of = rng.integers(0, lanes, sampled.size)
        lb = score[sampled] - (qa + qb * e[sampled])
        lane_max = np.full(lanes, -np.inf)
        lane_arg = np.full(lanes, -1)
        for lane in range(lanes):
            mine = np.flatnonzero(lane_of == lane)
            if mine.size:
                best = mine[np.argmax(lb[mine])]
                lane_max[lane], lane_arg[lane] = lb[best], sampled[best]
        nv = int((lane_max > -np.inf).sum())
        theta_today = (np.sort(lane_max)[::-1][k - 1] if nv >= k else -8.0) - qa
        C = min(lanes, max(32, 2 * k + 12))
        best_lanes = [lane for lane in np.argsort(-lane_max)[:C] if lane_arg[lane] >= 0]
        s2 = cos[lane_arg[best_lanes]] + (2.0 * rng.random(len(best_lanes)) - 1.0) * e2
        lp = np.sort(s2 - e2)[::-1][k - 1] if len(best_lanes) >= k else -np.inf
        theta = max(theta_today, lp - qa)
        c_k = np.sort(cos)[::-1][k - 1]
        assert theta <= c_k - qa + 1e-12
        top = np.argsort(-cos)[:k]
        assert (score[top] >= theta - qb * e[top] - 1e-12).all()
        assert theta >= theta_today
