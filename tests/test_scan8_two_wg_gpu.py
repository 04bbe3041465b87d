"""The int8 scan's two-workgroup form (scan8_kernel<KC, MODE, 2, false, 4, 8>): batches of 129-256
queries on a plain int8 copy up to 512 dims run on two 4-wave workgroups per CU, 2 x CUs lane sets.  Bar: ids, dists and
scores bit-equal to the EXACT path and to the oracle, and to the one-workgroup-per-CU form (MEMEX_HIP_SCAN8_PAIR=0).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import bits  # noqa: E402


def _same(a, b):
    ids, sc, di, nf = a
    ids2, sc2, di2, nf2 = b
    np.testing.assert_array_equal(ids, ids2)
    np.testing.assert_array_equal(bits(di), bits(di2))
    np.testing.assert_array_equal(bits(sc), bits(sc2))
    np.testing.assert_array_equal(nf, nf2)


def _exact(idx, Q, k):
    from memex_amd.index import SEARCH_AUTO, SEARCH_EXACT
    idx.set_search_mode(SEARCH_EXACT)
    try:
        return idx.search(Q, k)
    finally:
        idx.set_search_mode(SEARCH_AUTO)


def _fast(idx, Q, k):
    idx.reset_stats()
    out = idx.search(Q, k)
    st = idx.stats()
    assert st.fallback_queries == 0
    return out, st


# rows: not a multiple of 64 (the int8 tile) nor of 512 tiles (the grid's tile stride on 256 CUs)
@pytest.mark.parametrize("d,n", [(128, 200_037), (384, 150_001), (512, 70_019)])
def test_256_queries_bit_equal_to_exact(d, n, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(d)
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((256, d), dtype=np.float32)
    Q[:64] = X[rng.integers(0, n, 64)] + 0.05 * rng.standard_normal((64, d), dtype=np.float32)  # near neighbours
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.set_filter_copy("i8")
        out, st = _fast(idx, Q, 10)
        assert st.retry_queries == 0
        _same(out, _exact(idx, Q, 10))


def test_256_queries_bit_equal_to_oracle(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(5)
    n, d = 40_003, 384
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((256, d), dtype=np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.set_filter_copy("i8")
        out, _ = _fast(idx, Q, 10)
    oi, od, os_, onf = oracle.search(X, Q, 10)
    _same(out, (oi, os_, od, onf))


@pytest.mark.parametrize("B", [129, 200])
def test_partial_batches(B, lib_built):
    """129 queries: three of the eight virtual waves are padding (theta = +inf), and they multiply anyway."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(B)
    n, d = 120_011, 384
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((B, d), dtype=np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.set_filter_copy("i8")
        out, _ = _fast(idx, Q, 10)
        _same(out, _exact(idx, Q, 10))


def test_lane_overflow_and_retry_pass(lib_built):
    """Every 64-row tile of ONE workgroup of either form (tile % 512 == 7 is tile % 256 == 7 as well) holds rows close to
    query 3 (cosines 0.99 .. 0.79, distinct), which the sample never visits (it strides over tiles of one parity): that
    query's lanes overflow their 64 records and the batch takes the retry pass -- on the same geometry."""
    from memex_amd.index import FlatIndex
    from test_search_gpu import _rows_with_cosine
    rng = np.random.default_rng(77)
    n, d = 1_400_000, 128
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((200, d), dtype=np.float32)
    tiles = np.arange(7, n // 64, 512)
    rows = (64 * tiles[:, None] + np.arange(64)[None, :]).ravel()
    X[rows] = _rows_with_cosine(rng, Q[3], np.linspace(0.99, 0.79, len(rows)))
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.set_filter_copy("i8")
        out, st = _fast(idx, Q, 10)
        assert st.retry_queries >= 1
        _same(out, _exact(idx, Q, 10))


@pytest.mark.parametrize("B", [200, 256])
def test_forcing_the_old_geometry_gives_the_same_outputs(B, monkeypatch, lib_built):
    """MEMEX_HIP_SCAN8_PAIR=0 (read when an index is created) keeps one 8-wave workgroup per CU."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(11)
    n, d = 250_001, 384
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((B, d), dtype=np.float32)
    outs = []
    for pair in ("1", "0"):
        monkeypatch.setenv("MEMEX_HIP_SCAN8_PAIR", pair)
        with FlatIndex(d) as idx:
            idx.add(X)
            idx.set_filter_copy("i8")
            outs.append(_fast(idx, Q, 10)[0])
    _same(outs[0], outs[1])
