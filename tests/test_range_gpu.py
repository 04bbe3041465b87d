"""Range search (mx_index_search_range): every live row whose score reaches the query's threshold, best first up to a cap, and
the exact count.  The expected answer comes from the oracle's distances: score_from_dist, mask score >= t, order by (dist, id).
Everything is compared with integer equality: ids, dist bits, score bits, n_found, n_in_range.  The first n_found entries must also
equal those of search(k = cap), bit for bit."""
import threading

import numpy as np
import pytest

from conftest import bits
from oracle.search_oracle import score_from_dist
from range_model import oracle_dists, range_oracle  # noqa: F401  (other modules take them from here)
from test_remove_gpu import corpus

pytestmark = pytest.mark.gpu


def same(got, want, what):
    ids, sc, di, nf, nr = got
    oi, os_, od, onf, onr = want
    np.testing.assert_array_equal(nr, onr, err_msg=f"{what}: n_in_range")
    np.testing.assert_array_equal(nf, onf, err_msg=f"{what}: n_found")
    np.testing.assert_array_equal(ids, oi, err_msg=f"{what}: ids")
    np.testing.assert_array_equal(bits(di), bits(od), err_msg=f"{what}: dists")
    np.testing.assert_array_equal(bits(sc), bits(os_), err_msg=f"{what}: scores")


def check(idx, D, alive, Q, t, cap, what, off=0, topk=True):
    got = idx.search_range(Q, t, cap)
    same(got, range_oracle(D, alive, t, cap, off), what)
    if topk:  # the in-range rows are a prefix of the (dist, id) order
        ids, sc, di, nf = idx.search(Q, cap)
        for b in range(Q.shape[0]):
            m = int(got[3][b])
            np.testing.assert_array_equal(got[0][b, :m], ids[b, :m], err_msg=f"{what}: prefix of top-{cap}, query {b}")
            np.testing.assert_array_equal(bits(got[2][b, :m]), bits(di[b, :m]), err_msg=f"{what}: prefix dists, query {b}")
            np.testing.assert_array_equal(bits(got[1][b, :m]), bits(sc[b, :m]), err_msg=f"{what}: prefix scores, query {b}")
    return got


def thresholds(D, alive, rng, cap):
    """Per query: threshold sets that sit exactly on a live row's score (included), one ulp above it (excluded), give counts
    below, equal to and above cap, and lie above every score"""
    S = np.sort(np.where(alive, score_from_dist(D), -np.inf), axis=1)[:, ::-1]
    B = D.shape[0]
    out = []
    for j in (0, 4, cap - 1, cap, 3 * cap):
        j = min(j, int(alive.sum()) - 1)
        t = S[np.arange(B), j].astype(np.float32)
        out.append((f"score of the {j + 1}-th row", t))
        out.append((f"one ulp above the {j + 1}-th row", np.nextafter(t, np.float32(2.0)).astype(np.float32)))
    mixed = S[np.arange(B), rng.integers(0, min(3 * cap, int(alive.sum())), B)].astype(np.float32)
    out.append(("mixed ranks per query", mixed))
    out.append(("above every score", np.full(B, 1.0000001, np.float32)))
    return out


# (name, dim, rows, setup, cone)
_KINDS = [
    ("int8", 384, 40000, lambda idx: idx.set_filter_copy("i8"), False),
    ("centred_int8", 384, 40000, "centre_i8", True),
    ("bf16", 384, 30000, lambda idx: idx.set_filter_copy("bf16"), False),
    ("centred_bf16", 384, 30000, lambda idx: idx.set_filter_copy("bf16"), True),
    ("f32", 384, 20000, lambda idx: idx.set_filter_copy(False), False),
    ("compressed", 384, 30000, lambda idx: idx.set_corpus_mode("bf16"), False),
    ("dim3", 3, 20000, None, False),
    ("dim768", 768, 20000, None, False),
    ("dim1024", 1024, 16000, None, False),
    ("dim1536", 1536, 16000, None, False),
]


@pytest.mark.parametrize("name,d,n,setup,cone", _KINDS, ids=[c[0] for c in _KINDS])
def test_every_copy_kind_matches_oracle(name, d, n, setup, cone, oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    X = corpus(rng, n, d, cone=cone)
    if name == "compressed":
        X[[11, n - 100]] = rng.standard_normal((2, d)).astype(np.float32)  # (wide norms send a compressed corpus to the EXACT path)
    if d == 3:
        X[[11, n - 100]] = rng.standard_normal((2, d)).astype(np.float32)  # (no 1e20 rows at 3 dims: their products overflow f32)
    with FlatIndex(d) as idx:
        if name == "compressed":
            setup(idx)
        idx.add(X)
        if setup == "centre_i8":
            idx.set_filter_copy(False)
            idx.set_filter_copy("i8")                          # rebuilt from a populated cone: centred
            assert idx.stats().filter_centred == 1
        elif setup is not None and name != "compressed":
            setup(idx)
        if name == "centred_bf16":
            assert idx.stats().filter_centred == 1
        rows = idx.get_rows(0, n) if name == "compressed" else X
        alive = np.ones(n, dtype=bool)
        Q = rng.standard_normal((24, d)).astype(np.float32)
        Q[::3] = rows[rng.integers(0, n, 8)] + Q[::3] * 0.02      # queries with close neighbours
        Q[1] = rows[99] * 3.0                                      # a duplicated row
        Q[2] = rows[2000]
        D = oracle_dists(oracle, rows, Q)
        cap = 50
        idx.reset_stats()
        for what, t in thresholds(D, alive, rng, cap):
            check(idx, D, alive, Q, t, cap, f"{name}: {what}")
        if name in ("int8", "centred_int8", "bf16", "f32", "dim1536"):
            assert idx.stats().fallback_queries == 0, name
        # MX_SEARCH_EXACT answers every case alike
        idx.set_search_mode(1)
        for what, t in thresholds(D, alive, rng, cap)[::3]:
            check(idx, D, alive, Q, t, cap, f"{name}, EXACT mode: {what}", topk=False)


def test_boundary_adversary_needs_the_f64_decision(oracle, lib_built):
    """Rows whose cosines with the query straddle the threshold within a few ulps: only the exact DistCosine decides them."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(41)
    d, n = 384, 12000                                              # (every candidate set fits a block: no EXACT fallback)
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    noise = rng.standard_normal((n, d))
    noise -= (noise @ q)[:, None] * q
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    c = np.where(np.arange(n) < n // 2, 0.8, 0.99999) + rng.uniform(-3e-7, 3e-7, n)
    X = (c[:, None] * q + np.sqrt(1 - c * c)[:, None] * noise) * rng.uniform(0.5, 2.0, (n, 1))
    X = X.astype(np.float32)
    X[n // 2 + n // 4:] = q.astype(np.float32) + rng.standard_normal((n - n // 2 - n // 4, d)).astype(np.float32) * 2e-4
    Q = np.stack([q, q * 3.0, q + rng.standard_normal(d) * 1e-5]).astype(np.float32)
    for kind in ("i8", "bf16", False):
        with FlatIndex(d) as idx:
            idx.set_filter_copy(kind)
            idx.add(X)
            alive = np.ones(n, dtype=bool)
            D = oracle_dists(oracle, X, Q)
            S = score_from_dist(D)
            for lo, hi in ((0, n // 2), (n // 2, n // 2 + n // 4), (n // 2 + n // 4, n)):
                med = np.sort(S[:, lo:hi], axis=1)[:, (hi - lo) // 2].astype(np.float32)
                for t in (med, np.nextafter(med, np.float32(2.0)), np.nextafter(med, np.float32(-2.0))):
                    check(idx, D, alive, Q, t.astype(np.float32), 4096, f"adversary, copy {kind}, rows {lo}..{hi}", topk=False)
            assert idx.stats().fallback_queries == 0, kind


@pytest.mark.parametrize("B", [1, 100, 200, 300, 512, 700])
def test_batch_geometries(B, oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(42 + B)
    d, n = 384, 20000
    X = corpus(rng, n, d)
    Q = rng.standard_normal((B, d)).astype(np.float32)
    Q[::2] = X[rng.integers(0, n, (B + 1) // 2)] + Q[::2] * 0.05
    with FlatIndex(d) as idx:
        idx.add(X)
        alive = np.ones(n, dtype=bool)
        D = oracle_dists(oracle, X, Q)
        S = np.sort(score_from_dist(D), axis=1)[:, ::-1]
        t = S[np.arange(B), rng.integers(0, 200, B)].astype(np.float32)   # a different rank per query
        t[::7] = np.nextafter(t[::7], np.float32(2.0))
        got = check(idx, D, alive, Q, t, 64, f"B = {B}, plain int8")
        if B >= 100:
            assert (got[4] > 64).any() and (got[4] < 64).any()
        idx.set_filter_copy("bf16")
        check(idx, D, alive, Q, t, 64, f"B = {B}, bf16", topk=False)


def test_side_lists_masks_and_compaction(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(43)
    d, n = 256, 30000
    X = corpus(rng, n, d)                                          # zero-norm rows, 1e20-norm rows, duplicates
    Q = rng.standard_normal((10, d)).astype(np.float32)
    Q[0] = 0.0                                                     # a zero-norm query: every live row, first cap by id
    Q[1] = X[11]                                                   # a 1e20-norm row
    Q[2] = X[99]
    with FlatIndex(d) as idx:
        idx.add(X)
        alive = np.ones(n, dtype=bool)
        D = oracle_dists(oracle, X, Q)
        cap = 100
        for what, t in [("t = 1", np.ones(10, np.float32)), ("t = 0.2", np.full(10, 0.2, np.float32)),
                        ("t = 0.05", np.full(10, 0.05, np.float32)), ("t above 1", np.full(10, 1.5, np.float32))]:
            got = check(idx, D, alive, Q, t, cap, what)
            if what != "t above 1":
                assert got[4][0] == n                              # the zero-norm query selects every row
                assert got[4][3] >= 3                              # the zero-norm rows are in range for every t <= 1
        gone = np.unique(np.r_[rng.choice(n, 3000, replace=False), 7, 300, 11, 99:108])
        idx.remove(gone + 1)
        alive[gone] = False
        for what, t in [("removed, t = 0.2", np.full(10, 0.2, np.float32)), ("removed, t = 1", np.ones(10, np.float32))]:
            got = check(idx, D, alive, Q, t, cap, what)
            assert got[4][0] == alive.sum()
        kept = idx.compact() - 1
        keep_rows = X[kept.astype(np.int64)]
        with FlatIndex(d) as fresh:
            fresh.add(keep_rows)
            t = np.full(10, 0.1, np.float32)
            a = idx.search_range(Q, t, cap)
            b = fresh.search_range(Q, t, cap)
            same(a, b, "compacted vs fresh")
            same(a, range_oracle(oracle_dists(oracle, keep_rows, Q), np.ones(len(kept), bool), t, cap), "compacted vs oracle")


def test_exact_fallbacks(oracle, lib_built):
    """t = -1 (every row) and 20k exact duplicates of a query: more candidates than a block holds -> the EXACT range path."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(44)
    d, n = 128, 30000
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[5000:25000] = X[17]
    Q = np.stack([X[17], rng.standard_normal(d), X[17] * 2.0, rng.standard_normal(d)]).astype(np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        alive = np.ones(n, dtype=bool)
        D = oracle_dists(oracle, X, Q)
        idx.reset_stats()
        t = np.array([0.5, -1.0, 0.999, -1.0], np.float32)
        for cap in (1, 4096):
            got = check(idx, D, alive, Q, t, cap, f"fallbacks, cap = {cap}", topk=cap <= 256)
            assert got[4][1] == n and got[4][0] >= 20001
        assert idx.stats().fallback_queries >= 4


def test_id_offset_sharded_and_concurrent_callers(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(45)
    d, n = 384, 30000
    X = corpus(rng, n, d)
    Q = rng.standard_normal((17, d)).astype(np.float32)
    Q[0] = X[1234]
    Q[1] = 0.0
    Q[2:10] = X[rng.integers(0, n, 8)] + Q[2:10] * 0.05
    gone = np.unique(np.r_[rng.choice(n, 300, replace=False), 1234, 96:200])
    alive = np.ones(n, dtype=bool)
    alive[gone] = False
    D = oracle_dists(oracle, X, Q)
    t = np.sort(score_from_dist(D), axis=1)[:, ::-1][np.arange(17), rng.integers(0, 300, 17)].astype(np.float32)
    with FlatIndex(d) as plain, FlatIndex(d, devices=[0, 0, 0], block_rows=96) as sh, FlatIndex(d) as offs:
        for idx in (plain, sh):
            idx.add(X)
            idx.remove(gone + 1)
        offs.set_id_offset(5000)
        offs.add(X)
        offs.remove(gone + 5001)
        for cap in (10, 300):
            a = sh.search_range(Q, t, cap)
            same(a, plain.search_range(Q, t, cap), f"3 shards vs plain, cap = {cap}")
            same(a, range_oracle(D, alive, t, cap), f"3 shards vs oracle, cap = {cap}")
            check(offs, D, alive, Q, t, cap, f"id_offset, cap = {cap}", off=5000)
        # concurrent range (two caps), top-k and filtered callers on one handle: each gets its own answer
        jobs = []
        for j in range(18):
            sel = rng.integers(0, 17, int(rng.integers(1, 4)))
            jobs.append((j % 3, sel))
        want = []
        for kind, sel in jobs:
            if kind == 0:
                want.append(range_oracle(D[sel], alive, t[sel], 10 if sel[0] % 2 else 40))
            elif kind == 1:
                want.append(plain.search(Q[sel], 10))
            else:
                want.append(plain.search_filtered(Q[sel], 10, ranges=[[1, 15001]]))
        got = [None] * len(jobs)
        errs = []

        def run(i):
            try:
                kind, sel = jobs[i]
                for _ in range(4):
                    if kind == 0:
                        got[i] = plain.search_range(Q[sel], t[sel], 10 if sel[0] % 2 else 40)
                    elif kind == 1:
                        got[i] = plain.search(Q[sel], 10)
                    else:
                        got[i] = plain.search_filtered(Q[sel], 10, ranges=[[1, 15001]])
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        for i, (kind, _) in enumerate(jobs):
            if kind == 0:
                same(got[i], want[i], f"thread {i}, range")
            else:
                for a, b in zip(got[i], want[i]):
                    np.testing.assert_array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b,
                                                  err_msg=f"thread {i}, kind {kind}")


def test_range_passes_leave_the_copy_heuristics_alone(lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(46)
    d, n = 384, 40000
    X = corpus(rng, n, d)
    with FlatIndex(d) as idx:
        idx.add(X)
        before = idx.stats()
        for i in range(12):
            Q = rng.standard_normal((64, d)).astype(np.float32)
            idx.search_range(Q, -1.0 if i % 2 else 0.1, 16)            # every row: overflows on every query
        after = idx.stats()
        assert after.filter_kind == before.filter_kind
        assert after.filter_demotions == before.filter_demotions
        assert after.filter_promotions == before.filter_promotions
        assert after.filter_centred == before.filter_centred
        assert after.queries - before.queries == 12 * 64
        assert after.fallback_queries - before.fallback_queries == 6 * 64


def test_store_search_above_before_and_after_compact(lib_built, tmp_path):
    from memex_amd import storage
    rng = np.random.default_rng(47)
    d = 64
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    base = rng.standard_normal(d).astype(np.float32)
    near = [base + rng.standard_normal(d).astype(np.float32) * s for s in (0.0, 0.01, 0.05, 0.2, 1.0, 3.0)]
    st.bulk_insert([storage.VectorData(_id=f"n{i}", document_id="d", text="", vector=list(map(float, v))) for i, v in enumerate(near)])
    st.bulk_insert([storage.VectorData(_id=f"r{i}", document_id="r", text="", vector=list(map(float, v)))
                    for i, v in enumerate(rng.standard_normal((500, d)).astype(np.float32))])
    q = list(map(float, base))
    top = st.search(q, 506)
    for t in (0.99, 0.9, 0.5, 0.0, -1.0):
        got = st.search_above(q, t, 4096)
        assert got == [r for r in top if r[1] >= np.float32(t)], t
    assert st.search_above(q, 0.9, 2) == st.search(q, 2)
    assert st.search_above(q, 1.5, 10) == []
    before = st.search_above(q, 0.5, 100)
    assert [i for i, _ in before[:3]] == ["n0", "n1", "n2"]
    st.remove(["n1", "r3"])
    after = st.search_above(q, 0.5, 100)
    assert after == [r for r in before if r[0] not in ("n1", "r3")]
    st.compact()
    assert st.search_above(q, 0.5, 100) == after
