"""Filtered search (mx_index_search_filtered): the exact top-k among the rows whose ids lie in caller-given ranges.  Every answer
must be bit-identical to the oracle run on the allowed rows that have not been removed, with the oracle's row numbers mapped back
to the index's ids (the oracle orders ties by row, and that order is monotone in id, so the tie order carries over)."""
import threading

import numpy as np
import pytest

from conftest import bits
from filtered_model import allowed_mask, subset_oracle
from test_remove_gpu import corpus

pytestmark = pytest.mark.gpu


def same(got, want, what):
    """both in FlatIndex.search order: (ids, scores, dists, n_found)"""
    ids, sc, di, nf = got
    oi, os_, od, onf = want
    np.testing.assert_array_equal(nf, onf, err_msg=what)
    np.testing.assert_array_equal(ids, oi, err_msg=what)
    np.testing.assert_array_equal(bits(di), bits(od), err_msg=what)
    np.testing.assert_array_equal(bits(sc), bits(os_), err_msg=what)


def check(idx, oracle, rows, alive, Q, k, ranges, what, off=0):
    got = idx.search_filtered(Q, k, ranges=ranges)
    keep = alive & allowed_mask(rows.shape[0], ranges, off)
    same(got, subset_oracle(oracle, rows, keep, Q, k, off), what)
    return got, int(keep.sum())


def both_paths(monkeypatch, idx, Q, k, ranges):
    """The same filtered search forced onto the masked pipeline and onto the subset kernel: identical bits."""
    monkeypatch.setenv("MEMEX_HIP_DEBUG", "filt_subset=0")
    a = idx.search_filtered(Q, k, ranges=ranges)
    monkeypatch.setenv("MEMEX_HIP_DEBUG", "filt_subset=1")
    b = idx.search_filtered(Q, k, ranges=ranges)
    monkeypatch.delenv("MEMEX_HIP_DEBUG")
    same(a, b, f"masked pipeline vs subset kernel, k = {k}")
    return a


def shapes(rng, n):
    tiles = np.arange(0, n // 64, 2)
    return [
        ("small range", np.array([[101, 171]])),                                     # 70 rows: the subset kernel
        ("5000 scattered ids", np.stack([ids := np.sort(rng.choice(n, 5000, replace=False)) + 1, ids + 1], 1)),
        ("half the corpus", np.array([[n // 4, n // 4 + n // 2]])),
        ("every other tile", np.stack([64 * tiles + 1, 64 * tiles + 65], 1)),
        ("all ids", np.array([[1, n + 1]])),
        ("empty", np.zeros((0, 2), dtype=np.uint64)),
        ("past the end", np.array([[n - 40, n + 1000], [n + 5000, n + 6000]])),
        ("unsorted, overlapping", np.array([[5000, 9000], [100, 300], [8000, 12000], [250, 260], [100, 300], [3, 3]])),
    ]


# (name, dim, rows, setup before add, setup after add)
_KINDS = [
    ("int8", 384, 40000, None, lambda idx: idx.set_filter_copy("i8")),
    ("centred_int8", 384, 40000, None, "centre_i8"),
    ("bf16", 384, 30000, None, lambda idx: idx.set_filter_copy("bf16")),
    ("centred_bf16", 384, 30000, None, "centre_bf16"),
    ("f32", 384, 20000, None, lambda idx: idx.set_filter_copy(False)),
    ("compressed", 384, 30000, lambda idx: idx.set_corpus_mode("bf16"), None),
    ("wide_1536", 1536, 20000, None, lambda idx: idx.set_filter_copy("bf16")),
]


@pytest.mark.parametrize("name,d,n,pre,post", _KINDS, ids=[c[0] for c in _KINDS])
def test_filter_shapes_match_oracle(name, d, n, pre, post, oracle, lib_built, monkeypatch):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(sum(map(ord, name)) + 3)
    cone = name.startswith("centred")
    X = corpus(rng, n, d, cone=cone)           # zero-norm rows 7, 300, n/2+1; 1e20-norm rows 11, n-100; duplicates 99..107
    if name == "compressed":
        X[[11, n - 100]] = rng.standard_normal((2, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        if pre:
            pre(idx)
        idx.add(X)
        if callable(post):
            post(idx)
        elif post:
            idx.set_filter_copy(False)
            idx.set_filter_copy("i8" if post == "centre_i8" else "bf16")
            assert idx.stats().filter_centred == 1
        rows = idx.get_rows(0, n) if name == "compressed" else X
        alive = np.ones(n, dtype=bool)
        Q = rng.standard_normal((16, d)).astype(np.float32)
        if cone:
            Q[::2] = rows[rng.integers(0, n, 8)] + Q[::2] * 0.01
        Q[1] = rows[130] * 2.0
        Q[2] = rows[8000]
        Q[3] = 0.0                                                                # zero query: the first allowed rows
        for phase in ("nothing removed", "removals"):
            if phase == "removals":
                gone = np.r_[rng.choice(n, n // 50, replace=False), 120:140, 7, 11, 8000, 5000:5064]
                assert idx.remove(np.unique(gone) + 1) > 0
                alive[gone] = False
            for what, r in shapes(rng, n):
                got, m = check(idx, oracle, rows, alive, Q, 10, r, f"{name}, {phase}, {what}, k = 10")
                # k = 1: the oracle's first column
                one = tuple(a[:, :1] for a in got[:3]) + (np.minimum(got[3], 1),)
                same(idx.search_filtered(Q, 1, ranges=r), one, f"{name}, {phase}, {what}, k = 1")
                if 0 < m <= 16384:
                    same(both_paths(monkeypatch, idx, Q, 10, r), got, f"{name}, {phase}, {what}: both paths")
            check(idx, oracle, rows, alive, Q[:6], 256, np.array([[1, n // 2]]), f"{name}, {phase}, k = 256")
            check(idx, oracle, rows, alive, Q[:6], 300, np.array([[1, n // 3], [n // 2, n]]), f"{name}, {phase}, k = 300")
            # all ids: what search gives, bit for bit
            full = idx.search(Q, 10)
            same(idx.search_filtered(Q, 10, ranges=[[1, n + 1]]), full, f"{name}, {phase}: all ids == search")


def test_int8_batch_geometries_and_large_k(oracle, lib_built, monkeypatch):
    """int8 at B = 1, 100, 200 (the pair geometry) and 512 (two query groups per wave); k = 4096 on the subset kernel."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(31)
    d, n = 384, 60000
    X = corpus(rng, n, d)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.set_filter_copy("i8")
        alive = np.ones(n, dtype=bool)
        alive[rng.choice(n, 600, replace=False)] = False
        idx.remove(np.flatnonzero(~alive) + 1)
        for B in (1, 100, 200, 512):
            Q = rng.standard_normal((B, d)).astype(np.float32)
            Q[0] = X[20000]
            for r in (np.array([[20001, 20071]]), np.array([[1, 40001]]), np.array([[17, 29000], [31000, 60001]])):
                check(idx, oracle, X, alive, Q, 10, r, f"int8, B = {B}, {r.tolist()}")
        Q = rng.standard_normal((4, d)).astype(np.float32)
        r = np.array([[1001, 9001]])
        got, m = check(idx, oracle, X, alive, Q, 4096, r, "k = 4096 (the masked pipeline: EXACT)")
        assert (got[3] == min(4096, m)).all()
        same(both_paths(monkeypatch, idx, Q, 4096, r), got, "k = 4096, both paths")
        r = np.array([[1, 16000], [30000, 30385]])                                 # more than 2048 rows: the select pass
        got, m = check(idx, oracle, X, alive, Q, 50, r, "16k rows")
        same(both_paths(monkeypatch, idx, Q, 50, r), got, "16k rows, both paths")


def test_id_offset(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(32)
    d, n, off = 128, 20000, 1_000_000
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((8, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.set_id_offset(off)
        alive = np.ones(n, dtype=bool)
        for r in ([[off + 50, off + 120]], [[0, off + 5000], [off + 15000, off + 10 ** 9]], [[off - 10, off + 1]]):
            got, m = check(idx, oracle, X, alive, Q, 10, np.array(r, dtype=np.uint64), f"offset, {r}", off=off)
            assert (got[0][got[0] > 0] > off).all()


def test_adversarial_block_of_near_copies_outside_the_filter(oracle, lib_built):
    """Rows near cosine 0.3 to the queries inside the filter, 20k near-copies of the queries outside it.  A sample that ignored
    the filter would set theta near 1 from the copies and drop the allowed neighbours without any overflow to catch it."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(33)
    d, n, B = 384, 60000, 64
    Q = rng.standard_normal((B, d))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    owner = rng.integers(0, B, n)
    noise = rng.standard_normal((n, d))
    noise -= (noise * Q[owner]).sum(1, keepdims=True) * Q[owner]
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    c = rng.uniform(0.28, 0.32, (n, 1))
    X = (c * Q[owner] + np.sqrt(1 - c * c) * noise).astype(np.float32)
    copies = (Q[rng.integers(0, B, 20000)] + rng.standard_normal((20000, d)) * 1e-3).astype(np.float32)
    rows = np.concatenate([X[:30000], copies, X[30000:]])                      # the copies sit inside the span
    alive = np.ones(rows.shape[0], dtype=bool)
    r = np.array([[1, 30001], [50001, 80001]])
    for kind in ("i8", "bf16", False):
        with FlatIndex(d) as idx:
            idx.set_filter_copy(kind)
            idx.add(rows)
            idx.reset_stats()
            check(idx, oracle, rows, alive, Q.astype(np.float32), 10, r, f"adversarial, copy {kind}")
            st = idx.stats()
            assert st.fallback_queries == 0, kind
            assert st.filter_demotions == 0, kind


def test_side_lists_inside_and_outside_the_filter(oracle, lib_built, monkeypatch):
    """Zero-norm and 1e20-norm rows on both sides of the filter: finish_kernel tests each listed row's bit."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(34)
    d, n = 256, 30000
    X = rng.standard_normal((n, d)).astype(np.float32)
    zero, wild = [40, 41, 20000, 20001], [45, 20005]
    X[zero] = 0
    # norm 1e20 with every element at 1e20 / sqrt(d): no f32 product of the row overflows (DistCosine stays defined)
    X[wild] = np.sign(rng.standard_normal((2, d))).astype(np.float32) * np.float32(1e20 / np.sqrt(d))
    Q = rng.standard_normal((12, d)).astype(np.float32)
    Q[0] = X[45]
    Q[1] = 0.0
    with FlatIndex(d) as idx:
        idx.add(X)
        alive = np.ones(n, dtype=bool)
        for r in (np.array([[1, 10001]]), np.array([[10001, n + 1]]), np.array([[30, 60], [19990, 20010]])):
            for k in (10, 300):
                got, m = check(idx, oracle, X, alive, Q, k, r, f"side lists, {r.tolist()}, k = {k}")
                if m <= 16384:
                    same(both_paths(monkeypatch, idx, Q, k, r), got, "side lists, both paths")


def test_copy_state_unchanged_by_selective_filters(oracle, lib_built):
    """Many selective filtered batches on an automatically chosen int8 copy: no demotion, no promotion, no counted batch."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(35)
    d, n = 384, 80000
    X = corpus(rng, n, d)
    with FlatIndex(d) as idx:
        idx.add(X)
        before = idx.stats()
        alive = np.ones(n, dtype=bool)
        for i in range(24):
            Q = (X[rng.integers(0, n, 64)] + rng.standard_normal((64, d)).astype(np.float32) * 0.05).astype(np.float32)
            lo = int(rng.integers(1, n - 30000))
            r = np.array([[lo, lo + 20000 + 500 * i]])
            if i % 6 == 0:
                check(idx, oracle, X, alive, Q, 10, r, f"batch {i}")
            else:
                idx.search_filtered(Q, 10, ranges=r)
        after = idx.stats()
        assert after.filter_kind == before.filter_kind == 2
        assert after.filter_demotions == before.filter_demotions
        assert after.filter_promotions == before.filter_promotions


def test_sharded_equals_plain(oracle, lib_built, monkeypatch):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(36)
    d, n = 384, 30000
    X = corpus(rng, n, d)
    Q = rng.standard_normal((17, d)).astype(np.float32)
    Q[0] = X[1234]
    Q[1] = 0.0
    gone = np.r_[rng.choice(n, 300, replace=False), 1234, 96:200]
    with FlatIndex(d) as plain, FlatIndex(d, devices=[0, 0, 0], block_rows=96) as sh:
        for idx in (plain, sh):
            idx.add(X)
            idx.remove(np.unique(gone) + 1)
        alive = np.ones(n, dtype=bool)
        alive[gone] = False
        for what, r in shapes(rng, n) + [("block edges", np.array([[95, 98], [191, 290], [288 * 5, 288 * 5 + 97]]))]:
            for k in (10, 300):
                a = sh.search_filtered(Q, k, ranges=r)
                same(a, plain.search_filtered(Q, k, ranges=r), f"3 shards vs plain, {what}, k = {k}")
                keep = alive & allowed_mask(n, r)
                same(a, subset_oracle(oracle, X, keep, Q, k), f"3 shards vs oracle, {what}, k = {k}")
        sh.reset_stats()
        sh.search_filtered(Q, 10, ranges=[[1001, 1071]])                    # (rows 96..199 are removed)
        st = sh.stats()
        assert st.filtered_queries == 17 and st.subset_queries == 17


def test_concurrent_filtered_and_unfiltered_calls(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(37)
    d, n = 256, 40000
    X = rng.standard_normal((n, d)).astype(np.float32)
    filters = [None, np.array([[1, 20001]]), np.array([[1, 20001]]), np.array([[501, 571]]), np.array([[10001, n + 1], [3, 9]])]
    with FlatIndex(d) as idx:
        idx.add(X)
        alive = np.ones(n, dtype=bool)
        jobs = []
        for t in range(20):
            Q = rng.standard_normal((int(rng.integers(1, 4)), d)).astype(np.float32)
            jobs.append((Q, filters[t % len(filters)]))
        want = []
        for Q, r in jobs:
            keep = alive if r is None else alive & allowed_mask(n, r)
            want.append(subset_oracle(oracle, X, keep, Q, 10))
        got = [None] * len(jobs)
        errs = []

        def run(i):
            try:
                Q, r = jobs[i]
                for _ in range(5):
                    got[i] = idx.search(Q, 10) if r is None else idx.search_filtered(Q, 10, ranges=r)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        for i in range(len(jobs)):
            same(got[i], want[i], f"thread {i}, filter {jobs[i][1]}")


def test_stats_count_filtered_and_subset_queries(lib_built, monkeypatch):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(38)
    d, n = 128, 20000
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((5, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.reset_stats()
        idx.search(Q, 10)
        idx.search_filtered(Q, 10, ranges=[[1, 71]])                   # the subset kernel
        idx.search_filtered(Q, 10, ranges=[[1, 20001]])                # more rows than the subset cap: the masked pipeline
        monkeypatch.setenv("MEMEX_HIP_DEBUG", "filt_subset=0")
        idx.search_filtered(Q[:2], 10, ranges=[[1, 71]])
        monkeypatch.delenv("MEMEX_HIP_DEBUG")
        idx.search_filtered(Q[:3], 10, ranges=[])                      # the empty set: served, nothing found
        st = idx.stats()
        assert st.queries == 20
        assert st.filtered_queries == 15
        assert st.subset_queries == 5


def test_store_search_within_before_and_after_compact(lib_built, tmp_path):
    from memex_amd import storage
    rng = np.random.default_rng(39)
    d = 64
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    docs = {f"doc{j}": rng.standard_normal((int(rng.integers(3, 40)), d)).astype(np.float32) for j in range(30)}
    for j, (doc, v) in enumerate(docs.items()):
        st.bulk_insert([storage.VectorData(_id=f"{doc}/{i}", document_id=doc, text="", vector=list(map(float, row)))
                        for i, row in enumerate(v)])
    q = list(map(float, docs["doc3"][1] + 0.01))
    segs = [f"doc3/{i}" for i in range(len(docs["doc3"]))] + [f"doc7/{i}" for i in range(len(docs["doc7"]))]
    before = st.search_within(q, 10, segs + ["nope"])
    assert before and before[0][0] == "doc3/1"
    assert {i for i, _ in before} <= set(segs)
    assert len(before) == min(10, len(segs))
    assert st.search_within(q, 10, ["nope"]) == []
    # the same answer as a plain search over a store holding only those rows
    only = storage.HipFlatStore.new(str(tmp_path / "only"))
    only.bulk_insert([storage.VectorData(_id=s, document_id="", text="", vector=list(map(float, docs[s.split("/")[0]][int(s.split("/")[1])])))
                      for s in segs])
    assert before == only.search(q, 10)
    st.remove([f"doc{j}/0" for j in range(0, 30, 2)])
    st.compact()                                                          # ids renumbered; the _ids answer the same
    assert st._index.removed == 0 and len(st._id_map) < sum(len(v) for v in docs.values())
    assert st.search_within(q, 10, segs) == before                      # (doc3 and doc7 lost nothing)
    gone = st.search_within(q, 10, segs + ["doc2/0", "doc2/1"])          # doc2/0 is gone for good, doc2/1 stayed
    assert "doc2/0" not in {i for i, _ in gone}
