"""Diversified search (mx_index_search_mmr) on the GPU against its NumPy statement (tests/mmr_model.py).  Every case compares ids, score
bits, dist bits and n_found with integer equality.  The corpora are clusters of near-copies (overlapping windows of one document), so
the selection really departs from the plain top-k; the shapes are small because the selection never looks past `fetch` rows."""
import threading

import numpy as np
import pytest

from conftest import bits
from mmr_model import mmr_model, near_copy_corpus, queries_near_centres

pytestmark = pytest.mark.gpu

_CACHE = {}


def base(d=384, clusters=150, B=37):
    """the near-copy corpus of the model test at `d` dims and B queries near cluster centres (built once per shape)"""
    key = ("base", d, clusters, B)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 + d + clusters + B)
        X, centres = near_copy_corpus(rng, clusters=clusters, d=d)
        _CACHE[key] = (X, centres, queries_near_centres(rng, centres, B))
    return _CACHE[key]


def model(oracle, key, rows, Q, k, fetch, lam, **kw):
    """mmr_model, computed once per named case and shared by the tests that need it"""
    key = (key, k, fetch, lam)
    if key not in _CACHE:
        _CACHE[key] = mmr_model(oracle, rows, Q, k, fetch=fetch, lam=lam, **kw)
    return _CACHE[key]


def same(got, want, what):
    ids, sc, di, nf = got
    oi, os_, od, onf = want
    np.testing.assert_array_equal(nf, onf, err_msg=f"{what}: n_found")
    np.testing.assert_array_equal(ids, oi, err_msg=f"{what}: ids")
    np.testing.assert_array_equal(bits(di), bits(od), err_msg=f"{what}: dists")
    np.testing.assert_array_equal(bits(sc), bits(os_), err_msg=f"{what}: scores")


# (name, dim, clusters, setup)
_KINDS = [
    ("int8", 384, 150, lambda idx: idx.set_filter_copy("i8")),
    ("bf16", 384, 150, lambda idx: idx.set_filter_copy("bf16")),
    ("f32", 384, 150, lambda idx: idx.set_filter_copy(False)),
    ("compressed", 384, 150, "compressed"),
    ("dim100", 100, 150, None),
    ("dim1536", 1536, 30, None),
]


@pytest.mark.parametrize("name,d,clusters,setup", _KINDS, ids=[c[0] for c in _KINDS])
def test_every_copy_kind_matches_the_model(name, d, clusters, setup, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q = base(d, clusters)
    with FlatIndex(d) as idx:
        if setup == "compressed":
            idx.set_corpus_mode("bf16")
        idx.add(X)
        if callable(setup):
            setup(idx)
        rows = idx.get_rows(0, len(X)) if setup == "compressed" else X
        assert setup != "compressed" or (rows != X).any()              # the model is fed what the index stores
        want = model(oracle, ("kind", d, clusters, setup == "compressed"), rows, Q, 10, 64, 0.5)
        got = idx.search_mmr(Q, 10, fetch=64, lam=0.5)
        same(got, want, name)
        plain = idx.search(Q, 10)
        assert (got[0] != plain[0]).any(axis=1).sum() >= len(Q) // 2, "the corpus does not exercise the selection"
        np.testing.assert_array_equal(got[0][:, 0], plain[0][:, 0])


@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_lambda(lam, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    with FlatIndex(384) as idx:
        idx.add(X)
        got = idx.search_mmr(Q, 10, fetch=64, lam=lam)
        same(got, model(oracle, ("kind", 384, 150, False), X, Q, 10, 64, lam), f"lam = {lam}")
        if lam == 1.0:                                                  # the plain top-k itself
            same(got, idx.search(Q, 10), "lam = 1 vs search")
        got = idx.search_mmr(Q[:5], 10, lam=lam)                        # fetch = None: min(max(4 k, 32), 1024) = 40
        same(got, model(oracle, "default fetch", X, Q[:5], 10, 40, lam), f"lam = {lam}, default fetch")


@pytest.mark.parametrize("k,fetch,B", [(10, 10, 37), (10, 256, 8), (10, 257, 8), (64, 1024, 2)],
                         ids=["fetch=k", "fetch=256", "fetch=257", "fetch=1024"])
def test_fetch(k, fetch, B, oracle, lib_built):
    """fetch = k: a permutation of the plain top-k; 256: the last AUTO candidate stage; 257 and 1024: the EXACT path"""
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    Q = Q[:B]
    with FlatIndex(384) as idx:
        idx.add(X)
        idx.reset_stats()
        got = idx.search_mmr(Q, k, fetch=fetch, lam=0.5)
        st = idx.stats()
        assert st.searches == 1 and st.queries == B                    # the candidate stage is one plain pass
        same(got, model(oracle, "fetch", X, Q, k, fetch, 0.5), f"fetch = {fetch}")
        if fetch == k:
            plain = idx.search(Q, k)
            np.testing.assert_array_equal(got[0][:, 0], plain[0][:, 0])
            np.testing.assert_array_equal(np.sort(got[0], axis=1), np.sort(plain[0], axis=1))
            assert (got[0] != plain[0]).any()


def test_fetch_beyond_the_live_rows(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    with FlatIndex(384) as idx:
        idx.add(X[:40])
        got = idx.search_mmr(Q[:6], 50, fetch=64, lam=0.5)
        assert (got[3] == 40).all()
        assert (got[0][:, 40:] == 0).all() and (got[1][:, 40:] == 0).all() and np.isposinf(got[2][:, 40:]).all()
        same(got, mmr_model(oracle, X[:40], Q[:6], 50, fetch=64, lam=0.5), "40 rows, fetch 64, k 50")
    with FlatIndex(384) as idx:                                         # an empty index finds nothing
        ids, sc, di, nf = idx.search_mmr(Q[:3], 5, fetch=8)
        assert (nf == 0).all() and (ids == 0).all() and (sc == 0).all() and np.isposinf(di).all()


@pytest.mark.parametrize("B", [1, 300, 600])
def test_batch_sizes(B, oracle, lib_built):
    """600 crosses the 512-query split"""
    from memex_amd.index import FlatIndex
    X, centres, _ = base()
    Q = queries_near_centres(np.random.default_rng(50 + B), centres, B)
    with FlatIndex(384) as idx:
        idx.add(X)
        same(idx.search_mmr(Q, 10, fetch=32, lam=0.5), mmr_model(oracle, X, Q, 10, fetch=32, lam=0.5), f"B = {B}")


def test_special_rows(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, centres, _ = base()
    rng = np.random.default_rng(61)
    Q = queries_near_centres(rng, centres[5:6], 6)                      # cluster 5: rows 100 .. 119
    Q = np.concatenate([Q, queries_near_centres(rng, centres, 6)])
    # exact duplicates and a 1e20-norm row among the candidates
    A = X.copy()
    A[101:105] = A[100]
    A[110] *= np.float32(1e20) / np.float32(np.linalg.norm(A[110]))
    A[2500] *= np.float32(1e20) / np.float32(np.linalg.norm(A[2500]))
    # a zero-norm row: DistCosine 0 against everything, so it leads every candidate list and its similarity to every row is 1
    Z = X.copy()
    Z[107] = 0
    for what, rows in (("duplicates and 1e20 rows", A), ("zero-norm row", Z)):
        with FlatIndex(384) as idx:
            idx.add(rows)
            for lam in (0.5, 0.0):
                got = idx.search_mmr(Q, 10, fetch=64, lam=lam)
                same(got, mmr_model(oracle, rows, Q, 10, fetch=64, lam=lam), f"{what}, lam = {lam}")
            if rows is A:                                               # (conditions on the inputs)
                top = idx.search(Q[:6], 64)[0]
                assert (top == 111).any(axis=1).all() and (top == 103).any(axis=1).all()
            else:
                assert (got[0][:, 0] == 108).all()


def test_remove_compact_and_id_offset(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, centres, Q = base()
    rng = np.random.default_rng(62)
    Q = np.concatenate([queries_near_centres(rng, centres[7:8], 5), Q[:12]])   # cluster 7: rows 140 .. 159
    gone = np.unique(np.r_[140:150, rng.choice(len(X), 400, replace=False)])
    alive = np.ones(len(X), dtype=bool)
    alive[gone] = False
    with FlatIndex(384) as idx, FlatIndex(384) as offs:
        idx.add(X)
        idx.remove(gone + 1)
        got = idx.search_mmr(Q, 10, fetch=64, lam=0.5)
        assert not np.isin(got[0], gone + 1).any()                      # removed rows never appear
        same(got, mmr_model(oracle, X, Q, 10, fetch=64, lam=0.5, alive=alive), "removed rows")
        kept = idx.compact().astype(np.int64) - 1
        np.testing.assert_array_equal(kept, np.flatnonzero(alive))
        same(idx.search_mmr(Q, 10, fetch=64, lam=0.5), mmr_model(oracle, X[kept], Q, 10, fetch=64, lam=0.5), "compacted")
        offs.set_id_offset(5000)
        offs.add(X)
        offs.remove(gone + 5001)
        same(offs.search_mmr(Q, 10, fetch=64, lam=0.5), mmr_model(oracle, X, Q, 10, fetch=64, lam=0.5, alive=alive, id_offset=5000),
             "id_offset and removed rows")


def test_sharded_equals_plain(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    gone = np.arange(200, 230)
    with FlatIndex(384) as plain, FlatIndex(384, devices=[0, 0, 0], block_rows=96) as sh:
        for idx in (plain, sh):
            idx.set_id_offset(77)
            idx.add(X)
            idx.remove(gone + 78)
        alive = np.ones(len(X), dtype=bool)
        alive[gone] = False
        for k, fetch, lam in ((10, 64, 0.5), (10, 300, 0.3)):
            a = sh.search_mmr(Q[:9], k, fetch=fetch, lam=lam)
            same(a, plain.search_mmr(Q[:9], k, fetch=fetch, lam=lam), f"3 shards vs plain, fetch = {fetch}")
            same(a, mmr_model(oracle, X, Q[:9], k, fetch=fetch, lam=lam, alive=alive, id_offset=77), f"3 shards vs model, fetch = {fetch}")


def test_device_pointer_variant_equals_the_host_variant(lib_built):
    import torch
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    with FlatIndex(384) as plain, FlatIndex(384, devices=[0, 0], block_rows=64) as sh:
        for idx in (plain, sh):
            idx.add(X)
            for k, fetch, dists in ((10, 64, True), (7, None, False)):
                q = torch.from_numpy(Q).cuda()
                ids = torch.full((len(Q), k), -1, dtype=torch.int64, device="cuda")
                sc = torch.full((len(Q), k), -1.0, dtype=torch.float32, device="cuda")
                di = torch.full((len(Q), k), -1.0, dtype=torch.float32, device="cuda") if dists else None
                nf = torch.full((len(Q),), -1, dtype=torch.int32, device="cuda")
                idx.search_mmr_device(q, k, ids, sc, di, nf, fetch=fetch, lam=0.4)
                h = idx.search_mmr(Q, k, fetch=fetch, lam=0.4)
                np.testing.assert_array_equal(ids.cpu().numpy().astype(np.uint64), h[0])
                np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(h[1]))
                if dists:
                    np.testing.assert_array_equal(bits(di.cpu().numpy()), bits(h[2]))
                np.testing.assert_array_equal(nf.cpu().numpy(), h[3])


def test_concurrent_callers(lib_built):
    """four threads issue diversified searches (two parameter sets) while a fifth issues plain searches: every answer equals its
    single-threaded one"""
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    jobs = [("mmr", Q[:8], 10, 64, 0.5), ("mmr", Q[8:20], 5, 32, 0.2), ("mmr", Q[20:23], 10, 64, 0.5), ("mmr", Q[23:37], 12, 300, 0.7),
            ("plain", Q, 10, None, None)]
    with FlatIndex(384) as idx:
        idx.add(X)

        def call(job):
            kind, q, k, fetch, lam = job
            return idx.search(q, k) if kind == "plain" else idx.search_mmr(q, k, fetch=fetch, lam=lam)

        want = [call(j) for j in jobs]
        got = [None] * len(jobs)
        errs = []

        def run(i):
            try:
                for _ in range(5):
                    got[i] = call(jobs[i])
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        for i in range(len(jobs)):
            same(got[i], want[i], f"thread {i}")


def test_store_search_diverse_before_and_after_compact(oracle, lib_built, tmp_path):
    from memex_amd import storage
    rng = np.random.default_rng(63)
    X, centres = near_copy_corpus(rng, clusters=12, per=8, d=64)
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    st.bulk_insert([storage.VectorData(_id=f"s{i}", document_id=f"d{i // 8}", text="", vector=list(map(float, v))) for i, v in enumerate(X)])
    q = queries_near_centres(rng, centres[3:4], 1)

    def expect(rows, names, k, fetch, lam):
        ids, sc, _, nf = mmr_model(oracle, rows, q, k, fetch=fetch, lam=lam)
        return [(names[int(i) - 1], float(s)) for i, s in zip(ids[0, :nf[0]], sc[0, :nf[0]])]

    names = [f"s{i}" for i in range(len(X))]
    assert st.search_diverse(list(map(float, q[0])), 6) == expect(X, names, 6, 32, 0.5)
    assert st.search_diverse(list(map(float, q[0])), 6, fetch=20, lam=0.2) == expect(X, names, 6, 20, 0.2)
    assert st.search_diverse(list(map(float, q[0])), 6, lam=1.0) == st.search(list(map(float, q[0])), 6)
    assert st.search_diverse(list(map(float, q[0])), 6) != st.search(list(map(float, q[0])), 6)
    st.remove(["s24", "s25", "s3"])
    keep = [i for i in range(len(X)) if i not in (24, 25, 3)]
    after = st.search_diverse(list(map(float, q[0])), 6)
    assert after == expect(X[keep], [names[i] for i in keep], 6, 32, 0.5)
    st.compact()
    assert st.search_diverse(list(map(float, q[0])), 6) == after
