"""Fused search (mx_index_search_fused) on the GPU against its statement in Python floats (tests/fused_model.py).  Every case compares
ids, n_found and best_sub with integer equality and scores, dists (f32) and fused (f64) by their bits.  The shapes are small: the
fusion never looks past the m top-`fetch` lists, whatever the corpus."""
import threading

import numpy as np
import pytest

from conftest import bits
from fused_model import MAX, RRF, fused_model, tripled_corpus
from mmr_model import near_copy_corpus, queries_near_centres

pytestmark = pytest.mark.gpu

_CACHE = {}


def base():
    """the near-copy corpus (150 clusters x 20 rows x 384 dims) and R = 5 requests of m = 3 sub-queries: two near one cluster centre,
    the third near another, so the lists overlap partly"""
    if "base" not in _CACHE:
        rng = np.random.default_rng(1313)
        X, centres = near_copy_corpus(rng, clusters=150, per=20, d=384)
        c = rng.choice(len(centres), (5, 2), replace=False)
        Q = np.stack([queries_near_centres(rng, centres[[a]], 2).tolist() + queries_near_centres(rng, centres[[b]], 1).tolist()
                      for a, b in c]).astype(np.float32)
        _CACHE["base"] = (X, centres, Q)
    return _CACHE["base"]


def small(n=2000, d=64, seed=5):
    key = ("small", n, d, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        X, centres = near_copy_corpus(rng, clusters=n // 10, per=10, d=d)
        _CACHE[key] = (X, centres)
    return _CACHE[key]


def requests(rng, centres, R, m):
    """R requests of m sub-queries, the first half of each near one centre, the rest near another"""
    out = []
    for _ in range(R):
        a, b = rng.choice(len(centres), 2, replace=False)
        h = (m + 1) // 2
        out.append(np.concatenate([queries_near_centres(rng, centres[[a]], h), queries_near_centres(rng, centres[[b]], m - h)]) if m > h
                   else queries_near_centres(rng, centres[[a]], h))
    return np.stack(out).astype(np.float32)


def model(oracle, key, *a, **kw):
    """fused_model, computed once per named case"""
    if key not in _CACHE:
        _CACHE[key] = fused_model(oracle, *a, **kw)
    return _CACHE[key]


def same(got, want, what):
    ids, sc, di, nf, best, fused = got
    oi, os_, od, onf, ob, of = want
    np.testing.assert_array_equal(nf, onf, err_msg=f"{what}: n_found")
    np.testing.assert_array_equal(ids, oi, err_msg=f"{what}: ids")
    np.testing.assert_array_equal(best, ob, err_msg=f"{what}: best_sub")
    np.testing.assert_array_equal(bits(di), bits(od), err_msg=f"{what}: dists")
    np.testing.assert_array_equal(bits(sc), bits(os_), err_msg=f"{what}: scores")
    np.testing.assert_array_equal(np.ascontiguousarray(fused, np.float64).view(np.uint64),
                                  np.ascontiguousarray(of, np.float64).view(np.uint64), err_msg=f"{what}: fused")


def blanks_ok(got):
    ids, sc, di, nf, best, fused = got
    for r in range(len(nf)):
        n = int(nf[r])
        assert (ids[r, n:] == 0).all() and (sc[r, n:] == 0).all() and np.isposinf(di[r, n:]).all()
        assert (best[r, n:] == -1).all() and (fused[r, n:] == 0).all()


@pytest.mark.parametrize("mode", [MAX, RRF])
def test_both_modes_match_the_model(mode, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    with FlatIndex(384) as idx:
        idx.add(X)
        idx.reset_stats()
        got = idx.search_fused(Q, 10, mode=mode, fetch=40)
        st = idx.stats()
        assert st.searches == 1 and st.queries == 15                    # the candidate stage is one plain pass over R * m queries
        same(got, model(oracle, ("base", mode), X, Q, 10, mode=mode, fetch=40), mode)
        assert (got[3] == 10).all()
        # (conditions on the inputs) the lists overlap partly: some rows are best in a later list, and the union exceeds one list
        assert (got[4] > 0).any() and (got[4] == 0).any()
        one = idx.search_fused(Q[0], 10, mode=mode, fetch=40)           # [m, dim]: one request
        same(one, tuple(a[:1] for a in got), f"{mode}, one request")


def test_one_sub_query(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    q = Q[:, :1]                                                        # [5, 1, 384]
    with FlatIndex(384) as idx:
        idx.add(X)
        ids, sc, di, nf = idx.search(q[:, 0], 10)
        got = idx.search_fused(q, 10, mode=MAX)
        np.testing.assert_array_equal(got[0], ids)
        np.testing.assert_array_equal(bits(got[1]), bits(sc))
        np.testing.assert_array_equal(bits(got[2]), bits(di))
        np.testing.assert_array_equal(got[3], nf)
        assert (got[4] == 0).all()
        np.testing.assert_array_equal(got[5], sc.astype(np.float64))
        ids, sc, di, nf = idx.search(q[:, 0], 32)
        w = np.float32(2.5)
        got = idx.search_fused(q, 10, mode=RRF, fetch=32, weights=np.full((5, 1), w), rrf_c=60.0)
        np.testing.assert_array_equal(got[0], ids[:, :10])
        np.testing.assert_array_equal(bits(got[1]), bits(sc[:, :10]))
        np.testing.assert_array_equal(bits(got[2]), bits(di[:, :10]))
        want = np.asarray([float(w) / (60.0 + float(r)) for r in range(1, 11)])
        np.testing.assert_array_equal(got[5], np.broadcast_to(want, (5, 10)))


def test_identical_sub_queries(oracle, lib_built):
    """every id forms a run of full length"""
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    q = np.repeat(Q[:, :1], 4, axis=1)                                  # [5, 4, 384]
    with FlatIndex(384) as idx:
        idx.add(X)
        ids, sc, di, nf = idx.search(q[:, 0], 40)
        got = idx.search_fused(q, 10, mode=MAX, fetch=10)
        np.testing.assert_array_equal(got[0], ids[:, :10])
        np.testing.assert_array_equal(bits(got[1]), bits(sc[:, :10]))
        np.testing.assert_array_equal(bits(got[2]), bits(di[:, :10]))
        assert (got[4] == 0).all() and (got[3] == 10).all()
        got = idx.search_fused(q, 10, mode=RRF, fetch=40)
        np.testing.assert_array_equal(got[0], ids[:, :10])              # the list order is kept
        assert (got[4] == 0).all()
        t = [1.0 / (60.0 + float(r)) for r in range(1, 11)]
        np.testing.assert_array_equal(got[5], np.broadcast_to(np.asarray([((x + x) + x) + x for x in t]), (5, 10)))
        same(got, fused_model(oracle, X, q, 10, mode=RRF, fetch=40), "identical sub-queries")


def test_ties(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(7)
    X, centres = tripled_corpus(rng, clusters=40, per=10, d=64)          # every row three times
    Q = requests(rng, centres, 4, 4)
    with FlatIndex(64) as idx:
        idx.add(X)
        for mode, fetch in ((MAX, 10), (MAX, 30), (RRF, 30)):
            got = idx.search_fused(Q, 10, mode=mode, fetch=fetch)
            same(got, fused_model(oracle, X, Q, 10, mode=mode, fetch=fetch), f"tripled rows, {mode}, fetch {fetch}")
        assert (np.diff(bits(got[2]).astype(np.int64), axis=1) == 0).any()   # (condition on the input: equal dists are reported)
    # two rows at mirrored ranks in two equally weighted lists: bit-equal fused, id order
    rows = np.eye(8, dtype=np.float32)
    q = np.zeros((1, 2, 8), np.float32)
    q[0, 0, :2] = (1.0, 0.5)
    q[0, 1, :2] = (0.5, 1.0)
    with FlatIndex(8) as idx:
        idx.add(rows)
        for w in (1.0, 0.3):
            got = idx.search_fused(q, 2, mode=RRF, fetch=2, weights=[[w, w]])
            assert list(got[0][0]) == [1, 2] and list(got[4][0]) == [0, 1]
            assert got[5][0, 0].tobytes() == got[5][0, 1].tobytes()
            same(got, fused_model(oracle, rows, q, 2, mode=RRF, fetch=2, weights=[[w, w]]), "mirrored pair")


@pytest.mark.parametrize("m,fetch", [(16, 256), (3, 100)], ids=["4096-entries", "300-entries"])
def test_the_limits(m, fetch, oracle, lib_built):
    """16 x 256 fills the workgroup's 4096 entries; 3 x 100 is no power of two, so the sort is padded"""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(90 + m)
    X = rng.standard_normal((5000, 32)).astype(np.float32)
    Q = (X[rng.integers(0, 5000, (3, m))] + 0.3 * rng.standard_normal((3, m, 32))).astype(np.float32)
    Q[1, m // 2:] = Q[1, : m - m // 2]                                    # one request with every list twice
    with FlatIndex(32) as idx:
        idx.add(X)
        for mode in (MAX, RRF):
            got = idx.search_fused(Q, fetch, mode=mode, fetch=fetch)
            same(got, fused_model(oracle, X, Q, fetch, mode=mode, fetch=fetch), f"m = {m}, fetch = k = {fetch}, {mode}")
            assert (got[3] == fetch).all()


@pytest.mark.parametrize("m,R", [(3, 200), (16, 40)], ids=["m=3-R=200", "m=16-R=40"])
def test_chunking(m, R, lib_built):
    """600 and 640 queries: passes of floor(512 / m) whole requests (170 and 32).  The batch equals the per-request calls."""
    from memex_amd.index import FlatIndex
    X, centres = small()
    Q = requests(np.random.default_rng(40 + m), centres, R, m)
    W = np.random.default_rng(41).integers(0, 4, (R, m)).astype(np.float32)   # ragged: some weights are 0
    with FlatIndex(64) as idx:
        idx.add(X)
        for mode in (MAX, RRF):
            got = idx.search_fused(Q, 5, mode=mode, fetch=8, weights=W)
            each = [idx.search_fused(Q[r], 5, mode=mode, fetch=8, weights=W[r:r + 1]) for r in range(R)]
            same(got, tuple(np.concatenate([e[i] for e in each]) for i in range(6)), f"m = {m}, R = {R}, {mode}")


def test_few_rows(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, centres, Q = base()
    with FlatIndex(384) as idx:
        idx.add(X[:7])
        for mode in (MAX, RRF):
            got = idx.search_fused(Q, 10, mode=mode, fetch=20)
            assert (got[3] == 7).all()
            blanks_ok(got)
            same(got, fused_model(oracle, X[:7], Q, 10, mode=mode, fetch=20), f"7 rows, {mode}")
    with FlatIndex(384) as idx:                                         # an empty index finds nothing
        got = idx.search_fused(Q, 5, mode=RRF, fetch=8)
        assert (got[3] == 0).all()
        blanks_ok(got)
    with FlatIndex(384) as idx:
        idx.add(X)
        best = int(idx.search_fused(Q[0], 1)[0][0, 0])                  # request 0's best row, and two more
        gone = np.asarray([best, int(idx.search_fused(Q[1], 1)[0][0, 0]), int(idx.search_fused(Q[2], 1)[0][0, 0])], dtype=np.uint64)
        assert len(set(gone.tolist())) == 3
        idx.remove(gone)
        alive = np.ones(len(X), dtype=bool)
        alive[gone.astype(np.int64) - 1] = False
        for mode in (MAX, RRF):
            got = idx.search_fused(Q, 10, mode=mode, fetch=40)
            assert not np.isin(got[0], gone).any()
            same(got, fused_model(oracle, X, Q, 10, mode=mode, fetch=40, alive=alive), f"removed rows, {mode}")


def test_weights(oracle, lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    W = np.asarray([[1.0, 0.25, 3.0], [0.5, 0.5, 0.5], [2.0, 1.0, 1e-3], [1.0, 7.0, 1.0], [0.1, 0.2, 0.3]], np.float32)
    with FlatIndex(384) as idx:
        idx.add(X)
        got = idx.search_fused(Q, 10, mode=RRF, fetch=40, weights=W, rrf_c=10.0)
        same(got, fused_model(oracle, X, Q, 10, mode=RRF, fetch=40, weights=W, rrf_c=10.0), "non-uniform weights")
        assert (got[0] != model(oracle, ("base", RRF), X, Q, 10, mode=RRF, fetch=40)[0]).any()      # the weights matter
        # a weight of 0 = the call without that sub-query, best_sub mapped
        W0 = np.ones((5, 3), np.float32)
        W0[:, 1] = 0
        for mode in (MAX, RRF):
            a = idx.search_fused(Q, 10, mode=mode, fetch=40, weights=W0)
            b = idx.search_fused(Q[:, [0, 2]], 10, mode=mode, fetch=40)
            same(a, b[:4] + (np.asarray([0, 2, -1], np.int32)[b[4]], b[5]), f"weight 0, {mode}")
            assert (a[4] == 2).any()
        # all weights 0: nothing found, MX_OK
        got = idx.search_fused(Q, 10, mode=RRF, fetch=40, weights=np.zeros((5, 3), np.float32))
        assert (got[3] == 0).all()
        blanks_ok(got)
        # a NaN sub-query is rejected like a plain NaN query, also under weight 0
        bad = Q.copy()
        bad[3, 1, 5] = np.nan
        with pytest.raises(_lib.MemexHipError) as plain:
            idx.search(bad[3], 10)
        with pytest.raises(_lib.MemexHipError) as fused:
            idx.search_fused(bad, 10, weights=W0)
        assert fused.value.code == plain.value.code == _lib.MX_EINVAL


def test_id_offset(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    with FlatIndex(384) as idx:
        idx.set_id_offset(77)
        idx.add(X)
        for mode in (MAX, RRF):
            got = idx.search_fused(Q, 10, mode=mode, fetch=40)
            want = model(oracle, ("base", mode), X, Q, 10, mode=mode, fetch=40)
            same(got, (np.where(want[0] != 0, want[0] + np.uint64(77), 0).astype(np.uint64),) + want[1:], f"id_offset, {mode}")
            same(got, fused_model(oracle, X, Q, 10, mode=mode, fetch=40, id_offset=77), f"id_offset vs model, {mode}")


def test_device_pointer_variant_equals_the_host_variant(lib_built):
    import torch
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    W = np.asarray([[1.0, 0.0, 2.0]] * 5, np.float32)
    with FlatIndex(384) as plain, FlatIndex(384, devices=[0, 0], block_rows=64) as sh:
        for idx in (plain, sh):
            idx.add(X)
            for mode, k, fetch, extras, w in ((MAX, 10, None, True, None), (RRF, 7, 40, True, W), (RRF, 7, None, False, None)):
                q = torch.from_numpy(Q).cuda()
                ids = torch.full((5, k), -1, dtype=torch.int64, device="cuda")
                sc = torch.full((5, k), -1.0, dtype=torch.float32, device="cuda")
                di = torch.full((5, k), -1.0, dtype=torch.float32, device="cuda") if extras else None
                best = torch.full((5, k), -7, dtype=torch.int32, device="cuda") if extras else None
                fu = torch.full((5, k), -1.0, dtype=torch.float64, device="cuda") if extras else None
                nf = torch.full((5,), -1, dtype=torch.int32, device="cuda")
                idx.search_fused_device(q, k, ids, sc, di, nf, best, fu, mode=mode, fetch=fetch, weights=w)
                h = idx.search_fused(Q, k, mode=mode, fetch=fetch, weights=w)
                np.testing.assert_array_equal(ids.cpu().numpy().astype(np.uint64), h[0])
                np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(h[1]))
                np.testing.assert_array_equal(nf.cpu().numpy(), h[3])
                if extras:
                    np.testing.assert_array_equal(bits(di.cpu().numpy()), bits(h[2]))
                    np.testing.assert_array_equal(best.cpu().numpy(), h[4])
                    np.testing.assert_array_equal(fu.cpu().numpy().view(np.uint64), h[5].view(np.uint64))


def test_sharded_equals_plain(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    gone = np.arange(200, 230)
    with FlatIndex(384) as plain, FlatIndex(384, devices=[0, 0, 0], block_rows=96) as sh:
        for idx in (plain, sh):
            idx.add(X)
            idx.remove(gone + 1)
        alive = np.ones(len(X), dtype=bool)
        alive[gone] = False
        for mode in (MAX, RRF):
            a = sh.search_fused(Q, 10, mode=mode, fetch=40)
            same(a, plain.search_fused(Q, 10, mode=mode, fetch=40), f"3 shards vs plain, {mode}")
            same(a, fused_model(oracle, X, Q, 10, mode=mode, fetch=40, alive=alive), f"3 shards vs model, {mode}")


# (name, setup)
_KINDS = [
    ("int8", lambda idx: idx.set_filter_copy("i8")),
    ("bf16", lambda idx: idx.set_filter_copy("bf16")),
    ("f32", lambda idx: idx.set_filter_copy(False)),
    ("compressed", "compressed"),
    ("exact", "exact"),
]


@pytest.mark.parametrize("name,setup", _KINDS, ids=[c[0] for c in _KINDS])
def test_every_copy_kind_and_mode_matches_the_model(name, setup, oracle, lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    X, _, Q = base()
    with FlatIndex(384) as idx:
        if setup == "compressed":
            idx.set_corpus_mode("bf16")
        idx.add(X)
        if callable(setup):
            setup(idx)
        if setup == "exact":
            idx.set_search_mode(_lib.MX_SEARCH_EXACT)
        rows = idx.get_rows(0, len(X)) if setup == "compressed" else X
        assert setup != "compressed" or (rows != X).any()              # the model is fed what the index stores
        for mode in (MAX, RRF):
            want = model(oracle, ("kind", setup == "compressed", mode), rows, Q[:3], 10, mode=mode, fetch=16)
            same(idx.search_fused(Q[:3], 10, mode=mode, fetch=16), want, f"{name}, {mode}")


def test_store_and_tasks(oracle, lib_built, tmp_path):
    from memex_amd import storage, tasks
    rng = np.random.default_rng(63)
    X, centres = near_copy_corpus(rng, clusters=12, per=8, d=64)
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    st.bulk_insert([storage.VectorData(_id=f"s{i}", document_id=f"d{i // 8}", text="", vector=list(map(float, v))) for i, v in enumerate(X)])
    q = requests(rng, centres, 1, 3)[0]
    vecs = [list(map(float, v)) for v in q]
    names = [f"s{i}" for i in range(len(X))]

    def expect(rows, names, k, mode, **kw):
        ids, sc, _, nf, _, _ = fused_model(oracle, rows, q, k, mode=mode, **kw)
        return [(names[int(i) - 1], float(s)) for i, s in zip(ids[0, :nf[0]], sc[0, :nf[0]])]

    assert st.search_fused(vecs, 6) == expect(X, names, 6, MAX)
    assert st.search_fused(vecs, 6, mode="rrf") == expect(X, names, 6, RRF)
    assert st.search_fused(vecs, 6, mode="rrf", fetch=12, weights=[1.0, 0.0, 2.0]) == expect(X, names, 6, RRF, fetch=12, weights=[[1.0, 0.0, 2.0]])
    gone = st.search_fused(vecs, 1)[0][0]                                # the best segment of the request
    st.remove([gone])
    alive = np.asarray([n != gone for n in names])
    after = st.search_fused(vecs, 6)
    assert gone not in [n for n, _ in after]
    assert after == expect(X, names, 6, MAX, alive=alive)
    assert storage.VectorStorage(st).search_fused(vecs, 6) == after

    class Hit:
        def __init__(self, v):
            self.vector = v

    class Embedder:                                                     # text -> one of the request's vectors
        def encode_single(self, text):
            return Hit(vecs[int(text)]) if text else None

    assert tasks.search_docs_multi(storage.VectorStorage(st), Embedder(), ["0", "1", "2"], limit=6) == after
    assert tasks.search_docs_multi(st, Embedder(), ["0", "1", "2"], limit=6, mode="rrf") == st.search_fused(vecs, 6, mode="rrf")
    with pytest.raises(ValueError, match="Invalid query"):
        tasks.search_docs_multi(st, Embedder(), ["0", ""], limit=6)


def test_concurrent_callers_beside_an_appender(oracle, lib_built):
    """two threads issue fused searches while a third appends: every answer equals the model for SOME prefix of the corpus"""
    from memex_amd.index import FlatIndex
    X, centres = small()
    rng = np.random.default_rng(77)
    jobs = [(requests(rng, centres, 4, 3), 5, MAX, 8), (requests(rng, centres, 3, 4), 6, RRF, 16)]
    prefixes = [800, 1200, 1600, 2000]
    want = [[fused_model(oracle, X[:n], Q, k, mode=mode, fetch=fetch) for n in prefixes] for Q, k, mode, fetch in jobs]
    with FlatIndex(64) as idx:
        idx.add(X[:prefixes[0]])
        got = [[] for _ in jobs]
        errs = []

        def search(i):
            Q, k, mode, fetch = jobs[i]
            try:
                for _ in range(6):
                    got[i].append(idx.search_fused(Q, k, mode=mode, fetch=fetch))
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        def append():
            try:
                for a, b in zip(prefixes[:-1], prefixes[1:]):
                    idx.add(X[a:b])
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=search, args=(i,)) for i in range(len(jobs))] + [threading.Thread(target=append)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        for i in range(len(jobs)):
            assert len(got[i]) == 6
            for g in got[i]:
                ok = [all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(g, w))
                      for w in want[i]]
                assert any(ok), f"job {i}: an answer matches no prefix of the corpus"
        # the last state is the whole corpus
        for i, (Q, k, mode, fetch) in enumerate(jobs):
            same(idx.search_fused(Q, k, mode=mode, fetch=fetch), want[i][-1], f"job {i} after the appends")
