"""Search by examples (mx_index_search_like) on the GPU against its contract.  Every case checks three things,
all by integer equality on ids, score bits, dist bits and counts:

  1. ``combined`` is bit-equal to tests/like_model.py fed with ``get_rows`` (the blend's arithmetic),
  2. the lists equal ``idx.search(combined, k + E)`` with the used examples dropped and cut to k (the drop kernel),
  3. the ids equal the oracle's brute force over the live rows minus the used examples (so the check does not rest on the code
     under test).

The corpus is clusters of near-copies (tests/mmr_model.py), as in test_by_id_gpu.py: every row has near-copies, so examples and
their neighbours crowd the head of every list."""
import threading

import numpy as np
import pytest

from conftest import bits
from like_model import drop_examples, like_combined
from mmr_model import near_copy_corpus
from test_mmr_gpu import _KINDS

pytestmark = pytest.mark.gpu

_CACHE = {}


def corpus(d=384, clusters=150):
    key = (d, clusters)
    if key not in _CACHE:
        _CACHE[key] = near_copy_corpus(np.random.default_rng(2000 + d + clusters), clusters=clusters, d=d)[0]
    return _CACHE[key]


def same(got, want, what):
    names = ("ids", "scores", "dists", "n_found", "n_used", "combined")
    assert len(got) == len(want)
    for g, w, n in zip(got, want, names):
        if n in ("scores", "dists", "combined"):
            g, w = bits(g), bits(w)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {n}")


def check(idx, oracle, ex, k, w=None, q=None, qw=None, e=True, off=0, dead=(), what=""):
    """one search_like call against the three checks -> (what it returned, the used-example mask)"""
    ex = np.asarray(ex, dtype=np.uint64)
    ex = ex[None, :] if ex.ndim == 1 else ex
    R, m = ex.shape
    got = idx.search_like(ex, k, w, q, qw, exclude_examples=e)
    n = len(idx)
    rows = idx.get_rows(0, n) if n else np.zeros((0, idx.dim), np.float32)
    alive = np.ones(n, bool)
    alive[np.asarray(dead, dtype=np.int64) - off - 1] = False
    rows_of = lambda i: rows[i - off - 1] if off < i <= off + n and alive[i - off - 1] else None  # noqa: E731
    comb, used, n_used = like_combined(rows_of, ex, w, q, qw, dim=idx.dim)
    np.testing.assert_array_equal(bits(got[5]), bits(comb), err_msg=f"{what}: combined")                 # 1
    np.testing.assert_array_equal(got[4], n_used, err_msg=f"{what}: n_used")
    E = m if e else 0
    want = drop_examples(idx.search(comb, k + E), ex, used, comb, k, e)                                  # 2
    same(got[:4], want, what)
    row_ids = np.arange(n, dtype=np.uint64) + np.uint64(off + 1)
    for r in range(R):                                                                                   # 3
        if not comb[r].any():
            assert got[3][r] == 0 and not got[0][r].any() and np.isposinf(got[2][r]).all(), f"{what}: blank request {r}"
            continue
        gone = ex[r][used[r]] if e else np.zeros(0, np.uint64)
        keep = np.flatnonzero(alive & ~np.isin(row_ids, gone))
        oi, _, _, onf = oracle.search(rows[keep], comb[r], k)
        assert got[3][r] == onf[0] == min(k, len(keep)), f"{what}: request {r}"
        np.testing.assert_array_equal(got[0][r, :onf[0]], row_ids[keep[oi[0, :onf[0]].astype(np.int64) - 1]], err_msg=f"{what}: oracle, request {r}")
        assert not e or not np.isin(got[0][r], gone).any()
    return got, used


def requests(n, R, m, seed, signed=True):
    """R requests of m distinct example ids across 1 .. n (the first and the last row among them), weights of both signs"""
    rng = np.random.default_rng(seed)
    ex = np.stack([rng.choice(np.arange(1, n + 1), m, replace=False) for _ in range(R)]).astype(np.uint64) if R else np.zeros((0, m), np.uint64)
    if R:
        ex[0, 0], ex[-1, -1] = 1, n
    w = rng.uniform(0.25, 2.0, (R, m)).astype(np.float32)
    if signed:
        w[:, 1::2] *= np.float32(-0.5)
    return ex, w


@pytest.mark.parametrize("name,d,clusters,setup", _KINDS, ids=[c[0] for c in _KINDS])
def test_every_copy_kind(name, d, clusters, setup, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus(d, clusters)
    with FlatIndex(d) as idx:
        if setup == "compressed":
            idx.set_corpus_mode("bf16")
        idx.add(X)
        if callable(setup):
            setup(idx)
        ex, w = requests(len(X), 37, 2, 31)
        q = X[np.random.default_rng(32).integers(0, len(X), 37)] * np.float32(3.0)
        check(idx, oracle, ex, 10, w, what=f"{name}, examples")
        got, used = check(idx, oracle, ex, 10, w, q, np.float32(0.8), what=f"{name}, examples and a caller vector")
        assert used.all() and (got[3] == 10).all()


@pytest.mark.parametrize("d", [384, 130, 3])
def test_dims_and_example_counts(d, oracle, lib_built):
    """dim 130 and 3: rows of the blocks are not 16-byte aligned (element stores); m = 1, 2 and the most a request may have"""
    from memex_amd.index import FlatIndex
    X = corpus(d, 150)
    with FlatIndex(d) as idx:
        idx.add(X)
        for m in (1, 2, 16):
            ex, w = requests(len(X), 37, m, 40 + m)
            check(idx, oracle, ex, 10, w, what=f"dim {d}, m = {m}")
        ex, w = requests(len(X), 1, 2, 43)
        check(idx, oracle, ex[0], 10, w[0], what=f"dim {d}, one request given as [m]")
        got = idx.search_like(np.zeros((0, 2), np.uint64), 10)
        assert [a.shape for a in got] == [(0, 10), (0, 10), (0, 10), (0,), (0,), (0, d)]


def test_two_passes(oracle, lib_built):
    """R = 33 with m = 16: passes of 32 and 1 requests"""
    from memex_amd.index import FlatIndex
    X = corpus()
    with FlatIndex(384) as idx:
        idx.add(X)
        ex, w = requests(len(X), 33, 16, 51)
        q = X[np.random.default_rng(52).integers(0, len(X), 33)]
        got, _ = check(idx, oracle, ex, 10, w, q, what="R = 33, m = 16")
        one, _ = check(idx, oracle, ex[32:], 10, w[32:], q[32:], what="the last request alone")
        same([a[32:] for a in got], one, "second pass")


def head_examples(X, idx):
    """16 examples, four from each of four clusters, the clusters weighted 1, 0.8, 0.6, 0.4: the list starts with the 80 rows of those
    clusters, cluster by cluster, so the examples sit in every 20-entry stretch of the first 80 entries"""
    ex = np.array([[c * 20 + j for c in (3, 50, 97, 140) for j in (1, 7, 13, 20)]], dtype=np.uint64)
    w = np.repeat(np.array([1.0, 0.8, 0.6, 0.4], np.float32), 4)[None, :]
    comb = idx.search_like(ex, 1, w)[5]
    pos = np.flatnonzero(np.isin(idx.search(comb, 129)[0][0], ex[0]))
    assert len(pos) == 16 and pos.min() < 20 and pos.max() >= 64, pos                # (condition on the inputs)
    return ex, w


@pytest.mark.parametrize("kk", [64, 65, 129])
def test_compaction_across_chunks(kk, oracle, lib_built):
    """positives only, k + E = 64, 65 and 129: examples are dropped at the head of the list and on both sides of a 64-entry chunk"""
    from memex_amd.index import FlatIndex
    X = corpus()
    with FlatIndex(384) as idx:
        idx.add(X)
        ex, w = head_examples(X, idx)
        got, used = check(idx, oracle, ex, kk - 16, w, what=f"k + E = {kk}")
        assert used.all() and got[3][0] == kk - 16


def test_wide_list_takes_the_exact_path(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    with FlatIndex(384) as idx:
        idx.add(X)
        ex, w = requests(len(X), 3, 16, 61)
        hx, hw = head_examples(X, idx)
        ex[0], w[0] = hx[0], hw[0]
        got, _ = check(idx, oracle, ex, 250, w, what="k = 250, m = 16")             # the pass runs at k = 266
        assert (got[3] == 250).all()


def test_negatives_only_and_kept_examples(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    with FlatIndex(384) as idx:
        idx.add(X)
        ex, w = requests(len(X), 5, 4, 71, signed=False)
        got, used = check(idx, oracle, ex, 10, -w, what="negatives only")
        assert used.all()
        comb = got[5]
        same(got[:4], idx.search(comb, 10), "no example is listed: the plain list, cut")
        check(idx, oracle, ex, 10, w, e=False, what="exclude_examples = 0")         # the plain list of the blend, cut to k


def test_special_requests_in_one_pass(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus().copy()
    X[107] = 0                                                    # id 108: a zero row
    rng = np.random.default_rng(81)
    with FlatIndex(384) as idx:
        idx.add(X)
        ex = np.array([[500, 500, 1200],                          # 0: an id twice -- it counts twice and is dropped once
                       [500, 500, 0],                             # 1: a row as +w and -w: blank
                       [7, 2999, 1500],                           # 2: an ordinary request between the blank ones
                       [108, 640, 641],                           # 3: a zero-row example is skipped
                       [1, 2, 3],                                 # 4: the caller vector alone, every slot absent
                       [1, 2, 3],                                 # 5: ... a caller vector of zeros: blank
                       [900, 901, 2000],                          # 6: caller vector and examples
                       [108, 108, 108]], dtype=np.uint64)         # 7: nothing but the zero row: blank
        w = np.array([[1, 1, 1], [0.5, -0.5, 0], [1, -0.25, 1], [1, 1, -0.5], [0, 0, 0], [0, 0, 0], [0.75, 0.75, -0.15], [1, 1, 1]], np.float32)
        q = rng.standard_normal((8, 384)).astype(np.float32)
        q[5] = 0
        qw = np.array([0, 0, 0, 0, 1, 1, 1, 0], np.float32)       # (a caller weight of 0: no caller term)
        for e in (True, False):
            got, used = check(idx, oracle, ex, 10, w, q, qw, e=e, what=f"special requests, exclude = {e}")
            np.testing.assert_array_equal(got[4], [3, 2, 3, 2, 0, 0, 3, 0])
            np.testing.assert_array_equal(got[3], [10, 0, 10, 10, 10, 0, 10, 0])
            assert not got[5][[1, 5, 7]].any()
        both, _ = check(idx, oracle, ex[:1], 10, w[:1], what="duplicate id")
        once, _ = check(idx, oracle, ex[:1, 1:], 10, np.array([[2, 1]], np.float32), what="the same row once, at twice the weight")
        np.testing.assert_array_equal(both[0], once[0])           # (2 * u and u + u are the same f64 value)
        same(check(idx, oracle, ex[4:5], 10, w[4:5], q[4:5], what="caller alone")[0][:4], idx.search(got[5][4:5], 10), "caller alone == search")


def test_nan_caller_vector_is_rejected_as_search_rejects_it(lib_built):
    import torch
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    X = corpus()
    with FlatIndex(384) as idx:
        idx.add(X)
        q = X[:2].copy()
        q[1, 5] = np.nan
        with pytest.raises(_lib.MemexHipError) as plain:
            idx.search(q, 10)
        with pytest.raises(_lib.MemexHipError) as host:
            idx.search_like([[1, 2], [3, 4]], 10, queries=q)
        dq = torch.from_numpy(q).cuda()
        with pytest.raises(_lib.MemexHipError) as plain_dev:
            idx.search_device(dq, 10, *_outputs(2, 10, 384)[:4])
        with pytest.raises(_lib.MemexHipError) as dev:
            ids, sc, di, nf, nu, cb = _outputs(2, 10, 384)
            idx.search_like_device([[1, 2], [3, 4]], 10, ids, sc, di, nf, nu, cb, queries=dq)
        assert host.value.code == plain.value.code == _lib.MX_EINVAL and dev.value.code == plain_dev.value.code == _lib.MX_EINVAL
        assert idx.search_like([[1, 2], [3, 4]], 10, queries=X[:2])[3].tolist() == [10, 10]      # the index is fine afterwards


def _outputs(R, k, d, dists=True):
    import torch
    return (torch.full((R, k), -1, dtype=torch.int64, device="cuda"), torch.full((R, k), -1.0, dtype=torch.float32, device="cuda"),
            torch.full((R, k), -1.0, dtype=torch.float32, device="cuda") if dists else None,
            torch.full((R,), -1, dtype=torch.int32, device="cuda"), torch.full((R,), -1, dtype=torch.int32, device="cuda"),
            torch.full((R, d), -1.0, dtype=torch.float32, device="cuda"))


def test_dead_and_invalid_ids_and_id_offset(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    n = len(X)
    with FlatIndex(384) as idx:
        idx.add(X)
        gone = np.array([41, 42, 900, 2999], dtype=np.uint64)
        idx.remove(gone)
        ex = np.array([[7, 41, 0, 8], [n + 1, 2999, 43, 2 ** 40], [n, 900, 42, 41], [41, 42, 900, 2999]], dtype=np.uint64)
        w = np.array([[1, 1, 1, -0.5]] * 4, np.float32)
        for e in (True, False):
            got, used = check(idx, oracle, ex, 10, w, dead=gone, e=e, what=f"dead ids, exclude = {e}")
            np.testing.assert_array_equal(got[4], [2, 1, 1, 0])
            np.testing.assert_array_equal(got[3], [10, 10, 10, 0])
            assert not np.isin(got[0], gone).any()
        before, _ = check(idx, oracle, [43, 901, n], 10, dead=gone, what="before compact")
        kept = idx.compact()
        new = np.array([int(np.flatnonzero(kept == i)[0]) + 1 for i in (43, 901, n)], dtype=np.uint64)
        after, _ = check(idx, oracle, new, 10, what="compacted")
        np.testing.assert_array_equal(kept[after[0].astype(np.int64) - 1], before[0])
        np.testing.assert_array_equal(bits(after[5]), bits(before[5]))
    with FlatIndex(384) as idx:                                   # results and example ids shift together
        idx.set_id_offset(1000)
        idx.add(X)
        ex = np.array([[1000, 1001], [1000 + n, 1001 + n], [5, 1500], [1, 2]], dtype=np.uint64)
        got, _ = check(idx, oracle, ex, 10, off=1000, what="id_offset")
        np.testing.assert_array_equal(got[4], [1, 1, 1, 0])
        assert (got[0][got[0] != 0] > 1000).all()
    with FlatIndex(384) as idx:                                   # an empty index finds nothing
        got = idx.search_like([[1, 2]], 3)
        assert got[3][0] == 0 and got[4][0] == 0 and not got[0].any() and not got[5].any()


def test_sharded_equals_plain(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    gone = np.arange(200, 230, dtype=np.uint64)
    with FlatIndex(384) as plain, FlatIndex(384, devices=[0, 0, 0], block_rows=96) as sh:
        for idx in (plain, sh):
            idx.set_id_offset(77)
            idx.add(X)
            idx.remove(gone + np.uint64(78))
        ex, w = requests(len(X), 37, 4, 91)
        ex += np.uint64(77)
        shard = ((ex.astype(np.int64) - 78) // 96) % 3
        assert len(set(shard.ravel())) == 3 and any(len(set(r)) == 3 for r in shard)     # examples on every shard, also of one request
        ex[5, 2], ex[6, 0] = 77 + 210, 3                                                 # a removed row, an id below the offset
        q = X[np.random.default_rng(92).integers(0, len(X), 37)]
        for e in (True, False):
            a = sh.search_like(ex, 10, w, q, exclude_examples=e)
            same(a, plain.search_like(ex, 10, w, q, exclude_examples=e), f"3 shards vs plain, exclude = {e}")
        check(plain, oracle, ex, 10, w, q, off=77, dead=gone + np.uint64(78), what="plain vs model")


def test_exact_copies_of_an_example_stay(oracle, lib_built):
    """40 copies of one new row: the example goes, its copies stay and keep their id order"""
    from memex_amd.index import FlatIndex
    X = corpus()
    v = np.random.default_rng(7).standard_normal(384).astype(np.float32)
    with FlatIndex(384) as idx:
        idx.add(X)
        first = idx.add(np.repeat(v[None, :], 40, axis=0))
        ex = np.array([[first + 5], [first + 39], [first]], dtype=np.uint64)
        got, _ = check(idx, oracle, ex, 10, what="ties")
        np.testing.assert_array_equal(got[0][0], [first + j for j in range(11) if j != 5])      # entry 5 of the 11 listed is dropped
        np.testing.assert_array_equal(got[0][1], np.arange(first, first + 10))                  # the last copy is not among the 11
        np.testing.assert_array_equal(got[0][2], np.arange(first + 1, first + 11))
        got, _ = check(idx, oracle, [[first + 5, first + 6, first + 39]], 38, what="ties, three examples")
        assert got[3][0] == 38                                                              # 37 copies and one other row
        np.testing.assert_array_equal(got[0][0, :37], [first + j for j in range(40) if j not in (5, 6, 39)])


def test_device_variant_equals_the_host_variant(lib_built):
    import torch
    from memex_amd.index import FlatIndex
    X = corpus()
    ex, w = requests(len(X), 37, 3, 95)
    q = X[np.random.default_rng(96).integers(0, len(X), 37)]
    with FlatIndex(384) as plain, FlatIndex(384, devices=[0, 0], block_rows=64) as sh:
        for idx in (plain, sh):
            idx.add(X)
            for k, full in ((10, True), (7, False)):
                ids, sc, di, nf, nu, cb = _outputs(37, k, 384, dists=full)
                dq = torch.from_numpy(q).cuda() if full else None
                idx.search_like_device(ex, k, ids, sc, di, nf, nu if full else None, cb if full else None, weights=w, queries=dq,
                                       query_weights=0.5 if full else None)
                h = idx.search_like(ex, k, w, q if full else None, 0.5 if full else None)
                dev = [ids.cpu().numpy().astype(np.uint64), sc.cpu().numpy(), di.cpu().numpy() if full else h[2], nf.cpu().numpy(),
                       nu.cpu().numpy() if full else h[4], cb.cpu().numpy() if full else h[5]]
                same(dev, h, f"device variant, k = {k}")


def test_store_search_like_after_remove_and_compact(lib_built, tmp_path):
    from memex_amd import storage
    X = near_copy_corpus(np.random.default_rng(63), clusters=12, per=8, d=64)[0]
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    names = [f"s{i}" for i in range(len(X))]
    names[21] = "s20"                                            # one _id inserted twice (rows 20 and 21 of cluster 2)
    st.bulk_insert([storage.VectorData(_id=nm, document_id=f"d{i // 8}", text="", vector=list(map(float, v)))
                    for i, (nm, v) in enumerate(zip(names, X))])
    vec = X[40] * np.float32(2.0)

    def expect(pos_rows, neg_rows, limit, q=None):
        """the store's Rocchio weights through the index call, ids -> names"""
        ex = np.array(pos_rows + neg_rows, dtype=np.uint64)
        w = np.array([np.float32(0.75) / np.float32(len(pos_rows))] * len(pos_rows) +       # f32 divisions of the f32 parameters
                     [-np.float32(0.15) / np.float32(len(neg_rows))] * len(neg_rows), np.float32)
        ids, sc, _, nf, nu, _ = st._index.search_like(ex, limit, w, q, None if q is None else 1.0)
        return [(st._id_map[int(i)], float(s)) for i, s in zip(ids[0, :nf[0]], sc[0, :nf[0]])], int(nu[0])
    got = st.search_like(["s20", "s16", "nobody"], ["s90"], 5)
    assert got == expect([21, 22, 17], [91], 5)[0] and len(got) == 5
    assert {g[0] for g in got} <= {f"s{i}" for i in (17, 18, 19, 22, 23)}             # the rest of cluster 2, the examples left out
    with_vec = st.search_like(["s20"], ["s90"], 5, vec=list(map(float, vec)))
    assert with_vec == expect([21, 22], [91], 5, vec)[0] and with_vec != got
    assert st.search_like(["nobody"], [], 5) == [] and st.search_like(["s20"], limit=0) == []
    assert [g[0] for g in st.search_like([], [], 3, vec=list(map(float, X[40])))] == [g[0] for g in st.search(list(map(float, X[40])), 3)]
    with pytest.raises(ValueError):
        st.search_like([f"s{i}" for i in range(30, 47)], [], 5)
    st.remove(["s16", "s17"])
    after = st.search_like(["s20", "s16"], ["s90"], 5)
    want, n_used = expect([21, 22, 17], [91], 5)
    assert after == want and n_used == 3 and "s17" not in [g[0] for g in after]       # the removed example no longer takes part
    live = st.search_like(["s20"], ["s90"], 5, vec=list(map(float, vec)))
    st.compact()
    assert st.search_like(["s20"], ["s90"], 5, vec=list(map(float, vec))) == live     # the same rows under new ids: the same names and scores
    assert [g[0] for g in st.search_like(["s20", "s16"], ["s90"], 5)] == [g[0] for g in after]   # (s16 now names nothing)


def test_search_like_beside_add_remove_and_compact(oracle, lib_built):
    """one thread loops search_like while another appends, removes and compacts: every answer is the answer of ONE state the index went
    through (the call holds the index from the id translation to its last kernel), and nothing raises"""
    from memex_amd.index import FlatIndex
    X = corpus()
    extra = near_copy_corpus(np.random.default_rng(71), clusters=5, d=384)[0]
    ex, w = requests(len(X), 12, 3, 97)
    gone = np.unique(np.r_[ex[3, 0], ex[7, 1], np.arange(500, 700, dtype=np.uint64)])

    def steps(idx):
        yield
        idx.add(extra)
        yield
        idx.remove(gone)
        yield
        idx.compact()
        yield

    with FlatIndex(384) as ref:                                   # every state, checked on a quiet index
        ref.add(X)
        states = []
        for i, _ in enumerate(steps(ref)):
            states.append(check(ref, oracle, ex, 10, w, dead=gone if i == 2 else (), what=f"state {i}")[0])
    assert len(states) == 4

    def which(ans):
        for i, s in enumerate(states):
            if all(np.array_equal(a, b) if a.dtype.kind in "ui" else np.array_equal(bits(a), bits(b)) for a, b in zip(ans, s)):
                return i
        return -1

    with FlatIndex(384) as idx:
        idx.add(X)
        answers, errs = [], []
        done, tick = threading.Event(), threading.Event()

        def searcher():
            try:
                while True:
                    last = done.is_set()
                    answers.append(idx.search_like(ex, 10, w))
                    tick.set()
                    if last:
                        return
            except Exception as e:  # noqa: BLE001
                errs.append(e)
            finally:
                tick.set()

        def mutator():
            try:
                for _ in steps(idx):
                    tick.clear()
                    tick.wait(30)                               # an answer lands between any two mutations
            except Exception as e:  # noqa: BLE001
                errs.append(e)
            finally:
                done.set()

        ths = [threading.Thread(target=searcher), threading.Thread(target=mutator)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        seen = [which(a) for a in answers]
        assert answers and min(seen) >= 0, seen
        assert seen == sorted(seen) and seen[-1] == 3            # states are passed in order; the last answer is the final state's
