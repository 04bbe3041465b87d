"""Scoring of named rows (mx_index_score_ids) on the GPU.  The reference of every case is the plain call on the same index:
``idx.search(q, k=len(idx))`` lists every live row with a defined dist, so an entry is found iff its id is in that list, and then holds
that list's score and dist; ``order`` is the found positions sorted by (place in the plain list, position).  Every comparison is integer
equality on score bits, dist bits, order and counts.  The corpora stay at or below 4096 rows, the ABI's cap on k."""
import ctypes
import threading

import numpy as np
import pytest

from conftest import bits
from mmr_model import near_copy_corpus
from score_ids_model import from_plain_lists
from test_mmr_gpu import _KINDS

pytestmark = pytest.mark.gpu

_CACHE = {}
INF_BITS = 0x7F800000


def corpus(d=384, clusters=150):
    key = (d, clusters)
    if key not in _CACHE:
        _CACHE[key] = near_copy_corpus(np.random.default_rng(4100 + d + clusters), clusters=clusters, d=d)[0]
    return _CACHE[key]


def queries(X, B, seed):
    """half of them perturbed stored rows, half Gaussian"""
    rng = np.random.default_rng(seed)
    near = X[rng.integers(0, len(X), B // 2)] * (1.0 + 0.05 * rng.standard_normal((B // 2, X.shape[1])))
    return np.concatenate([near, rng.standard_normal((B - B // 2, X.shape[1]))]).astype(np.float32)


def lists(n, B, m, seed, off=0, specials=True):
    """m ids per query drawn across all n ids; with specials one repeated id, one id 0, one id n + 1 and one id 2**63 in each list"""
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, n, (B, m)) + 1 + off).astype(np.uint64)
    if specials:
        assert m >= 8
        for b in range(B):
            at = rng.permutation(m)[:5]
            a[b, at[0]] = a[b, at[1]]
            a[b, at[2]] = 0
            a[b, at[3]] = n + 1 + off
            a[b, at[4]] = 2 ** 63
    return a


def expected(idx, Q, ids, off=0):
    """(scores, dists, order, n_found) from the plain search of the same index"""
    cache = idx.__dict__.setdefault("_plain_lists", {})                    # computed once per state of the index, kept on the object
    key = (Q.tobytes(), off, len(idx), idx.removed)
    if key not in cache:
        cache[key] = idx.search(Q, len(idx))
    pnf = cache[key][3]
    n = len(idx)
    for b in range(ids.shape[0]):
        assert pnf[b] == n - idx.removed                                   # every live row has a defined dist in these corpora
    return from_plain_lists(cache[key], n, ids, off)


def same(got, want, what):
    for g, w, nm in zip(got, want, ("scores", "dists", "order", "n_found")):
        if g is None:
            continue
        if g.dtype == np.float32:
            g, w = bits(g), bits(w)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {nm}")


def check(idx, Q, ids, what, off=0):
    got = idx.score_ids(Q, ids)
    want = expected(idx, Q, np.asarray(ids, np.uint64), off)
    same(got, want, what)
    blank = got[2].shape[1] - got[3]                                       # blanks are where they must be
    assert ((bits(got[1]) == INF_BITS) & (bits(got[0]) == 0)).sum(axis=1).tolist() == blank.tolist(), what
    return got


def raw(idx, Q, ids, dists=True, order=True, nf=True):
    """the host entry point itself, with NULL for the outputs that are not wanted"""
    from memex_amd._lib import check as ok, lib
    Q = np.ascontiguousarray(Q, np.float32)
    ids = np.ascontiguousarray(ids, np.uint64)
    B, m = ids.shape
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                        # noqa: E731
    sc = np.full((B, m), -1, np.float32)
    di = np.full((B, m), -1, np.float32) if dists else None
    od = np.full((B, m), -7, np.int32) if order else None
    n = np.full(B, -7, np.int32) if nf else None
    ok(lib().mx_index_score_ids(idx._h, p(Q), B, p(ids), m, p(sc), p(di) if dists else None, p(od) if order else None, p(n) if nf else None))
    return sc, di, od, n


@pytest.mark.parametrize("name,d,clusters,setup", _KINDS, ids=[c[0] for c in _KINDS])
def test_every_copy_kind(name, d, clusters, setup, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus(d, clusters)
    Q = queries(X, 37, 11)
    ids = lists(len(X), 37, 64, 12)
    with FlatIndex(d) as idx:
        if setup == "compressed":
            idx.set_corpus_mode("bf16")
        idx.add(X)
        if callable(setup):
            setup(idx)
        idx.reset_stats()
        got = idx.score_ids(Q, ids)
        st = idx.stats()
        assert st.searches == 0 and st.queries == 0                        # the call is not a search pass
        same(got, expected(idx, Q, ids), name)
        assert (got[3] >= 64 - 4).all() and (got[3] <= 64 - 3).all()       # id 0, n + 1 and 2**63 are blank (the repeat may hit one)
        check(idx, Q, ids, name)


def test_against_the_oracle_directly(lib_built):
    """one anchor that does not pass through the library's own search: DistCosine in NumPy on the rows as stored"""
    from memex_amd.index import SEARCH_EXACT, FlatIndex
    from oracle.search_oracle import dist_cosine_np, score_from_dist
    X = corpus()
    Q = queries(X, 20, 21)
    ids = lists(len(X), 20, 8, 22, specials=False)
    with FlatIndex(384) as idx:
        idx.add(X)
        rows = idx.get_rows(0, len(X))
        sc, di, order, nf = idx.score_ids(Q, ids)
        for b in range(20):
            d = dist_cosine_np(Q[b], rows[int(ids[b, 3]) - 1])
            assert bits(di[b, 3]) == bits(d) and bits(sc[b, 3]) == bits(score_from_dist(d)), b
        assert (nf == 8).all()
        idx.set_search_mode(SEARCH_EXACT)                                  # no dependence on the search mode
        same(idx.score_ids(Q, ids), (sc, di, order, nf), "EXACT mode")


@pytest.mark.parametrize("B,m,rows", [(5, 1, 3000), (5, 1025, 3000), (3, 4096, 3000), (513, 8, 500)], ids=["m=1", "m=1025", "m=4096", "B=513"])
def test_shapes_at_the_kernels_edges(B, m, rows, lib_built):
    """one id; one more than the workgroup; the cap, with repeats (4096 draws from 3000 ids); two passes of 512 and 1 queries"""
    from memex_amd.index import FlatIndex
    X = corpus()[:rows]
    Q = queries(X, B, 31)
    ids = lists(len(X), B, m, 32, specials=m >= 8)
    with FlatIndex(384) as idx:
        idx.add(X)
        got = check(idx, Q, ids, f"B = {B}, m = {m}")
        if m == 4096:
            assert all(len(set(r)) < m for r in ids.tolist()) and (got[3] > 3000).all()


def test_blank_lists_and_null_outputs(lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    Q = queries(X, 6, 41)
    ids = lists(len(X), 6, 40, 42)
    ids[2] = [0, len(X) + 1, 2 ** 63, 2 ** 64 - 1] * 10                    # a list of blanks only
    with FlatIndex(384) as idx:
        idx.add(X)
        full = check(idx, Q, ids, "blank list")
        assert full[3][2] == 0 and (full[2][2] == -1).all() and not full[0][2].any()
        for kw in (dict(order=False), dict(dists=False), dict(nf=False), dict(dists=False, order=False, nf=False)):
            same(raw(idx, Q, ids, **kw), full, str(kw))
        sc, di, order, nf = idx.score_ids(Q[:2], [[5, 7, 9], [11]])        # ragged lists are padded with id 0
        assert nf.tolist() == [3, 1] and order[1].tolist() == [0, -1, -1] and bits(di[1, 1:]).tolist() == [INF_BITS] * 2


def test_ties_order_by_id_then_position(lib_built):
    """40 exact copies of one vector, that vector as the query: dist bits 0 everywhere, order by id, a repeated id by position"""
    from memex_amd.index import FlatIndex
    X = corpus()[:500]
    v = np.random.default_rng(7).standard_normal(384).astype(np.float32)
    with FlatIndex(384) as idx:
        idx.add(X)
        first = idx.add(np.repeat(v[None, :], 40, axis=0))
        c = (first + np.random.default_rng(8).permutation(40)).astype(np.uint64)
        c[10] = c[30]                                                      # one id twice: positions 10 and 30
        sc, di, order, nf = check(idx, v[None, :], c[None, :], "ties")
        assert nf[0] == 40 and not bits(di).any() and (sc == 1.0).all()
        ranked = c[order[0]]
        assert (np.diff(ranked.astype(np.int64)) >= 0).all()
        at = np.flatnonzero(ranked == c[10])
        assert order[0, at].tolist() == [10, 30]


def test_removed_rows_compaction_and_id_offset(lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    Q = queries(X, 9, 51)
    ids = lists(len(X), 9, 64, 52)
    gone = np.unique(np.r_[ids[0, :3], ids[4, 10], np.arange(700, 760, dtype=np.uint64)])
    gone = gone[(gone >= 1) & (gone <= len(X))]
    ids[1, :8] = gone[:8]
    with FlatIndex(384) as idx:
        idx.add(X)
        before = idx.score_ids(Q, ids)
        idx.remove(gone)
        got = check(idx, Q, ids, "removed rows")
        dead = np.isin(ids, gone)
        assert dead.sum() >= 8 and (bits(got[1])[dead] == INF_BITS).all() and (got[0][dead] == 0).all()
        np.testing.assert_array_equal(bits(got[0])[~dead], bits(before[0])[~dead])
        kept = idx.compact()                                               # the renumbered ids against the new plain search
        assert len(idx) == len(X) - len(gone) and len(kept) == len(idx)
        new_ids = lists(len(idx), 9, 64, 53)
        check(idx, Q, new_ids, "after compact")
        idx.set_id_offset(1000)
        shifted = new_ids.copy()
        real = (new_ids >= 1) & (new_ids <= len(idx))
        shifted[real] += np.uint64(1000)
        a = check(idx, Q, shifted, "id offset", off=1000)
        b = check(idx, Q, new_ids, "ids below the offset", off=1000)
        assert a[3].min() >= 60 and (b[3] == np.isin(new_ids, np.arange(1001, len(idx) + 1001)).sum(axis=1)).all()


def test_special_rows_and_the_zero_query(lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()[:500]
    rng = np.random.default_rng(61)
    special = np.stack([np.zeros(384, np.float32), X[3] * np.float32(1e-20), X[4] * np.float32(1e18), X[5]])
    Q = np.concatenate([queries(X, 5, 62), np.zeros((1, 384), np.float32), X[3:5] * np.float32(1e-20)])
    with FlatIndex(384) as idx:
        idx.add(X)
        first = idx.add(special)
        ids = lists(len(idx), len(Q), 32, 63)
        ids[:, 20:24] = np.arange(first, first + 4, dtype=np.uint64)
        ids[:, 24] = rng.integers(1, 500, len(Q))
        got = check(idx, Q, ids, "special rows")
        real = (ids[5] >= 1) & (ids[5] <= len(idx))
        assert real.sum() >= 28 and not bits(got[1][5])[real].any()         # the zero query: dist 0 against every row
        assert not bits(got[1][:, 20]).any()                               # the zero-norm row: dist 0 for every query


@pytest.mark.parametrize("devices,block", [([0, 0, 0], 96), ([0, 0], 64)], ids=["3x96", "2x64"])
def test_sharded_equals_plain(devices, block, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    Q = queries(X, 37, 71)
    ids = lists(len(X), 37, 64, 72, off=77)
    gone = np.r_[np.arange(200, 230), np.arange(300, 310)].astype(np.uint64)    # rows of two different shards
    G = len(devices)
    assert len({int(r) // block % G for r in gone}) >= 2
    ids[3, :6] = gone[::7][:6] + np.uint64(78)
    with FlatIndex(384) as plain, FlatIndex(384, devices=devices, block_rows=block) as sh:
        for idx in (plain, sh):
            idx.set_id_offset(77)
            idx.add(X)
            idx.remove(gone + np.uint64(78))
        real = ids[(ids >= 78) & (ids <= 77 + len(X))].astype(np.int64)
        assert len(set(((real - 78) // block % G).tolist())) == G            # candidates on every shard
        want = check(plain, Q, ids, "plain", off=77)
        same(sh.score_ids(Q, ids), want, f"{G} shards vs plain")
        big = lists(len(X), 3, 1500, 73, off=77)
        same(sh.score_ids(Q[:3], big), plain.score_ids(Q[:3], big), f"{G} shards vs plain, m = 1500")


def test_device_variant_equals_the_host_variant(lib_built):
    import torch
    from memex_amd.index import FlatIndex
    X = corpus()
    Q = queries(X, 37, 81)
    ids = lists(len(X), 37, 70, 82)
    with FlatIndex(384) as plain, FlatIndex(384, devices=[0, 0], block_rows=64) as sh:
        for idx in (plain, sh):
            idx.add(X)
            h = idx.score_ids(Q, ids)
            for full in (True, False):
                side = torch.cuda.Stream()
                with torch.cuda.stream(side):                              # the queries are produced on the caller's stream
                    dq = torch.from_numpy(Q).cuda() * 1.0
                    sc = torch.full((37, 70), -1.0, dtype=torch.float32, device="cuda")
                    di = torch.full((37, 70), -1.0, dtype=torch.float32, device="cuda") if full else None
                    od = torch.full((37, 70), -7, dtype=torch.int32, device="cuda") if full else None
                    nf = torch.full((37,), -7, dtype=torch.int32, device="cuda") if full else None
                    idx.score_ids_device(dq, ids, sc, di, od, nf)
                side.synchronize()
                dev = [sc.cpu().numpy()] + [t.cpu().numpy() if t is not None else None for t in (di, od, nf)]
                same(dev, h, f"device variant, full = {full}")
            bad = torch.from_numpy(Q[:2]).cuda()
            bad[1, 5] = float("nan")
            from memex_amd import _lib
            with pytest.raises(_lib.MemexHipError) as ei:                  # rejected as the plain device search rejects it
                idx.score_ids_device(bad, ids[:2], sc[:2].contiguous())
            assert ei.value.code == _lib.MX_EINVAL
            with pytest.raises(_lib.MemexHipError) as ei:
                idx.score_ids(bad.cpu().numpy(), ids[:2])
            assert ei.value.code == _lib.MX_EINVAL


def test_concurrent_callers(lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    jobs = [(queries(X, 9 + t, 90 + t), lists(len(X), 9 + t, 40 + 300 * t, 95 + t)) for t in range(4)]
    with FlatIndex(384) as idx:
        idx.add(X)
        serial = [idx.score_ids(q, c) for q, c in jobs]
        out, errs = [None] * 4, []

        def run(t):
            try:
                for _ in range(3):
                    out[t] = idx.score_ids(*jobs[t])
            except Exception as e:                                         # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=run, args=(t,)) for t in range(4)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs, errs
        for t in range(4):
            same(out[t], serial[t], f"thread {t}")


def test_store_rerank(lib_built, tmp_path):
    from memex_amd import storage
    X = near_copy_corpus(np.random.default_rng(63), clusters=12, per=8, d=64)[0]
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    names = [f"s{i}" for i in range(len(X))]
    names[21] = "s20"                                            # one _id inserted twice (rows 20 and 21)
    st.bulk_insert([storage.VectorData(_id=nm, document_id=f"d{i // 8}", text="", vector=list(map(float, v)))
                    for i, (nm, v) in enumerate(zip(names, X))])
    vec = list(map(float, X[40] * np.float32(2.0)))
    everything = st.search(vec, len(X))                          # (name, score) of every row, best first
    asked = ["s90", "s20", "nobody", "s41", "s3", "s40", "s20"]
    want = []
    for nm, s in everything:
        if nm in asked and nm not in [w[0] for w in want]:       # a segment is ranked by its best row and listed once
            want.append((nm, s))
    got = st.rerank(vec, asked)
    assert got == want and [g[0] for g in got[:2]] == ["s40", "s41"] and len(got) == 5
    assert st.rerank(vec, asked, 2) == want[:2] and st.rerank(vec, asked, 0) == []
    assert st.rerank(vec, ["nobody"]) == [] and st.rerank(vec, []) == []
    assert storage.VectorStorage(st).rerank(vec, asked, 3) == want[:3]
    st.remove(["s41"])
    assert st.rerank(vec, asked) == [w for w in want if w[0] != "s41"]
