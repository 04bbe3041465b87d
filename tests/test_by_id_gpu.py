"""Search by stored row (mx_index_search_by_id / mx_index_search_range_by_id) on the GPU against its contract,
which is stated through the PLAIN calls on the same index: feed ``get_rows`` of the named row to ``search`` at k + 1 (or to
``search_range`` at a cap that lists everything in range), drop the own id, cut.  Every comparison is integer equality on ids, score
bits, dist bits and counts.  The corpus is clusters of near-copies (tests/mmr_model.py): it crosses 64-row tiles and 32-row
quantisation groups and every row has near-copies, so the own row is never the only thing near the top."""
import threading

import numpy as np
import pytest

from by_id_model import blank, drop_own
from conftest import bits
from mmr_model import near_copy_corpus
from test_mmr_gpu import _KINDS

pytestmark = pytest.mark.gpu

_CACHE = {}


def corpus(d=384, clusters=150):
    key = (d, clusters)
    if key not in _CACHE:
        _CACHE[key] = near_copy_corpus(np.random.default_rng(2000 + d + clusters), clusters=clusters, d=d)[0]
    return _CACHE[key]


def stored_rows(idx, qids, off=0):
    """-> (the stored rows of the ids that name a row [B, dim] (zeros elsewhere), mask of those ids)"""
    qids = np.asarray(qids, dtype=np.int64)
    ok = (qids > off) & (qids <= off + len(idx))
    rows = np.zeros((len(qids), idx.dim), np.float32)
    for b in np.flatnonzero(ok):
        rows[b] = idx.get_rows(int(qids[b]) - off - 1, 1)[0]
    return rows, ok


def topk_model(idx, qids, k, e, off=0, dead=()):
    rows, ok = stored_rows(idx, qids, off)
    ok &= ~np.isin(np.asarray(qids, dtype=np.int64), np.asarray(dead, dtype=np.int64))
    return drop_own(idx.search(rows, k + e), qids, ok, k, e)


def range_model(idx, qids, thr, cap, e, off=0, dead=()):
    rows, ok = stored_rows(idx, qids, off)
    ok &= ~np.isin(np.asarray(qids, dtype=np.int64), np.asarray(dead, dtype=np.int64))
    ids, sc, di, nf, nr = idx.search_range(rows, thr, 4096)
    return drop_own((ids, sc, di, nf), qids, ok, cap, e, counts=nr)


def same(got, want, what):
    names = ("ids", "scores", "dists", "n_found", "n_in_range")
    assert len(got) == len(want)
    for g, w, n in zip(got, want, names):
        if n in ("scores", "dists"):
            g, w = bits(g), bits(w)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {n}")


def spread_ids(n, B=37, seed=5):
    """B distinct ids drawn across 1 .. n, the first and the last row among them"""
    rng = np.random.default_rng(seed)
    return np.unique(np.r_[1, n, rng.choice(np.arange(2, n), B - 2, replace=False)]).astype(np.uint64)


@pytest.mark.parametrize("name,d,clusters,setup", _KINDS, ids=[c[0] for c in _KINDS])
def test_every_copy_kind_matches_the_plain_calls(name, d, clusters, setup, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus(d, clusters)
    with FlatIndex(d) as idx:
        if setup == "compressed":
            idx.set_corpus_mode("bf16")
        idx.add(X)
        if callable(setup):
            setup(idx)
        q = spread_ids(len(X))
        assert len(q) == 37
        for e in (1, 0):
            got = idx.search_by_id(q, 10, exclude_self=bool(e))
            same(got, topk_model(idx, q, 10, e), f"{name}, exclude_self = {e}")
            assert (got[3] == 10).all()
            if e:
                assert not (got[0] == q[:, None]).any()
            else:                                               # the own row, or an exact copy with a smaller id, leads
                assert (got[0][:, 0] <= q).all() and (bits(got[2][:, 0]) == 0).all()
        thr = idx.search_by_id(q, 12, exclude_self=True)[1][:, 11]      # the 12th-best other row's score: 12 or more in range
        for e in (1, 0):
            same(idx.search_range_by_id(q, thr, 8, exclude_self=bool(e)), range_model(idx, q, thr, 8, e), f"{name}, range, exclude_self = {e}")


def test_ties_with_exact_copies(lib_built):
    """40 copies of one new row: the last copy's own row is not among the k + 1 listed and nothing is dropped; the first copy's is entry
    0 and is dropped.  Either way 39 other rows are in range."""
    from memex_amd.index import FlatIndex
    X = corpus()
    v = np.random.default_rng(7).standard_normal(384).astype(np.float32)
    with FlatIndex(384) as idx:
        idx.add(X)
        first = idx.add(np.repeat(v[None, :], 40, axis=0))
        last = first + 39
        q = np.array([last, first, first + 17], dtype=np.uint64)
        plain = idx.search(np.repeat(v[None, :], 3, axis=0), 11)
        np.testing.assert_array_equal(plain[0][0], np.arange(first, first + 11))    # (condition on the inputs: ties in id order)
        got = idx.search_by_id(q, 10, exclude_self=True)
        same(got, topk_model(idx, q, 10, 1), "ties, top-k")
        np.testing.assert_array_equal(got[0][0], np.arange(first, first + 10))      # last copy: nothing dropped
        np.testing.assert_array_equal(got[0][1], np.arange(first + 1, first + 11))  # first copy: entry 0 dropped
        np.testing.assert_array_equal(got[0][2], np.arange(first, first + 10))      # a middle copy: not among the 11 either
        got = idx.search_range_by_id(q, 0.999, 10, exclude_self=True)
        same(got, range_model(idx, q, 0.999, 10, 1), "ties, range")
        assert (got[4] == 39).all() and (got[3] == 10).all()
        np.testing.assert_array_equal(got[0][0], np.arange(first, first + 10))
        np.testing.assert_array_equal(got[0][1], np.arange(first + 1, first + 11))
        got = idx.search_range_by_id(q, 0.999, 10, exclude_self=False)
        assert (got[4] == 40).all()


def test_k_plus_one_crosses_into_the_exact_path(lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    with FlatIndex(384) as idx:
        idx.add(X)
        q = spread_ids(len(X), 8, seed=11)
        got = idx.search_by_id(q, 256, exclude_self=True)                # the pass runs at k = 257
        same(got, topk_model(idx, q, 256, 1), "k = 256")
        same(idx.search_by_id(q, 256, exclude_self=False), topk_model(idx, q, 256, 0), "k = 256, own row kept")


def test_batch_crosses_the_pass_split(lib_built):
    """B = 600: two batches at the entry point (512 + 88), the first split again inside the pass; the model in two plain calls"""
    from memex_amd.index import FlatIndex
    X = corpus()
    with FlatIndex(384) as idx:
        idx.add(X)
        q = spread_ids(len(X), 600, seed=13)
        np.random.default_rng(14).shuffle(q)
        want = [np.concatenate(p) for p in zip(topk_model(idx, q[:300], 10, 1), topk_model(idx, q[300:], 10, 1))]
        same(idx.search_by_id(q, 10), want, "B = 600")
        thr = want[1][:, 4].copy()
        want = [np.concatenate(p) for p in zip(range_model(idx, q[:300], thr[:300], 8, 1), range_model(idx, q[300:], thr[300:], 8, 1))]
        same(idx.search_range_by_id(q, thr, 8), want, "B = 600, range")


@pytest.mark.parametrize("cap", [8, 64])
def test_range_thresholds_and_caps(cap, lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    with FlatIndex(384) as idx:
        idx.add(X)
        q = spread_ids(len(X))
        top = idx.search(stored_rows(idx, q)[0], 100)[1]
        over = under = 0
        for rank in (5, 20, 100):
            thr = top[:, rank - 1].copy()                        # the query's own rank-th best score (the own row counts as one)
            for e in (1, 0):
                got = idx.search_range_by_id(q, thr, cap, exclude_self=bool(e))
                same(got, range_model(idx, q, thr, cap, e), f"rank {rank}, cap {cap}, exclude_self = {e}")
                assert (got[4] >= rank - e).all()
                over += int((got[4] > cap).sum())
                under += int((got[4] <= cap).sum())
        assert over > 0 and under > 0


def test_rows_on_the_side_lists(lib_built):
    """a zero-norm row and a row scaled by 1e20 (the wide-norm list), each as a query id"""
    from memex_amd.index import FlatIndex
    X = corpus().copy()
    X[107] = 0
    X[1210] *= np.float32(1e20) / np.float32(np.linalg.norm(X[1210]))
    with FlatIndex(384) as idx:
        idx.add(X)
        q = np.array([108, 1211, 1212, 55], dtype=np.uint64)
        for e in (1, 0):
            same(idx.search_by_id(q, 10, exclude_self=bool(e)), topk_model(idx, q, 10, e), f"side lists, exclude_self = {e}")
            for thr, cap in ((0.99, 8), (0.99, 64), (-1.0, 8)):
                same(idx.search_range_by_id(q, thr, cap, exclude_self=bool(e)), range_model(idx, q, thr, cap, e),
                     f"side lists, range {thr} cap {cap}, exclude_self = {e}")
        got = idx.search_range_by_id(q[:1], 0.5, 8)              # the zero-norm row scores 1 against every row: all others are in range
        assert got[4][0] == len(X) - 1 and not (got[0] == 108).any()


def test_dead_and_invalid_ids(lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    n = len(X)
    with FlatIndex(384) as idx:
        idx.add(X)
        gone = np.array([41, 42, 900, 2999], dtype=np.uint64)
        idx.remove(gone)
        q = np.array([7, 41, 0, 8, n + 1, 2999, 43, 2 ** 40, n], dtype=np.uint64)
        bad = np.array([False, True, True, False, True, True, False, True, False])
        for e in (1, 0):
            got = idx.search_by_id(q, 10, exclude_self=bool(e))
            same(got, topk_model(idx, q, 10, e, dead=gone), f"dead ids, exclude_self = {e}")
            assert (got[3][bad] == 0).all() and (got[0][bad] == 0).all() and np.isposinf(got[2][bad]).all() and (got[3][~bad] == 10).all()
            assert not np.isin(got[0], gone).any()
            got = idx.search_range_by_id(q, 0.99, 8, exclude_self=bool(e))
            same(got, range_model(idx, q, 0.99, 8, e, dead=gone), f"dead ids, range, exclude_self = {e}")
            assert (got[4][bad] == 0).all() and (got[3][bad] == 0).all() and (got[4][~bad] > 0).all()
        same(idx.search_by_id(gone, 5), blank(4, 5), "only dead ids")                # no pass at all
        same(idx.search_range_by_id(gone, 0.5, 5), blank(4, 5, True), "only dead ids, range")
        # after compact() the same rows are reached under their new ids
        before = idx.search_by_id(np.array([43, 901, n], dtype=np.uint64), 10)
        kept = idx.compact()
        new = np.array([int(np.flatnonzero(kept == i)[0]) + 1 for i in (43, 901, n)], dtype=np.uint64)
        after = idx.search_by_id(new, 10)
        same(after, topk_model(idx, new, 10, 1), "compacted")
        np.testing.assert_array_equal(kept[after[0].astype(np.int64) - 1], before[0])
        np.testing.assert_array_equal(bits(after[2]), bits(before[2]))
    with FlatIndex(384) as idx:                                   # results and query ids shift together
        idx.set_id_offset(1000)
        idx.add(X)
        q = np.array([1000, 1001, 1000 + n, 1001 + n, 5, 1500], dtype=np.uint64)
        got = idx.search_by_id(q, 10)
        same(got, topk_model(idx, q, 10, 1, off=1000), "id_offset")
        np.testing.assert_array_equal(got[3], [0, 10, 10, 0, 0, 10])
        assert (got[0][got[0] != 0] > 1000).all()
        same(idx.search_range_by_id(q, 0.99, 8), range_model(idx, q, 0.99, 8, 1, off=1000), "id_offset, range")
    with FlatIndex(384) as idx:                                   # an empty index finds nothing
        same(idx.search_by_id([1, 2], 3), blank(2, 3), "empty index")


def test_sharded_equals_plain(lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    gone = np.arange(200, 230, dtype=np.uint64)
    with FlatIndex(384) as plain, FlatIndex(384, devices=[0, 0, 0], block_rows=96) as sh:
        for idx in (plain, sh):
            idx.set_id_offset(77)
            idx.add(X)
            idx.remove(gone + np.uint64(78))
        q = spread_ids(len(X)) + np.uint64(77)
        assert len(set(((q.astype(np.int64) - 78) // 96) % 3)) == 3       # query rows on every shard
        q = np.r_[q, np.uint64(77 + 210), np.uint64(3)]                  # a removed row, an id below the offset
        for e in (1, 0):
            a = sh.search_by_id(q, 10, exclude_self=bool(e))
            same(a, plain.search_by_id(q, 10, exclude_self=bool(e)), f"3 shards vs plain, exclude_self = {e}")
            same(a, topk_model(plain, q, 10, e, off=77, dead=gone + np.uint64(78)), f"3 shards vs model, exclude_self = {e}")
            thr = a[1][:, 5].copy()
            b = sh.search_range_by_id(q, thr, 8, exclude_self=bool(e))
            same(b, plain.search_range_by_id(q, thr, 8, exclude_self=bool(e)), f"3 shards vs plain, range, exclude_self = {e}")
            same(b, range_model(plain, q, thr, 8, e, off=77, dead=gone + np.uint64(78)), f"3 shards vs model, range, exclude_self = {e}")


def test_device_pointer_variants_equal_the_host_variants(lib_built):
    import torch
    from memex_amd.index import FlatIndex
    X = corpus()
    q = spread_ids(len(X))
    B = len(q)
    with FlatIndex(384) as plain, FlatIndex(384, devices=[0, 0], block_rows=64) as sh:
        for idx in (plain, sh):
            idx.add(X)
            for k, dists in ((10, True), (7, False)):
                ids = torch.full((B, k), -1, dtype=torch.int64, device="cuda")
                sc = torch.full((B, k), -1.0, dtype=torch.float32, device="cuda")
                di = torch.full((B, k), -1.0, dtype=torch.float32, device="cuda") if dists else None
                nf = torch.full((B,), -1, dtype=torch.int32, device="cuda")
                nr = torch.full((B,), -1, dtype=torch.int64, device="cuda")
                idx.search_by_id_device(q, k, ids, sc, di, nf)
                h = idx.search_by_id(q, k)
                dev = [ids.cpu().numpy().astype(np.uint64), sc.cpu().numpy(), di.cpu().numpy() if dists else h[2], nf.cpu().numpy()]
                same(dev, h, f"device top-k, k = {k}")
                idx.search_range_by_id_device(q, 0.995, k, ids, sc, di, nf, nr)
                h = idx.search_range_by_id(q, 0.995, k)
                dev = [ids.cpu().numpy().astype(np.uint64), sc.cpu().numpy(), di.cpu().numpy() if dists else h[2], nf.cpu().numpy(),
                       nr.cpu().numpy().astype(np.uint64)]
                same(dev, h, f"device range, cap = {k}")


def pair_model(idx, min_score):
    """brute force over the plain range call: every pair of rows in range of each other, from both ends"""
    n = len(idx)
    seen = {}
    for lo in range(0, n, 512):
        ids, sc, _, nf, nr = idx.search_range(idx.get_rows(lo, min(512, n - lo)), min_score, 4096)
        assert (nr == nf).all()
        for b in range(len(nf)):
            own = lo + b + 1
            for j in range(int(nf[b])):
                o = int(ids[b, j])
                if o != own:
                    seen.setdefault((min(own, o), max(own, o)), {})[own] = int(bits(sc[b, j]))
    return seen


def test_near_duplicates(lib_built):
    from memex_amd.index import FlatIndex
    X = corpus()
    with FlatIndex(384) as idx:
        idx.add(X)
        seen = pair_model(idx, 0.98)
        want = sorted(seen)
        assert len(want) >= 1000
        assert all(len(v) == 2 and len(set(v.values())) == 1 for v in seen.values())      # symmetric, bit for bit, on every pair
        pairs, scores, truncated = idx.near_duplicates(0.98, per_row=64)
        assert truncated.size == 0 and pairs.dtype == np.uint64 and scores.dtype == np.float32
        np.testing.assert_array_equal(pairs, np.array(want, dtype=np.uint64))               # the pairs, each once, in order
        assert (pairs[:, 0] < pairs[:, 1]).all()
        np.testing.assert_array_equal(bits(scores), np.array([next(iter(seen[p].values())) for p in want], dtype=np.uint32))
        # the score from i's list equals the one from j's, for 200 sampled pairs, through the by-id call itself
        pick = np.random.default_rng(17).choice(len(want), 200, replace=False)
        ends = pairs[pick]
        fa = idx.search_range_by_id(ends[:, 0], 0.98, 64)
        fb = idx.search_range_by_id(ends[:, 1], 0.98, 64)
        for t in range(200):
            ja = int(np.flatnonzero(fa[0][t] == ends[t, 1])[0])
            jb = int(np.flatnonzero(fb[0][t] == ends[t, 0])[0])
            assert bits(fa[1][t, ja]) == bits(fb[1][t, jb]) == bits(scores[pick[t]])
        # lists cut at 4: every row of a 20-row cluster is truncated here, and so is every pair with both ends in `truncated` allowed to go
        p4, s4, t4 = idx.near_duplicates(0.98, per_row=4)
        assert t4.size > 0
        cut = set(int(i) for i in t4)
        got4 = set(map(tuple, p4.tolist()))
        assert got4 <= set(want)
        assert all(p in got4 for p in want if p[0] not in cut or p[1] not in cut)
        # a threshold only the closest pairs reach, so that some rows are cut at 4 and others are not
        hi = float(np.sort(scores)[int(0.85 * len(scores))])
        seen_hi = pair_model(idx, hi)
        p4, s4, t4 = idx.near_duplicates(hi, per_row=4, block=300)
        cut = set(int(i) for i in t4)
        assert 0 < len(cut) < len(X)
        got4 = dict(zip(map(tuple, p4.tolist()), bits(s4).tolist()))
        assert set(got4) <= set(seen_hi)
        must = [p for p in seen_hi if p[0] not in cut or p[1] not in cut]
        assert len(must) > 100 and all(p in got4 and got4[p] == next(iter(seen_hi[p].values())) for p in must)
        assert p4.tolist() == sorted(p4.tolist())


def test_store_more_like_and_find_duplicates(lib_built, tmp_path):
    from memex_amd import storage
    rng = np.random.default_rng(63)
    X = near_copy_corpus(rng, clusters=12, per=8, d=64)[0]
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    names = [f"s{i}" for i in range(len(X))]
    names[21] = "s20"                                            # one _id inserted twice (rows 20 and 21 of cluster 2)
    st.bulk_insert([storage.VectorData(_id=nm, document_id=f"d{i // 8}", text="", vector=list(map(float, v)))
                    for i, (nm, v) in enumerate(zip(names, X))])
    got = st.more_like("s20", 5)
    assert len(got) == 5 and "s20" not in [g[0] for g in got]
    assert {g[0] for g in got} <= {f"s{i}" for i in (16, 17, 18, 19, 22, 23)}          # the other members of its cluster
    # the union of the two rows' plain answers, ranked by best score, each row once
    best = {}
    for r in (20, 21):
        ids, sc, di, nf = st._index.search(X[r], 12)
        for i, s, d_ in zip(ids[0, :nf[0]], sc[0, :nf[0]], di[0, :nf[0]]):
            if int(i) not in (21, 22) and (int(i) not in best or d_ < best[int(i)][0]):
                best[int(i)] = (float(d_), float(s))
    want = sorted(best.items(), key=lambda kv: (kv[1][0], kv[0]))[:5]
    assert got == [(names[i - 1], s) for i, (_, s) in want]
    assert st.more_like("nobody", 5) == [] and st.more_like("s20", 0) == []
    assert len(st.more_like("s3", 200)) == len(X) - 1
    pairs, truncated = st.find_duplicates(0.98)
    ip, isc, it = st._index.near_duplicates(0.98)
    assert truncated == [] and it.size == 0 and len(pairs) == len(ip) >= 12 * 28
    assert pairs == [(names[int(a) - 1], names[int(b) - 1], float(s)) for (a, b), s in zip(ip, isc)]
    assert ("s16", "s17") in [p[:2] for p in pairs]
    st.remove(["s17"])
    after, _ = st.find_duplicates(0.98)
    assert not any("s17" in p[:2] for p in after) and len(after) == len(pairs) - 7
    assert "s17" not in [g[0] for g in st.more_like("s16", 7)]
    _, cut = st.find_duplicates(0.98, per_row=2)
    assert cut and set(cut) <= set(names) and "s17" not in cut


def test_by_id_beside_add_remove_and_compact(lib_built):
    """one thread loops search_by_id while another appends, removes and compacts: every answer is the answer of ONE state the index
    went through (the call holds the index from the id translation to its last kernel), and nothing raises"""
    from memex_amd.index import FlatIndex
    X = corpus()
    extra = near_copy_corpus(np.random.default_rng(71), clusters=5, d=384)[0]
    q = spread_ids(len(X), 12, seed=19)
    gone = np.unique(np.r_[q[3], q[7] + np.uint64(1), np.arange(500, 700, dtype=np.uint64)])

    def steps(idx):
        yield
        idx.add(extra)
        yield
        idx.remove(gone)
        yield
        idx.compact()
        yield

    with FlatIndex(384) as ref:                                   # the model of every state, on a quiet index
        ref.add(X)
        states = []
        dead = np.zeros(0, np.uint64)
        for i, _ in enumerate(steps(ref)):
            dead = gone if i == 2 else np.zeros(0, np.uint64)
            states.append(topk_model(ref, q, 10, 1, dead=dead))
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
                    answers.append(idx.search_by_id(q, 10))
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
