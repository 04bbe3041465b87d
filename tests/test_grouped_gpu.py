"""Grouped search (mx_grouping, mx_index_search_grouped) on the GPU against its statement in NumPy
(tests/grouped_model.py).  Every case compares ids, keys, group_rows, n_found and complete with integer equality and scores and dists
by their bits.  The shapes are small: the grouping never looks past the top-`fetch` list, whatever the corpus."""
import threading

import numpy as np
import pytest

from conftest import bits
from grouped_model import GroupingModel, brute_force_groups, candidate_lists, group_lists, grouped_model, random_keys
from mmr_model import near_copy_corpus, queries_near_centres

pytestmark = pytest.mark.gpu

N, D = 2000, 64
_CACHE = {}


def small():
    """the near-copy corpus (200 clusters x 10 rows x 64 dims), 6 queries near cluster centres, and keys: groups of 1 - 4 rows cut
    from the rows in cluster order (so the lists hold several rows of a group), a fifth of the rows ungrouped"""
    if "small" not in _CACHE:
        rng = np.random.default_rng(3160)
        X, centres = near_copy_corpus(rng, clusters=N // 10, per=10, d=D)
        Q = queries_near_centres(rng, centres[rng.choice(len(centres), 6, replace=False)], 6).astype(np.float32)
        _CACHE["small"] = (X, centres, Q, random_keys(rng, N, order=np.arange(N)))
    return _CACHE["small"]


def model(oracle, key, *a, **kw):
    """grouped_model, computed once per named case"""
    if key not in _CACHE:
        _CACHE[key] = grouped_model(oracle, *a, **kw)
    return _CACHE[key]


def same(got, want, what):
    for name, g, w in zip(("ids", "scores", "dists", "keys", "group_rows", "n_found", "complete"), got, want):
        if name in ("scores", "dists"):
            g, w = bits(g), bits(w)
        np.testing.assert_array_equal(np.asarray(g), np.asarray(w), err_msg=f"{what}: {name}")


def blanks_ok(got, k):
    ids, sc, di, gk, rows, nf, _ = got
    for b in range(len(nf)):
        n = int(nf[b])
        assert 0 <= n <= k
        assert (ids[b, n:] == 0).all() and (sc[b, n:] == 0).all() and np.isposinf(di[b, n:]).all()
        assert (gk[b, n:] == 0).all() and (rows[b, n:] == 0).all()


def from_lists(idx, grouping_keys, Q, k, fetch, flt=None, id_offset=0):
    """the model over the lists the index itself returns for k = fetch in this run"""
    ci, cs, cd, cnf = idx.search(Q, fetch) if flt is None else idx.search_with(flt, Q, fetch)
    return group_lists(ci, cs, cd, cnf, grouping_keys, k, fetch, id_offset)


def set_keys(grp, keys, id_offset=0):
    grp.set_ids(np.arange(1, len(keys) + 1, dtype=np.uint64) + np.uint64(id_offset), keys)


# ---- the grouping object ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sharded", [False, True], ids=["plain", "3-shards"])
def test_edits_match_the_numpy_array(sharded, lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    X = small()[0]
    rng = np.random.default_rng(3161)
    kw = dict(devices=[0, 0, 0], block_rows=96) if sharded else {}
    with FlatIndex(D, **kw) as idx:
        idx.add(X[:1200])
        off, size = 0, 1200
        m = GroupingModel()
        alive = np.ones(N, bool)

        def check(grp, what):
            probe = np.concatenate([np.arange(0, size + 40, dtype=np.uint64) + np.uint64(max(off - 20, 0)),
                                    np.asarray([0, 1, off, off + size + 1, 2 ** 40, 2 ** 64 - 1], dtype=np.uint64)])
            np.testing.assert_array_equal(grp.keys_of(probe), m.keys_of(probe, off, size), err_msg=what)
            assert grp.count() == m.count(size, alive), what

        with idx.make_grouping() as grp:
            check(grp, "a new grouping: key 0 everywhere")
            assert grp.count() == (0, 0)
            for step in range(12):
                if step == 4:                                           # rows appended after an edit: key 0 until named; the next
                    idx.add(X[1200:1700])                               # edit that names one regrows the array
                    size = 1700
                    check(grp, "after an append")
                if step == 6:
                    off = 5000
                    idx.set_id_offset(off)                              # the ids move along with the rows
                    check(grp, "after set_id_offset")
                if step == 8:
                    idx.add(X[1700:])
                    size = N
                    gone = rng.choice(size, 150, replace=False)
                    idx.remove(gone.astype(np.uint64) + np.uint64(off + 1))
                    alive[gone] = False                                 # removed rows keep their key
                    check(grp, "after removals")
                if step % 2 == 0:
                    cuts = np.sort(rng.choice(np.arange(1, size + 60), 24, replace=False)) + off
                    r = np.stack([cuts[0::2], cuts[1::2]], axis=1).astype(np.uint64)        # 12 disjoint ranges, some past the rows
                    r = r[rng.permutation(len(r))]                                          # in any order
                    k = rng.integers(0, 50, len(r)).astype(np.uint32)                       # key 0 un-groups
                    k[0] = 0
                    grp.set_ranges(r, k)
                    m.set_ranges(r, k, off, size)
                else:
                    i = rng.integers(max(off - 5, 0), off + size + 30, 300).astype(np.uint64)
                    i = np.concatenate([i, i[:40]])                                         # repeats, with the same key
                    k = (i % np.uint64(7)).astype(np.uint32) * np.uint32(step)              # a function of the id: never two keys
                    grp.set_ids(i, k)
                    m.set_ids(i, k, off, size)
                check(grp, f"step {step}")
            assert m.count(size)[0] > 100 and m.count(size, alive)[1] < m.count(size)[0]    # (conditions on the input)
            # refused edits change nothing
            before = grp.keys_of(np.arange(off + 1, off + size + 1, dtype=np.uint64))
            for bad in (lambda: grp.set_ranges([[off + 10, off + 20], [off + 19, off + 30]], [1, 2]),
                        lambda: grp.set_ranges([[off + 10, off + 20], [off + 1, off + 11]], [1, 2]),
                        lambda: grp.set_ranges([[off + 30, off + 20]], [1]),
                        lambda: grp.set_ids([off + 5, off + 9, off + 5], [3, 3, 4])):
                with pytest.raises(_lib.MemexHipError) as e:
                    bad()
                assert e.value.code == _lib.MX_EINVAL
                np.testing.assert_array_equal(grp.keys_of(np.arange(off + 1, off + size + 1, dtype=np.uint64)), before)
            grp.set_ranges([[off + 10, off + 20], [off + 20, off + 30], [off + 15, off + 15]], [1, 2, 9])   # touching and empty: fine
            grp.set_ids([off + 5, off + 5], [3, 3])
            m.set_ranges([[off + 10, off + 20], [off + 20, off + 30]], [1, 2], off, size)
            m.set_ids([off + 5], [3], off, size)
            check(grp, "touching ranges, an empty range, an id twice with one key")


# ---- search against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10])
def test_search_equals_the_model(k, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q, keys = small()
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(X)
        set_keys(grp, keys)
        for fetch in sorted({k, 32, 256}):
            idx.reset_stats()
            got = idx.search_grouped(grp, Q, k, fetch=fetch)
            st = idx.stats()
            assert st.searches == 1 and st.queries == len(Q)            # the candidate stage is one plain pass
            same(got, model(oracle, ("small", k, fetch), X, Q, k, keys, fetch=fetch), f"k {k} fetch {fetch}")
            same(got, from_lists(idx, keys, Q, k, fetch), f"k {k} fetch {fetch}: the lists of this run")
            blanks_ok(got, k)
            ci, cs, cd, cnf = idx.search(Q, fetch)                      # every reported entry is literally an entry of the list
            for b in range(len(Q)):
                at = [list(ci[b]).index(i) for i in got[0][b, :got[5][b]]]
                assert at == sorted(at)
                np.testing.assert_array_equal(bits(got[1][b, :got[5][b]]), bits(cs[b, at]))
                np.testing.assert_array_equal(bits(got[2][b, :got[5][b]]), bits(cd[b, at]))
        if k == 10:                                                     # (conditions on the input)
            short = model(oracle, ("small", 10, 10), X, Q, 10, keys, fetch=10)
            assert (~short[6]).any() and (short[5] < 10).any(), "fetch = k falls short where rows of a group meet in the list"
            full = model(oracle, ("small", 10, 256), X, Q, 10, keys, fetch=256)
            assert full[6].all() and (full[4] > 1).any() and (full[3] == 0).any()
            for b in range(len(Q)):                                     # complete: the true top-k groups over all rows
                wi, wd, wk = brute_force_groups(oracle, X, Q[b], 10, keys)
                np.testing.assert_array_equal(full[0][b], wi)
                np.testing.assert_array_equal(bits(full[2][b]), bits(wd))
        one = idx.search_grouped(grp, Q[0], k)                          # [dim]: one query, the default fetch
        same(one, tuple(a[:1] for a in model(oracle, ("small", k, "default"), X, Q, k, keys)), "one query, default fetch")


def test_ties(oracle, lib_built):
    """every row stored three times, the copies under three different keys: bit-equal dists, heads in id order"""
    from memex_amd.index import FlatIndex
    X, centres, _, _ = small()
    V = X[:600]
    T = np.ascontiguousarray(np.concatenate([V, V, V]))
    Q = queries_near_centres(np.random.default_rng(3162), centres[:5], 5).astype(np.float32)
    keys = (np.arange(1800) // 600 + 1 + 3 * (np.arange(1800) % 600 // 2)).astype(np.uint32)   # copy c of rows 2 j, 2 j + 1: key 3 j + c + 1
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(T)
        set_keys(grp, keys)
        for k, fetch in ((3, 3), (6, 12), (10, 40)):
            got = idx.search_grouped(grp, Q, k, fetch=fetch)
            same(got, grouped_model(oracle, T, Q, k, keys, fetch=fetch), f"tripled rows, k {k} fetch {fetch}")
        assert (np.diff(bits(got[2]).astype(np.int64), axis=1) == 0).any()     # (condition on the input: equal dists are reported)
        first = idx.search_grouped(grp, Q, 3, fetch=3)
        for b in range(5):                                              # the three copies of the best row: ids i, i + 600, i + 1200
            assert list(first[0][b]) == [first[0][b, 0], first[0][b, 0] + 600, first[0][b, 0] + 1200]
            assert len(set(bits(first[2][b]).tolist())) == 1 and len(set(first[3][b].tolist())) == 3


def big():
    """5000 rows at d = 64; rows 1000 .. 1299 are near-copies of the query, all under key 7"""
    if "big" not in _CACHE:
        rng = np.random.default_rng(3163)
        X = rng.standard_normal((5000, D)).astype(np.float32)
        q = rng.standard_normal(D).astype(np.float32)
        X[1000:1300] = q + 1e-3 * rng.standard_normal((300, D)).astype(np.float32)
        keys = np.zeros(5000, np.uint32)
        keys[1000:1300] = 7
        _CACHE["big"] = (X, q, keys)
    return _CACHE["big"]


def test_incomplete_then_complete(oracle, lib_built, tmp_path):
    from memex_amd import storage
    from memex_amd.index import FlatIndex
    X, q, keys = big()
    outside = np.ones(5000, bool)
    outside[1000:1300] = False
    best_outside = candidate_lists(oracle, X, q, 1, alive=outside)[0][0, 0]
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(X)
        grp.set_ranges([[1001, 1301]], [7])
        short = idx.search_grouped(grp, q, 2, fetch=256)
        same(short, model(oracle, ("big", 256), X, q, 2, keys, fetch=256), "fetch 256")
        assert not short[6][0] and short[5][0] == 1 and short[3][0, 0] == 7 and short[4][0, 0] == 256
        full = idx.search_grouped(grp, q, 2, fetch=4096)               # the EXACT path
        same(full, model(oracle, ("big", 4096), X, q, 2, keys, fetch=4096), "fetch 4096")
        assert full[6][0] and full[5][0] == 2 and full[4][0, 0] == 300 and full[0][0, 1] == best_outside and full[3][0, 1] == 0
        assert full[0][0, 0] == short[0][0, 0]
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    st.bulk_insert([storage.VectorData(_id=f"s{i}", document_id="", text="", vector=v) for i, v in enumerate(X)])
    with st.make_grouping({"long": [f"s{i}" for i in range(1000, 1300)]}) as grp:
        hits, complete = st.search_documents(q, 2, grp)                # 32 candidates first, then 4096: by itself
        assert complete is True
        assert [(h[0], h[1], h[3]) for h in hits] == [("long", f"s{int(full[0][0, 0]) - 1}", 300), (None, f"s{int(best_outside) - 1}", 1)]
        assert [np.float32(h[2]) for h in hits] == [full[1][0, 0], full[1][0, 1]]
        hits, complete = st.search_documents(q, 2, grp, fetch=4096)
        assert complete and len(hits) == 2


def test_the_limits(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, q, keys = big()
    Q = np.stack([q, X[17] + 0.1, -q]).astype(np.float32)
    rk = random_keys(np.random.default_rng(3164), 5000, order=np.arange(5000))
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(X)
        set_keys(grp, rk)
        got = idx.search_grouped(grp, Q, 4096, fetch=4096)             # every thread of the workgroup owns four entries
        same(got, grouped_model(oracle, X, Q, 4096, rk, fetch=4096), "k = fetch = 4096")
        assert (got[5] < 4096).all() and (got[5] > 1000).all() and not got[6].any()
        blanks_ok(got, 4096)
        got = idx.search_grouped(grp, Q, 1000, fetch=4096)
        same(got, grouped_model(oracle, X, Q, 1000, rk, fetch=4096), "k = 1000, fetch = 4096")
        assert (got[5] == 1000).all() and got[6].all()
    with FlatIndex(D) as idx, idx.make_grouping() as grp:               # fetch larger than the live rows: the short-list branch
        idx.add(X[1000:1300])
        idx.remove(np.arange(1, 101, dtype=np.uint64))
        alive = np.ones(300, bool)
        alive[:100] = False
        grp.set_ranges([[1, 301]], [7])                                 # all rows under one key
        for fetch in (256, 1024):
            got = idx.search_grouped(grp, Q, 5, fetch=fetch)
            same(got, grouped_model(oracle, X[1000:1300], Q, 5, np.full(300, 7), fetch=fetch, alive=alive), f"200 live rows, fetch {fetch}")
            assert (got[5] == 1).all() and got[6].all() and (got[4][:, 0] == 200).all()
        got = idx.search_grouped(grp, Q, 5, fetch=100)                  # the same group, a full list: one head and no certificate
        assert (got[5] == 1).all() and not got[6].any() and (got[4][:, 0] == 100).all()
    with FlatIndex(D) as idx, idx.make_grouping() as grp:               # an empty grouping: every row is a head
        idx.add(X[:N])
        for k, fetch in ((10, 10), (10, 40), (300, 300)):
            got = idx.search_grouped(grp, Q, k, fetch=fetch)
            ids, sc, di, nf = idx.search(Q, k)
            np.testing.assert_array_equal(got[0], ids)
            np.testing.assert_array_equal(bits(got[1]), bits(sc))
            np.testing.assert_array_equal(bits(got[2]), bits(di))
            np.testing.assert_array_equal(got[5], nf)
            assert (got[3] == 0).all() and (got[4] == 1).all() and got[6].all()
        got = idx.search_grouped(grp, np.zeros((0, D), np.float32), 5)  # B = 0
        assert got[0].shape == (0, 5) and got[5].shape == (0,)
    with FlatIndex(D) as idx, idx.make_grouping() as grp:               # an index without rows finds nothing, completely
        got = idx.search_grouped(grp, Q, 5)
        assert (got[5] == 0).all() and got[6].all()
        blanks_ok(got, 5)


def test_two_batches(lib_built):
    """600 queries: batches of 512 and 88.  The batch equals the per-query calls."""
    from memex_amd.index import FlatIndex
    X, centres, _, keys = small()
    Q = queries_near_centres(np.random.default_rng(3165), centres, 600).astype(np.float32)
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(X)
        set_keys(grp, keys)
        got = idx.search_grouped(grp, Q, 5, fetch=6)
        same(got, from_lists(idx, keys, Q, 5, 6), "600 queries")
        assert (~got[6]).any() and got[6].any()                         # (condition on the input)
        for b in (0, 511, 512, 599):
            same(idx.search_grouped(grp, Q[b], 5, fetch=6), tuple(a[b:b + 1] for a in got), f"query {b} alone")


def test_removed_rows(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q, keys = small()
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(X)
        set_keys(grp, keys)
        before = idx.search_grouped(grp, Q, 10, fetch=64)
        b, j = next((b, j) for b in range(len(Q)) for j in range(3) if before[4][b, j] > 1)     # a head with company in its list
        head, key = int(before[0][b, j]), int(before[3][b, j])
        whole = int(before[3][(b + 1) % len(Q), 0]) or int(before[3][(b + 1) % len(Q), 1])       # a whole group of another query
        assert whole != 0 and whole != key
        gone = np.concatenate([[head - 1], np.flatnonzero(keys == whole)])
        idx.remove(gone.astype(np.uint64) + np.uint64(1))
        alive = np.ones(N, bool)
        alive[gone] = False
        after = idx.search_grouped(grp, Q, 10, fetch=64)
        same(after, grouped_model(oracle, X, Q, 10, keys, fetch=64, alive=alive), "after removals")
        assert not np.isin(after[0], gone + 1).any() and not (after[3] == whole).any()
        at = list(after[3][b]).index(key)                               # the group's next best row heads it now
        assert after[0][b, at] != head and after[4][b, at] == before[4][b, j] - 1
        assert grp.count() == (int((keys != 0).sum()), int(((keys != 0) & alive).sum()))


def test_with_a_resident_filter(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q, keys = small()
    allowed = np.zeros(N, bool)
    allowed[300:1500] = True
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(X)
        flt = idx.make_filter(ranges=[[301, 1501]])
        set_keys(grp, keys)
        idx.remove(np.arange(400, 420, dtype=np.uint64))
        alive = np.ones(N, bool)
        alive[399:419] = False
        for k, fetch in ((10, 40), (5, 300)):
            got = idx.search_grouped(grp, Q, k, fetch=fetch, flt=flt)
            same(got, grouped_model(oracle, X, Q, k, keys, fetch=fetch, alive=alive, allowed=allowed), f"filtered, k {k} fetch {fetch}")
            same(got, from_lists(idx, keys, Q, k, fetch, flt=flt), "the lists of search_with")
            ids = got[0][got[0] != 0].astype(np.int64) - 1
            assert allowed[ids].all() and alive[ids].all()
        flt.close()
        with idx.make_filter() as empty:                                # the empty filter finds nothing: a short list, complete
            got = idx.search_grouped(grp, Q, 3, flt=empty)
            assert (got[5] == 0).all() and got[6].all()


def test_staleness_and_foreign_handles(oracle, lib_built, tmp_path):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    X, _, Q, keys = small()

    def stale(idx, grp):
        for call in (lambda: idx.search_grouped(grp, Q, 5), lambda: grp.set_ranges([[1, 5]], [1]), lambda: grp.set_ids([3], [1]),
                     lambda: grp.keys_of([1, 2]), grp.count):
            with pytest.raises(_lib.MemexHipError, match="stale") as e:
                call()
            assert e.value.code == _lib.MX_EINVAL
        grp.close()                                                     # still works

    with FlatIndex(D) as idx, FlatIndex(D) as other:
        idx.add(X)
        other.add(X[:100])
        grp = idx.make_grouping()
        set_keys(grp, keys)
        assert idx.compact().size == N                                  # nothing removed: a no-op, the grouping stays valid
        same(idx.search_grouped(grp, Q, 10, fetch=40), model(oracle, ("small", 10, 40), X, Q, 10, keys, fetch=40), "after a no-op compact")
        with pytest.raises(_lib.MemexHipError, match="another index") as e:
            other.search_grouped(grp, Q, 5)
        assert e.value.code == _lib.MX_EINVAL
        with other.make_filter(ranges=[[1, 50]]) as foreign, pytest.raises(_lib.MemexHipError, match="another index") as e:
            idx.search_grouped(grp, Q, 5, flt=foreign)
        assert e.value.code == _lib.MX_EINVAL
        idx.remove([5, 150])
        idx.compact()
        stale(idx, grp)
        grp = idx.make_grouping()
        idx.save(str(tmp_path))
        idx.load(str(tmp_path))
        stale(idx, grp)
        grp = idx.make_grouping()
        idx.clear()
        stale(idx, grp)
    # a grouping keeps the rows of a keyed index after the owner dropped its handle
    owner = FlatIndex(D, key="grouping-lifetime")
    owner.add(X)
    grp = owner.make_grouping()
    set_keys(grp, keys)
    want = owner.search_grouped(grp, Q, 10, fetch=40)
    owner.close()
    again = FlatIndex(D, key="grouping-lifetime")                       # the same resident rows: the grouping's reference kept them
    try:
        assert len(again) == N
        same(again.search_grouped(grp, Q, 10, fetch=40), want, "after the owner closed")
    finally:
        grp.close()
        again.clear()
        again.close()


def test_device_pointer_variant_equals_the_host_variant(lib_built):
    import torch
    from memex_amd.index import FlatIndex
    X, _, Q, keys = small()
    with FlatIndex(D) as plain, FlatIndex(D, devices=[0, 0], block_rows=64) as sh:
        for idx in (plain, sh):
            idx.add(X)
            with idx.make_grouping() as grp, idx.make_filter(ranges=[[301, 1501]]) as flt:
                set_keys(grp, keys)
                for k, fetch, extras, f in ((10, None, True, None), (7, 300, True, flt), (7, 12, False, None)):
                    B = len(Q)
                    q = torch.from_numpy(Q).cuda()
                    ids = torch.full((B, k), -1, dtype=torch.int64, device="cuda")
                    sc = torch.full((B, k), -1.0, dtype=torch.float32, device="cuda")
                    nf = torch.full((B,), -1, dtype=torch.int32, device="cuda")
                    di = torch.full((B, k), -1.0, dtype=torch.float32, device="cuda") if extras else None
                    gk = torch.full((B, k), -7, dtype=torch.int32, device="cuda") if extras else None
                    rows = torch.full((B, k), -7, dtype=torch.int32, device="cuda") if extras else None
                    done = torch.full((B,), 9, dtype=torch.uint8, device="cuda") if extras else None
                    idx.search_grouped_device(grp, q, k, ids, sc, di, gk, rows, nf, done, fetch=fetch, flt=f)
                    h = idx.search_grouped(grp, Q, k, fetch=fetch, flt=f)
                    np.testing.assert_array_equal(ids.cpu().numpy().astype(np.uint64), h[0])
                    np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(h[1]))
                    np.testing.assert_array_equal(nf.cpu().numpy(), h[5])
                    if extras:
                        np.testing.assert_array_equal(bits(di.cpu().numpy()), bits(h[2]))
                        np.testing.assert_array_equal(gk.cpu().numpy().view(np.uint32), h[3])
                        np.testing.assert_array_equal(rows.cpu().numpy(), h[4])
                        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), h[6])


@pytest.mark.parametrize("shards,block", [(3, 96), (2, 64)], ids=["3-shards", "2-shards"])
def test_sharded_equals_plain(shards, block, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q, keys = small()
    gone = np.concatenate([np.arange(block, block + 30), np.arange(2 * block + 5, 2 * block + 25)])   # rows of the second and third block
    alive = np.ones(N, bool)
    alive[gone] = False
    with FlatIndex(D) as plain, FlatIndex(D, devices=[0] * shards, block_rows=block) as sh:
        grps = []
        for idx in (plain, sh):
            idx.add(X)
            idx.remove(gone.astype(np.uint64) + np.uint64(1))
            grps.append(idx.make_grouping())
            set_keys(grps[-1], keys)
        try:
            for k, fetch in ((10, 40), (10, 10), (5, 300)):
                a = sh.search_grouped(grps[1], Q, k, fetch=fetch)
                same(a, plain.search_grouped(grps[0], Q, k, fetch=fetch), f"{shards} shards vs plain, k {k} fetch {fetch}")
                same(a, grouped_model(oracle, X, Q, k, keys, fetch=fetch, alive=alive), f"{shards} shards vs model, k {k} fetch {fetch}")
            assert grps[1].count() == grps[0].count() == (int((keys != 0).sum()), int(((keys != 0) & alive).sum()))
            with sh.make_filter(ranges=[[301, 1501]]) as fs, plain.make_filter(ranges=[[301, 1501]]) as fp:
                same(sh.search_grouped(grps[1], Q, 10, fetch=40, flt=fs), plain.search_grouped(grps[0], Q, 10, fetch=40, flt=fp),
                     f"{shards} shards vs plain, filtered")
        finally:
            for g in grps:
                g.close()


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
    X, _, Q, keys = small()
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        if setup == "compressed":
            idx.set_corpus_mode("bf16")
        idx.add(X)
        if callable(setup):
            setup(idx)
        if setup == "exact":
            idx.set_search_mode(_lib.MX_SEARCH_EXACT)
        set_keys(grp, keys)
        rows = idx.get_rows(0, len(X)) if setup == "compressed" else X
        assert setup != "compressed" or (rows != X).any()              # the model is fed what the index stores
        want = model(oracle, ("kind", setup == "compressed"), rows, Q[:3], 10, keys, fetch=16)
        same(idx.search_grouped(grp, Q[:3], 10, fetch=16), want, name)


def test_store_and_tasks(oracle, lib_built, tmp_path):
    from memex_amd import storage, tasks
    rng = np.random.default_rng(3166)
    X, centres = near_copy_corpus(rng, clusters=12, per=8, d=D)         # 96 segments: document i holds the 8 rows of cluster i
    data = [storage.VectorData(_id=f"s{i}", document_id=f"d{i // 8}", text="", vector=list(map(float, v)), segment_id=i % 8)
            for i, v in enumerate(X)]
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    st.bulk_insert(data[:80])
    q = queries_near_centres(rng, centres[[3]], 1)[0].astype(np.float32)
    docs = {f"d{d}": [f"s{i}" for i in range(8 * d, 8 * d + 8)] for d in range(9)}
    docs["unknown"] = ["nobody"]                                        # unknown _ids add nothing
    with st.make_grouping(docs) as grp:
        assert grp.count() == (72, 72)
        tasks.group_document(grp, data[72:80])                          # document 9, the way the worker would after process_embeddings
        st.bulk_insert(data[80:])                                       # documents 10 and 11 arrive later: ungrouped until assigned
        assert grp.count() == (80, 80)
        keys = np.zeros(96, np.uint32)
        keys[:80] = np.arange(80) // 8 + 1                              # keys 1, 2, ... in the order the names were first seen

        def expect(k, fetch, alive=None):
            ids, sc, _, gk, rows, nf, done = grouped_model(oracle, X, q, k, keys, fetch=fetch, alive=alive)
            return [(f"d{int(g) - 1}" if g else None, f"s{int(i) - 1}", float(s), int(r))
                    for i, s, g, r in zip(ids[0, :nf[0]], sc[0, :nf[0]], gk[0, :nf[0]], rows[0, :nf[0]])], bool(done[0])

        def ladder(k, alive=None):                                      # what search_documents does: once more at 4096 if need be
            first = expect(k, 32, alive)
            return first if first[1] else expect(k, 4096, alive)

        hits, complete = st.search_documents(q, 4, grp)
        assert (hits, complete) == expect(4, 32) and complete
        assert hits[0][0] == "d3" and hits[0][3] == 8 and len({h[0] for h in hits if h[0]}) == len([h for h in hits if h[0]])
        plain = st.search(q, 4)                                         # what search_docs gives: four windows of one document
        assert {n for n, _ in plain} <= set(docs["d3"]) and hits[0][1] == plain[0][0]
        assert st.search_documents(q, 4, grp, fetch=8) == expect(4, 4096)          # 8 candidates are all of d3: asks again by itself
        assert storage.VectorStorage(st).search_documents(q, 4, grp) == (hits, complete)
        grp.assign("d10", [f"s{i}" for i in range(80, 88)])
        keys[80:88] = 11
        grp.release(["s24", "s25"])                                     # two segments of d3 leave it
        keys[24:26] = 0
        assert st.search_documents(q, 6, grp) == ladder(6)
        best = hits[0][1]
        st.remove([best])
        alive = np.asarray([f"s{i}" != best for i in range(96)])
        after, _ = st.search_documents(q, 6, grp)
        assert (after, True) == ladder(6, alive) and best not in [h[1] for h in after]
        with pytest.raises(storage.SearchError):                        # one segment under two documents in one edit
            grp.assign_all({"a": ["s1"], "b": ["s1"]})

        class Hit:
            def __init__(self, v):
                self.vector = v

        class Embedder:
            def encode_single(self, text):
                return Hit(list(map(float, q))) if text else None

        assert tasks.search_documents(storage.VectorStorage(st), Embedder(), grp, "a question", limit=6) == (after, True)
        assert tasks.search_documents(st, Embedder(), grp, "a question", limit=6) == (after, True)
        with pytest.raises(ValueError, match="Invalid query"):
            tasks.search_documents(st, Embedder(), grp, "")
        st.compact()                                                    # the rows were renumbered: the grouping says so
        with pytest.raises(storage.SearchError, match="stale"):
            st.search_documents(q, 4, grp)


def test_a_concurrent_caller_beside_an_appender(oracle, lib_built):
    """one thread issues grouped searches while another appends: every answer equals the model for SOME prefix of the corpus.  Rows
    appended later have key 0 until named, so the model has the keys of the first prefix only."""
    from memex_amd.index import FlatIndex
    X, centres, _, keys = small()
    Q = queries_near_centres(np.random.default_rng(3167), centres[[70, 100, 130, 170]], 8).astype(np.float32)   # rows of every prefix
    prefixes = [800, 1200, 1600, 2000]
    first = keys[:prefixes[0]]                                          # rows past it stay ungrouped
    want = [grouped_model(oracle, X[:n], Q, 5, first, fetch=16) for n in prefixes]
    assert all(any((a != b).any() for a, b in zip(u, v)) for u, v in zip(want, want[1:]))   # (condition on the input: every append shows)
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(X[:prefixes[0]])
        set_keys(grp, first)
        got, errs = [], []

        def search():
            try:
                for _ in range(8):
                    got.append(idx.search_grouped(grp, Q, 5, fetch=16))
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        def append():
            try:
                for a, b in zip(prefixes[:-1], prefixes[1:]):
                    idx.add(X[a:b])
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=search), threading.Thread(target=append)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        assert len(got) == 8
        for g in got:
            ok = [all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(g, w))
                  for w in want]
            assert any(ok), "an answer matches no prefix of the corpus"
        same(idx.search_grouped(grp, Q, 5, fetch=16), want[-1], "after the appends")
