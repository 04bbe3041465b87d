"""Removing single rows (mx_index_remove): tombstones masked in every search path.  After each removal pattern a search must
be bit-identical to the oracle run on the LIVE rows only, with the oracle's row numbers mapped back to the original ids
(the oracle orders ties by row, and that order is monotone in id, so the tie order carries over)."""
import os
import threading

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu


def live_oracle(oracle, rows, alive, Q, k):
    """The oracle on the live rows, ids mapped back to the index's ids (1-based, all rows)."""
    live_ids = np.flatnonzero(alive).astype(np.uint64) + 1
    oi, od, os_, onf = oracle.search(rows[alive], Q, k)
    mapped = np.where(oi > 0, live_ids[np.maximum(oi.astype(np.int64) - 1, 0)], 0).astype(np.uint64)
    return mapped, od, os_, onf


def check(idx, oracle, rows, alive, Q, k, what=""):
    ids, sc, di, nf = idx.search(Q, k)
    oi, od, os_, onf = live_oracle(oracle, rows, alive, Q, k)
    np.testing.assert_array_equal(nf, onf, err_msg=what)
    np.testing.assert_array_equal(ids, oi, err_msg=what)
    np.testing.assert_array_equal(bits(di), bits(od), err_msg=what)
    np.testing.assert_array_equal(bits(sc), bits(os_), err_msg=what)
    dead = np.flatnonzero(~alive) + 1
    assert not np.isin(ids[ids > 0], dead).any(), what


def remove(idx, alive, rows0):
    """rows0: 0-based rows -> ids; checks the newly-removed count against the host mirror"""
    rows0 = np.asarray(rows0, dtype=np.int64)
    expect = int(np.unique(rows0[alive[rows0]]).size)
    assert idx.remove(rows0 + 1) == expect
    alive[rows0] = False
    assert idx.removed == int((~alive).sum())


def corpus(rng, n, d, cone=False):
    X = rng.standard_normal((n, d))
    if cone:
        axis = rng.standard_normal(d)
        axis /= np.linalg.norm(axis)
        X = axis + X * (0.6 / np.sqrt(d))
    X = (X * rng.uniform(0.1, 10.0, (n, 1))).astype(np.float32)
    X[[7, 300, n // 2 + 1]] = 0                              # zero-norm rows
    wild = [11, n - 100]
    X[wild] *= np.float32(1e20) / np.linalg.norm(X[wild], axis=1, keepdims=True)  # norms of 1e20 (listed rows)
    X[100:108] = X[99]                                       # duplicates
    return X


# (name, dim, rows, setup): setup(idx) picks the path
_KINDS = [
    ("int8", 384, 50000, lambda idx: idx.set_filter_copy("i8")),
    ("bf16", 384, 40000, lambda idx: idx.set_filter_copy("bf16")),
    ("f32", 384, 20000, lambda idx: idx.set_filter_copy(False)),
    ("compressed", 384, 40000, lambda idx: idx.set_corpus_mode("bf16")),
    ("centred_int8", 384, 50000, None),
    ("wide_1536", 1536, 20000, lambda idx: idx.set_filter_copy("bf16")),
    ("exact", 384, 20000, lambda idx: idx.set_search_mode(1)),
]


@pytest.mark.parametrize("name,d,n,setup", _KINDS, ids=[c[0] for c in _KINDS])
def test_remove_patterns_match_oracle_on_live_rows(name, d, n, setup, oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(sum(map(ord, name)))
    cone = name == "centred_int8"
    X = corpus(rng, n, d, cone=cone)
    if name == "compressed":
        X[[11, n - 100]] = rng.standard_normal((2, d)).astype(np.float32)  # (wide norms send a compressed corpus to the EXACT path)
    with FlatIndex(d) as idx:
        if setup is not None and name == "compressed":
            setup(idx)
        idx.add(X)
        if setup is not None and name != "compressed":
            setup(idx)
        if cone:
            idx.set_filter_copy(False)                         # (asking for the kind the index already has rebuilds nothing)
            idx.set_filter_copy("i8")                          # rebuilt from a populated cone: centred
            assert idx.stats().filter_centred == 1
        rows = idx.get_rows(0, n) if name == "compressed" else X
        alive = np.ones(n, dtype=bool)
        Q = rng.standard_normal((40, d)).astype(np.float32)
        if cone:
            Q[::2] = rows[rng.integers(0, n, 20)] + Q[::2] * 0.01
        Q[1] = rows[99] * 3.0                                  # a query that is a (duplicated) row
        Q[2] = rows[2000]                                      # the query's own exact duplicate
        check(idx, oracle, rows, alive, Q, 10, f"{name}: nothing removed")

        steps = [
            ("1% random", rng.choice(n, n // 100, replace=False)),
            ("whole 64-row tiles", np.r_[64 * 3:64 * 4, 64 * 40:64 * 43]),
            ("first and last row of half tiles", np.r_[32 * 9, 32 * 9 + 31, 32 * 101, 32 * 101 + 31]),
            ("the query's exact duplicate", np.r_[2000, 99:108]),
            ("zero-norm and 1e20-norm rows", np.r_[7, 300, 11]),
            ("every other row", np.arange(0, n, 2)),
        ]
        for what, r in steps:
            remove(idx, alive, r)
            check(idx, oracle, rows, alive, Q, 10, f"{name}: {what}")
        check(idx, oracle, rows, alive, Q[:8], 300, f"{name}: k = 300")
        # all but k - 1 rows: every query finds k - 1
        keep = np.flatnonzero(alive)[rng.choice(int(alive.sum()), 9, replace=False)]
        gone = np.setdiff1d(np.flatnonzero(alive), keep)
        remove(idx, alive, gone)
        ids, sc, di, nf = idx.search(Q, 10)
        assert (nf == 9).all()
        check(idx, oracle, rows, alive, Q, 10, f"{name}: all but k-1")
        assert len(idx) == n                                   # size counts every row ever added
        np.testing.assert_array_equal(bits(idx.get_rows(0, 4)), bits(rows[:4]))  # removed rows keep their values


def test_remove_validates_before_changing_anything(lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(3)
    with FlatIndex(64) as idx:
        idx.add(rng.standard_normal((100, 64)).astype(np.float32))
        for bad in ([5, 0], [5, 101], [2 ** 63]):
            with pytest.raises(_lib.MemexHipError) as ei:
                idx.remove(bad)
            assert ei.value.code == _lib.MX_EINVAL
            assert idx.removed == 0
        assert idx.remove([5, 5, 6]) == 2                      # repeated within the call: counted once
        assert idx.remove([5, 7]) == 1                         # already removed: not an error
        assert idx.remove([]) == 0
        assert idx.removed == 3 and len(idx) == 100
        idx.set_id_offset(1000)
        with pytest.raises(_lib.MemexHipError):
            idx.remove([8])                                    # ids carry the offset
        assert idx.remove([1008]) == 1
        ids, _, _, _ = idx.search(rng.standard_normal((4, 64)).astype(np.float32), 100)
        assert not np.isin(ids, [1005, 1006, 1007, 1008]).any() and (ids[:, :96] > 1000).all()
        idx.clear()                                            # forgets every removal
        assert idx.removed == 0
        idx.add(rng.standard_normal((10, 64)).astype(np.float32))
        ids, _, _, nf = idx.search(rng.standard_normal((2, 64)).astype(np.float32), 10)
        assert (nf == 10).all()


def test_adversarial_sample_block_of_removed_near_copies(oracle, lib_built):
    """Rows near cosine 0.3 to the queries, then 20k near-copies of the queries, then the copies removed.  A sample launch that
    ignored the mask would set theta near 1 from the copies and drop the live neighbours without any overflow to catch it."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(11)
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
    rows = np.concatenate([X, copies])
    alive = np.ones(rows.shape[0], dtype=bool)
    Qf = Q.astype(np.float32)
    for kind in ("i8", "bf16", False):
        with FlatIndex(d) as idx:
            idx.set_filter_copy(kind)
            idx.add(rows)
            a = alive.copy()
            remove(idx, a, np.arange(n, n + 20000))
            idx.reset_stats()
            check(idx, oracle, rows, a, Qf, 10, f"adversarial, copy {kind}")
            st = idx.stats()
            assert st.fallback_queries == 0, kind
            assert st.filter_demotions == 0, kind


def test_sharded_remove_matches_oracle(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(5)
    d, n = 384, 30000
    X = corpus(rng, n, d)
    Q = rng.standard_normal((33, d)).astype(np.float32)
    Q[0] = X[1234]
    for G, R in ((2, 4096), (3, 96)):
        with FlatIndex(d, devices=[0] * G, block_rows=R) as idx:
            idx.add(X)
            alive = np.ones(n, dtype=bool)
            for r in (rng.choice(n, 300, replace=False), np.r_[1234, 0:64, R - 1:R + 1], np.arange(1, n, 2)):
                remove(idx, alive, r)
                check(idx, oracle, X, alive, Q, 10, f"{G} shards")
            check(idx, oracle, X, alive, Q[:4], 300, f"{G} shards, k = 300")
            with pytest.raises(Exception):
                idx.remove([1, n + 1])                         # all-or-nothing across shards
            assert idx.removed == int((~alive).sum())
            # fewer live rows than k on the whole handle: n_found counts live rows, the merged tail holds no empty slots
            keep = np.flatnonzero(alive)[rng.choice(int(alive.sum()), 200, replace=False)]
            remove(idx, alive, np.setdiff1d(np.flatnonzero(alive), keep))
            check(idx, oracle, X, alive, Q[:4], 300, f"{G} shards, k = 300 > 200 live rows")
            remove(idx, alive, keep[9:])
            ids, _, _, nf = idx.search(Q, 10)
            assert (nf == 9).all(), f"{G} shards: all but k-1"
            check(idx, oracle, X, alive, Q, 10, f"{G} shards, all but k-1")
            Z = np.zeros((2, d), dtype=np.float32)                 # zero queries: the first live rows by id
            check(idx, oracle, X, alive, Z, 10, f"{G} shards, zero query")


def test_zero_query_after_a_long_removed_prefix(oracle, lib_built):
    """A zero query ties every row at dist 0 and takes the first live rows by id: with 150k removed rows in front of them."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(21)
    d, n = 64, 200000
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = np.zeros((3, d), dtype=np.float32)
    Q[1] = X[160000]
    for mode in (0, 1):                                         # the fast path and the EXACT path
        with FlatIndex(d) as idx:
            idx.set_search_mode(mode)
            idx.add(X)
            alive = np.ones(n, dtype=bool)
            remove(idx, alive, np.r_[0:150000, 150001:150003, 150500])
            check(idx, oracle, X, alive, Q, 40, f"mode {mode}")
            check(idx, oracle, X, alive, Q, 300, f"mode {mode}, k = 300")


def test_side_lists_count_live_rows(oracle, lib_built):
    """Removed zero-norm rows leave the zero-row list: 1000 of them, 900 removed, 500 more appended = 600 live ones, within the
    list's 1024 -- the fast path keeps serving (it did not when removed rows still counted), bit-exact to the oracle."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(22)
    d, n = 128, 40000
    X = rng.standard_normal((n, d)).astype(np.float32)
    zero = rng.choice(n, 1000, replace=False)
    X[zero] = 0
    Q = rng.standard_normal((16, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        alive = np.ones(n, dtype=bool)
        remove(idx, alive, zero[:900])
        Y = rng.standard_normal((3000, d)).astype(np.float32)
        Y[rng.choice(3000, 500, replace=False)] = 0
        idx.add(Y)
        rows = np.concatenate([X, Y])
        alive = np.r_[alive, np.ones(3000, dtype=bool)]
        idx.reset_stats()
        check(idx, oracle, rows, alive, Q, 10, "600 live zero-norm rows")
        assert idx.stats().scan_launches > 0                   # the scan pipeline, not the EXACT path
        assert idx.stats().fallback_queries == 0
        remove(idx, alive, np.flatnonzero((np.abs(rows).sum(1) == 0) & alive)[:100])
        check(idx, oracle, rows, alive, Q, 10, "after removing 100 more")


# ---- persistence ---------------------------------------------------------------------------------------------------
def dead_path(p):
    return os.path.join(str(p), "vectors.mxdead")


def test_remove_save_load_roundtrip_and_append(oracle, lib_built, tmp_path):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(8)
    d, n = 128, 5000
    X = corpus(rng, n, d)
    Q = rng.standard_normal((16, d)).astype(np.float32)
    alive = np.ones(n, dtype=bool)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.save(str(tmp_path))
        assert not os.path.exists(dead_path(tmp_path))         # nothing removed: no companion file
        remove(idx, alive, [3, 4, 5, 4999])
        idx.save(str(tmp_path))
        s1 = os.path.getsize(dead_path(tmp_path))
        assert s1 == 16 + 8 * 4
        remove(idx, alive, [5, 6, 7])                          # 5 again: only two new removals
        idx.save(str(tmp_path))
        assert os.path.getsize(dead_path(tmp_path)) == s1 + 8 * 2
        idx.save(str(tmp_path))                                # nothing new
        assert os.path.getsize(dead_path(tmp_path)) == s1 + 8 * 2
        idx.add(X[:10])                                        # new rows and a new removal in one save
        alive = np.r_[alive, np.ones(10, dtype=bool)]
        remove(idx, alive, [n + 2])
        idx.save(str(tmp_path))
        assert os.path.getsize(dead_path(tmp_path)) == s1 + 8 * 3
        rows = np.concatenate([X, X[:10]])
        check(idx, oracle, rows, alive, Q, 10, "before reload")
        idx.load(str(tmp_path))                                # O(1) re-attach keeps the removals
        assert idx.removed == int((~alive).sum())
        check(idx, oracle, rows, alive, Q, 10, "re-attached")
    with FlatIndex(d) as fresh:
        fresh.load(str(tmp_path))
        assert fresh.removed == int((~alive).sum()) and len(fresh) == n + 10
        check(fresh, oracle, rows, alive, Q, 10, "fresh handle")
    with FlatIndex(d) as other:                                # a handle with unsaved removals takes the file's on reload
        other.load(str(tmp_path))
        other.remove([100])
        other.load(str(tmp_path))
        assert other.removed == int((~alive).sum())
        FlatIndex.remove_files(str(tmp_path))
    assert not os.path.exists(dead_path(tmp_path)) and not FlatIndex.has_store(str(tmp_path))


def test_damaged_companion_file_fails_load_and_leaves_index(oracle, lib_built, tmp_path):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(9)
    d, n = 64, 3000
    X = corpus(rng, n, d)
    Q = rng.standard_normal((8, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.remove([1, 2, 3])
        idx.save(str(tmp_path))
    good = open(dead_path(tmp_path), "rb").read()
    bad_files = {
        "truncated": good[:-4],
        "short header": good[:10],
        "wrong magic": b"XXDEAD01" + good[8:],
        "row past the end": good[:16] + np.uint64(n).tobytes() + good[24:],
        "count too large": good[:8] + np.uint64(4).tobytes() + good[16:],
    }
    alive = np.ones(n, dtype=bool)
    alive[[10, 11]] = False
    for what, data in bad_files.items():
        with open(dead_path(tmp_path), "wb") as f:
            f.write(data)
        with FlatIndex(d) as idx:
            idx.add(X)
            idx.remove([11, 12])
            with pytest.raises(_lib.MemexHipError) as ei:
                idx.load(str(tmp_path))
            assert ei.value.code == _lib.MX_EIO, what
            assert len(idx) == n and idx.removed == 2, what  # left as it was
            check(idx, oracle, X, alive, Q, 10, what)
    os.remove(dead_path(tmp_path))                            # a store written before removals existed: loads unchanged
    with FlatIndex(d) as idx:
        idx.load(str(tmp_path))
        assert idx.removed == 0 and len(idx) == n
        check(idx, oracle, X, np.ones(n, dtype=bool), Q, 10, "no companion file")


def test_store_remove_roundtrip(lib_built, tmp_path):
    from memex_amd import storage
    rng = np.random.default_rng(12)
    d = 32
    vecs = rng.standard_normal((50, d)).astype(np.float32)
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    st.bulk_insert([storage.VectorData(_id=f"seg{i % 40}", document_id="doc", text="", vector=list(map(float, v))) for i, v in enumerate(vecs)])
    assert st.remove("seg3") == 2                              # inserted twice under one _id: both rows go
    assert st.remove(["seg5", "nope"]) == 2
    assert st.remove("nope") == 0                              # unknown _id: a no-op
    st.bulk_insert([storage.VectorData(_id="seg3", document_id="doc", text="", vector=list(map(float, vecs[3])))])
    assert st.remove(["seg3"]) == 1                            # the reverse map follows inserts
    res = st.search(list(map(float, vecs[3])), 60)
    assert all(r[0] not in ("seg3", "seg5") for r in res) and len(res) == 51 - 5
    storage.evict_resident()
    again = storage.HipFlatStore.load(str(tmp_path / "col"))
    res2 = again.search(list(map(float, vecs[3])), 60)
    assert res2 == res
    with pytest.raises(NotImplementedError):
        again.delete("seg1")                                   # delete keeps the reference's contract
    again.delete_all()
    assert not os.path.exists(dead_path(tmp_path / "col"))


# ---- concurrency ---------------------------------------------------------------------------------------------------
def test_search_after_remove_never_returns_removed(lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(13)
    d, n = 128, 40000
    X = rng.standard_normal((n, d)).astype(np.float32)
    order = rng.permutation(n)[:4000] + 1
    Qs = X[order - 1] + rng.standard_normal((4000, d)).astype(np.float32) * 0.01  # queries whose best row is being removed
    done_upto = [0]                                            # ids order[:done_upto] have been removed (remove returned)
    stop = threading.Event()
    errors = []
    with FlatIndex(d) as idx:
        idx.add(X)

        def searcher(seed):
            r = np.random.default_rng(seed)
            try:
                while not stop.is_set():
                    upto = done_upto[0]                        # read BEFORE the call starts
                    j = r.integers(0, 4000, 8)
                    ids, _, _, _ = idx.search(Qs[j], 5)
                    gone = set(order[:upto].tolist())
                    hit = [int(i) for i in ids.ravel() if int(i) in gone]
                    if hit:
                        errors.append(hit)
                        return
            except Exception as e:                            # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=searcher, args=(s,)) for s in range(4)]
        for t in threads:
            t.start()
        try:
            for c in range(0, 4000, 100):
                idx.remove(order[c:c + 100])
                done_upto[0] = c + 100
        finally:
            stop.set()
            for t in threads:
                t.join()
    assert not errors, errors[:3]
