"""Compaction (mx_index_compact): removed rows are dropped for good and the live rows get dense ids again.  After every
removal pattern and for every scan kind a search must be bit-identical to the oracle run on the live rows with the new ids, and
the old -> new map applied to the answer before compaction must give the same ids, scores and dists."""
import os
import struct
import threading

import numpy as np
import pytest

from conftest import bits
from test_remove_gpu import _KINDS, corpus

pytestmark = pytest.mark.gpu


def oracle_check(idx, oracle, live_rows, Q, k, what=""):
    ids, sc, di, nf = idx.search(Q, k)
    oi, od, os_, onf = oracle.search(live_rows, Q, k)
    np.testing.assert_array_equal(nf, onf, err_msg=what)
    np.testing.assert_array_equal(ids, oi.astype(np.uint64), err_msg=what)
    np.testing.assert_array_equal(bits(di), bits(od), err_msg=what)
    np.testing.assert_array_equal(bits(sc), bits(os_), err_msg=what)
    return ids, sc, di, nf


def build(name, d, setup, X, cone):
    from memex_amd.index import FlatIndex
    idx = FlatIndex(d)
    if setup is not None and name == "compressed":
        setup(idx)
    idx.add(X)
    if setup is not None and name != "compressed":
        setup(idx)
    if cone:
        idx.set_filter_copy(False)
        idx.set_filter_copy("i8")                              # rebuilt from a populated cone: centred
        assert idx.stats().filter_centred == 1
    return idx


def fresh_filter_bytes(name, d, live_rows):
    """filter_copy_bytes of a fresh index of the same filter kind and corpus mode holding the live rows (reserved up front: a
    large host add grows in 64 MiB pieces, by half the capacity at a time)"""
    from memex_amd.index import FlatIndex
    with FlatIndex(d) as f:
        if name == "compressed":
            f.set_corpus_mode("bf16")
        elif name == "bf16" or name == "wide_1536":
            f.set_filter_copy("bf16")
        elif name == "f32":
            f.set_filter_copy(False)
        elif name == "centred_int8":
            f.set_filter_copy("i8")
        f.reserve(len(live_rows))
        f.add(live_rows)
        return f.stats().filter_copy_bytes


def patterns(rng, n):
    runs = np.concatenate([np.arange(s, min(s + int(rng.integers(50, 700)), n)) for s in rng.choice(n - 1, 12, replace=False)])
    return [
        ("1% random", rng.choice(n, n // 100, replace=False)),
        ("runs", runs),
        ("the whole first tile", np.arange(64)),
        ("every other row", np.arange(0, n, 2)),
        ("all but k-1", np.setdiff1d(np.arange(n), rng.choice(n, 9, replace=False))),
        ("all rows", np.arange(n)),
    ]


@pytest.mark.parametrize("name,d,n,setup", _KINDS, ids=[c[0] for c in _KINDS])
def test_compact_patterns_match_oracle_on_live_rows(name, d, n, setup, oracle, lib_built):
    rng = np.random.default_rng(100 + sum(map(ord, name)))
    cone = name == "centred_int8"
    X = corpus(rng, n, d, cone=cone)
    if name == "compressed":
        X[[11, n - 100]] = rng.standard_normal((2, d)).astype(np.float32)
    Q = rng.standard_normal((16, d)).astype(np.float32)
    Q[1] = X[99] * 3.0
    Q[2] = X[2000]
    Q[3] = 0.0                                                 # a zero query: the first live rows by id
    for what, r in patterns(rng, n):
        idx = build(name, d, setup, X, cone)
        try:
            rows = idx.get_rows(0, n) if name == "compressed" else X
            alive = np.ones(n, dtype=bool)
            alive[r] = False
            idx.remove(np.asarray(r, dtype=np.uint64) + 1)
            before = idx.search(Q, 10)
            kept = idx.compact()
            L = int(alive.sum())
            np.testing.assert_array_equal(kept, np.flatnonzero(alive).astype(np.uint64) + 1, err_msg=f"{name}: {what}")
            assert len(idx) == L and idx.removed == 0, f"{name}: {what}"
            if L == 0:
                assert (idx.search(Q, 10)[3] == 0).all()
                continue
            ids, sc, di, nf = oracle_check(idx, oracle, rows[alive], Q, 10, f"{name}: {what}")
            # the old -> new map: the answer before compaction, renumbered, is the answer after it
            old = np.where(ids > 0, kept[np.maximum(ids.astype(np.int64) - 1, 0)], 0)
            np.testing.assert_array_equal(old, before[0], err_msg=f"{name}: {what}")
            np.testing.assert_array_equal(bits(sc), bits(before[1]), err_msg=f"{name}: {what}")
            np.testing.assert_array_equal(bits(di), bits(before[2]), err_msg=f"{name}: {what}")
            np.testing.assert_array_equal(nf, before[3], err_msg=f"{name}: {what}")
            np.testing.assert_array_equal(bits(idx.get_rows(0, L)), bits(rows[alive]), err_msg=f"{name}: {what}")
            assert idx.stats().filter_copy_bytes == fresh_filter_bytes(name, d, rows[alive]), f"{name}: {what}: capacity released"
            if cone:
                assert idx.stats().filter_centred == 1         # the centring the index had
        finally:
            idx.close()


def test_compact_with_nothing_removed_is_a_noop_and_saves_append(lib_built, tmp_path):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(3)
    X = rng.standard_normal((3000, 64)).astype(np.float32)
    with FlatIndex(64) as idx:
        idx.add(X)
        idx.save(str(tmp_path))
        ino = os.stat(tmp_path / "vectors.mxflat").st_ino
        before = idx.search(X[:5], 10)
        np.testing.assert_array_equal(idx.compact(), np.arange(1, 3001, dtype=np.uint64))
        idx.add(X[:10])
        idx.save(str(tmp_path))
        assert os.stat(tmp_path / "vectors.mxflat").st_ino == ino   # appended, not rewritten
        assert open(tmp_path / "vectors.mxflat", "rb").read(8) == b"MXFLAT01"
        after = idx.search(X[:5], 10)
        assert (after[3] == before[3]).all()


def test_compact_restores_overflowed_side_list(oracle, lib_built):
    """80 rows with a norm of 1e20 overflow their list (cap 64): the index answers on the EXACT path.  Removing 30 and compacting
    makes the list complete again: the index leaves the EXACT path with oracle-exact answers."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(9)
    n, d = 6000, 128
    X = rng.standard_normal((n, d)).astype(np.float32)
    wild = rng.choice(n, 80, replace=False)
    X[wild] *= np.float32(1e20) / np.linalg.norm(X[wild], axis=1, keepdims=True)
    Q = rng.standard_normal((8, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.reset_stats()
        oracle_check(idx, oracle, X, Q, 10, "overflowed list")
        assert idx.stats().scan_launches == 0                  # the EXACT path
        alive = np.ones(n, dtype=bool)
        alive[wild[:30]] = False
        idx.remove(wild[:30] + 1)
        idx.compact()
        idx.reset_stats()
        oracle_check(idx, oracle, X[alive], Q, 10, "after compaction")
        st = idx.stats()
        assert st.fallback_queries == 0 and st.scan_launches > 0
        assert st.listed_rows == 50


def test_appends_removals_and_a_second_compaction(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(21)
    d = 384
    X = corpus(rng, 20000, d)
    Q = rng.standard_normal((12, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        model = list(range(20000))                             # model[i] = row of X behind id i + 1
        gone = set(rng.choice(20000, 3000, replace=False).tolist())
        idx.remove(np.array(sorted(gone), dtype=np.uint64) + 1)
        idx.compact()
        model = [r for r in model if r not in gone]
        Y = rng.standard_normal((5000, d)).astype(np.float32)
        assert idx.add(Y) == len(model) + 1                    # ids continue at live + 1
        allrows = np.concatenate([X, Y])
        model += list(range(20000, 25000))
        oracle_check(idx, oracle, allrows[model], Q, 10, "append after compaction")
        drop = rng.choice(len(model), 4000, replace=False)
        idx.remove(drop.astype(np.uint64) + 1)
        kept = idx.compact()
        keep_mask = np.ones(len(model), dtype=bool)
        keep_mask[drop] = False
        np.testing.assert_array_equal(kept, np.flatnonzero(keep_mask).astype(np.uint64) + 1)
        model = [m for m, k in zip(model, keep_mask) if k]
        oracle_check(idx, oracle, allrows[model], Q, 10, "second compaction")
        np.testing.assert_array_equal(bits(idx.get_rows(0, len(model))), bits(allrows[model]))


@pytest.mark.parametrize("G", [2, 3, 8])
def test_sharded_compaction_matches_plain(G, oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(40 + G)
    d, n = 384, 30000
    X = corpus(rng, n, d)
    Q = rng.standard_normal((20, d)).astype(np.float32)
    Q[0] = X[1234]
    gone = np.unique(np.concatenate([rng.choice(n, 3000, replace=False), np.arange(0, 64), np.arange(4096, 4300)]))
    alive = np.ones(n, dtype=bool)
    alive[gone] = False
    with FlatIndex(d, devices=[0] * G, block_rows=4096 if G < 8 else 96) as sh, FlatIndex(d) as plain:
        sh.add(X)
        sh.remove(gone.astype(np.uint64) + 1)
        kept = sh.compact()
        np.testing.assert_array_equal(kept, np.flatnonzero(alive).astype(np.uint64) + 1)
        assert len(sh) == int(alive.sum()) and sh.removed == 0
        plain.add(X[alive])
        a, b = sh.search(Q, 10), plain.search(Q, 10)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8))
        oracle_check(sh, oracle, X[alive], Q, 10, f"{G} shards")
        np.testing.assert_array_equal(bits(sh.get_rows(0, int(alive.sum()))), bits(X[alive]))


# ---- persistence ----------------------------------------------------------------------------------------------------
def _files(p):
    return {name: open(os.path.join(p, name), "rb").read() for name in ("vectors.mxflat", "vectors.mxdead") if os.path.exists(os.path.join(p, name))}


def _put(p, files):
    os.makedirs(p, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(p, name), "wb") as f:
            f.write(data)


def test_compacted_save_load_and_reattach(oracle, lib_built, tmp_path):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(31)
    d, n = 96, 5000
    X = corpus(rng, n, d)
    Q = rng.standard_normal((10, d)).astype(np.float32)
    alive = np.ones(n, dtype=bool)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.save(str(tmp_path))
        r = rng.choice(n, 700, replace=False)
        idx.remove(r + 1)
        alive[r] = False
        idx.save(str(tmp_path))
        idx.compact()
        idx.save(str(tmp_path))
        raw = open(tmp_path / "vectors.mxflat", "rb").read(40)
        assert raw[:8] == b"MXFLAT02" and struct.unpack("<Q", raw[16:24])[0] == alive.sum() and struct.unpack("<Q", raw[24:32])[0] == 1
        assert not os.path.exists(tmp_path / "vectors.mxdead")
        ref = oracle_check(idx, oracle, X[alive], Q, 10, "compacted")
        idx.load(str(tmp_path))                                # O(1) re-attach
        oracle_check(idx, oracle, X[alive], Q, 10, "re-attached")
        # removals and appends after a compaction persist in the new generation
        idx.remove([1, 2])
        idx.add(X[:3])
        idx.save(str(tmp_path))
        assert open(tmp_path / "vectors.mxdead", "rb").read(8) == b"MXDEAD02"
        live2 = np.concatenate([X[alive][2:], X[:3]])
        with FlatIndex(d) as cold:
            cold.load(str(tmp_path))
            assert len(cold) == int(alive.sum()) + 3 and cold.removed == 2
            ids, *_ = cold.search(Q, 10)
            assert not np.isin(ids, [1, 2]).any()
            kept = cold.compact()
            oracle_check(cold, oracle, live2, Q, 10, "cold load, compacted again")
            assert kept[0] == 3
            cold.save(str(tmp_path / "g2"))
            assert struct.unpack("<Q", open(tmp_path / "g2" / "vectors.mxflat", "rb").read(32)[24:32])[0] == 2
        del ref


def test_every_crash_state_of_the_write_order_loads_old_or_new(oracle, lib_built, tmp_path):
    """a save after a compaction writes vectors.mxflat.tmp, renames it over vectors.mxflat, then removes (or
    replaces) vectors.mxdead.  Every intermediate file state loads as the old store, the new one, or fails with MX_EIO."""
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(44)
    d, n = 64, 3000
    X = rng.standard_normal((n, d)).astype(np.float32)
    r = rng.choice(n, 500, replace=False)
    alive = np.ones(n, dtype=bool)
    alive[r] = False
    old_dir, new_dir = str(tmp_path / "old"), str(tmp_path / "new")
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.remove(r + 1)
        idx.save(old_dir)
        idx.compact()
        idx.save(new_dir)
    old, new = _files(old_dir), _files(new_dir)
    assert old["vectors.mxflat"][:8] == b"MXFLAT01" and old["vectors.mxdead"][:8] == b"MXDEAD01"
    assert new["vectors.mxflat"][:8] == b"MXFLAT02" and "vectors.mxdead" not in new
    states = {
        "before the save": dict(old),
        "tmp written, not renamed": {**old, "vectors.mxflat.tmp": new["vectors.mxflat"]},
        "tmp half written": {**old, "vectors.mxflat.tmp": new["vectors.mxflat"][:1000]},
        "renamed, old removal file still there": {"vectors.mxflat": new["vectors.mxflat"], "vectors.mxdead": old["vectors.mxdead"]},
        "after the save": dict(new),
    }
    Q = rng.standard_normal((6, d)).astype(np.float32)
    want_old = oracle.search(X[alive], Q, 10)
    for what, files in states.items():
        p = str(tmp_path / what.replace(" ", "_").replace(",", ""))
        _put(p, files)
        with FlatIndex(d) as idx:
            try:
                idx.load(p)
            except _lib.MemexHipError as e:
                assert e.code == _lib.MX_EIO, what
                continue
            if len(idx) == n:                                  # the old store: its removals apply
                assert idx.removed == 500, what
                ids, *_ = idx.search(Q, 10)
                live_ids = np.flatnonzero(alive).astype(np.uint64) + 1
                np.testing.assert_array_equal(ids, live_ids[want_old[0].astype(np.int64) - 1], err_msg=what)
            else:                                              # the new one: nothing removed, dense ids
                assert len(idx) == int(alive.sum()) and idx.removed == 0, what
                oracle_check(idx, oracle, X[alive], Q, 10, what)
                np.testing.assert_array_equal(bits(idx.get_rows(0, len(idx))), bits(X[alive]), err_msg=what)
                idx.save(p)                                    # a stale removal file is replaced (here: removed) on the next save
                assert not os.path.exists(os.path.join(p, "vectors.mxdead")), what


def test_store_compact_survives_reload(lib_built, tmp_path):
    from memex_amd import storage
    rng = np.random.default_rng(12)
    d = 32
    vecs = rng.standard_normal((60, d)).astype(np.float32)
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    st.bulk_insert([storage.VectorData(_id=f"seg{i}", document_id="doc", text="", vector=list(map(float, v))) for i, v in enumerate(vecs)])
    assert st.remove([f"seg{i}" for i in range(0, 60, 4)]) == 15
    kept = st.compact()
    assert kept.size == 45 and st._id_map == {i + 1: f"seg{int(k) - 1}" for i, k in enumerate(kept)}
    res = st.search(list(map(float, vecs[5])), 50)
    assert res[0][0] == "seg5" and len(res) == 45
    st.bulk_insert([storage.VectorData(_id="late", document_id="doc", text="", vector=list(map(float, vecs[0])))])
    assert st._id_map[46] == "late"
    res = st.search(list(map(float, vecs[5])), 50)
    storage.evict_resident()                                   # (st lets go of its index: a cold load follows)
    again = storage.HipFlatStore.load(str(tmp_path / "col"))
    assert again._id_map == st._id_map
    assert again.search(list(map(float, vecs[5])), 50) == res
    assert again.remove("seg5") == 1                            # the reverse map follows the renumbering
    assert all(r[0] != "seg5" for r in again.search(list(map(float, vecs[5])), 50))


def test_store_crash_between_vectors_and_id_map_fails_load(lib_built, tmp_path):
    """vectors rewritten by the compaction, vectors.meta.json still the old one: load raises FileIOError, never maps wrongly"""
    import shutil
    from memex_amd import storage
    rng = np.random.default_rng(13)
    vecs = rng.standard_normal((40, 16)).astype(np.float32)
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    st.bulk_insert([storage.VectorData(_id=f"s{i}", document_id="d", text="", vector=list(map(float, v))) for i, v in enumerate(vecs)])
    st.remove("s3")
    shutil.copy(tmp_path / "col" / "vectors.meta.json", tmp_path / "meta.old")
    st.compact()
    crash = tmp_path / "crash"
    os.makedirs(crash)
    shutil.copy(tmp_path / "col" / "vectors.mxflat", crash / "vectors.mxflat")
    shutil.copy(tmp_path / "meta.old", crash / "vectors.meta.json")
    with pytest.raises(storage.FileIOError):
        storage.HipFlatStore.load(str(crash))


# ---- concurrency ------------------------------------------------------------------------------------------------------
def test_searches_during_compaction_see_old_or_new(lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(77)
    d, n = 384, 60000
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = X[rng.choice(n, 8, replace=False)] + 0.01 * rng.standard_normal((8, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.remove(rng.choice(n, 6000, replace=False) + 1)
        old = [idx.search(Q[i:i + 1], 10) for i in range(8)]
        results, errors = [], []
        stop = threading.Event()

        def worker(i):
            try:
                while not stop.is_set():
                    results.append((i, idx.search(Q[i:i + 1], 10)))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
        for t in th:
            t.start()
        idx.compact()
        new = [idx.search(Q[i:i + 1], 10) for i in range(8)]
        stop.set()
        for t in th:
            t.join()
        assert not errors
        same = lambda a, b: all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) for u, v in zip(a, b))  # noqa: E731
        for i, r in results:
            assert same(r, old[i]) or same(r, new[i])
