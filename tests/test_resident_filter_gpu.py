"""Resident filters (mx_filter): an allow-set kept as a bitmap next to the rows and named in a search.  Every
search answer is held, bit for bit, against two references: the per-call filtered search on the same index with the ranges the
filter reports, and the oracle run on the allowed rows that are not removed.  The set itself (ranges(), count()) is held against a
NumPy boolean model."""
import threading
import time

import numpy as np
import pytest

from filtered_model import allowed_mask, ids_of, model_ranges, subset_oracle
from test_filtered_gpu import same, shapes
from test_remove_gpu import corpus

pytestmark = pytest.mark.gpu

D, N = 384, 20037                      # deliberately no multiple of 64


def check_set(flt, model, alive, what, off=0):
    np.testing.assert_array_equal(flt.ranges(), model_ranges(model, off), err_msg=what)
    assert flt.count() == (int(model.sum()), int((model & alive).sum())), what


def check_search(idx, flt, oracle, rows, model, alive, Q, k, what, off=0):
    """resident == per-call with the reported ranges == oracle on the allowed live rows"""
    got = idx.search_with(flt, Q, k)
    same(got, idx.search_filtered(Q, k, ranges=flt.ranges()), what + ": per-call filter")
    same(got, subset_oracle(oracle, rows, model & alive, Q, k, off), what + ": oracle")
    return got


def both_paths(monkeypatch, idx, flt, Q, k, want, what):
    for v in ("0", "1"):
        monkeypatch.setenv("MEMEX_HIP_DEBUG", "filt_subset=" + v)
        same(idx.search_with(flt, Q, k), want, f"{what}: filt_subset={v}")
    monkeypatch.delenv("MEMEX_HIP_DEBUG")


def queries(rng, rows):
    Q = rng.standard_normal((16, rows.shape[1])).astype(np.float32)
    Q[1] = rows[130] * 2.0
    Q[2] = rows[min(8000, rows.shape[0] - 1)]
    Q[3] = 0.0                          # the zero query: the first allowed live rows by id
    return Q


_KINDS = [("int8", None, lambda idx: idx.set_filter_copy("i8")),
          ("f32", None, lambda idx: idx.set_filter_copy(False)),
          ("compressed", lambda idx: idx.set_corpus_mode("bf16"), None)]


@pytest.mark.parametrize("name,pre,post", _KINDS, ids=[c[0] for c in _KINDS])
def test_shapes(name, pre, post, oracle, lib_built, monkeypatch):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(sum(map(ord, name)) + 11)
    X = corpus(rng, N, D)
    if name == "compressed":
        X[[11, N - 100]] = rng.standard_normal((2, D)).astype(np.float32)
    with FlatIndex(D) as idx:
        if pre:
            pre(idx)
        idx.add(X)
        if post:
            post(idx)
        rows = idx.get_rows(0, N) if name == "compressed" else X
        Q = queries(rng, rows)
        alive = np.ones(N, dtype=bool)
        cases = shapes(rng, N)
        for phase in ("nothing removed", "removals"):
            if phase == "removals":             # allowed rows, a whole tile, the zero-norm and the 1e20-norm rows
                gone = np.unique(np.r_[rng.choice(N, N // 50, replace=False), 120:140, 7, 300, 11, N - 100, 8000, 5056:5120])
                assert idx.remove(gone + 1) > 0
                alive[gone] = False
            for what, r in cases:
                model = allowed_mask(N, r)
                built = [("ranges", dict(ranges=r))]
                if model.sum() <= 20000:
                    built.append(("ids", dict(ids=rng.permutation(np.r_[ids_of(r), ids_of(r)[:50]]))))
                for how, kw in built:
                    tag = f"{name}, {phase}, {what}, by {how}"
                    with idx.make_filter(**kw) as flt:
                        check_set(flt, model, alive, tag)
                        got = check_search(idx, flt, oracle, rows, model, alive, Q, 10, tag + ", k = 10")
                        check_search(idx, flt, oracle, rows, model, alive, Q[:4], 300, tag + ", k = 300")
                        if 0 < (model & alive).sum() <= 16384:
                            both_paths(monkeypatch, idx, flt, Q, 10, got, tag)


def test_word_edges(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(21)
    n = N
    X = corpus(rng, n, D)
    Q = queries(rng, X)
    alive = np.ones(n, dtype=bool)
    j = 17
    edges = [[[64 * j, 64 * j + 1]], [[64 * j + 63, 64 * j + 65]], [[64 * j + 1, 64 * j + 64]], [[1, 2]], [[n, n + 1]],
             [[64 * j + 10, 64 * j + 20]], [[n - 5, n + 1000]], [[64, 128], [128, 129], [191, 193]],
             [[1, n + 1]]]
    with FlatIndex(D) as idx:
        idx.add(X)
        for r in edges:
            r = np.array(r)
            for how in ("ranges", "ids"):
                ids = rng.permutation(np.r_[ids_of(r), ids_of(r)[:7], ids_of(r)[:7]])   # repeats; some name no row
                with (idx.make_filter(ranges=r) if how == "ranges" else idx.make_filter(ids=ids)) as flt:
                    model = allowed_mask(n, r)
                    check_set(flt, model, alive, f"{r.tolist()} by {how}")
                    check_search(idx, flt, oracle, X, model, alive, Q[:4], 10, f"{r.tolist()} by {how}")
                    # the same rows taken away from the full set, through the other kernel's opposite operation
                    flt.allow(ranges=[[1, n + 1]])
                    if how == "ranges":
                        flt.deny(ranges=r)
                    else:
                        flt.deny(ids=ids)
                    check_set(flt, ~model, alive, f"all but {r.tolist()} by {how}")
                    check_search(idx, flt, oracle, X, ~model, alive, Q[:4], 10, f"all but {r.tolist()} by {how}")
        with idx.make_filter() as flt:                                  # the empty filter finds nothing
            assert flt.count() == (0, 0) and flt.ranges().shape == (0, 2)
            ids_, sc, di, nf = idx.search_with(flt, Q, 10)
            assert (nf == 0).all() and (ids_ == 0).all() and np.isinf(di).all()
            flt.allow(ids=np.zeros(0, np.uint64))
            flt.allow(ids=[0, n + 1, 2 ** 63])                          # ids that name no row are ignored
            assert flt.count() == (0, 0)
            with pytest.raises(Exception, match="lo > hi"):
                flt.allow(ranges=[[1, 50], [9, 8]])
            assert flt.count() == (0, 0)                                # a failing call changes nothing


def test_set_algebra(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(22)
    X = corpus(rng, N, D)
    Q = queries(rng, X)
    alive = np.ones(N, dtype=bool)
    gone = rng.choice(N, 400, replace=False)
    alive[gone] = False
    with FlatIndex(D) as idx:
        idx.add(X)
        idx.remove(gone + 1)
        model = np.zeros(N, dtype=bool)
        with idx.make_filter() as flt:
            for step in range(40):
                allow = bool(rng.integers(0, 3))                        # two allows to one deny
                if rng.integers(0, 2):
                    m = int(rng.integers(1, 30))
                    lo = rng.integers(0, N + 200, m)
                    r = np.stack([lo, lo + rng.integers(0, (3000 if step % 4 else 40), m)], 1)
                    (flt.allow if allow else flt.deny)(ranges=r)
                    model[allowed_mask(N, r)] = allow
                else:
                    ids = rng.integers(0, N + 200, int(rng.integers(1, 4000)))
                    (flt.allow if allow else flt.deny)(ids=ids)
                    ok = ids[(ids >= 1) & (ids <= N)]
                    model[ok - 1] = allow
                check_set(flt, model, alive, f"step {step}")
                if step % 10 == 9:
                    check_search(idx, flt, oracle, X, model, alive, Q, 10, f"step {step}")


def test_growth(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(23)
    n, more = 3000, 5000
    X = corpus(rng, n + more, D)
    Q = queries(rng, X)
    with FlatIndex(D) as idx:
        idx.reserve(n)
        idx.add(X[:n])
        with idx.make_filter(ranges=[[n - 40, n + 1000]]) as flt:       # "past the end" when it was made
            idx.add(X[n:])                                              # past a capacity growth
            alive = np.ones(n + more, dtype=bool)
            model = allowed_mask(n, [[n - 40, n + 1]])
            model = np.r_[model, np.zeros(more, dtype=bool)]
            check_set(flt, model, alive, "after growth: none of the new rows")
            check_search(idx, flt, oracle, X, model, alive, Q, 10, "after growth")
            flt.allow(ids=np.arange(n + 1, n + more + 1)[::3])
            model[n::3] = True
            check_set(flt, model, alive, "new ids allowed")
            got = check_search(idx, flt, oracle, X, model, alive, Q, 10, "new ids allowed")
            np.testing.assert_array_equal(got[0][3], np.flatnonzero(model)[:10] + 1)   # the zero query
            flt.allow(ranges=[[n + 1, n + more + 1]])
            model[n:] = True
            check_set(flt, model, alive, "new range allowed")
            check_search(idx, flt, oracle, X, model, alive, Q, 300, "new range allowed, k = 300")


@pytest.mark.parametrize("r", [[[1001, 1201]], [[N // 4, N // 4 + N // 2]]], ids=["subset", "masked"])
def test_removals_after_creation(r, oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(24)
    X = corpus(rng, N, D)
    Q = queries(rng, X)
    alive = np.ones(N, dtype=bool)
    model = allowed_mask(N, r)
    with FlatIndex(D) as idx:
        idx.add(X)
        with idx.make_filter(ranges=r) as flt:
            idx.reset_stats()
            first = check_search(idx, flt, oracle, X, model, alive, Q, 10, "before")
            st = idx.stats()
            assert st.filtered_queries == 32                            # the resident and the per-call search, 16 queries each
            assert st.subset_queries == (32 if model.sum() == 200 else 0)   # 200 rows: the subset kernel; half the corpus: the masked scan
            same(idx.search_with(flt, Q, 10), first, "again, from the cached list and counts")
            gone = np.flatnonzero(model)[::3]
            gone = np.r_[gone, first[0][0, 0] - 1].astype(np.int64)     # and the best row of query 0
            idx.remove(np.unique(gone) + 1)
            alive[gone] = False
            check_set(flt, model, alive, "after removals")              # n_live drops, n_allowed stays
            second = check_search(idx, flt, oracle, X, model, alive, Q, 10, "after removals")
            assert not np.isin(second[0], gone + 1).any()


def test_staleness_and_lifetime(oracle, lib_built, tmp_path):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(25)
    n = 5000
    X = corpus(rng, n, D)
    Q = queries(rng, X)
    alive = np.ones(n, dtype=bool)

    def stale(idx, flt):
        for call in (lambda: idx.search_with(flt, Q, 10), lambda: flt.allow(ranges=[[1, 5]]), lambda: flt.allow(ids=[3]),
                     flt.count, flt.ranges):
            with pytest.raises(_lib.MemexHipError, match="stale") as e:
                call()
            assert e.value.code == _lib.MX_EINVAL
        flt.close()                                                     # still works

    with FlatIndex(D) as idx, FlatIndex(D) as other:
        idx.add(X)
        other.add(X[:100])
        model = allowed_mask(n, [[100, 2000]])
        flt = idx.make_filter(ranges=[[100, 2000]])
        assert idx.compact().size == n                                  # nothing removed: a no-op, the filter stays valid
        check_search(idx, flt, oracle, X, model, alive, Q, 10, "after a no-op compact")
        with pytest.raises(_lib.MemexHipError, match="another index") as e:
            other.search_with(flt, Q, 10)
        assert e.value.code == _lib.MX_EINVAL
        idx.remove([5, 150])
        idx.compact()
        stale(idx, flt)
        flt = idx.make_filter(ids=[1, 2, 3])
        idx.save(str(tmp_path))
        idx.load(str(tmp_path))
        stale(idx, flt)
        flt = idx.make_filter(ids=[1, 2, 3])
        idx.clear()
        stale(idx, flt)
    # a filter keeps the rows of a keyed index after the owner dropped its handle
    owner = FlatIndex(D, key="resident-filter-lifetime")
    owner.add(X)
    flt = owner.make_filter(ranges=[[100, 2000]])
    want = owner.search_with(flt, Q, 10)
    owner.close()
    again = FlatIndex(D, key="resident-filter-lifetime")                # the same resident rows: the filter's reference kept them
    try:
        assert len(again) == n
        same(again.search_with(flt, Q, 10), want, "after the owner closed")
        same(want, subset_oracle(oracle, X, model, Q, 10), "oracle")
    finally:
        flt.close()
        again.clear()
        again.close()


def test_id_offset(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(26)
    n, off = N, 1_000_000
    X = corpus(rng, n, D)
    Q = queries(rng, X)
    alive = np.ones(n, dtype=bool)
    with FlatIndex(D) as idx:
        idx.add(X)
        idx.set_id_offset(off)                                          # before creation
        r = np.array([[off + 50, off + 120], [0, off + 3], [off + 15000, off + 10 ** 9]])
        model = allowed_mask(n, r, off)
        with idx.make_filter(ranges=r) as flt:
            check_set(flt, model, alive, "offset before", off)
            check_search(idx, flt, oracle, X, model, alive, Q, 10, "offset before", off)
            flt.deny(ids=[off + 51, 51, off])                           # only off + 51 names a row of the set
            model[50] = False
            check_set(flt, model, alive, "deny under the offset", off)
            idx.set_id_offset(77)                                       # after creation: the rows stay, their ids move
            check_set(flt, model, alive, "offset after", 77)
            got = check_search(idx, flt, oracle, X, model, alive, Q, 10, "offset after", 77)
            assert (got[0][got[0] > 0] > 77).all() and (got[0] <= 77 + n).all()


@pytest.mark.parametrize("G", [2, 3])
def test_sharded(G, oracle, lib_built, monkeypatch):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(27)
    X = corpus(rng, N, D)
    Q = queries(rng, X)
    alive = np.ones(N, dtype=bool)
    gone = np.unique(np.r_[rng.choice(N, 300, replace=False), 64:128])
    alive[gone] = False
    cases = [c for c in shapes(rng, N) if c[0] in ("5000 scattered ids", "every other tile", "past the end")]
    with FlatIndex(D) as plain, FlatIndex(D, devices=[0] * G, block_rows=64) as sh:
        for idx in (plain, sh):
            idx.add(X)
            idx.remove(gone + 1)
        for what, r in cases:
            model = allowed_mask(N, r)
            for how, kw in (("ranges", dict(ranges=r)), ("ids", dict(ids=rng.permutation(ids_of(r))))):
                tag = f"{G} shards, {what}, by {how}"
                with plain.make_filter(**kw) as fp, sh.make_filter(**kw) as fs:
                    check_set(fs, model, alive, tag)
                    for k in (10, 300):
                        got = check_search(sh, fs, oracle, X, model, alive, Q, k, f"{tag}, k = {k}")
                        same(got, plain.search_with(fp, Q, k), f"{tag}, k = {k}: the unsharded index")
                        assert (got[3] == min(k, int((model & alive).sum()))).all()
                    fs.deny(ranges=[[1000, 1100]])
                    fs.deny(ids=np.arange(3000, 3200, 2))
                    model2 = model.copy()
                    model2[999:1099] = False
                    model2[2999:3199:2] = False
                    check_set(fs, model2, alive, tag + ", after deny")
                    check_search(sh, fs, oracle, X, model2, alive, Q, 10, tag + ", after deny")


def test_concurrency(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(28)
    X = corpus(rng, N, D)
    Q = rng.standard_normal((64, D)).astype(np.float32)
    ra, rb = np.array([[1, N // 2]]), np.array([[N // 2, N + 1]])
    with FlatIndex(D) as idx:
        idx.add(X)
        with idx.make_filter(ranges=ra) as flt:
            want_a = idx.search_with(flt, Q, 10)
            errors, out = [], [None] * 8

            def eight(t):
                try:
                    out[t] = [idx.search_with(flt, Q[i:i + 1], 10) for i in range(t * 8, t * 8 + 8)]
                except Exception as e:                                  # noqa: BLE001
                    errors.append(e)

            th = [threading.Thread(target=eight, args=(t,)) for t in range(8)]
            [t.start() for t in th]
            [t.join() for t in th]
            assert not errors, errors
            for t in range(8):
                for i in range(8):
                    same(out[t][i], tuple(a[t * 8 + i:t * 8 + i + 1] for a in want_a), f"thread {t}, query {i}")
            # set B = A and the ids of rb: one allow call flips A -> B, one deny call flips back, so a search sees A or B whole
            flt.allow(ranges=rb)
            want_b = idx.search_with(flt, Q, 10)
            stop, seen = threading.Event(), [0] * 4

            def writer():
                try:
                    deadline = time.monotonic() + 1.0
                    while time.monotonic() < deadline:
                        flt.deny(ranges=rb)
                        flt.allow(ranges=rb)
                except Exception as e:                                  # noqa: BLE001
                    errors.append(e)
                stop.set()

            def searcher(t):
                try:
                    while not stop.is_set():
                        i = (t * 17 + seen[t]) % 64
                        got = idx.search_with(flt, Q[i:i + 1], 10)
                        ok = [all(np.array_equal(g, w[i:i + 1]) for g, w in zip(got, want)) for want in (want_a, want_b)]
                        if not any(ok):
                            errors.append(AssertionError(f"query {i}: the answer under neither A nor B"))
                            return
                        seen[t] += 1
                except Exception as e:                                  # noqa: BLE001
                    errors.append(e)

            th = [threading.Thread(target=writer)] + [threading.Thread(target=searcher, args=(t,)) for t in range(4)]
            [t.start() for t in th]
            [t.join() for t in th]
            assert not errors, errors[:3]
            assert min(seen) > 0
