"""Filters built from what the rows carry (mx_filter_set_where / set_keys / combine / invert).  The set itself --
ranges(), count(), n_selected -- is held after every edit against the NumPy statement in where_model.py; every search through such a
filter is held, bit for bit, against the per-call filtered search with the ranges the filter reports and against the oracle on the
model's allowed live rows.  A sharded handle is held against the same model and against the plain index's answers."""
import ctypes

import numpy as np
import pytest

import where_model as wm
from filtered_model import allowed_mask
from test_filtered_gpu import same
from test_remove_gpu import corpus
from test_resident_filter_gpu import both_paths, check_search, check_set

pytestmark = pytest.mark.gpu

D, N = 64, 20037                       # deliberately no multiple of 64
DOC = 70                               # rows per document
DENORMAL = np.float32(1e-40)


def queries(rng, rows):
    Q = rng.standard_normal((16, rows.shape[1])).astype(np.float32)
    Q[1] = rows[130] * 2.0
    Q[2] = rows[min(8000, rows.shape[0] - 1)]
    Q[3] = 0.0                          # the zero query: the first allowed live rows by id
    return Q


def fill_columns(rng, pri, grp, n, off=0):
    """-> (vals f32 [n], keys u32 [n]) as written: documents of DOC rows by set_ranges, scattered rows by set_ids"""
    vals = np.zeros(n, np.float32)
    keys = np.zeros(n, np.uint32)
    docs = np.arange(0, n - DOC, DOC)[: (n // DOC) * 3 // 4]            # the last quarter stays unset: value 0, key 0
    doc_vals = rng.choice(np.array([0.25, 0.5, 1.0, 2.5, -1.0, -0.0, DENORMAL, 1e30], np.float32), docs.size)
    doc_keys = rng.permutation(docs.size).astype(np.uint32) + 1
    doc_keys[5] = 0xFFFFFFFF
    r = np.stack([docs + 1 + off, docs + DOC + 1 + off], 1).astype(np.uint64)
    pri.set_ranges(r, doc_vals)
    grp.set_ranges(r, doc_keys)
    for d, v, k in zip(docs, doc_vals, doc_keys):
        vals[d:d + DOC] = v
        keys[d:d + DOC] = k
    some = rng.choice(n, n // 7, replace=False)
    sv = rng.uniform(-2.0, 3.0, some.size).astype(np.float32)
    sv[:3] = 7.125                                                      # a value present in exactly three rows
    sv[3:40] = -0.0
    pri.set_ids(some.astype(np.uint64) + 1 + off, sv)
    vals[some] = sv
    three = rng.choice(n, 200, replace=False)
    grp.set_ids(three.astype(np.uint64) + 1 + off, np.full(200, 3, np.uint32))
    keys[three] = 3
    return vals, keys


class Tracked:
    """a filter and its model, edited together; every edit is checked"""

    def __init__(self, idx, n, alive, off=0):
        self.idx, self.n, self.alive, self.off = idx, n, alive, off
        self.flt = idx.make_filter()
        self.model = np.zeros(n, bool)

    def check(self, what):
        check_set(self.flt, self.model, self.alive, what, self.off)

    def where(self, pri, vals, lo, hi, allow, what):
        got = (self.flt.allow_where if allow else self.flt.deny_where)(pri, lo, hi)
        self.model, want = wm.edit(self.model, wm.select_where(vals, self.n, lo, hi), allow)
        assert got == want, what
        self.check(what)
        return got

    def keys(self, grp, keys, wanted, allow, what):
        got = (self.flt.allow_keys if allow else self.flt.deny_keys)(grp, wanted)
        self.model, want = wm.edit(self.model, wm.select_keys(keys, self.n, wanted), allow)
        assert got == want, what
        self.check(what)
        return got

    def invert(self, what):
        self.flt.invert()
        self.model = wm.invert(self.model)
        self.check(what)

    def close(self):
        self.flt.close()


def test_where_against_the_model_and_predicate_edges(lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(31)
    X = corpus(rng, N, D)
    alive = np.ones(N, bool)
    inf = np.inf
    with FlatIndex(D) as idx, idx.make_prior() as pri, idx.make_grouping() as grp:
        idx.add(X)
        vals, _ = fill_columns(rng, pri, grp, N)
        gone = rng.choice(N, 300, replace=False)
        idx.remove(gone + 1)
        alive[gone] = False                                             # removed rows are selected like any other row
        t = Tracked(idx, N, alive)
        assert t.where(pri, vals, 7.125, 7.125, 1, "lo == hi on a value in three rows") == 3
        t.where(pri, vals, 0.0, 0.0, 1, "[0, 0]: +0.0, the stored -0.0 and the rows nobody set")
        assert t.model[vals == 0].all() and np.signbit(vals[t.model]).sum() >= 37
        t.where(pri, vals, -0.0, -0.0, 0, "[-0, -0] takes the same rows away")
        assert t.model.sum() == 3
        t.where(pri, vals, 0.8, inf, 1, "one-sided: >= 0.8")
        t.where(pri, vals, -inf, -0.5, 1, "one-sided: <= -0.5")
        t.where(pri, vals, 1.0, 0.5, 1, "lo > hi selects nothing")
        assert t.where(pri, vals, 1.0, 0.5, 0, "lo > hi takes nothing away") == 0
        t.where(pri, vals, DENORMAL, DENORMAL, 1, "a denormal bound, both sides")
        assert t.where(pri, vals, float(DENORMAL), 0.2, 0, "a denormal lower bound: 0 stays outside") > 0
        t.where(pri, vals, -float(DENORMAL), float(DENORMAL), 1, "denormal bounds around 0")
        assert t.where(pri, vals, -inf, inf, 0, "everything taken away") == N and not t.model.any()
        assert t.where(pri, vals, -inf, inf, 1, "everything") == N and t.model.all()
        t.where(pri, vals, 0.25, 2.5, 0, "deny a band")
        t.where(pri, vals, 3e38, inf, 1, "above every value")
        t.invert("inverted")
        t.invert("inverted twice")
        # refused calls change nothing
        before = t.model.copy()
        nan = float("nan")
        for lo, hi in ((nan, 1.0), (0.0, nan), (nan, nan)):
            with pytest.raises(_lib.MemexHipError, match="NaN") as e:
                t.flt.allow_where(pri, lo, hi)
            assert e.value.code == _lib.MX_EINVAL
        n_sel = ctypes.c_uint64(99)
        for allow in (2, -1):
            assert lib_built.mx_filter_set_where(t.flt._h, pri._h, 0.0, 1.0, allow, ctypes.byref(n_sel)) == _lib.MX_EINVAL
            assert lib_built.mx_filter_set_keys(t.flt._h, grp._h, None, 0, allow, ctypes.byref(n_sel)) == _lib.MX_EINVAL
        assert lib_built.mx_filter_set_where(t.flt._h, pri._h, 0.0, 1.0, 1, None) == _lib.MX_OK   # n_selected may be NULL
        t.model |= wm.select_where(vals, N, 0.0, 1.0)
        assert n_sel.value == 99
        np.testing.assert_array_equal(before | wm.select_where(vals, N, 0.0, 1.0), t.model)
        t.check("after the refused calls and one without n_selected")
        t.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 4097])
def test_word_and_wave_edges(n, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(32 + n)
    X = rng.standard_normal((n, D)).astype(np.float32)
    alive = np.ones(n, bool)
    vals = np.where(np.arange(n) % 2 == 0, 1.0, 2.0).astype(np.float32)   # every other row
    vals[n - 1] = 5.0                                                    # only the last row
    keys = (np.arange(n) % 2 + 1).astype(np.uint32)
    keys[n - 1] = 9
    ids = np.arange(1, n + 1, dtype=np.uint64)
    with FlatIndex(D) as idx, idx.make_prior() as pri, idx.make_grouping() as grp:
        idx.add(X)
        pri.set_ids(ids, vals)
        grp.set_ids(ids, keys)
        for what, (lo, hi), wanted in (("everything", (0.5, 9.0), [1, 2, 9]), ("nothing", (3.0, 4.0), [4, 0]), ("the last row", (5.0, 5.0), [9]),
                                       ("every other row", (1.0, 1.0), [1])):
            for how in ("where", "keys"):
                t = Tracked(idx, n, alive)
                tag = f"n = {n}, {what}, by {how}"
                if how == "where":
                    t.where(pri, vals, lo, hi, 1, tag)
                else:
                    t.keys(grp, keys, wanted, 1, tag)
                t.invert(tag + ", inverted")
                got = idx.search_with(t.flt, X[:1], min(n, 10))
                assert got[3][0] == min(int(t.model.sum()), 10) and np.isin(got[0][0][: got[3][0]] - 1, np.flatnonzero(t.model)).all(), tag
                if how == "where":
                    t.where(pri, vals, lo, hi, 1, tag + ", and the selection back: all rows")
                else:
                    t.keys(grp, keys, wanted, 1, tag + ", and the selection back: all rows")
                assert t.model.all()
                t.invert(tag + ", all rows inverted: none")
                assert t.flt.count() == (0, 0)
                t.close()


def test_columns_shorter_than_the_rows(lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(33)
    n, more = 3000, 5037
    X = corpus(rng, n + more, D)
    with FlatIndex(D) as idx:
        idx.reserve(n)
        idx.add(X[:n])
        with idx.make_prior() as pri, idx.make_grouping() as grp:
            vals = np.full(n, 1.5, np.float32)
            keys = np.full(n, 6, np.uint32)
            pri.set_ranges([[1, n + 1]], [1.5])
            grp.set_ranges([[1, n + 1]], [6])
            idx.add(X[n:])                                              # the columns end at the old rows (rounded up to 1024)
            alive = np.ones(n + more, bool)
            t = Tracked(idx, n + more, alive)
            assert t.where(pri, vals, 0.0, 0.0, 1, "[0, 0] selects the rows past the prior") == more
            assert t.model[n:].all() and not t.model[:n].any()
            assert t.where(pri, vals, 1.0, 2.0, 0, "a positive range selects none of them") == n
            assert t.model.sum() == more
            t.invert("inverted: the old rows")
            assert t.keys(grp, keys, [0], 1, "key 0 selects the rows past the grouping") == more
            assert t.model.all()
            assert t.keys(grp, keys, [6, 6, 7], 0, "a real key selects none of them") == n
            assert t.model.sum() == more
            t.close()
    with FlatIndex(D) as idx, idx.make_prior() as pri, idx.make_grouping() as grp:   # columns made on an index without rows
        idx.add(X[:200])
        alive = np.ones(200, bool)
        t = Tracked(idx, 200, alive)
        assert t.where(pri, np.zeros(0), -1.0, 1.0, 1, "an empty prior reads 0 everywhere") == 200
        assert t.keys(grp, np.zeros(0), [5, 0], 0, "an empty grouping reads key 0 everywhere") == 200
        t.close()


def test_a_filter_made_before_an_append(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(34)
    n, more = 3000, 5037
    total = n + more
    X = corpus(rng, total, D)
    Q = queries(rng, X)
    alive = np.ones(total, bool)
    with FlatIndex(D) as idx, idx.make_prior() as pri:
        idx.reserve(n)
        idx.add(X[:n])
        old = idx.make_filter(ranges=[[n - 1000, n + 1]])              # its bitmap covers the old capacity
        m_old = wm.grown(allowed_mask(n, [[n - 1000, n + 1]]), total)
        idx.add(X[n:])                                                  # past a capacity growth: the rows and every bitmap move
        vals = rng.choice(np.array([0.0, 1.0, 2.0], np.float32), total)
        pri.set_ids(np.arange(1, total + 1, dtype=np.uint64), vals)
        new = idx.make_filter()
        assert new.allow_where(pri, 1.0, 1.0) == int((vals == 1.0).sum())
        m_new = vals == 1.0
        for op in ("and", "or", "andnot", "xor"):
            with idx.combine_filters(old, new, op) as out:              # the old filter's missing words are zeros
                check_set(out, wm.combine(m_old, m_new, op), alive, f"old {op} new")
            with idx.combine_filters(new, old, op) as out:
                check_set(out, wm.combine(m_new, m_old, op), alive, f"new {op} old")
        check_set(old, m_old, alive, "the old filter as an operand: unchanged")
        with idx.combine_filters(new, old, "andnot") as out:
            check_search(idx, out, oracle, X, m_new & ~m_old, alive, Q, 10, "new - old")
        old.invert()                                                    # the complement within the rows of NOW
        check_set(old, ~m_old, alive, "the old filter inverted after the append")
        check_search(idx, old, oracle, X, ~m_old, alive, Q, 10, "the old filter inverted after the append")
        old.close()
        new.close()


def test_keys(lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(35)
    X = corpus(rng, N, D)
    alive = np.ones(N, bool)
    with FlatIndex(D) as idx, idx.make_prior() as pri, idx.make_grouping() as grp:
        idx.add(X)
        _, keys = fill_columns(rng, pri, grp, N)
        present = np.unique(keys[keys != 0])
        t = Tracked(idx, N, alive)
        assert t.keys(grp, keys, [int(present[4])] * 5, 1, "one key five times") == int((keys == present[4]).sum())
        pick = rng.permutation(np.r_[present[10:40], present[10:25], [0x7FFFFFFF, 123456789]]).astype(np.uint32)
        t.keys(grp, keys, pick, 1, "unsorted, repeats, keys no row has")
        assert t.keys(grp, keys, [0xFFFFFFFF], 1, "key 0xffffffff") > 0
        assert t.keys(grp, keys, [3], 1, "a key given by set_ids") >= 150
        n0 = t.keys(grp, keys, [0], 1, "key 0: the ungrouped rows")
        assert n0 == int((keys == 0).sum()) > N // 5
        t.keys(grp, keys, pick[::-1], 0, "the unsorted list taken away")
        t.keys(grp, keys, np.zeros(0, np.uint32), 1, "no keys: a no-op")
        t.keys(grp, keys, present, 0, "every key but 0 denied")
        assert t.model.sum() == n0
        # 2^20 keys are accepted, one more is refused
        big = np.arange(1, (1 << 20) + 2, dtype=np.uint32)
        rng.shuffle(big[: 1 << 20])
        t.keys(grp, keys, big[: 1 << 20], 1, "2^20 keys")
        before = t.model.copy()
        with pytest.raises(_lib.MemexHipError) as e:
            t.flt.allow_keys(grp, big)
        assert e.value.code == _lib.MX_EUNSUPPORTED
        n_sel = ctypes.c_uint64(5)
        assert lib_built.mx_filter_set_keys(t.flt._h, grp._h, None, 3, 1, ctypes.byref(n_sel)) == _lib.MX_EINVAL and n_sel.value == 5
        np.testing.assert_array_equal(before, t.model)
        t.check("after the refused calls")
        t.close()


def test_combine(lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(36)
    X = corpus(rng, N, D)
    alive = np.ones(N, bool)
    with FlatIndex(D) as idx, FlatIndex(D) as other:
        idx.add(X)
        other.add(X[:500])
        gone = rng.choice(N, 200, replace=False)
        idx.remove(gone + 1)
        alive[gone] = False
        for p, q in ((0.5, 0.5), (0.01, 0.9), (1.0, 0.3), (0.0, 0.5)):
            ma, mb = rng.random(N) < p, rng.random(N) < q
            a = idx.make_filter(ids=np.flatnonzero(ma) + 1)
            b = idx.make_filter(ids=np.flatnonzero(mb) + 1)
            for op in ("and", "or", "andnot", "xor"):
                tag = f"p = {p}, q = {q}, {op}"
                want = wm.combine(ma, mb, op)
                with idx.combine_filters(a, b, op) as out:
                    check_set(out, want, alive, tag)
                with idx.combine_filters(a, b, wm.OPS[op]) as out:       # the number of the enum
                    check_set(out, want, alive, tag + ", by number")
                with {"and": a & b, "or": a | b, "andnot": a - b, "xor": a ^ b}[op] as out:
                    check_set(out, want, alive, tag + ", by operator")
                with idx.make_filter(ranges=[[5, 900]]) as out:          # an out that held something else
                    assert idx.combine_filters(a, b, op, out=out) is out
                    check_set(out, want, alive, tag + ", into a used filter")
                with idx.make_filter(ids=np.flatnonzero(ma) + 1) as a2:  # dst aliasing a
                    idx.combine_filters(a2, b, op, out=a2)
                    check_set(a2, want, alive, tag + ", dst is a")
                with idx.make_filter(ids=np.flatnonzero(mb) + 1) as b2:  # dst aliasing b
                    idx.combine_filters(a, b2, op, out=b2)
                    check_set(b2, want, alive, tag + ", dst is b")
                with idx.combine_filters(a, a, op) as out:               # a is b
                    check_set(out, wm.combine(ma, ma, op), alive, tag + ", a is b")
                with idx.make_filter(ids=np.flatnonzero(ma) + 1) as a3:  # all three the same
                    idx.combine_filters(a3, a3, op, out=a3)
                    check_set(a3, wm.combine(ma, ma, op), alive, tag + ", dst is a is b")
            check_set(a, ma, alive, "operand a unchanged")
            check_set(b, mb, alive, "operand b unchanged")
            a.close()
            b.close()
        # refused: an op outside the enum, a foreign index, a stale operand -- dst stays as it was
        ma = rng.random(N) < 0.3
        a = idx.make_filter(ids=np.flatnonzero(ma) + 1)
        dst = idx.make_filter(ranges=[[100, 300]])
        m_dst = allowed_mask(N, [[100, 300]])
        foreign = other.make_filter(ranges=[[1, 100]])
        for op in (4, -1, 99):
            with pytest.raises(_lib.MemexHipError) as e:
                idx.combine_filters(a, a, op, out=dst)
            assert e.value.code == _lib.MX_EINVAL
        for args in ((a, foreign), (foreign, a)):
            with pytest.raises(_lib.MemexHipError, match="another index") as e:
                idx.combine_filters(*args, "or", out=dst)
            assert e.value.code == _lib.MX_EINVAL
        with pytest.raises(_lib.MemexHipError, match="another index"):
            idx.combine_filters(a, a, "or", out=foreign)
        check_set(dst, m_dst, alive, "dst after the refused calls")
        check_set(foreign, allowed_mask(500, [[1, 100]]), np.ones(500, bool), "the foreign filter after the refused calls")
        with other.make_prior() as fp, other.make_grouping() as fg:
            with pytest.raises(_lib.MemexHipError, match="another index"):
                dst.allow_where(fp, 0.0, 0.0)
            with pytest.raises(_lib.MemexHipError, match="another index"):
                dst.allow_keys(fg, [0])
        check_set(dst, m_dst, alive, "dst after a foreign prior and grouping")
        stale_f, stale_p, stale_g = other.make_filter(ranges=[[1, 50]]), other.make_prior(), other.make_grouping()
        other.clear()
        other.add(X[:500])
        fresh = other.make_filter(ranges=[[1, 50]])
        for call in (lambda: other.combine_filters(fresh, stale_f, "or"), lambda: other.combine_filters(stale_f, fresh, "and"),
                     lambda: other.combine_filters(fresh, fresh, "or", out=stale_f), stale_f.invert, lambda: stale_f.allow_where(stale_p),
                     lambda: fresh.allow_where(stale_p, 0.0, 0.0), lambda: fresh.allow_keys(stale_g, [0]), lambda: stale_f.allow_keys(stale_g, [0])):
            with pytest.raises(_lib.MemexHipError, match="stale") as e:
                call()
            assert e.value.code == _lib.MX_EINVAL
        check_set(fresh, allowed_mask(500, [[1, 50]]), np.ones(500, bool), "the fresh filter after the refused calls")
        for h in (a, dst, foreign, stale_f, stale_p, stale_g, fresh):
            h.close()


@pytest.mark.parametrize("phase", ["removed", "offset"])
def test_searches(phase, oracle, lib_built, monkeypatch):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(37)
    n = N if phase == "removed" else N + 30000                          # the larger one: sets wide enough for the masked scan
    off = 0 if phase == "removed" else 1_000_000
    X = corpus(rng, n, D)
    Q = queries(rng, X)
    alive = np.ones(n, bool)
    with FlatIndex(D) as idx, idx.make_prior() as pri, idx.make_grouping() as grp:
        idx.add(X)
        if off:
            idx.set_id_offset(off)
        vals, keys = fill_columns(rng, pri, grp, n, off)
        if phase == "removed":
            gone = np.unique(np.r_[rng.choice(n, n // 50, replace=False), 120:140, 7, 300, 11, n - 100, 8000, 5056:5120])
            assert idx.remove(gone + 1) > 0
            alive[gone] = False
        present = np.unique(keys[keys != 0])
        w = Tracked(idx, n, alive, off)
        w.where(pri, vals, 0.9, 1.1, 1, "value 1.0")
        k_ = Tracked(idx, n, alive, off)
        k_.keys(grp, keys, rng.permutation(present[:120]), 1, "120 documents")
        wide = Tracked(idx, n, alive, off)
        wide.where(pri, vals, -np.inf, 2.6, 1, "<= 2.6: most rows")
        small = Tracked(idx, n, alive, off)
        small.keys(grp, keys, present[40:43], 1, "three documents")
        built = [("where", w.flt, w.model), ("keys", k_.flt, k_.model), ("where, wide", wide.flt, wide.model), ("keys, small", small.flt, small.model)]
        both = idx.combine_filters(w.flt, k_.flt, "and")
        either_not = idx.combine_filters(wide.flt, k_.flt, "andnot")
        built += [("where and keys", both, w.model & k_.model), ("where - keys", either_not, wide.model & ~k_.model)]
        assert (wide.model & alive).sum() > 16384 >= (small.model & alive).sum() > 0
        idx.reset_stats()
        for how, flt, model in built:
            tag = f"{phase}, by {how}"
            check_set(flt, model, alive, tag, off)
            got = check_search(idx, flt, oracle, X, model, alive, Q, 10, tag + ", k = 10", off)
            check_search(idx, flt, oracle, X, model, alive, Q[:4], 300, tag + ", k = 300", off)
            if 0 < (model & alive).sum() <= 16384:
                both_paths(monkeypatch, idx, flt, Q, 10, got, tag)
            # grouped and boosted search take the filter as they take any other
            with idx.make_grouping() as none:                            # an empty grouping: every row heads a group
                g = idx.search_grouped(none, Q, 10, flt=flt)
            np.testing.assert_array_equal(g[0], got[0], err_msg=tag + ": grouped")
            b = idx.search_boosted(pri, Q, 10, weight=0.0, flt=flt)     # weight 0: the list in its own order
            np.testing.assert_array_equal(b[0], got[0], err_msg=tag + ": boosted")
            np.testing.assert_array_equal(b[3][got[0] > 0], vals[(got[0] - 1 - off).astype(np.int64)[got[0] > 0]], err_msg=tag + ": priors")
        st = idx.stats()
        assert 0 < st.subset_queries < st.filtered_queries               # both the subset kernel and the masked scan answered
        for t in (w, k_, wide, small):
            t.close()
        both.close()
        either_not.close()


def test_sharded(oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(38)
    G, R = 3, 96                        # blocks of one and a half words; 20037 rows: a partial last block that ends mid-word
    X = corpus(rng, N, D)
    Q = queries(rng, X)
    alive = np.ones(N, bool)
    gone = np.unique(np.r_[rng.choice(N, 300, replace=False), 64:128])
    alive[gone] = False
    with FlatIndex(D) as plain, FlatIndex(D, devices=[0] * G, block_rows=R) as sh:
        assert sh.n_shards == G and N % R != 0 and N % 64 != 0
        state = {}
        for name, idx in (("plain", plain), ("sharded", sh)):
            idx.add(X)
            idx.remove(gone + 1)
            pri, grp = idx.make_prior(), idx.make_grouping()
            vals, keys = fill_columns(np.random.default_rng(380), pri, grp, N)
            state[name] = (idx, pri, grp)
        present = np.unique(keys[keys != 0])
        answers = {}
        for name, (idx, pri, grp) in state.items():
            t = Tracked(idx, N, alive)
            u = Tracked(idx, N, alive)
            t.where(pri, vals, 0.9, 1.1, 1, name + ": value 1.0")
            t.where(pri, vals, 0.0, 0.0, 1, name + ": value 0")
            t.where(pri, vals, -np.inf, -1.5, 1, name + ": <= -1.5")
            t.where(pri, vals, 7.125, 7.125, 0, name + ": three rows denied")
            u.keys(grp, keys, rng.permutation(present[:150]), 1, name + ": 150 documents")
            u.keys(grp, keys, [0, 0xFFFFFFFF, 3], 1, name + ": key 0, the largest key, key 3")
            u.keys(grp, keys, present[100:120], 0, name + ": 20 documents denied")
            u.where(pri, vals, float(vals[N - 1]), float(vals[N - 1]), 1, name + ": the last row's value")
            assert u.model[N - 1]
            got = {}
            for op in ("and", "or", "andnot", "xor"):
                with idx.combine_filters(t.flt, u.flt, op) as out:
                    m = wm.combine(t.model, u.model, op)
                    check_set(out, m, alive, f"{name}: {op}")
                    got[op] = [check_search(idx, out, oracle, X, m, alive, Q, k, f"{name}: {op}, k = {k}") for k in (10, 300)]
            t.invert(name + ": inverted")
            got["inv"] = [check_search(idx, t.flt, oracle, X, t.model, alive, Q, 10, name + ": inverted")]
            c = Tracked(idx, N, alive)                                   # every row, then none: the tail word of every shard
            c.where(pri, vals, -np.inf, np.inf, 1, name + ": every row")
            assert c.model.all()
            c.invert(name + ": every row inverted")
            assert c.flt.count() == (0, 0)
            c.close()
            answers[name] = got
            t.close()
            u.close()
        for key, lists in answers["plain"].items():
            for a, b in zip(lists, answers["sharded"][key]):
                same(b, a, f"sharded against plain: {key}")
        for _, pri, grp in state.values():
            pri.close()
            grp.close()


def test_store_level(lib_built, tmp_path):
    from memex_amd.storage import HipFlatStore, SearchError, VectorData
    rng = np.random.default_rng(39)
    d, n_docs = 64, 60
    store = HipFlatStore.new(str(tmp_path / "c"))
    docs, stamp, vec_of = {}, {}, {}
    points = []
    for i in range(n_docs):
        name = f"doc{i:02d}"
        docs[name] = [f"{name}/s{j}" for j in range(int(rng.integers(1, 6)))]
        stamp[name] = float(rng.choice([0.25, 0.5, 1.0, 2.0, 4.0]))
        for s in docs[name]:
            vec_of[s] = rng.standard_normal(d).astype(np.float32)
            points.append(VectorData(_id=s, document_id=name, text="", vector=vec_of[s].tolist()))
    store.bulk_insert(points)
    try:
        pri, grp = store.make_prior(), store.make_grouping(docs)
        for name in list(docs)[:50]:                                    # the last ten documents are never stamped: they read 0
            pri.set_document(docs[name], stamp[name])
        for name in list(docs)[50:]:
            stamp[name] = 0.0
        seg_doc = {s: name for name, ss in docs.items() for s in ss}
        everything = set(seg_doc)

        def found(flt):
            """the _ids a search through the filter can return: all of them, the store is small"""
            return {h[0] for h in store.search_in(np.ones(d, np.float32), len(seg_doc), flt)}

        recent = store.make_filter()
        m_recent = {s for s in seg_doc if 1.0 <= stamp[seg_doc[s]]}
        assert recent.allow_where(pri, 1.0) == len(m_recent)
        assert found(recent) == m_recent and recent.count() == (len(m_recent), len(m_recent))
        assert recent.deny_where(pri, 4.0, 4.0) == sum(stamp[seg_doc[s]] == 4.0 for s in seg_doc)
        m_recent = {s for s in m_recent if stamp[seg_doc[s]] != 4.0}
        assert found(recent) == m_recent
        chosen = store.make_filter()
        names = ["doc03", "doc17", "doc03", "no such document", "doc55", "doc40"]
        keys_before = dict(grp._key_of)
        m_chosen = {s for s in seg_doc if seg_doc[s] in names}
        assert chosen.allow_documents(grp, names) == len(m_chosen)
        assert grp._key_of == keys_before                               # no key handed out for the unknown name
        assert found(chosen) == m_chosen
        assert chosen.allow_documents(grp, ["nobody", "nothing"]) == 0 and found(chosen) == m_chosen
        assert chosen.deny_documents(grp, "doc17") == len(docs["doc17"])
        m_chosen -= set(docs["doc17"])
        assert found(chosen) == m_chosen
        for op, want in (("and", m_recent & m_chosen), ("or", m_recent | m_chosen), ("andnot", m_recent - m_chosen), ("xor", m_recent ^ m_chosen)):
            out = store.combine_filters(recent, chosen, op)
            assert found(out) == want and out.count()[0] == len(want), op
            out.close()
        assert store.combine_filters(recent, chosen, "or", out=chosen) is chosen
        m_chosen |= m_recent
        assert found(chosen) == m_chosen
        chosen.invert()
        assert found(chosen) == everything - m_chosen
        chosen.invert()
        assert found(chosen) == m_chosen
        hits, complete = store.search_boosted(np.ones(d, np.float32), 5, pri, 0.0, None, recent)
        assert complete and {h[0] for h in hits} <= m_recent and len(hits) == 5
        with pytest.raises(SearchError):
            recent.allow_where(pri, float("nan"), 1.0)
        with pytest.raises(SearchError):
            store.combine_filters(recent, chosen, "nand")
        for h in (pri, grp, recent, chosen):
            h.close()
    finally:
        store.delete_all()
