"""Every search form on rows of 1 to 65536 dims (tests/WIDTH_AXIS.md): the lattice of tests/width_axis_cases.py -- a width either side
of every point where the width of a row changes the code that serves it -- against the oracle and the host models beside this file.
Everything is compared bit for bit: ids and counts by equality, scores and dists by their bits; there is no tolerance anywhere.
tests/test_width_axis_model.py shows on the CPU that the corpora put their edge rows among the answers compared here.

Every case prints `WIDTH | ...` lines with the route mx_index_stats showed and its wall time; WIDTH_AXIS.md quotes them."""
import ctypes
import time

import numpy as np
import pytest

import width_axis_cases as W
from boosted_model import boosted_model
from conftest import bits
from group_rows_model import capped_model, group_rows_model
from index_model import SEARCH_AUTO, SEARCH_EXACT, IndexModel
from random_walk import STEPS, run

pytestmark = pytest.mark.gpu

LIMIT = W.MAX_KC16 * W.CHUNK      # 1536: the widest padded row with a scan


def same(got, want, what):
    """two tuples of arrays, field by field: floats by their bits, everything else by equality"""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: field {i}: shape {g.shape} != {w.shape}"
        if w.dtype == np.float32 or g.dtype == np.float32:
            g, w = bits(g), bits(w)
        elif w.dtype == np.float64 or g.dtype == np.float64:
            g, w = np.ascontiguousarray(g, np.float64).view(np.uint64), np.ascontiguousarray(w, np.float64).view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: field {i}")


def oracle_lists(oracle, rows, Q, k):
    ids, dists, scores, nf = oracle.search(rows, Q, k)
    return ids, scores, dists, nf          # (FlatIndex.search's order)


def device_search(idx, Q, k):
    import torch
    B = len(Q)
    dq = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    ids = torch.zeros((B, k), dtype=torch.int64, device="cuda")
    sc = torch.zeros((B, k), dtype=torch.float32, device="cuda")
    di = torch.zeros((B, k), dtype=torch.float32, device="cuda")
    nf = torch.zeros(B, dtype=torch.int32, device="cuda")
    idx.search_device(dq, k, ids, sc, di, nf)
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), di.cpu().numpy(), nf.cpu().numpy()


def open_kind(dim, kind, **kw):
    from memex_amd.index import FlatIndex
    idx = FlatIndex(dim, **kw)
    try:
        if kind == "compressed":
            idx.set_corpus_mode("bf16")
        else:
            idx.set_filter_copy(kind)       # MX_OK at every width, also where no copy can exist
    except Exception:
        idx.close()
        raise
    return idx


# ---- a. plain search over the whole lattice -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", W.LATTICE)
def test_plain_search_at_every_width_and_copy_kind(dim, oracle, lib_built):
    X, _ = W.corpus(dim)
    ds, n = W.ds_of(dim), W.n_rows(dim)
    tiled = (n + W.TILE8_ROWS - 1) // W.TILE8_ROWS * W.TILE8_ROWS            # (700 rows fill 704 rows of tiles of 32 and of 64)
    want = {}
    for kind in W.KINDS:
        r = W.route(dim, kind)
        if r is None:
            continue                                                         # (the refusal: test_refusals_name_their_limit)
        t0 = time.perf_counter()
        seen = []
        with open_kind(dim, kind) as idx:
            assert idx.add(X) == 1
            rows = X
            if kind == "compressed":
                rows = idx.get_rows(0, n)                                    # exact with respect to the stored rows
            st = idx.stats()
            assert st.filter_kind == r["filter_kind"], (dim, kind, st.filter_kind)
            assert st.filter_copy_bytes == W.FIRST_CAPACITY * ds * r["elem_bytes"], (dim, kind, st.filter_copy_bytes, ds)
            for B in W.batch_sizes(dim):
                Q = W.queries(dim, B)
                for k in W.KS:
                    key = (B, k, kind == "compressed")
                    if key not in want:
                        want[key] = oracle_lists(oracle, rows, Q, k)
                    idx.reset_stats()
                    same(idx.search(Q, k), want[key], f"dim {dim} {kind} B {B} k {k}")
                    st = idx.stats()
                    seen.append((B, k, st.scan_launches, st.fallback_queries))
                    assert st.queries == B and st.subset_queries == 0
                    what = (dim, kind, B, k, st.scan_launches, st.scan_bytes, st.fallback_queries, st.filter_demotions, st.filter_kind)
                    assert st.fallback_queries == W.FALLBACK_QUERIES and st.filter_demotions == W.FILTER_DEMOTIONS, what
                    assert st.filter_kind == r["filter_kind"], what
                    if kind == "compressed" or not r["scan"] or k > 256:     # (the two out-of-range norms send a compressed corpus
                        assert st.scan_launches == 0 and st.scan_bytes == 0, what   # to the EXACT path: test_compressed_corpus scans one)
                    else:
                        assert st.scan_launches == W.passes(dim, kind, B), what
                        assert st.scan_bytes == st.scan_launches * tiled * ds * r["scan_elem_bytes"], what
                    same(device_search(idx, Q, k), want[key], f"dim {dim} {kind} B {B} k {k}: search_device")
            end = idx.stats()
        print(f"WIDTH | plain | dim {dim} ds {ds} | {kind} | filter_kind {end.filter_kind} copy_bytes {end.filter_copy_bytes} | "
              f"(B, k, scan_launches, fallback_queries) {seen} | {time.perf_counter() - t0:.2f} s")


# ---- b. every row-touching form on the reduced lattice ------------------------------------------------------------------------------
def forms_pair(dim, oracle):
    """an index with the automatic copy and its model, both holding the corpus with REMOVED_ROW removed"""
    from memex_amd.index import FlatIndex
    X, _ = W.corpus(dim)
    idx = FlatIndex(dim)
    model = IndexModel(dim, oracle)
    assert idx.add(X) == model.add(X) == 1
    assert idx.remove([W.REMOVED_ROW + 1]) == model.remove([W.REMOVED_ROW + 1]) == 1
    return idx, model


@pytest.mark.parametrize("dim", W.REDUCED)
def test_filtered_and_range_forms(dim, oracle, lib_built):
    ds, n = W.ds_of(dim), W.n_rows(dim)
    Q = W.form_queries(dim)
    t0 = time.perf_counter()
    idx, model = forms_pair(dim, oracle)
    with idx:
        doc = np.array([[200, 270]], np.uint64)                               # a 70-row document, its removed row among them
        span = np.array([[10, 130], [180, 290]], np.uint64)                   # several tiles, two runs
        modes = (SEARCH_AUTO, SEARCH_EXACT) if ds <= LIMIT else (SEARCH_AUTO,)
        for mode in modes:
            idx.set_search_mode(mode)
            for k in (10, 80):
                idx.reset_stats()
                same(idx.search_filtered(Q, k, ranges=doc), model.search_filtered(Q, k, ranges=doc), f"dim {dim} mode {mode} filtered doc k {k}")
                st = idx.stats()
                assert st.filtered_queries == len(Q)
                assert st.subset_queries == (len(Q) if W.route(dim, "auto")["subset"] else 0), (dim, mode, st.subset_queries)
                same(idx.search_filtered(Q, k, ranges=span), model.search_filtered(Q, k, ranges=span), f"dim {dim} mode {mode} filtered span k {k}")
                for r in (doc, span):
                    with idx.make_filter(ranges=r) as flt:
                        same(idx.search_with(flt, Q, k), model.search_with(model.make_filter(ranges=r), Q, k),
                             f"dim {dim} mode {mode} search_with {r.tolist()} k {k}")
            alive = model.alive
            t5, t_all = W.range_thresholds(oracle, dim, alive)
            t = np.full(len(Q), 0.5, np.float32)
            for thr in (t5, t_all):
                t[W.Q_RANGE] = thr
                got = idx.search_range(Q, t, 1024)
                same(got, model.search_range(Q, t, 1024), f"dim {dim} mode {mode} range t {thr}")
                assert int(got[4][W.Q_RANGE]) == (5 if thr == t5 else n - 1), (dim, mode, thr, got[4])
        idx.set_search_mode(SEARCH_AUTO)
    print(f"WIDTH | filtered, with, range | dim {dim} ds {ds} | modes {modes} | {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("dim", W.REDUCED)
def test_forms_that_read_stored_rows(dim, oracle, lib_built):
    ds, n = W.ds_of(dim), W.n_rows(dim)
    X, _ = W.corpus(dim)
    Q = W.form_queries(dim)
    rng = np.random.default_rng(dim)
    t0 = time.perf_counter()
    idx, model = forms_pair(dim, oracle)
    with idx:
        if ds <= W.MMR_MAX_DS:                                                # (the refusal above: test_refusals_name_their_limit)
            for fetch in (32, 257):
                same(idx.search_mmr(Q, 10, fetch=fetch, lam=0.5), model.search_mmr(Q, 10, fetch=fetch, lam=0.5), f"dim {dim} mmr fetch {fetch}")
            for m in (70, 1025):
                cand = rng.integers(1, n + 1, (len(Q), m)).astype(np.uint64)
                cand[:, 0] = 0                                                # id 0
                cand[:, 1] = W.REMOVED_ROW + 1                                # a removed id
                cand[:, 2] = cand[:, 3] = W.DUP_FIRST + 3                     # a repeat (and of a duplicated row)
                cand[:, 4], cand[:, 5], cand[:, 6] = W.ZERO_ROW + 1, W.ENDS_ROW + 1, n + 7
                same(idx.score_ids(Q, cand), model.score_ids(Q, cand), f"dim {dim} score_ids m {m}")
        qids = np.array([W.DUP_FIRST + 1, W.ZERO_ROW + 1, W.REMOVED_ROW + 1, W.ENDS_ROW + 1, W.HUGE_ROW + 1, 17, n + 5], np.uint64)
        t5, _ = W.range_thresholds(oracle, dim, model.alive)
        for ex in (True, False):
            same(idx.search_by_id(qids, 10, exclude_self=ex), model.search_by_id(qids, 10, exclude_self=ex), f"dim {dim} by_id exclude {ex}")
            for thr in (np.float32(0.999), t5, np.float32(-1.0)):
                same(idx.search_range_by_id(qids, thr, 1024, exclude_self=ex), model.search_range_by_id(qids, thr, 1024, exclude_self=ex),
                     f"dim {dim} range_by_id t {thr} exclude {ex}")
        ex_ids = np.array([[17, W.ENDS_ROW + 1, 33], [W.DUP_FIRST + 1, W.REMOVED_ROW + 1, 90]], np.uint64)
        wts = np.array([[1.0, -0.5, 1.0], [0.5, 1.0, 2.0]], np.float32)
        qv = np.ascontiguousarray(Q[3:5])
        for ex in (True, False):
            got = idx.search_like(ex_ids, 10, weights=wts, queries=qv, query_weights=0.75, exclude_examples=ex)
            want = model.search_like(ex_ids, 10, weights=wts, queries=qv, query_weights=0.75, exclude_examples=ex)
            same(got, want, f"dim {dim} like exclude {ex}")                   # (`combined` is the last field: bit for bit)
            assert got[5].shape == (2, dim) and np.abs(got[5]).sum() > 0
    print(f"WIDTH | mmr, score_ids, by_id, range_by_id, like | dim {dim} ds {ds} | {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("dim", W.LISTS_ONLY)
def test_forms_over_candidate_lists(dim, oracle, lib_built):
    """fused, grouped, group_rows, capped and boosted search read only lists, but the lists come from the EXACT path here"""
    n = W.n_rows(dim)
    X, _ = W.corpus(dim)
    Q = W.form_queries(dim)
    rng = np.random.default_rng(dim)
    keys = rng.integers(0, 40, n).astype(np.uint32)                           # (0: ungrouped)
    pv = rng.uniform(-0.2, 0.3, n).astype(np.float32)
    everyone = np.arange(1, n + 1, dtype=np.uint64)
    t0 = time.perf_counter()
    idx, model = forms_pair(dim, oracle)
    with idx, idx.make_grouping() as grp, idx.make_prior() as pri:
        mg = model.make_grouping()
        grp.set_ids(everyone, keys)
        mg.set_ids(everyone, keys)
        pri.set_ids(everyone, pv)
        F = np.ascontiguousarray(Q[:4].reshape(2, 2, dim))
        for mode in ("max", "rrf"):
            same(idx.search_fused(F, 10, mode=mode, fetch=40), model.search_fused(F, 10, mode=mode, fetch=40), f"dim {dim} fused {mode}")
        same(idx.search_grouped(grp, Q, 10, fetch=64), model.search_grouped(mg, Q, 10, fetch=64), f"dim {dim} grouped")
        alive = model.alive
        same(idx.search_group_rows(grp, Q, 5, 3, fetch=64), group_rows_model(oracle, X, Q, 5, 3, keys, fetch=64, alive=alive), f"dim {dim} group_rows")
        same(idx.search_capped(grp, Q, 10, 2, fetch=64), capped_model(oracle, X, Q, 10, 2, keys, 64, alive=alive), f"dim {dim} capped")
        hi = np.float32(max(0.0, float(pv.max())))
        same(idx.search_boosted(pri, Q, 10, weight=0.5, fetch=64), boosted_model(oracle, X, Q, 10, pv, w=0.5, hi=hi, fetch=64, alive=alive),
             f"dim {dim} boosted")
    print(f"WIDTH | fused, grouped, group_rows, capped, boosted | dim {dim} | {time.perf_counter() - t0:.2f} s")


# ---- c. the row movers --------------------------------------------------------------------------------------------------------------
def answers(idx, dim, with_score_ids):
    """what a handle is asked after its rows moved: a search, a range search and (up to 8192 padded dims) score_ids"""
    Q = W.form_queries(dim)
    n = len(idx)
    out = [idx.search(Q, 10), idx.search(Q, 300), idx.search_range(Q, np.float32(0.2), 512)]
    if with_score_ids:
        cand = np.random.default_rng(dim).integers(0, n + 3, (len(Q), 70)).astype(np.uint64)
        out.append(idx.score_ids(Q, cand))
    return out


def same_answers(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, f"{what}: answer {i}")


@pytest.mark.parametrize("dim", W.MOVERS)
def test_row_movers(dim, oracle, lib_built, tmp_path):
    import torch
    from memex_amd.index import FlatIndex
    ds, n = W.ds_of(dim), W.n_rows(dim)
    X, _ = W.corpus(dim)
    Q = W.form_queries(dim)
    with_score = ds <= W.MMR_MAX_DS
    t0 = time.perf_counter()
    store = str(tmp_path / "store")
    with FlatIndex(dim) as idx:
        assert idx.add(X) == 1
        np.testing.assert_array_equal(bits(idx.get_rows(0, n)), bits(X), err_msg=f"dim {dim}: get_rows")
        np.testing.assert_array_equal(bits(idx.get_rows(W.ENDS_ROW, 3)), bits(X[W.ENDS_ROW:W.ENDS_ROW + 3]))
        want = [oracle_lists(oracle, X, Q, 10), oracle_lists(oracle, X, Q, 300)]
        full = answers(idx, dim, with_score)
        same_answers(full[:2], want, f"dim {dim}: the plain handle")
        idx.save(store)
        with FlatIndex(dim) as dev:                                           # add_device equals add
            assert dev.add_device(torch.from_numpy(np.ascontiguousarray(X)).cuda()) == 1
            np.testing.assert_array_equal(bits(dev.get_rows(0, n)), bits(X), err_msg=f"dim {dim}: get_rows after add_device")
            same_answers(answers(dev, dim, with_score), full, f"dim {dim}: add_device")
        with FlatIndex(dim) as back:                                          # load into a fresh plain handle
            back.load(store)
            assert len(back) == n
            same_answers(answers(back, dim, with_score), full, f"dim {dim}: loaded")
        with FlatIndex(dim, devices=[0, 0, 0], block_rows=64) as sh:          # ... and into a 3-shard handle
            sh.load(store)
            assert len(sh) == n and sh.n_shards == 3
            same_answers(answers(sh, dim, with_score), full, f"dim {dim}: loaded into 3 shards")
        with FlatIndex(dim, devices=[0, 0, 0], block_rows=64) as sh:          # a 3-shard handle built by add
            assert sh.add(X) == 1
            np.testing.assert_array_equal(bits(sh.get_rows(0, n)), bits(X), err_msg=f"dim {dim}: get_rows of 3 shards")
            same_answers(answers(sh, dim, with_score), full, f"dim {dim}: 3 shards built by add")
        # remove a whole 64-row tile and scattered rows, compact, search
        gone = np.unique(np.r_[np.arange(64, 128), [0, W.ZERO_ROW, 63, 128, 200, W.DUP_FIRST + 5 + 64, n - 1]])
        assert idx.remove(gone + 1) == len(gone)
        keep = np.setdiff1d(np.arange(n), gone)
        same(idx.search(Q, 10), oracle_search_kept(oracle, X, keep, Q, 10), f"dim {dim}: removed, before compact")
        kept = idx.compact()
        np.testing.assert_array_equal(kept, keep.astype(np.uint64) + 1, err_msg=f"dim {dim}: kept_ids")
        assert len(idx) == len(keep) and idx.removed == 0
        rows = np.ascontiguousarray(X[keep])
        np.testing.assert_array_equal(bits(idx.get_rows(0, len(keep))), bits(rows), err_msg=f"dim {dim}: get_rows after compact")
        for k in (10, 300):
            same(idx.search(Q, k), oracle_lists(oracle, rows, Q, k), f"dim {dim}: after compact k {k}")
    print(f"WIDTH | get_rows, add_device, save / load, 3 shards, remove, compact | dim {dim} ds {ds} | {time.perf_counter() - t0:.2f} s")


def oracle_search_kept(oracle, X, keep, Q, k):
    """the oracle on the kept rows, under the ids the rows had before the compaction -> one tuple of the four lists"""
    ids, sc, di, nf = oracle_lists(oracle, np.ascontiguousarray(X[keep]), Q, k)
    old = np.where(ids != 0, (keep.astype(np.uint64) + 1)[np.maximum(ids.astype(np.int64) - 1, 0)], 0).astype(np.uint64)
    return old, sc, di, nf


@pytest.mark.parametrize("dim", W.COMPRESSED)
def test_compressed_corpus(dim, oracle, lib_built):
    X, _ = W.corpus(dim)
    Q = W.form_queries(dim)
    n = W.n_rows(dim)
    t0 = time.perf_counter()
    with open_kind(dim, "compressed") as idx:
        assert idx.add(X) == 1
        rows = idx.get_rows(0, n)
        assert rows.shape == X.shape and np.isfinite(rows).all() and not rows[W.ZERO_ROW].any()
        model = IndexModel(dim, oracle, compressed=True)
        model.add(rows)
        for k in (10, 300):
            same(idx.search(Q, k), oracle_lists(oracle, rows, Q, k), f"dim {dim} compressed k {k}")
        doc = np.array([[200, 270]], np.uint64)
        same(idx.search_filtered(Q, 10, ranges=doc), model.search_filtered(Q, 10, ranges=doc), f"dim {dim} compressed filtered")
        same(idx.search_range(Q, np.float32(0.2), 512), model.search_range(Q, np.float32(0.2), 512), f"dim {dim} compressed range")
        qids = np.array([W.DUP_FIRST + 1, W.ENDS_ROW + 1, 17], np.uint64)
        same(idx.search_by_id(qids, 10), model.search_by_id(qids, 10), f"dim {dim} compressed by_id")
        cand = np.random.default_rng(dim).integers(0, n + 3, (len(Q), 70)).astype(np.uint64)
        same(idx.score_ids(Q, cand), model.score_ids(Q, cand), f"dim {dim} compressed score_ids")
        same(idx.search_mmr(Q, 10, fetch=32), model.search_mmr(Q, 10, fetch=32), f"dim {dim} compressed mmr")
        assert idx.stats().scan_launches == 0, "(condition on the input) the two out-of-range norms keep this corpus on the EXACT path"
    # the same rows without the two out-of-range norms: the scan over the compressed rows answers
    T = W.tame_corpus(dim)
    seen = []
    with open_kind(dim, "compressed") as idx:
        assert idx.add(T) == 1
        rows = idx.get_rows(0, n)
        for B in W.batch_sizes(dim):
            Qb = W.queries(dim, B)
            idx.reset_stats()
            same(idx.search(Qb, 10), oracle_lists(oracle, rows, Qb, 10), f"dim {dim} compressed, no out-of-range norm, B {B}")
            st = idx.stats()
            seen.append((B, st.scan_launches, st.fallback_queries))
            assert st.scan_launches == W.passes(dim, "compressed", B) and st.fallback_queries == W.FALLBACK_QUERIES, (dim, B, seen)
            assert st.scan_bytes == st.scan_launches * 704 * W.ds_of(dim) * 2, (dim, B, st.scan_bytes)
        doc = np.array([[200, 270]], np.uint64)
        model = IndexModel(dim, oracle, compressed=True)
        model.add(rows)
        same(idx.search_filtered(Q, 10, ranges=doc), model.search_filtered(Q, 10, ranges=doc), f"dim {dim} compressed, tame, filtered")
        same(idx.search_range(Q, np.float32(0.2), 512), model.search_range(Q, np.float32(0.2), 512), f"dim {dim} compressed, tame, range")
    print(f"WIDTH | compressed corpus without out-of-range norms | dim {dim} | (B, scan_launches, fallback_queries) {seen}")
    print(f"WIDTH | compressed corpus | dim {dim} ds {W.ds_of(dim)} | {time.perf_counter() - t0:.2f} s")


# ---- d. refusals --------------------------------------------------------------------------------------------------------------------
def refused(call, code, *words):
    from memex_amd import _lib
    with pytest.raises(_lib.MemexHipError) as e:
        call()
    assert e.value.code == code, (e.value.code, e.value.msg)
    for w in words:
        assert str(w) in e.value.msg, (w, e.value.msg)


def test_refusals_name_their_limit(oracle, lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    for dim in W.REFUSED:
        refused(lambda: FlatIndex(dim), _lib.MX_EINVAL, dim, W.MAX_DIM)
        refused(lambda: FlatIndex(dim, devices=[0, 0], block_rows=64), _lib.MX_EINVAL, dim, W.MAX_DIM)
    X, Q = W.corpus(1537)[0], W.form_queries(1537)
    with FlatIndex(1537) as idx:
        refused(lambda: idx.set_corpus_mode("bf16"), _lib.MX_EUNSUPPORTED, LIMIT)
        idx.add(X)
        same(idx.search(Q, 10), oracle_lists(oracle, X, Q, 10), "dim 1537 after the refused corpus mode")
    for dim in (8193, 65536):
        X, Q = W.corpus(dim)[0], W.form_queries(dim)
        with FlatIndex(dim) as idx:
            idx.add(X)
            want = oracle_lists(oracle, X, Q, 10)
            refused(lambda: idx.search_mmr(Q, 10, fetch=32), _lib.MX_EUNSUPPORTED, W.MMR_MAX_DS)
            same(idx.search(Q, 10), want, f"dim {dim} after the refused mmr")
            cand = np.arange(1, 11, dtype=np.uint64)[None, :].repeat(len(Q), 0)
            refused(lambda: idx.score_ids(Q, cand), _lib.MX_EUNSUPPORTED, W.MMR_MAX_DS)
            same(idx.search(Q, 10), want, f"dim {dim} after the refused score_ids")
            # nothing is written to the outputs: the raw calls with poisoned arrays
            L = _lib.lib()
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            q = np.ascontiguousarray(Q)
            ids = np.full((len(Q), 10), 0xABABABABABABABAB, np.uint64)
            sc, di = np.full((len(Q), 10), -7.5, np.float32), np.full((len(Q), 10), -7.5, np.float32)
            order, nf = np.full((len(Q), 10), -77, np.int32), np.full(len(Q), -77, np.int32)
            assert L.mx_index_search_mmr(idx._h, p(q), len(Q), 10, 32, 0.5, p(ids), p(sc), p(di), p(nf)) == _lib.MX_EUNSUPPORTED
            assert (ids == 0xABABABABABABABAB).all() and (sc == -7.5).all() and (di == -7.5).all() and (nf == -77).all()
            assert L.mx_index_score_ids(idx._h, p(q), len(Q), p(cand), 10, p(sc), p(di), p(order), p(nf)) == _lib.MX_EUNSUPPORTED
            assert (sc == -7.5).all() and (di == -7.5).all() and (order == -77).all() and (nf == -77).all()
            same(idx.search(Q, 10), want, f"dim {dim} after the raw refused calls")


def blank(B, k, counts=False):
    out = (np.zeros((B, k), np.uint64), np.zeros((B, k), np.float32), np.full((B, k), np.inf, np.float32), np.zeros(B, np.int32))
    return out + (np.zeros(B, np.uint64),) if counts else out


@pytest.mark.parametrize("dim", (3, 1536, 1537, 8193, 65536))
def test_nothing_to_find_is_an_answer_at_every_width(dim, lib_built):
    """An empty index, a filter that allows no row: the blank lists, not an error.  These calls end in finish_kernel /
    range_finish_kernel launches that only write blanks; above 1536 padded dims they used to ask for more LDS than the kernels'
    limit and failed (tests/WIDTH_AXIS.md, findings)."""
    from memex_amd.index import FlatIndex
    X, Q = W.corpus(dim)[0], W.form_queries(dim)
    B, n = len(Q), W.n_rows(dim)
    with FlatIndex(dim) as idx:
        same(idx.search(Q, 10), blank(B, 10), f"dim {dim}: empty index")
        same(idx.search_filtered(Q, 10, ranges=[[1, 5]]), blank(B, 10), f"dim {dim}: empty index, filtered")
        same(idx.search_range(Q, np.float32(0.2), 16), blank(B, 16, True), f"dim {dim}: empty index, range")
        idx.add(X)
        same(idx.search_filtered(Q, 10, ranges=[[n + 10, n + 20]]), blank(B, 10), f"dim {dim}: a filter that names no row")
        with idx.make_filter() as flt:
            same(idx.search_with(flt, Q, 10), blank(B, 10), f"dim {dim}: an empty resident filter")
        with FlatIndex(dim, devices=[0, 0, 0], block_rows=64) as sh:
            same(sh.search(Q, 10), blank(B, 10), f"dim {dim}: empty 3-shard handle")
            same(sh.search_range(Q, np.float32(0.2), 16), blank(B, 16, True), f"dim {dim}: empty 3-shard handle, range")


# ---- the random walk on a width that has no scan ------------------------------------------------------------------------------------
def test_random_walk_without_a_scan(oracle, lib_built, tmp_path):
    """tests/random_walk.py at 1540 dims (1792 padded): every form across growth, compaction and load with the EXACT path under it.
    The layout is not one of random_walk.CASES (tests/test_random_walk_model.py asserts every event and defect for those); the CPU
    test walks the same seed on the model alone."""
    from memex_amd.index import FlatIndex
    assert W.ds_of(W.WALK["d"]) == 1792 and W.WALK["copy"] is None
    model = IndexModel(W.WALK["d"], oracle)
    t0 = time.perf_counter()
    with FlatIndex(W.WALK["d"]) as idx:
        run(idx, model, np.random.default_rng(W.WALK["seed"]), STEPS, store_dir=tmp_path, cone=False, tag=f"{W.WALK['name']} seed {W.WALK['seed']}")
        st = idx.stats()
        assert st.filter_kind == 0 and st.scan_launches == 0
    print(f"WIDTH | walk | {W.WALK['name']} seed {W.WALK['seed']}: {STEPS} steps in {time.perf_counter() - t0:.2f} s")
