"""The ``*_device`` twins of every search form, on caller-owned HBM (tests/DEVICE_TWINS.md; the tools are tests/device_twins.py).

A  the three twins no GPU test reached -- search_filtered_device, search_with_device, search_range_device -- branch by branch against
   the oracle, each case proving from mx_index_stats that it ran the branch it names; then B from 1 to 1025 for those three and for
   search_device, either side of a pass (256) and of a batch (512), where the pointer offsets of the split can be wrong.
B  every form, on guarded outputs with queries that are still being produced on a busy side stream, against its host twin.
C  non-finite queries at each of the five places the pipeline can notice them, and what the paths that read no query do.
D  the wrapper refuses tensors of the wrong device, dtype, shape or layout before the library sees a pointer.

Every comparison is exact: ids, counts, keys and orders as integers, scores, dists and combined by their bits; the guard zones around
every output must stay as they were.  Every case prints a `TWINS | ...` line with its wall time; DEVICE_TWINS.md quotes them."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import device_twins as DT
from filtered_model import allowed_mask
from oracle.search_oracle import score_from_dist
from range_model import oracle_dists, range_oracle

pytestmark = pytest.mark.gpu

DIM = 72


def device_answer(form, idx, c, Q, what, absent=()):
    """the form's device twin on guarded outputs, queries on the default stream -> the outputs, guards checked"""
    import torch
    q = None if Q is None else torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    o, checks = DT.make_outs(form, c.B, c, absent)
    torch.cuda.synchronize()
    form.call_device(idx, c, q, o)
    torch.cuda.synchronize()
    for name, check in checks.items():
        check(f"{what}: {name}")
    return o


def sentinels_left(form, o, what):
    for name, kind, _ in form.outs:
        if o.get(name) is not None:
            assert bool((o[name] == DT.KINDS[kind][1]).all()), f"{what}: {name} was written"


class Handle:
    """One index of section A with what its answers are compared with"""

    def __init__(self, oracle, X, gone, Q, D=None, **kw):
        from memex_amd.index import FlatIndex
        self.G = len(kw.get("devices", [0]))
        compressed = kw.pop("compressed", False)
        copy = kw.pop("copy", None)
        self.idx = FlatIndex(X.shape[1], **kw)
        if compressed:
            self.idx.set_corpus_mode("bf16")
        self.idx.add(X)
        if copy is not None:
            self.idx.set_filter_copy(copy)
        self.idx.set_id_offset(DT.ID_OFFSET)
        self.off, self.n = DT.ID_OFFSET, X.shape[0]
        self.alive = np.ones(self.n, bool)
        if len(gone):
            assert self.idx.remove(np.asarray(gone, np.uint64) + 1 + self.off) == len(gone)
            self.alive[gone] = False
        self.rows = self.idx.get_rows(0, self.n) if compressed else X
        self.Q = Q
        self.D = oracle_dists(oracle, self.rows, Q) if D is None else D
        self.filters = DT.filters(self.off, self.n)
        self._resident = {}

    def keep(self, ranges):
        return self.alive & allowed_mask(self.n, ranges, self.off)

    def resident(self, name):
        if name not in self._resident:
            self._resident[name] = self.idx.make_filter(ranges=self.filters[name])
        return self._resident[name]

    def close(self):
        for f in self._resident.values():
            f.close()
        self.idx.close()


@pytest.fixture(scope="module")
def world(oracle, lib_built):
    """Section A's corpus on a plain, a three-shard and a compressed handle, and the corpus of 17000 copies"""
    X, gone = DT.corpus(DIM)
    Q = DT.queries(X, 12)
    h = {"plain": Handle(oracle, X, gone, Q),
         "sharded": Handle(oracle, X, gone, Q, devices=[0, 0, 0], block_rows=64),
         "compressed": Handle(oracle, X, gone, Q, compressed=True)}
    C, row = DT.copies_corpus(DIM)
    Qc = np.stack([C[row], DT.queries(C, 1)[0], C[row] * 0.5]).astype(np.float32)
    h["copies"] = Handle(oracle, C, np.arange(2100, 2110), Qc)
    h["copies"].filters["copies"] = np.array([[DT.ID_OFFSET + row + 1, DT.ID_OFFSET + row + 1 + DT.N_COPIES]], np.uint64)
    assert h["plain"].idx.stats().filter_kind == 2 and h["compressed"].idx.stats().filter_kind == 3
    yield h
    for x in h.values():
        x.close()


# ---- A. top-k ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DT.TOPK_CASES, ids=[c.name for c in DT.TOPK_CASES])
def test_filtered_twins_branch_by_branch(case, world, monkeypatch):
    h = world[case.handle]
    idx, ranges = h.idx, h.filters[case.flt]
    Q = h.Q
    B = len(Q)
    want = DT.topk_from_dists(h.D, h.keep(ranges), case.k, h.off)
    c = SimpleNamespace(B=B, k=case.k, dim=DIM, ranges=ranges, flt={idx: h.resident(case.flt)})
    absent = () if case.dists else ("dists",)
    if case.force is not None:
        monkeypatch.setenv("MEMEX_HIP_DEBUG", f"filt_subset={case.force}")
    idx.set_search_mode(case.mode)
    try:
        for name in ("search_filtered_device", "search_with_device"):
            form = DT.BY_NAME[name]
            idx.reset_stats()
            t0 = time.perf_counter()
            o = device_answer(form, idx, c, Q, f"{case.name}: {name}", absent)
            ms = (time.perf_counter() - t0) * 1e3
            st = idx.stats()
            print(f"TWINS | A top-k | {case.name} | {name} | {case.branch} | subset {st.subset_queries} filtered {st.filtered_queries} "
                  f"scans {st.scan_launches} retry {st.retry_queries} fallback {st.fallback_queries} | {ms:.1f} ms")
            DT.prove(case.branch, st, B, h.G)
            DT.compare(form, o, want, f"{case.name}: {name}")
        if case.equals_search:
            form = DT.BY_NAME["search_device"]
            o = device_answer(form, idx, c, Q, f"{case.name}: search_device", absent)
            DT.compare(form, o, want, f"{case.name}: search_device")
    finally:
        idx.set_search_mode(0)


def test_resident_filter_after_remove_compact_and_on_each_copy_kind(oracle, lib_built):
    """One index of its own: the copy kinds in turn, then rows removed under a resident filter, then compact, which makes it stale"""
    from memex_amd import _lib
    X, gone = DT.corpus(DIM)
    Q = DT.queries(X, 12)
    h = Handle(oracle, X, gone, Q)
    try:
        idx, B = h.idx, len(Q)
        for kind, fk in (("bf16", 3), (False, 0), ("i8", 2)):
            idx.set_filter_copy(kind)
            assert idx.stats().filter_kind == fk
            for flt, branch in (("big", "masked"), ("small", "subset")):
                ranges = h.filters[flt]
                want = DT.topk_from_dists(h.D, h.keep(ranges), 10, h.off)
                c = SimpleNamespace(B=B, k=10, dim=DIM, ranges=ranges, flt={idx: h.resident(flt)})
                for name in ("search_filtered_device", "search_with_device"):
                    idx.reset_stats()
                    o = device_answer(DT.BY_NAME[name], idx, c, Q, f"copy {kind}, {flt}: {name}")
                    DT.prove(branch, idx.stats(), B)
                    DT.compare(DT.BY_NAME[name], o, want, f"copy {kind}, {flt}: {name}")
        # rows removed after the filters were made: both twins leave them out, the resident one without being told
        more = np.setdiff1d(np.r_[100:120, 12000:12100, DT.DUP_FIRST], gone)
        assert idx.remove(more.astype(np.uint64) + 1 + h.off) == len(more)
        h.alive[more] = False
        for flt, branch in (("big", "masked"), ("small", "subset")):
            ranges = h.filters[flt]
            want = DT.topk_from_dists(h.D, h.keep(ranges), 10, h.off)
            c = SimpleNamespace(B=B, k=10, dim=DIM, ranges=ranges, flt={idx: h.resident(flt)})
            for name in ("search_filtered_device", "search_with_device"):
                idx.reset_stats()
                o = device_answer(DT.BY_NAME[name], idx, c, Q, f"after remove, {flt}: {name}")
                DT.prove(branch, idx.stats(), B)
                DT.compare(DT.BY_NAME[name], o, want, f"after remove, {flt}: {name}")
        # compact renumbers: the per-call ranges name the new ids, the resident filter is stale and must raise before anything runs
        kept = idx.compact()
        live = np.flatnonzero(h.alive)
        np.testing.assert_array_equal(kept, live.astype(np.uint64) + 1 + h.off)
        D2, alive2 = h.D[:, live], np.ones(live.size, bool)
        ranges = np.array([[h.off + 1001, h.off + 1001 + 19000]], np.uint64)
        c = SimpleNamespace(B=B, k=10, dim=DIM, ranges=ranges, flt={idx: h.resident("big")})
        form = DT.BY_NAME["search_filtered_device"]
        idx.reset_stats()
        o = device_answer(form, idx, c, Q, "after compact: search_filtered_device")
        DT.prove("masked", idx.stats(), B)
        DT.compare(form, o, DT.topk_from_dists(D2, alive2 & allowed_mask(live.size, ranges, h.off), 10, h.off), "after compact")
        form = DT.BY_NAME["search_with_device"]
        before = idx.stats().searches
        import torch
        o, checks = DT.make_outs(form, B, c)
        with pytest.raises(_lib.MemexHipError, match="stale") as e:
            form.call_device(idx, c, torch.from_numpy(Q).cuda(), o)
        assert e.value.code == _lib.MX_EINVAL and idx.stats().searches == before
        torch.cuda.synchronize()
        sentinels_left(form, o, "stale filter")
        for check in checks.values():
            check("stale filter")
    finally:
        h.close()


# ---- A. range ------------------------------------------------------------------------------------------------------------------------
def range_thresholds(kind, D, alive, cap):
    """f32 [B]: per query, thresholds made from the oracle's own scores (test_range_gpu.thresholds' construction)"""
    B = D.shape[0]
    S = np.sort(np.where(alive, score_from_dist(D), -np.inf), axis=1)[:, ::-1]
    at = lambda j: S[np.arange(B), np.minimum(j, int(alive.sum()) - 1)].astype(np.float32)  # noqa: E731
    if kind == "on":
        return at(np.full(B, cap - 1))
    if kind == "above":
        return np.nextafter(at(np.full(B, cap - 1)), np.float32(2.0)).astype(np.float32)
    if kind == "all":
        return np.full(B, -1.0, np.float32)
    if kind == "below":
        return np.full(B, -1.5, np.float32)
    if kind == "none":
        return np.full(B, 1.0000001, np.float32)
    if kind == "rank3000":
        return at(np.full(B, 2999))
    if kind == "copies":
        return at(np.full(B, DT.N_COPIES - 100))
    assert kind == "mixed"
    t = at(np.resize(np.array([0, 3, cap - 1, cap, 2 * cap, 57, 400, 1]), B))
    t[B // 2] = np.float32(1.0000001)                                                 # one query of the batch finds nothing
    t[B // 3] = np.nextafter(t[B // 3], np.float32(2.0))
    return t


@pytest.mark.parametrize("case", DT.RANGE_CASES, ids=[c.name for c in DT.RANGE_CASES])
def test_range_twin_branch_by_branch(case, world):
    h = world[case.handle]
    idx = h.idx
    # the zero query scores 1 against every row: it belongs to the cases whose branch is the overflow or the EXACT path
    use = np.arange(len(h.Q)) if case.branch != "range-scan" or case.handle == "copies" else np.flatnonzero(h.Q.any(axis=1))
    Q, D = h.Q[use], h.D[use]
    B = len(Q)
    t = range_thresholds(case.t, D, h.alive, case.cap)
    want = range_oracle(D, h.alive, t, case.cap, h.off)
    if case.t in ("all", "below"):
        assert (want[4] == h.alive.sum()).all()
    if case.t == "none":
        assert not want[4].any()
    if case.t in ("on", "above"):
        assert (want[4] >= case.cap).all() if case.t == "on" else (want[4] < case.cap).all()
    form = DT.BY_NAME["search_range_device"]
    c = SimpleNamespace(B=B, cap=case.cap, dim=DIM, t=t)
    idx.set_search_mode(case.mode)
    try:
        idx.reset_stats()
        t0 = time.perf_counter()
        o = device_answer(form, idx, c, Q, case.name, () if case.dists else ("dists",))
        ms = (time.perf_counter() - t0) * 1e3
        st = idx.stats()
        print(f"TWINS | A range | {case.name} | {case.branch} | scans {st.scan_launches} fallback {st.fallback_queries} | "
              f"in range {int(want[4].min())} .. {int(want[4].max())} | {ms:.1f} ms")
        DT.prove(case.branch, st, B, h.G)
        DT.compare(form, o, want, case.name)
    finally:
        idx.set_search_mode(0)


# ---- A. the B axis -------------------------------------------------------------------------------------------------------------------
BMAX = max(DT.B_AXIS)


@pytest.fixture(scope="module")
def axis(oracle, lib_built):
    """(dim, handle) -> Handle with 1025 queries and the references of the four twins, computed once: the int8 copy at 72 dims, the
    bf16 copy at 520 (kc = 5: above kMaxKC8x2, so more than 256 queries are split into passes)"""
    out = {}
    for dim, copy in ((72, "i8"), (520, "bf16")):
        X, gone = DT.corpus(dim)
        Q = DT.queries(X, BMAX, seed=dim)
        for name, kw in (("plain", {}), ("sharded", dict(devices=[0, 0, 0], block_rows=64))):
            if name == "plain":
                h = first = Handle(oracle, X, gone, Q, copy=copy, **kw)
                h.k, h.cap = 10, 10
                h.t = range_thresholds("mixed", h.D, h.alive, h.cap)
                h.want = {"search_device": DT.topk_from_dists(h.D, h.alive, h.k, h.off),
                          "search_filtered_device": DT.topk_from_dists(h.D, h.keep(h.filters["big"]), h.k, h.off),
                          "search_range_device": range_oracle(h.D, h.alive, h.t, h.cap, h.off)}
                h.want["search_with_device"] = h.want["search_filtered_device"]
            else:                                                                      # the same rows and references, three shards
                h = Handle(oracle, X, gone, Q, D=first.D, copy=copy, **kw)
                h.k, h.cap, h.t, h.want = first.k, first.cap, first.t, first.want
            assert h.idx.stats().filter_kind == (2 if copy == "i8" else 3)
            out[dim, name] = h
    yield out
    for h in out.values():
        h.close()


@pytest.mark.parametrize("B", DT.B_AXIS)
@pytest.mark.parametrize("handle", ("plain", "sharded"))
@pytest.mark.parametrize("dim", (72, 520))
def test_batch_axis(dim, handle, B, axis):
    h = axis[dim, handle]
    idx, Q = h.idx, h.Q[:B]
    c = SimpleNamespace(B=B, k=h.k, cap=h.cap, dim=dim, ranges=h.filters["big"], flt={idx: h.resident("big")}, t=h.t)
    t0 = time.perf_counter()
    for name, want in h.want.items():
        form = DT.BY_NAME[name]
        o = device_answer(form, idx, c, Q, f"{dim} dims, {handle}, B = {B}: {name}")
        DT.compare(form, o, tuple(w[:B] for w in want), f"{dim} dims, {handle}, B = {B}: {name}")
    print(f"TWINS | A batch axis | {dim} dims | {handle} | B = {B} | {(time.perf_counter() - t0) * 1e3:.1f} ms for the four twins")


# ---- B. every form, guarded outputs, late queries, against the host twin -----------------------------------------------------------
N_SMALL = 5000
B_SMALL, B_SPLIT = 37, 600


@pytest.fixture(scope="module")
def small(lib_built):
    """5000 rows of 72 dims on a plain and a three-shard handle, with a grouping, a prior and a resident filter each, and the
    host-side arguments of every form for up to B_SPLIT queries"""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(2024)
    X = rng.standard_normal((N_SMALL, DIM)).astype(np.float32)
    X[40:44] = X[39]
    gone = np.unique(np.r_[rng.choice(N_SMALL, 60, replace=False), 41])
    off = 500
    subs = 3
    Qs = rng.standard_normal((2, B_SPLIT * subs, DIM)).astype(np.float32)              # [0]: the queries, [1]: the decoys
    Qs[0, :8] = X[rng.integers(0, N_SMALL, 8)] + 0.05 * Qs[0, :8]
    ranges = np.array([[off + 3001, off + 4501], [off + 11, off + 1500]], np.uint64)
    doc = np.arange(0, N_SMALL, 50)
    doc_ranges = np.stack([doc, doc + 35], 1).astype(np.uint64) + 1 + off               # 35 of every 50 rows belong to a document
    c = SimpleNamespace(dim=DIM, k=7, cap=9, n=3, subs=subs, m=11, ranges=ranges, flt={}, grp={}, pri={}, off=off, X=X, gone=gone,
                        t=rng.choice(np.array([0.2, 0.3, 0.45, 1.5, -0.05], np.float32), B_SPLIT),
                        qids=rng.integers(off, off + N_SMALL + 20, B_SPLIT).astype(np.uint64),
                        examples=rng.integers(off + 1, off + N_SMALL + 1, (B_SPLIT, 2)).astype(np.uint64), ex_w=np.array([1.0, -0.25], np.float32),
                        cand=rng.integers(off - 3, off + N_SMALL + 3, (B_SPLIT, 11)).astype(np.uint64), Q=Qs[0], decoy=Qs[1])
    c.cand[:, 4] = 0
    c.qids[:3] = gone[:3].astype(np.uint64) + 1 + off                                   # removed rows among the by-id queries
    handles = {"plain": FlatIndex(DIM), "sharded": FlatIndex(DIM, devices=[0, 0, 0], block_rows=64)}
    for idx in handles.values():
        idx.add(X)
        idx.set_id_offset(off)
        idx.remove(gone.astype(np.uint64) + 1 + off)
        c.flt[idx] = idx.make_filter(ranges=ranges)
        c.grp[idx] = idx.make_grouping()
        c.grp[idx].set_ranges(doc_ranges, (doc // 50 + 1).astype(np.uint32))
        c.pri[idx] = idx.make_prior()
        c.pri[idx].set_ranges(doc_ranges, rng.uniform(0, 0.5, len(doc)).astype(np.float32))
    c.handles = handles
    yield c
    for idx in handles.values():
        for d in (c.flt, c.grp, c.pri):
            d[idx].close()
        idx.close()


def _variants():
    for f in DT.SEARCH_FORMS:
        yield f.name, "all outputs"
        yield f.name, "optional outputs None"
        if f.name == "search_like_device":
            yield f.name, "no queries"


@pytest.mark.parametrize("B", (B_SMALL, B_SPLIT))
@pytest.mark.parametrize("handle", ("plain", "sharded"))
@pytest.mark.parametrize("name,variant", list(_variants()))
def test_every_form_on_guarded_outputs_with_late_queries(name, variant, handle, B, small):
    import torch
    form, idx = DT.BY_NAME[name], small.handles[handle]
    c = small
    c.B = B
    absent = form.optional if variant == "optional outputs None" else ()
    shape = None if variant == "no queries" else DT.query_shape(form, B, c)
    count = 0 if shape is None else int(np.prod(shape[:-1]))
    Q = None if shape is None else c.Q[:count].reshape(shape)
    # the host twin first: whatever the form allocates on first use (an allocation waits for the whole device, side stream included)
    # exists before the device call, which then has only mx_index_wait_stream between it and the decoy
    host = form.call_host(idx, c, Q)
    t0 = time.perf_counter()
    if shape is None:                                      # no query tensor: the outputs' pre-fill is the late work
        q, side = None, DT.busy_side()
    else:
        q, side = DT.late_queries(Q, c.decoy[:count].reshape(shape))
    with torch.cuda.stream(side):
        o, checks = DT.make_outs(form, B, c, absent)       # pre-filled on the side stream, behind the chain
        assert not side.query(), "the side stream went idle before the call: the chain is too short"
        form.call_device(idx, c, q, o)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    what = f"{name}, {variant}, {handle}, B = {B}"
    DT.compare(form, o, host, what)
    for n, check in checks.items():
        check(f"{what}: {n}")
    assert sum(v is not None for v in o.values()) == len(form.outs) - len(absent)
    print(f"TWINS | B | {name} | {variant} | {handle} | B = {B} | {ms:.1f} ms")


def test_add_device_takes_late_rows(small, oracle):
    """The one ``*_device`` method that is not a search: rows still being produced on the busy side stream, then searched"""
    import torch
    from memex_amd.index import FlatIndex
    X = small.X[:1000]
    for kw in ({}, dict(devices=[0, 0, 0], block_rows=64)):
        with FlatIndex(DIM, **kw) as idx:
            rows, side = DT.late_queries(X, small.X[1000:2000])
            with torch.cuda.stream(side):
                assert not side.query()
                assert idx.add_device(rows) == 1
            np.testing.assert_array_equal(idx.get_rows(0, 1000), X)
            ids, sc, di, nf = idx.search(small.Q[:5], 5)
            oi, od, os_, onf = oracle.search(X, small.Q[:5], 5)
            DT.same_bits(ids, oi, "ids")
            DT.same_bits(di, od, "dists")
            DT.same_bits(sc, os_, "scores")


# ---- C. non-finite queries -----------------------------------------------------------------------------------------------------------
# the five places a device call can notice a non-finite query (index.hip: search_batch and range_batch), and how to get there
SITES = [
    ("subset kernel", "search_filtered_device", dict(ranges="small"), 0),
    ("subset kernel, resident filter", "search_with_device", dict(ranges="small"), 0),
    ("AUTO top-k", "search_device", {}, 0),
    ("EXACT top-k (k = 300)", "search_device", dict(k=300), 0),
    ("EXACT top-k (MX_SEARCH_EXACT)", "search_device", {}, 1),
    ("AUTO range", "search_range_device", {}, 0),
    ("EXACT range", "search_range_device", {}, 1),
]


@pytest.mark.parametrize("bad", (np.nan, np.inf), ids=("nan", "inf"))
@pytest.mark.parametrize("handle", ("plain", "sharded"))
@pytest.mark.parametrize("site", SITES, ids=[s[0] for s in SITES])
def test_non_finite_queries_are_rejected_at_every_site(site, handle, bad, small):
    import torch
    from memex_amd import _lib
    what, name, args, mode = site
    form, idx = DT.BY_NAME[name], small.handles[handle]
    live = [r for r in range(70, 128) if r not in set(small.gone.tolist())]
    # rows 64 .. 127 are block 1: shard 1 of the three-shard handle holds the bad query's best rows
    Q = np.stack([small.Q[0], small.X[live[0]] + 0.01 * small.Q[1], small.Q[2]]).astype(np.float32)
    Qbad = Q.copy()
    Qbad[1, 17] = bad
    small_ranges = np.array([[small.off + 65, small.off + 129], [small.off + 2001, small.off + 2031]], np.uint64)
    c = SimpleNamespace(B=3, dim=DIM, k=args.get("k", 7), cap=9, t=np.array([0.2, 0.3, 0.2], np.float32),
                        ranges=small_ranges if args.get("ranges") else small.ranges, flt={})
    flt = idx.make_filter(ranges=c.ranges)
    c.flt[idx] = flt
    idx.set_search_mode(mode)
    try:
        o, checks = DT.make_outs(form, 3, c)
        before = idx.stats().searches
        with pytest.raises(_lib.MemexHipError, match="non-finite") as e:
            form.call_device(idx, c, torch.from_numpy(Qbad).cuda(), o)
        assert e.value.code == _lib.MX_EINVAL
        torch.cuda.synchronize()
        for n, check in checks.items():
            check(f"{what}: {n} after the refused call")
        assert idx.stats().searches == before
        # the same index answers the two good queries in the next call
        c.B, c.t = 2, c.t[[0, 2]]
        idx.reset_stats()
        good = Q[[0, 2]]
        o = device_answer(form, idx, c, good, f"{what}: the good queries afterwards")
        st = idx.stats()
        if "subset" in what:
            assert st.subset_queries == 2, what
        elif "EXACT" in what:
            assert st.scan_launches == 0, what
        else:
            assert st.scan_launches >= 1 and st.fallback_queries == 0, what
        DT.compare(form, o, form.call_host(idx, c, good), f"{what}: the good queries afterwards")
    finally:
        idx.set_search_mode(0)
        flt.close()


# What a device call does with a non-finite query when it answers without reading one (include/memex_hip.h, the stream contract):
# a top-k form with nothing to find -- an empty index or a filter that allows no live row -- returns MX_OK and the blank lists, since
# finish_kernel writes them without the flag words being looked at; an index whose rows are all removed is still scanned, and the range
# form looks at the flag words on every path: both refuse.
UNREAD = [
    ("empty index, top-k", "search_device", "empty", "ok"),
    ("empty index, filtered", "search_filtered_device", "empty", "ok"),
    ("empty index, range above 1", "search_range_device", "empty", "refused"),
    ("the empty filter", "search_filtered_device", "no filter rows", "ok"),
    ("the empty resident filter", "search_with_device", "no filter rows", "ok"),
    ("every row removed, top-k", "search_device", "all removed", "refused"),
    ("every row removed, range above 1", "search_range_device", "all removed", "refused"),
    ("range above 1 on live rows", "search_range_device", "live", "refused"),
]


@pytest.mark.parametrize("handle", ("plain", "sharded"))
@pytest.mark.parametrize("case", UNREAD, ids=[u[0] for u in UNREAD])
def test_non_finite_queries_on_the_paths_that_read_no_query(case, handle, small, lib_built):
    import torch
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    what, name, state, outcome = case
    form = DT.BY_NAME[name]
    kw = dict(devices=[0, 0, 0], block_rows=64) if handle == "sharded" else {}
    Q = small.Q[:3].copy()
    Q[1, 5] = np.nan
    Q[2, 70] = np.inf
    with FlatIndex(DIM, **kw) as idx:
        if state != "empty":
            idx.add(small.X[:600])
        if state == "all removed":
            idx.remove(np.arange(1, 601, dtype=np.uint64))
        ranges = np.zeros((0, 2), np.uint64) if state == "no filter rows" else np.array([[1, 601]], np.uint64)
        with idx.make_filter(ranges=ranges) as flt:
            c = SimpleNamespace(B=3, dim=DIM, k=7, cap=9, t=np.full(3, 1.0000001, np.float32), ranges=ranges, flt={idx: flt})
            o, checks = DT.make_outs(form, 3, c)
            if outcome == "refused":
                with pytest.raises(_lib.MemexHipError, match="non-finite") as e:
                    form.call_device(idx, c, torch.from_numpy(Q).cuda(), o)
                assert e.value.code == _lib.MX_EINVAL
            else:
                form.call_device(idx, c, torch.from_numpy(Q).cuda(), o)
                torch.cuda.synchronize()
                assert not o["n_found"].any() and not o["ids"].any() and not o["scores"].any()
                assert bool(torch.isinf(o["dists"]).all()) and bool((o["dists"] > 0).all())
            torch.cuda.synchronize()
            for n, check in checks.items():
                check(f"{what}: {n}")


# ---- D. the wrapper refuses what it cannot pass on -----------------------------------------------------------------------------------
def _spoil(form, how, q, o, c):
    """-> (q, o, the argument that must be named): one argument of the call made wrong"""
    import torch
    o = dict(o)
    two_d = [n for n, _, w in form.outs if w is not None]
    if how == "dtype":
        n = two_d[0]
        o[n] = o[n].to(torch.float64 if o[n].dtype != torch.float64 else torch.float32)
        return q, o, n
    if how == "strided":
        if q is not None:
            wide = torch.zeros(tuple(q.shape[:-1]) + (q.shape[-1] + 1,), device="cuda")
            wide[..., :-1] = q
            return wide[..., :-1], o, "queries" if form.name == "search_like_device" else "q"
        n = "scores"
        o[n] = torch.full(tuple(reversed(o[n].shape)), -1.0, device="cuda").t()
        return q, o, n
    assert how == "column"
    n = two_d[-1]
    o[n] = o[n][..., :-1].contiguous()
    return q, o, n


@pytest.mark.parametrize("how", ("dtype", "strided", "column"))
@pytest.mark.parametrize("name", [f.name for f in DT.SEARCH_FORMS])
def test_wrapper_refuses_mis_shaped_device_tensors(name, how, small):
    import torch
    from memex_amd import _lib
    form, idx = DT.BY_NAME[name], small.handles["plain"]
    c = small
    c.B = B = 5
    shape = DT.query_shape(form, B, c)
    Q = None if shape is None else c.Q[:int(np.prod(shape[:-1]))].reshape(shape)
    q = None if Q is None else torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    o, checks = DT.make_outs(form, B, c)
    q2, o2, arg = _spoil(form, how, q, o, c)
    before = idx.stats().searches
    with pytest.raises(_lib.MemexHipError, match=f"{arg}:") as e:
        form.call_device(idx, c, q2, o2)
    assert e.value.code == _lib.MX_EINVAL and e.value.msg.startswith(arg + ":"), e.value.msg
    torch.cuda.synchronize()
    assert idx.stats().searches == before
    sentinels_left(form, o, f"{name}, {how}")
    sentinels_left(form, {n: t for n, t in o2.items() if how != "dtype" or n != arg}, f"{name}, {how}")
    for n, check in checks.items():
        check(f"{name}, {how}: {n}")


def test_wrapper_refuses_other_devices_and_add_device_checks_too(small):
    import torch
    from memex_amd import _lib
    idx = small.handles["plain"]
    form = DT.BY_NAME["search_device"]
    c = small
    c.B = 4
    o, _ = DT.make_outs(form, 4, c)
    before = idx.stats().searches
    for spoil in ("q", "ids"):                               # a host tensor where a device tensor belongs
        q = torch.from_numpy(np.ascontiguousarray(c.Q[:4]))
        o2 = dict(o)
        if spoil == "q":
            pass
        else:
            q = q.cuda()
            o2["ids"] = torch.zeros((4, c.k), dtype=torch.int64)
        with pytest.raises(_lib.MemexHipError, match=f"{spoil}: expected a tensor on cuda:0") as e:
            form.call_device(idx, c, q, o2)
        assert e.value.code == _lib.MX_EINVAL
    rows = torch.zeros((3, DIM + 1), device="cuda")
    for t, arg in ((rows, "shape"), (rows[:, :DIM], "contiguous"), (rows[:, :DIM].contiguous().double(), "dtype"), (rows[0, :DIM], "shape")):
        n = len(idx)
        with pytest.raises(_lib.MemexHipError, match=f"rows: expected .*{arg}"):
            idx.add_device(t)
        assert len(idx) == n
    assert idx.stats().searches == before
    sentinels_left(form, o, "other devices")
