"""What the device-pointer twin tests share (tests/DEVICE_TWINS.md) -- TEST INFRASTRUCTURE, not product code, and no test functions.

Every search form of FlatIndex has a host-pointer method and a ``*_device`` twin that hands the CALLER's HBM pointers to the kernels.
Three things make a twin wrong while its host method stays right, and each has a tool here:

  guarded()       caller outputs as a caller really has them: an interior slice of a larger allocation, at an odd element offset (only
                  the element type's own alignment), pre-filled with values no result can be, between guard zones that must stay as
                  they were.  A kernel that strides by its own buffer's capacity, writes slot B*k, or stores wider than an element
                  is caught here and nowhere on the host path, whose outputs are the index's own over-sized buffers.
  late_queries()  inputs produced on a side stream that is still busy when the call is made: only mx_index_wait_stream orders them.
  FORMS           one row per ``*_device`` method: how to call it on guarded outputs, how to call its host twin, which outputs exist
                  and which of them may be None.  tests/test_device_twins_model.py fails when a method has no row.
"""
import time
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

LEAD = 65          # elements in front of the view: odd, so the view has its element type's alignment and no more; at least 64
TAIL = 66          # elements behind it

# kind -> (torch dtype name, the view's pre-fill: no result can be it)
KINDS = {
    "id": ("int64", -1),        # ids and n_in_range: u64 in the library, i64 in torch; no id is 2^64 - 1
    "f32": ("float32", -1.0),   # dists are >= 0; a score of -1.0 belongs to dist 2.0, which no row of these corpora has
    "f64": ("float64", -1.0),
    "i32": ("int32", -7),       # counts, positions, keys
    "u8": ("uint8", 249),       # flags are 0 or 1
}


def _guard_value(dtype):
    """The guard zones' sentinel: bytes 0x5a in an integer, -12345 in a float (neither is a pre-fill or a result)"""
    if dtype.is_floating_point:
        return -12345.0
    return int.from_bytes(b"\x5a" * dtype.itemsize, "little")


def guarded(shape, dtype, fill, device="cuda"):
    """-> (view, check): a contiguous tensor of ``shape`` holding ``fill``, cut out of a flat allocation LEAD elements from its start;
    ``check()`` asserts that the LEAD elements in front and the TAIL elements behind still hold the guard sentinel."""
    import torch
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    g = _guard_value(dtype)
    flat = torch.full((LEAD + n + TAIL,), g, dtype=dtype, device=device)
    view = flat[LEAD:LEAD + n].view(shape)
    view.fill_(fill)
    assert view.is_contiguous() and (view.data_ptr() - flat.data_ptr()) == LEAD * dtype.itemsize

    def check(what=""):
        front = torch.nonzero(flat[:LEAD] != g).flatten().cpu().numpy()
        back = torch.nonzero(flat[LEAD + n:] != g).flatten().cpu().numpy()
        assert front.size == 0, f"{what}: written {LEAD - int(front.max())} element(s) in front of the {list(shape)} {dtype} view"
        assert back.size == 0, f"{what}: written {int(back.min()) + 1} element(s) behind the {list(shape)} {dtype} view"

    return view, check


def out(kind, shape, device="cuda"):
    """guarded() for an output of one of KINDS"""
    import torch
    name, fill = KINDS[kind]
    return guarded(shape, getattr(torch, name), fill, device)


# ---- a busy side stream ------------------------------------------------------------------------------------------------------------
_state = SimpleNamespace(side=None, a=None, b=None, chain=None, chain_ms=None)
CHAIN_SIDE = 2048          # the matmuls of the chain: [2048, 2048] f32
CHAIN_HOLD = 0.004         # seconds after enqueueing at which the stream must still be busy
CHAIN_CAP = 1.0            # seconds of work at which the doubling gives up


def side_stream():
    import torch
    if _state.side is None:
        _state.side = torch.cuda.Stream()
        _state.a = torch.full((CHAIN_SIDE, CHAIN_SIDE), 1.0 / CHAIN_SIDE, device="cuda")
        _state.b = torch.empty_like(_state.a)
        with torch.cuda.stream(_state.side):
            _enqueue_chain(2)                      # (the BLAS library's one-time set-up is not part of what is sized below)
        torch.cuda.synchronize()
    return _state.side


def _enqueue_chain(n):
    """n dependent matmuls on the current stream"""
    import torch
    for _ in range(n):
        torch.mm(_state.a, _state.a, out=_state.b)


def chain_length():
    """Matmuls that keep the side stream busy: sized once per session by doubling until ``side.query()`` is still False CHAIN_HOLD
    after enqueueing (or the chain is CHAIN_CAP of work: the caller's ``assert not side.query()`` then says so)."""
    import torch
    if _state.chain is None:
        side = side_stream()
        n = 4
        while True:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(side):
                _enqueue_chain(n)
            t1 = time.perf_counter()
            while time.perf_counter() - t1 < CHAIN_HOLD:
                pass
            busy = not side.query()
            side.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if busy or ms > CHAIN_CAP * 1e3:
                break
            n *= 2
        _state.chain, _state.chain_ms = n, ms
        print(f"TWINS | late_queries chain: {n} matmuls of {CHAIN_SIDE}^3, {ms:.1f} ms")
    return _state.chain


def busy_side():
    """-> the side stream, with the chain enqueued on it"""
    import torch
    side = side_stream()
    n = chain_length()
    with torch.cuda.stream(side):
        _enqueue_chain(n)
    return side


def late_queries(Q, decoy):
    """-> (q, side): a device tensor that holds ``decoy`` now and will hold ``Q`` once the side stream has worked through the chain
    enqueued in front of the copy.  The caller makes its call inside ``torch.cuda.stream(side)`` right after ``assert not
    side.query()``: a library that does not wait reads the decoy -- finite queries of the same shape, so it returns their valid
    answers, which differ from Q's: a failed comparison, never a fault."""
    import torch
    Q, decoy = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(decoy, np.float32)
    assert Q.shape == decoy.shape and np.isfinite(decoy).all()
    side = side_stream()
    q = torch.from_numpy(decoy).cuda()
    src = torch.from_numpy(Q).cuda()
    torch.cuda.synchronize()
    busy_side()
    with torch.cuda.stream(side):
        q.copy_(src)
    return q, side


# ---- the table of forms ------------------------------------------------------------------------------------------------------------
@dataclass
class Form:
    name: str                      # the ``*_device`` method
    host: str                      # its host twin
    outs: tuple = ()               # (name, kind, width): width None [B], "k" [B,k], "cap" [B,cap], "kn" [B,k,n], "dim" [B,dim], "m" [B,m]
    optional: tuple = ()           # outputs that may be None
    queries: str = "q"             # "q": f32 [B, dim]; "qm": f32 [B, m, dim]; None: the form takes no query tensor
    call_device: object = None     # (idx, c, q, o) -> None; o: name -> tensor or None
    call_host: object = None       # (idx, c, Q) -> the host twin's tuple
    host_order: tuple = ()         # the names of that tuple's fields
    search: bool = True            # False: listed, but not a search (add_device)


_LISTS = (("ids", "id", "k"), ("scores", "f32", "k"), ("dists", "f32", "k"), ("n_found", "i32", None))
_RANGE = (("ids", "id", "cap"), ("scores", "f32", "cap"), ("dists", "f32", "cap"), ("n_found", "i32", None), ("n_in_range", "id", None))
_ORDER = ("ids", "scores", "dists", "n_found")


def shape_of(width, B, c):
    return {None: lambda: (B,), "k": lambda: (B, c.k), "cap": lambda: (B, c.cap), "kn": lambda: (B, c.k, c.n), "dim": lambda: (B, c.dim),
            "m": lambda: (B, c.m)}[width]()


def query_shape(form, B, c):
    return {"q": (B, c.dim), "qm": (B, c.subs, c.dim), None: None}[form.queries]


FORMS = [
    Form("add_device", "add", search=False),
    Form("search_device", "search", _LISTS, ("dists",),
         call_device=lambda i, c, q, o: i.search_device(q, c.k, o["ids"], o["scores"], o["dists"], o["n_found"]),
         call_host=lambda i, c, Q: i.search(Q, c.k), host_order=_ORDER),
    Form("search_filtered_device", "search_filtered", _LISTS, ("dists",),
         call_device=lambda i, c, q, o: i.search_filtered_device(q, c.k, o["ids"], o["scores"], o["dists"], o["n_found"], ranges=c.ranges),
         call_host=lambda i, c, Q: i.search_filtered(Q, c.k, ranges=c.ranges), host_order=_ORDER),
    Form("search_with_device", "search_with", _LISTS, ("dists",),
         call_device=lambda i, c, q, o: i.search_with_device(c.flt[i], q, c.k, o["ids"], o["scores"], o["dists"], o["n_found"]),
         call_host=lambda i, c, Q: i.search_with(c.flt[i], Q, c.k), host_order=_ORDER),
    Form("search_range_device", "search_range", _RANGE, ("dists",),
         call_device=lambda i, c, q, o: i.search_range_device(q, c.t[:len(q)], c.cap, o["ids"], o["scores"], o["dists"], o["n_found"],
                                                              o["n_in_range"]),
         call_host=lambda i, c, Q: i.search_range(Q, c.t[:len(Q)], c.cap), host_order=_ORDER + ("n_in_range",)),
    Form("search_mmr_device", "search_mmr", _LISTS, ("dists",),
         call_device=lambda i, c, q, o: i.search_mmr_device(q, c.k, o["ids"], o["scores"], o["dists"], o["n_found"], lam=0.4),
         call_host=lambda i, c, Q: i.search_mmr(Q, c.k, lam=0.4), host_order=_ORDER),
    Form("search_fused_device", "search_fused", _LISTS + (("best_sub", "i32", "k"), ("fused", "f64", "k")), ("dists", "best_sub", "fused"),
         queries="qm",
         call_device=lambda i, c, q, o: i.search_fused_device(q, c.k, o["ids"], o["scores"], o["dists"], o["n_found"], o["best_sub"],
                                                              o["fused"], mode="rrf"),
         call_host=lambda i, c, Q: i.search_fused(Q, c.k, mode="rrf"), host_order=_ORDER + ("best_sub", "fused")),
    Form("search_grouped_device", "search_grouped",
         _LISTS + (("keys", "i32", "k"), ("group_rows", "i32", "k"), ("complete", "u8", None)), ("dists", "keys", "group_rows", "complete"),
         call_device=lambda i, c, q, o: i.search_grouped_device(c.grp[i], q, c.k, o["ids"], o["scores"], o["dists"], o["keys"],
                                                                o["group_rows"], o["n_found"], o["complete"]),
         call_host=lambda i, c, Q: i.search_grouped(c.grp[i], Q, c.k),
         host_order=("ids", "scores", "dists", "keys", "group_rows", "n_found", "complete")),
    Form("search_group_rows_device", "search_group_rows",
         (("ids", "id", "kn"), ("scores", "f32", "kn"), ("dists", "f32", "kn"), ("keys", "i32", "k"), ("group_rows", "i32", "k"),
          ("n_members", "i32", "k"), ("members_complete", "u8", "k"), ("n_found", "i32", None), ("complete", "u8", None)),
         ("dists", "keys", "group_rows", "n_members", "members_complete", "complete"),
         call_device=lambda i, c, q, o: i.search_group_rows_device(c.grp[i], q, c.k, c.n, o["ids"], o["scores"], o["dists"], o["keys"],
                                                                   o["group_rows"], o["n_members"], o["members_complete"], o["n_found"],
                                                                   o["complete"]),
         call_host=lambda i, c, Q: i.search_group_rows(c.grp[i], Q, c.k, c.n),
         host_order=("ids", "scores", "dists", "keys", "group_rows", "n_members", "members_complete", "n_found", "complete")),
    Form("search_capped_device", "search_capped", _LISTS + (("keys", "i32", "k"), ("complete", "u8", None)), ("dists", "keys", "complete"),
         call_device=lambda i, c, q, o: i.search_capped_device(c.grp[i], q, c.k, 2, o["ids"], o["scores"], o["dists"], o["keys"],
                                                               o["n_found"], o["complete"]),
         call_host=lambda i, c, Q: i.search_capped(c.grp[i], Q, c.k, 2), host_order=("ids", "scores", "dists", "keys", "n_found", "complete")),
    Form("search_boosted_device", "search_boosted",
         _LISTS + (("priors", "f32", "k"), ("combined", "f64", "k"), ("complete", "u8", None)), ("dists", "priors", "combined", "complete"),
         call_device=lambda i, c, q, o: i.search_boosted_device(c.pri[i], q, c.k, o["ids"], o["scores"], o["dists"], o["priors"],
                                                                o["combined"], o["n_found"], o["complete"], weight=0.25),
         call_host=lambda i, c, Q: i.search_boosted(c.pri[i], Q, c.k, weight=0.25),
         host_order=("ids", "scores", "dists", "priors", "combined", "n_found", "complete")),
    Form("search_by_id_device", "search_by_id", _LISTS, ("dists",), queries=None,
         call_device=lambda i, c, q, o: i.search_by_id_device(c.qids[:c.B], c.k, o["ids"], o["scores"], o["dists"], o["n_found"]),
         call_host=lambda i, c, Q: i.search_by_id(c.qids[:c.B], c.k), host_order=_ORDER),
    Form("search_range_by_id_device", "search_range_by_id", _RANGE, ("dists",), queries=None,
         call_device=lambda i, c, q, o: i.search_range_by_id_device(c.qids[:c.B], c.t[:c.B], c.cap, o["ids"], o["scores"], o["dists"],
                                                                    o["n_found"], o["n_in_range"]),
         call_host=lambda i, c, Q: i.search_range_by_id(c.qids[:c.B], c.t[:c.B], c.cap), host_order=_ORDER + ("n_in_range",)),
    Form("search_like_device", "search_like", _LISTS + (("n_used", "i32", None), ("combined", "f32", "dim")), ("dists", "n_used", "combined"),
         call_device=lambda i, c, q, o: i.search_like_device(c.examples[:c.B], c.k, o["ids"], o["scores"], o["dists"], o["n_found"],
                                                             o["n_used"], o["combined"], weights=c.ex_w, queries=q,
                                                             query_weights=None if q is None else 0.5),
         call_host=lambda i, c, Q: i.search_like(c.examples[:c.B], c.k, weights=c.ex_w, queries=Q, query_weights=None if Q is None else 0.5),
         host_order=_ORDER + ("n_used", "combined")),
    Form("score_ids_device", "score_ids", (("scores", "f32", "m"), ("dists", "f32", "m"), ("order", "i32", "m"), ("n_found", "i32", None)),
         ("dists", "order", "n_found"),
         call_device=lambda i, c, q, o: i.score_ids_device(q, c.cand[:len(q)], o["scores"], o["dists"], o["order"], o["n_found"]),
         call_host=lambda i, c, Q: i.score_ids(Q, c.cand[:len(Q)]), host_order=("scores", "dists", "order", "n_found")),
]
BY_NAME = {f.name: f for f in FORMS}
SEARCH_FORMS = [f for f in FORMS if f.search]


def make_outs(form, B, c, absent=(), device="cuda"):
    """-> (o, checks): the form's outputs as guarded views (None for the optional ones named in ``absent``)"""
    o, checks = {}, {}
    for name, kind, width in form.outs:
        if name in absent:
            assert name in form.optional, name
            o[name] = None
            continue
        o[name], checks[name] = out(kind, shape_of(width, B, c), device)
    return o, checks


def as_host(t, like):
    """a device output as the array its host twin returns: ids and keys unsigned, flags bool"""
    a = t.cpu().numpy()
    like = np.asarray(like)
    if like.dtype == np.bool_:
        assert set(np.unique(a)) <= {0, 1}, f"a flag holds {np.unique(a)}"
        return a.astype(bool)
    if a.dtype != like.dtype:
        assert a.dtype.itemsize == like.dtype.itemsize and a.dtype.kind in "iu" and like.dtype.kind in "iu", (a.dtype, like.dtype)
        a = a.view(like.dtype)
    return a


def same_bits(got, want, what):
    """floats by their bits, everything else by equality; no tolerance"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} != {want.dtype}{want.shape}"
    if want.dtype.kind == "f":
        u = np.uint32 if want.dtype == np.float32 else np.uint64
        got, want = got.view(u), want.view(u)
    np.testing.assert_array_equal(got, want, err_msg=what)


def compare(form, o, host, what):
    """every present device output against the host twin's field of the same name"""
    for name, h in zip(form.host_order, host):
        if o.get(name) is not None:
            same_bits(as_host(o[name], h), h, f"{what}: {name}")


# ---- the corpora of section A (NumPy only: the model test looks at them without a GPU) ------------------------------------------------
N_ROWS = 20500             # 320 tiles of 64 and 20 rows: not a multiple of 64; above kCandCap = kSubsetCap = 16384
ID_OFFSET = 1000
ZERO_ROW, DUP_FIRST, DUP_COUNT = 777, 3000, 40
N_COPIES = 17000           # the rows of the duplicate corpus that are one vector: more than kCandCap


def corpus(dim, seed=72):
    """-> (X [N_ROWS, dim], removed rows): seeded Gaussian rows, a zero row, DUP_COUNT exact copies of row DUP_FIRST, some rows to remove"""
    rng = np.random.default_rng(seed + dim)
    X = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    X[ZERO_ROW] = 0.0
    X[DUP_FIRST + 1:DUP_FIRST + DUP_COUNT] = X[DUP_FIRST]
    gone = np.unique(np.r_[rng.choice(N_ROWS, 200, replace=False), 64:70, DUP_FIRST + 5, N_ROWS - 1])
    return X, gone


def queries(X, B, seed=5):
    """-> [B, dim]: near neighbours of stored rows first, then the duplicated row, the zero query, and Gaussian queries"""
    rng = np.random.default_rng(seed)
    n, dim = X.shape
    Q = rng.standard_normal((B, dim)).astype(np.float32)
    near = min(4, B)
    Q[:near] = X[rng.integers(0, n, near)] + 0.05 * Q[:near]
    if B > 4:
        Q[4] = X[DUP_FIRST] * 2.0
    if B > 5:
        Q[5] = 0.0
    return Q


def copies_corpus(dim=72, seed=9):
    """-> (X, the row that is copied): rows 2000 .. 2000 + N_COPIES are one vector, the rest Gaussian"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    X[2000:2000 + N_COPIES] = X[2000]
    return X, 2000


def topk_from_dists(D, keep, k, off=0):
    """The oracle's top-k from its distances D [B, n] (range_model.oracle_dists) over the rows of ``keep``: ordered by (dist, id), as
    oracle.search orders them -> (ids, scores, dists, n_found) as FlatIndex.search returns them.  tests/test_device_twins_model.py
    holds it to oracle.search."""
    from oracle.search_oracle import score_from_dist
    B = D.shape[0]
    ids = np.zeros((B, k), np.uint64)
    sc = np.zeros((B, k), np.float32)
    di = np.full((B, k), np.inf, np.float32)
    nf = np.zeros(B, np.int32)
    rows = np.flatnonzero(keep)
    for b in range(B):
        r, d = rows, D[b][rows]
        if r.size > k > 0:
            cut = d <= np.partition(d, k - 1)[k - 1]
            r, d = r[cut], d[cut]
        r = r[np.lexsort((r, d))][:k]
        m = r.size
        nf[b] = m
        ids[b, :m] = r.astype(np.uint64) + 1 + off
        di[b, :m] = D[b][r]
        sc[b, :m] = score_from_dist(D[b][r])
    return ids, sc, di, nf


# ---- section A: the cases and the branch each claims --------------------------------------------------------------------------------
# branch -> what mx_index_stats must show after reset_stats() and ONE call of B queries; G: shards that ran (1 on a plain handle)
BRANCHES = {
    "subset": "subset_queries == B and filtered_queries == B; no scan launch, no retry, no fallback",
    "masked": "filtered_queries == B and subset_queries == 0; 1 .. G scan launches (one per shard's first collect pass); no fallback.  "
              "A retry pass is part of this branch: these corpora have too few tiles for a sample pass, so more than kCandCap allowed "
              "rows overflow the first pass and are scanned again under the threshold it found",
    "nothing": "filtered_queries == B and subset_queries == 0; no scan launch (the trivial batch: finish_kernel writes the blanks)",
    "exact": "subset_queries == 0 and no scan launch: run_exact writes the caller's lists (MX_SEARCH_EXACT, or k > 256)",
    "overflow": "at least one scan launch, retry_queries >= 1 and fallback_queries >= 1: the retry pass overflowed again and the EXACT "
                "backstop answered",
    "range-scan": "1 .. G scan launches and no fallback: range_finish_kernel writes the caller's lists and counts",
    "range-overflow": "1 .. G scan launches and fallback_queries >= 1: more than kCandCap candidates, the EXACT range path answered",
    "range-exact": "no scan launch (MX_SEARCH_EXACT): run_exact_range answered every query",
}


def prove(branch, st, B, G=1, filtered=True):
    """assert that the counters of ``st`` (after reset_stats() and one call of B queries) show ``branch``"""
    seen = (f"subset {st.subset_queries} filtered {st.filtered_queries} scans {st.scan_launches} retry {st.retry_queries} "
            f"fallback {st.fallback_queries} queries {st.queries}")
    assert st.queries == B, seen
    if branch.startswith("range"):
        assert st.filtered_queries == 0 and st.subset_queries == 0, seen
    elif filtered:
        assert st.filtered_queries == B, seen
    ok = {
        "subset": st.subset_queries == B and st.scan_launches == 0 and st.retry_queries == 0 and st.fallback_queries == 0,
        "masked": st.subset_queries == 0 and 1 <= st.scan_launches <= G and st.fallback_queries == 0,
        "nothing": st.subset_queries == 0 and st.scan_launches == 0 and st.retry_queries == 0 and st.fallback_queries == 0,
        "exact": st.subset_queries == 0 and st.scan_launches == 0 and st.retry_queries == 0,
        "overflow": st.subset_queries == 0 and st.scan_launches >= 1 and st.retry_queries >= 1 and st.fallback_queries >= 1,
        "range-scan": 1 <= st.scan_launches <= G and st.fallback_queries == 0,
        "range-overflow": 1 <= st.scan_launches <= G and st.fallback_queries >= 1,
        "range-exact": st.scan_launches == 0,
    }[branch]
    assert ok, f"not the {branch} branch ({BRANCHES[branch]}): {seen}"


def filters(off=ID_OFFSET, n=N_ROWS, seed=3):
    """name -> id ranges [m, 2] of section A's allow-sets"""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(n, 5000, replace=False)).astype(np.uint64) + 1 + off
    return {
        "small": np.array([[off + 101, off + 171]], np.uint64),                               # 70 rows in one run
        "scattered": np.stack([ids, ids + 1], 1),                                             # 5000 rows all over the index
        "big": np.array([[off + 10001, off + n - 499], [off + 1, off + 9001]], np.uint64),    # 19000 rows > kSubsetCap, unsorted
        "empty": np.zeros((0, 2), np.uint64),
        "all": np.array([[0, off + n + 1000]], np.uint64),                                    # every id, and ids that name no row
    }


EXACT = 1   # MX_SEARCH_EXACT


@dataclass
class TopKCase:
    name: str
    branch: str
    handle: str = "plain"          # "plain", "sharded" (3 shards of blocks of 64 rows), "compressed" (bf16 corpus), "copies"
    flt: str = "big"
    k: int = 10
    mode: int = 0
    force: object = None           # MEMEX_HIP_DEBUG=filt_subset=<force>
    dists: bool = True
    equals_search: bool = False    # the answer must also be search_device's


TOPK_CASES = [
    TopKCase("70 rows in one run", "subset", flt="small"),
    TopKCase("5000 scattered rows", "subset", flt="scattered", force=1),
    TopKCase("5000 scattered rows on the masked scan", "masked", flt="scattered", force=0),
    TopKCase("19000 rows", "masked"),
    TopKCase("the empty filter", "nothing", flt="empty"),
    TopKCase("every id", "masked", flt="all", equals_search=True),
    TopKCase("MX_SEARCH_EXACT", "exact", mode=EXACT),
    TopKCase("k = 300", "exact", k=300),
    TopKCase("k = 1", "masked", k=1),
    TopKCase("k = 1 on the subset kernel", "subset", flt="small", k=1),
    TopKCase("k = 100 of 70 allowed rows", "subset", flt="small", k=100),
    TopKCase("k = 300 of 70 allowed rows on run_exact", "exact", flt="small", k=300, force=0),
    TopKCase("dists = None", "masked", dists=False),
    TopKCase("dists = None on the subset kernel", "subset", flt="scattered", force=1, dists=False),
    TopKCase("dists = None on run_exact", "exact", k=300, dists=False),
    TopKCase("17000 copies of the query", "overflow", handle="copies", flt="copies"),
    TopKCase("3 shards, 5000 scattered rows", "subset", handle="sharded", flt="scattered", force=1),
    TopKCase("3 shards, 19000 rows", "masked", handle="sharded"),
    TopKCase("3 shards, 70 rows of two shards", "subset", handle="sharded", flt="small"),
    TopKCase("3 shards, the empty filter", "nothing", handle="sharded", flt="empty"),
    TopKCase("3 shards, every id", "masked", handle="sharded", flt="all", equals_search=True),
    TopKCase("3 shards, k = 300", "exact", handle="sharded", k=300),
    TopKCase("3 shards, MX_SEARCH_EXACT", "exact", handle="sharded", mode=EXACT),
    TopKCase("compressed, 19000 rows", "masked", handle="compressed"),
    TopKCase("compressed, 5000 scattered rows", "subset", handle="compressed", flt="scattered", force=1),
    TopKCase("compressed, k = 300", "exact", handle="compressed", k=300),
]


@dataclass
class RangeCase:
    name: str
    branch: str
    handle: str = "plain"
    t: str = "on"                  # how the thresholds are made (test_device_twins_gpu.range_thresholds)
    cap: int = 10
    mode: int = 0
    dists: bool = True


RANGE_CASES = [
    RangeCase("on the score of the cap-th row", "range-scan", t="on"),
    RangeCase("one ulp above the score of the cap-th row", "range-scan", t="above"),
    RangeCase("threshold -1: every live row", "range-overflow", t="all"),
    RangeCase("threshold below -1", "range-overflow", t="below"),
    RangeCase("threshold above 1: nothing", "range-scan", t="none"),
    RangeCase("thresholds that differ inside the batch", "range-scan", t="mixed"),
    RangeCase("cap = 1", "range-scan", t="mixed", cap=1),
    RangeCase("cap = 4096", "range-scan", t="mixed", cap=4096),
    RangeCase("cap = 4096, 3000 rows in range", "range-scan", t="rank3000", cap=4096),
    RangeCase("dists = None", "range-scan", t="mixed", dists=False),
    RangeCase("17000 copies in range", "range-overflow", handle="copies", t="copies"),
    RangeCase("MX_SEARCH_EXACT", "range-exact", t="mixed", mode=EXACT),
    RangeCase("MX_SEARCH_EXACT, cap = 4096", "range-exact", t="rank3000", cap=4096, mode=EXACT),
    RangeCase("3 shards", "range-scan", handle="sharded", t="mixed"),
    RangeCase("3 shards, on and above a score", "range-scan", handle="sharded", t="on"),
    RangeCase("3 shards, every live row", "range-scan", handle="sharded", t="all", cap=4096),   # (under kCandCap rows per shard)
    RangeCase("3 shards, nothing", "range-scan", handle="sharded", t="none"),
    RangeCase("3 shards, MX_SEARCH_EXACT", "range-exact", handle="sharded", t="mixed", mode=EXACT),
    RangeCase("compressed", "range-scan", handle="compressed", t="mixed"),
    RangeCase("compressed, on a score", "range-scan", handle="compressed", t="on"),
]

B_AXIS = (1, 255, 256, 257, 512, 513, 600, 1025)      # either side of a pass (256), of a batch (512), and two batches and a rest
