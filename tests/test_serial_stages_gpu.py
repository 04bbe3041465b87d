"""Two short serial stages of finish_kernel in their two forms (MEMEX_HIP_DEBUG=serial=N, read when an index is created;
memex_amd/csrc/mx_debug.h): the prefiltered select of the first threshold (the k-th best lower bound among all of a query's
candidates) and two lanes per staged row in stage 3.  Neither moves a threshold, a bound or a candidate set, so an index created
with serial=0 (the older forms) and one with the default must give the same ids, dists, scores and n_found bit for bit AND the same
stats().candidates (the rows finish_kernel rescored in f32: equal counts mean the first select returned the same key).  One batch
per case is also held against MX_SEARCH_EXACT.

block_kth_largest_pre takes k <= 32 (kPreMaxK) and at most 512 keys at or above its pivot (kRankCap); what follows it depends on
how many rows survive (up to 64: a wave ranks them; more: radix passes), and stage 3 stages up to 32 rows.  Every case says from
candidates / queries which of these it is in, so that none passes without having run what it names; no case may need the retry
pass or the EXACT fallback (the inputs are confirmed: both counters stay 0).

Shapes: plain int8 copy, 128 and 384 dims.  Four scan tiles per CU and 130 queries run the sample and theta launches on the int8
scan's two-workgroup form, two tiles per CU and 40 queries on the 8-wave form (the CU count is read from the device).
"""
import functools

import numpy as np
import pytest

from conftest import bits  # noqa: E402

gpu = pytest.mark.gpu

KS = (1, 10, 32, 33, 256)  # block_kth_largest_pre's k limit sits between 32 and 33
VARIANTS = {"new": None, "old": "serial=0"}


def _same(a, b, msg=""):
    for x, y, name in zip(a, b, ("ids", "scores", "dists", "n_found")):
        x, y = (bits(x), bits(y)) if name in ("scores", "dists") else (x, y)
        np.testing.assert_array_equal(x, y, err_msg=f"{name} {msg}")


@functools.lru_cache(maxsize=None)
def _n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rows(tiles_per_cu):
    """Just over tiles_per_cu scan tiles of 64 rows per CU, not a multiple of the tile."""
    return 64 * (tiles_per_cu * min(_n_cu(), 256) + 64) + 37


def _gauss(rng, n, d):
    return rng.standard_normal((n, d), dtype=np.float32)


def _cone(rng, n, d, s):
    """Rows around one axis, axis + s g / sqrt(d): cosines to a query of the same kind spread by about s^2 / (1 + s^2) / sqrt(d)."""
    axis = np.random.default_rng(d).standard_normal(d)
    axis /= np.linalg.norm(axis)
    return (axis + rng.standard_normal((n, d)) * (s / np.sqrt(d))).astype(np.float32)


# name -> (tiles per CU, dims, batch, cone width or None, the values of k, {k: band of candidates / queries})
# cone widths: cosines spread by 0.018 (128 dims: 0.5; 384 dims: 0.75), and a tighter cone that brings thousands of keys to the
# first select (measured on an MI355X: 35 and 67 candidates per query on the Gaussian rows at k = 10, 326 .. 335 in the cones, 1900
# and 2800 in the tight ones, whose k = 1 and k = 256 need the retry pass and are left out)
WAVE, RANKED, RADIX = (0, 64), (64, 512), (1024, 16384)  # survivors: a wave ranks them / some hundreds / thousands
CORPORA = {
    "gauss_4x128": (4, 128, 130, None, KS, {10: WAVE, 32: RANKED}),
    "gauss_4x384": (4, 384, 130, None, KS, {1: WAVE, 32: RANKED}),
    "gauss_2x384": (2, 384, 40, None, KS, {1: WAVE, 32: RANKED}),
    "cone_4x128": (4, 128, 130, 0.5, KS, {10: RANKED, 256: RADIX}),
    "cone_4x384": (4, 384, 130, 0.75, KS, {10: RANKED, 256: RADIX}),
    "cone_2x128": (2, 128, 40, 0.5, KS, {10: RANKED, 256: RADIX}),
    "tight_4x128": (4, 128, 130, 0.35, (10, 32, 33), {10: RADIX, 32: RADIX}),
    "tight_4x384": (4, 384, 130, 0.45, (10, 32, 33), {10: RADIX, 32: RADIX}),
}


@functools.lru_cache(maxsize=None)
def _corpus(name):
    tiles, d, B, s = CORPORA[name][:4]
    rng = np.random.default_rng(sum(name.encode()))
    n = _rows(tiles)
    if s is None:
        X, Q = _gauss(rng, n, d), _gauss(rng, B, d)
        Q[:8] = X[rng.integers(0, n, 8)] + 0.05 * _gauss(rng, 8, d)  # near neighbours
    else:
        X, Q = _cone(rng, n, d, s), _cone(rng, B, d, s)
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


def _open(X, debug, pin="i8"):
    """An index over X created under MEMEX_HIP_DEBUG=debug, with the plain int8 copy pinned before the first row (a copy built
    with the rows is never centred, and a pinned one is neither rebuilt nor demoted)."""
    from memex_amd.index import FlatIndex
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("MEMEX_HIP_DEBUG", raising=False)
        mp.delenv("MEMEX_HIP_EXACT_THETA", raising=False)
        if debug:
            mp.setenv("MEMEX_HIP_DEBUG", debug)
        idx = FlatIndex(X.shape[1])
    idx.set_filter_copy(pin)
    idx.add(X)
    assert idx.stats().filter_centred == 0
    return idx


class _Pair:
    """The same rows in an index of either form."""

    def __init__(self, X, pin="i8"):
        self.idx = {v: _open(X, dbg, pin) for v, dbg in VARIANTS.items()}

    def close(self):
        for idx in self.idx.values():
            idx.close()

    def both(self, Q, k, label, clean=True):
        """Search both forms; the outputs and the candidate counts must agree.  -> (outputs, candidates / queries)"""
        out, st = {}, {}
        for v, idx in self.idx.items():
            idx.reset_stats()
            out[v] = idx.search(Q, k)
            st[v] = idx.stats()
        per_query = st["new"].candidates / max(1, st["new"].queries)
        print(f"{label} k={k}: candidates/query {per_query:.1f} (old {st['old'].candidates / max(1, st['old'].queries):.1f}) "
              f"retry {st['new'].retry_queries} fallback {st['new'].fallback_queries}")
        _same(out["new"], out["old"], f"{label} k={k}: serial default against serial=0")
        assert st["new"].candidates == st["old"].candidates, (label, k)
        for v in VARIANTS:
            assert st[v].scan_launches > 0, (label, k, v)  # the scan pipeline, not the EXACT path
            if clean:
                assert st[v].retry_queries == 0 and st[v].fallback_queries == 0, (label, k, v)
        return out["new"], per_query

    def one(self, Q, q, k, label):
        """Query q alone, both forms -> (outputs, the query's own candidate count m1: the rows that survived its first select)"""
        out, per_query = self.both(Q[q:q + 1], k, f"{label} query {q}")
        return out, int(round(per_query))

    def exact(self, Q, k):
        from memex_amd.index import SEARCH_AUTO, SEARCH_EXACT
        idx = self.idx["old"]
        idx.set_search_mode(SEARCH_EXACT)
        try:
            return idx.search(Q, k)
        finally:
            idx.set_search_mode(SEARCH_AUTO)


_pairs = {}


@pytest.fixture(scope="module")
def pairs(lib_built):
    """corpus name -> _Pair, opened on first use and closed with the module"""
    def get(name):
        if name not in _pairs:
            _pairs[name] = _Pair(_corpus(name)[0])
        return _pairs[name]
    yield get
    for p in _pairs.values():
        p.close()
    _pairs.clear()


@gpu
@pytest.mark.parametrize("name", list(CORPORA))
def test_selects_agree_in_every_band(name, pairs):
    """Gaussian rows leave a few dozen survivors of the first select per query on average, the cone a few hundred, the tighter cone
    thousands; k = 33 and 256 keep the first select on the radix passes, k <= 32 prefilters it (or falls back, where more than 512
    keys reach the pivot: test_duplicates_... forces that, these corpora do not show which queries do)."""
    Q = _corpus(name)[1]
    ks, bands = CORPORA[name][4:]
    pair = pairs(name)
    for k in ks:
        out, per_query = pair.both(Q, k, name)
        if k in bands:
            lo, hi = bands[k]
            assert lo < per_query <= hi, f"{name} k={k}: {per_query:.1f} candidates per query are outside ({lo}, {hi}]"
        if k == 10:
            _same(out, pair.exact(Q, k), f"{name} k={k}: against the EXACT path")


def _planted(d, seed, tiles=4, B=130):
    rng = np.random.default_rng(seed)
    X, Q = _gauss(rng, _rows(tiles), d), _gauss(rng, B, d)
    return rng, X, Q


@gpu
@pytest.mark.parametrize("d", [128, 384])
def test_duplicates_send_the_prefilter_back_to_the_radix_passes(d, lib_built):
    """2112 and 1536 exact copies of a near neighbour of queries 3 and 7, in whole 64-row tiles (so that every copy gets the same
    filter score): far more than 512 keys tie at or above any pivot, and the prefiltered select hands over to the radix passes.
    Ties are broken by id; 2112 keys also take finish's 64-bit select."""
    from test_search_gpu import _rows_with_cosine
    rng, X, Q = _planted(d, 11)
    X[64 * 100: 64 * 100 + 2112] = _rows_with_cosine(rng, Q[3], [0.97])[0] * 1.5
    X[64 * 300: 64 * 300 + 1536] = _rows_with_cosine(rng, Q[7], [0.95])[0]
    pair = _Pair(X)
    try:
        for k in (1, 10, 32, 33):
            out, per_query = pair.both(Q, k, f"duplicates d={d}")
            assert per_query * Q.shape[0] >= 2112 + 1536
            if k == 10:
                _same(out, pair.exact(Q, k), "duplicates: against the EXACT path")
                assert out[0][3].tolist() == list(range(6401, 6411)) and out[0][7].tolist() == list(range(19201, 19211))
    finally:
        pair.close()


@gpu
@pytest.mark.parametrize("d", [128, 384])
def test_ties_across_the_kth_place(d, lib_built):
    """Exact copies straddle the k-th place, inside one 32-row group (equal filter scores, equal f32 scores, equal dists): the
    selects return the tied key whichever way they count, and the order is the ids'.  Query 2: three copies at k = 2; queries 5
    and 9: 12 copies behind 4 better rows at k = 10, on Gaussian rows and with a crowd of 300 rows right below the tie."""
    from test_search_gpu import _rows_with_cosine
    rng, X, Q = _planted(d, 12)
    X[64 * 50: 64 * 50 + 3] = _rows_with_cosine(rng, Q[2], [0.9])[0]
    for q, t in ((5, 70), (9, 90)):
        X[64 * t + 32: 64 * t + 44] = _rows_with_cosine(rng, Q[q], [0.93])[0]
        X[64 * (t + 2): 64 * (t + 2) + 4] = _rows_with_cosine(rng, Q[q], [0.99, 0.98, 0.97, 0.96])
    far = rng.permutation(np.arange(64 * 400, X.shape[0]))[:300]
    X[far] = _rows_with_cosine(rng, Q[9], np.linspace(0.9299, 0.91, 300))  # a crowd right below the tie
    pair = _Pair(X)
    try:
        for k in (2, 10, 13):
            out, _ = pair.both(Q, k, f"ties d={d}")
            _same(out, pair.exact(Q, k), f"ties k={k}: against the EXACT path")
        out, _ = pair.both(Q, 10, f"ties d={d}")
        assert out[0][2][:3].tolist() == [3201, 3202, 3203]
        for q, t in ((5, 70), (9, 90)):
            assert out[0][q][4:].tolist() == list(range(64 * t + 33, 64 * t + 39))
        # each planted query alone: its own survivors of the first select.  The three copies and nothing else; the 16 planted rows
        # and nothing else (a wave ranks them); the 16 and much of the crowd (radix passes on the second select)
        for q, k, lo, hi in ((2, 2, 3, 3), (5, 10, 16, 16), (9, 10, 65, 16 + 300)):
            one, m1 = pair.one(Q, q, k, f"ties d={d}")
            assert lo <= m1 <= hi, (q, k, m1)
            _same(one, tuple(a[q:q + 1] for a in pair.exact(Q, k)), f"ties query {q} alone: against the EXACT path")
    finally:
        pair.close()


STAGED = {0: 1, 1: 10, 2: 21, 3: 32}  # query -> rows planted near it, far above every other row


@gpu
@pytest.mark.parametrize("d", [3, 128, 384, 1020, 1536])
def test_stage3_staged_rows(d, lib_built):
    """Stage 3 with its rows staged in LDS, where each row now has two lanes: every row width class (one 128-dim slot, three, the
    widest that still stages 32 rows, and 1536 dims, where 21 fit).  int8 copy up to 1024 dims, bf16 above.  12k rows: no sample
    pass, every row is a candidate of every query and all of them fit finish_kernel's list, so the first select runs on 12k keys,
    about 600 of which reach the pivot: queries fall on either side of the prefilter's 512.
    Queries 0 .. 3 have 1, 10, 21 and 32 rows planted at cosines no other row comes near; searched alone with k = that number,
    exactly those rows survive the first select (candidates == k), so at most that many reach stage 3: staged up to the stage's
    capacity (32 rows; 21 at 1536 dims, which the 21-row query fills exactly), read from global memory beyond it (32 rows at 1536
    dims, and k = 22 on the 21-row query, which stage 3 cannot get fewer than 22 rows for).  Three dims: the other rows lie in
    the half space the four queries point away from."""
    from test_search_gpu import _rows_with_cosine
    rng = np.random.default_rng(d)
    X, Q = _gauss(rng, 12_011, d), _gauss(rng, 33, d)
    Q[4:8] = X[rng.integers(0, X.shape[0], 4)] + 0.05 * _gauss(rng, 4, d)
    hi_cos, lo_cos = (0.99, 0.9)
    if d == 3:
        X[:, 0] = -np.abs(X[:, 0])
        Q[:4] = np.array([[1, .5, .5], [1, -.5, .5], [1, .5, -.5], [1, -.5, -.5]], dtype=np.float32) * 2.0
        hi_cos, lo_cos = (0.9995, 0.995)  # within 6 degrees of a query; the queries are 48 degrees and more apart
    planted = {}
    for q, n in STAGED.items():
        planted[q] = 1000 * (q + 1) + 37 * np.arange(n)
        X[planted[q]] = _rows_with_cosine(rng, Q[q], np.linspace(hi_cos, lo_cos, n)) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    stage_rows = 32 if d <= 1020 else 21
    pair = _Pair(X, pin="i8" if d <= 1024 else "bf16")
    try:
        for k in (1, 10, 21, 22, 32):
            out, _ = pair.both(Q, k, f"stage 3 d={d}")
            if k in (10, 21):
                _same(out, pair.exact(Q, k), f"stage 3 d={d} k={k}: against the EXACT path")
        for q, n in STAGED.items():
            out, m1 = pair.one(Q, q, n, f"stage 3 d={d}")
            assert m1 == n, f"query {q}: {m1} survivors of the first select, {n} planted"  # n <= stage_rows: staged, else global
            assert sorted(out[0][0].tolist()) == (planted[q] + 1).tolist()
            _same(out, pair.exact(Q[q:q + 1], n), f"stage 3 d={d} query {q} alone: against the EXACT path")
        assert STAGED[2] == 21 and (stage_rows == 21) == (STAGED[3] > stage_rows)
        out, m1 = pair.one(Q, 2, 22, f"stage 3 d={d}")  # one row more than planted: 22 rows or more reach stage 3
        assert m1 >= 22
        _same(out, pair.exact(Q[2:3], 22), f"stage 3 d={d} query 2, k = 22: against the EXACT path")
    finally:
        pair.close()


@gpu
def test_stage3_global_rows_are_left_alone(lib_built):
    """More than 32 survivors: nine rows better than 26 exact copies that hold the 10th place, 35 rows within 2 e2 of the threshold
    and so in stage 3, which reads them from global memory, one thread per row as before."""
    from test_search_gpu import _rows_with_cosine
    rng, X, Q = _planted(384, 13)
    X[64 * 60: 64 * 60 + 26] = _rows_with_cosine(rng, Q[4], [0.9])[0]
    X[64 * 62: 64 * 62 + 9] = _rows_with_cosine(rng, Q[4], np.linspace(0.99, 0.91, 9))
    pair = _Pair(X)
    try:
        out, _ = pair.both(Q, 10, "stage 3 global")
        _same(out, pair.exact(Q, 10), "stage 3 global: against the EXACT path")
        assert out[0][4][9] == 64 * 60 + 1
        one, m1 = pair.one(Q, 4, 10, "stage 3 global")  # the query alone: the 35 planted rows survive the first select, and the
        assert 35 <= m1 <= 64                           # second keeps them all (the 10th best score is the copies')
        _same(one, tuple(a[4:5] for a in out), "stage 3 global, query 4 alone against the batch")
    finally:
        pair.close()


@gpu
def test_the_switch_reaches_the_finish_launch(capfd, lib_built):
    """Every comparison above would hold trivially if serial=0 never arrived: with records=1 a batch prints the value its finish
    launch was given."""
    rng = np.random.default_rng(5)
    X, Q = _gauss(rng, 12_011, 128), _gauss(rng, 8, 128)
    for debug, want in (("records=1", 3), ("serial=0,records=1", 0), ("records=1,serial=2", 2), ("serial=1,records=1", 1)):
        idx = _open(X, debug)
        try:
            capfd.readouterr()
            idx.search(Q, 10)
            err = capfd.readouterr().err
        finally:
            idx.close()
        assert f" serial {want}\n" in err, (debug, err)
