"""Adversarial queries against the certificate of every filter copy (int8, centred int8, bf16, centred bf16, wide bf16).

The scan drops every row whose filter score is below theta - (its bound), so every answer of the AUTO path rests on
|filter score - cosine| <= qa + qb * e_h  (prep_queries_kernel, shadow8_kernel, shadow_kernel).  Random queries use about a seventh
of that bound (tests/test_filter_copy_model.py), so a bound several times too small passes every parity test that draws its
queries at random.  Here each query is built by the numpy model (tests/filter_copy_model.py) against ONE victim row: it points
along minus the row's quantisation error (and, "sharpened", its own elements sit 0.45 of a step beside their codes on the row's
side), and the range call's threshold is the oracle's score of the victim, bit for bit: the victim is in range with nothing to
spare, and the scan keeps it only if the bound really covers the under-score the query was built to cause.

Asserted per case: the range answer (ids, dist bits, score bits, n_found, n_in_range) and search(Q, 10) equal the oracle's; with
profiling on, max_abs_err <= approx_err_bound; LIVENESS: max_abs_err >= 0.9 * the largest under-score the model predicts for the
batch (the reference is the model, never the library; 10 % covers codes that flip between the model's f64 rotation and the
kernel's f32 one, and for centred copies the f32 sum order of the library's mean); no query took the EXACT path, no range query
a retry.  tests/CERTIFICATE_ADVERSARY.md has the measured shares and the mutants this file kills.

The last two tests are the on-axis query of a centred copy (a usable query whose residual r_q is exactly 0, or ~1e-8 long)."""
import numpy as np
import pytest

import filter_copy_model as M
from conftest import bits
from oracle.search_oracle import score_from_dist
from test_centred_gpu import cone_rows
from test_range_gpu import oracle_dists, range_oracle, same

pytestmark = pytest.mark.gpu

N = 40017            # 626 scan tiles of 64 rows (> 512: top-k calls run the sample and theta launches); N % 64 = 17
CAP = 64


def rotated_one_hot(d, j):
    """the row that is one-hot AFTER the rotation of mx_rotate.h (a plain one-hot row is spread by it and costs its half tile
    nothing): the row that makes an int8 half tile as coarse as it can be, step 1/127"""
    return (M.rotation(M.pad128(d))[j, :d] * 3.0).astype(np.float32)


def variants(cp, v, a):
    q = M.adversary(cp, v, a)
    yield q
    if cp.kind == "i8":
        yield M.sharpen(cp, v, q)
    elif cp.mean is None:
        yield M.sharpen_bf16(cp, v, q)
    if cp.mean is not None:                                   # a query off the cone: |r_q| = 1, the factor of e_h in the bound
        q = M.adversary(cp, v, max(a, 0.5), a_q=0.0)           # (its cosine with the victim is only a |r_c|: a larger a keeps the range small)
        yield q
        if cp.kind == "i8":
            yield M.sharpen(cp, v, q)


def n_variants(kind, centred):
    return (4 if kind == "i8" else 2) if centred else 2


class Case:
    """The corpus, the index operations that put the victims where the placement says, and the model of the half tiles they are in"""

    def __init__(self, kind, centred, d, placement, seed):
        self.kind, self.centred, self.d, self.placement = kind, centred, d, placement
        rng = np.random.default_rng(seed)
        self.rng = rng
        n = N + (3000 if placement == "compact" else 0)
        X = cone_rows(rng, n, d) if centred else rng.standard_normal((n, d), dtype=np.float32)
        self.coarse = []
        if placement == "coarse":
            # a coarse half tile next to an ordinary one in the same 64-row tile, once in each position
            self.coarse = [64 * 100 + 5, 64 * 300 + 32 + 9]
            for i, r in enumerate(self.coarse):
                X[r] = rotated_one_hot(d, 11 + i) if kind == "i8" else 0.0
                if kind != "i8":
                    X[r, 7 + i] = 3.0
        self.X = X
        self.split = 20010 if placement == "split" else None           # 20010 % 32 = 10: the append lands inside a half tile
        self.keep = np.arange(n)
        if placement == "compact":
            dead = np.zeros(n, dtype=bool)
            dead[5000:5100] = True                                       # a run of removed rows, and 2900 scattered ones: N stay
            dead[rng.choice(np.flatnonzero(~dead), 2900, replace=False)] = True
            self.keep = np.flatnonzero(~dead)
        self.rows = X[self.keep]
        # the victim's cosine with its query (centred, in the cone: of the two residual vectors): with the oracle alone at most 64 rows are in range
        self.a = 0.45 if d < 256 or centred else 0.3

    # -- the index ------------------------------------------------------------------------------------------------
    def open(self):
        from memex_amd.index import FlatIndex
        if self.placement == "shards":
            return FlatIndex(self.d, devices=[0, 0], block_rows=1024)
        return FlatIndex(self.d)

    def fill(self, idx):
        X = self.X
        first = X if self.split is None else X[: self.split]
        if self.centred:
            idx.add(first)
            idx.set_filter_copy("bf16" if self.kind == "i8" else False)
            idx.set_filter_copy(self.kind)                               # rebuilt from a populated cone: centred
        else:
            idx.set_filter_copy(self.kind)
            idx.add(first)
        if self.split is not None:
            idx.add(X[self.split:])                                      # the half tile it lands in is requantised as a whole
        if self.placement == "compact":
            gone = np.setdiff1d(np.arange(len(X)), self.keep)
            assert idx.remove(gone.astype(np.uint64) + 1) == gone.size
            idx.compact()                                                # copy rebuilt (a centred one re-centred)
            assert len(idx) == len(self.rows)
        st = idx.stats()
        assert st.filter_centred == (1 if self.centred else 0), st.filter_centred
        assert st.filter_kind == (2 if self.kind == "i8" else 3), st.filter_kind

    # -- the model ------------------------------------------------------------------------------------------------
    def mean(self):
        if not self.centred:
            return None
        if self.placement == "split":
            return M.mean_direction(self.X[: self.split])                # fixed when the copy was rebuilt; appends keep it
        return M.mean_direction(self.rows)

    def half_tiles(self):
        n = len(self.rows)
        last = (n - 1) // 32
        assert 1 <= n % 64 <= 31
        p = self.placement
        if p == "first":
            return [0, 1]
        if p == "last":
            return [last]
        if p == "split":
            return [self.split // 32]
        if p == "coarse":
            return sorted({h for r in self.coarse for h in (r // 32, r // 32 ^ 1)})
        pick = self.rng.choice(np.arange(2, last), 12, replace=False)
        return sorted(set(pick.tolist()) | {0, last})

    def queries(self, count):
        """-> (Q [B, d], victims [B] (rows of self.rows), predicted under-score [B], share of the model's bound [B])"""
        hts = self.half_tiles()
        local = np.concatenate([np.arange(32 * h, min(32 * h + 32, len(self.rows))) for h in hts])
        build = M.int8_copy if self.kind == "i8" else M.bf16_copy
        cp = build(self.rows[local], self.mean())                       # (half tiles in, half tiles out: the model keeps them whole)
        ok = np.array([i for i in range(len(local)) if local[i] not in self.coarse])
        per = n_variants(self.kind, self.centred)
        if self.placement == "coarse":                                   # victims in BOTH halves of each tile
            vs = np.concatenate([M.pick_victims(cp, ok[local[ok] // 32 == h], count // per // len(hts)) for h in hts])
        else:
            vs = M.pick_victims(cp, ok, count // per)
        Q, victims, under, share = [], [], [], []
        for v in vs:
            for q in variants(cp, v, self.a):
                qs = M.query_side(q, self.kind, None if cp.mean is None else cp.mean[: self.d], cp)
                _, u, b = M.predict(cp, qs)
                Q.append(q)
                victims.append(local[v])
                under.append(u[v])
                share.append(u[v] / b[v])
        return np.stack(Q).astype(np.float32), np.array(victims), np.array(under), np.array(share)


def run_case(case, oracle, B=256):
    wide = case.d > 1024
    Q, victims, under, share = case.queries(min(B, 256))
    if B > len(Q):                                                       # a batch of more than a pass: slots >= 256 are exercised
        extra = case.rng.permutation(len(Q))[: B - len(Q)]
        Q, victims, under = np.concatenate([Q, Q[extra]]), np.concatenate([victims, victims[extra]]), np.concatenate([under, under[extra]])
        order = case.rng.permutation(len(Q))                             # adversarial queries on both sides of the pass boundary
        Q, victims, under = Q[order], victims[order], under[order]
    rows = case.rows
    D = oracle_dists(oracle, rows, Q)
    t = score_from_dist(D[np.arange(len(Q)), victims]).astype(np.float32)
    alive = np.ones(len(rows), dtype=bool)
    want = range_oracle(D, alive, t, CAP)
    # conditions of the construction, decided by the oracle alone
    assert (want[4] >= 1).all() and (want[4] <= CAP).all(), (int(want[4].min()), int(want[4].max()))
    assert (under > 0).all()
    what = f"{case.kind}{' centred' if case.centred else ''} d={case.d} {case.placement} B={len(Q)}"
    with case.open() as idx:
        case.fill(idx)
        idx.reset_stats()
        same(idx.search_range(Q, t, CAP), want, what)
        st = idx.stats()
        assert st.scan_launches > 0 and st.fallback_queries == 0 and st.retry_queries == 0, (what, st.scan_launches, st.fallback_queries, st.retry_queries)
        oi, od, os_, onf = oracle.search(rows, Q, 10)
        ids, sc, di, nf = idx.search(Q, 10)
        np.testing.assert_array_equal(ids, oi, err_msg=what)
        np.testing.assert_array_equal(bits(di), bits(od), err_msg=what)
        np.testing.assert_array_equal(bits(sc), bits(os_), err_msg=what)
        np.testing.assert_array_equal(nf, onf, err_msg=what)
        assert idx.stats().fallback_queries == 0, what
        # one pass with profiling on: the error finish_kernel measures on the rows that passed the filter (the victim is in the
        # top 10, so it is one of them) against the batch's bound and against the model's prediction
        pb = 128 if wide else 256
        idx.reset_stats()
        idx.set_profiling(True)
        idx.search(Q[:pb], 10)
        st = idx.stats()
        predicted = float(under[:pb].max())
        print(f"{what}: share of the model's bound {share.min():.3f}-{share.max():.3f}; max_abs_err {st.max_abs_err:.3e}, "
              f"approx_err_bound {st.approx_err_bound:.3e}, predicted {predicted:.3e}, measured / predicted {st.max_abs_err / predicted:.3f}")
        assert st.max_abs_err <= st.approx_err_bound, (what, st.max_abs_err, st.approx_err_bound)
        assert st.max_abs_err >= 0.9 * predicted, (what, st.max_abs_err, predicted)
        assert st.fallback_queries == 0 and st.scan_launches > 0, what


_GRID = [("i8", False, d) for d in (128, 384, 640, 1024)] + [("i8", True, d) for d in (256, 384, 768)] + \
        [("bf16", False, 384), ("bf16", False, 768), ("bf16", True, 384), ("bf16", False, 1536)]


@pytest.mark.parametrize("kind,centred,d", _GRID, ids=[f"{k}{'_centred' if c else ''}_{d}" for k, c, d in _GRID])
def test_adversary_per_kind_and_width(kind, centred, d, oracle, lib_built):
    """Victims in the first tile, in the last (partly filled) half tile and in twelve half tiles between."""
    run_case(Case(kind, centred, d, "spread", 1000 + d + (7 if centred else 0)), oracle)


_PLACES = [("i8", False, p) for p in ("first", "last", "split", "coarse", "compact", "shards")] + \
          [("i8", True, p) for p in ("first", "last", "split", "coarse", "compact")] + \
          [("bf16", False, p) for p in ("last", "split", "coarse", "compact", "shards")] + \
          [("bf16", True, p) for p in ("split", "compact")]


@pytest.mark.parametrize("kind,centred,placement", _PLACES, ids=[f"{k}{'_centred' if c else ''}_{p}" for k, c, p in _PLACES])
def test_adversary_by_victim_placement(kind, centred, placement, oracle, lib_built):
    """first: the first tile.  last: the partly filled half tile at the end (n % 64 = 17).  split: the half tile an add boundary fell
    into, requantised as a whole by the second add (a centred copy keeps the centre of the first 20010 rows).  coarse: a half
    tile whose step one row inflates (int8: a row that is one-hot after the rotation) beside an ordinary half tile of the same
    64-row tile, once as the first and once as the second half, victims in all four: e_h read from the wrong half fails here.
    compact: after remove + compact (copy rebuilt, a centred one re-centred).  shards: two shards on one device."""
    run_case(Case(kind, centred, 384, placement, 2000 + sum(map(ord, placement))), oracle)


@pytest.mark.parametrize("kind,centred", [("i8", False), ("i8", True), ("bf16", False), ("bf16", True)],
                         ids=["i8", "i8_centred", "bf16", "bf16_centred"])
def test_adversary_in_a_batch_of_300(kind, centred, oracle, lib_built):
    """B = 300: two passes (one 512-query pass for the plain int8 copy); qa / qb of the slots from 256 on are what decides"""
    run_case(Case(kind, centred, 384, "spread", 3000), oracle, B=300)


# ---------------------------------------------------------------------------------------------
# the on-axis query of a centred copy
# ---------------------------------------------------------------------------------------------
def axis_corpus(rng, d, noise):
    """250 rows along -e0 and 6 along +e0, random lengths: the unit rows sum to -244 e0 exactly (|sum| / n = 0.95), the stored centre
    is -e0 and every other coordinate of the sum is exactly 0.  noise > 0: small off-axis components (the centre is then only close
    to -e0, and a query along the f64 mean has a residual of ~1e-8: the floor branch of the query's step)."""
    n = 256
    X = np.zeros((n, d), dtype=np.float32)
    X[:, 0] = -rng.uniform(0.5, 2.0, n).astype(np.float32)
    X[rng.choice(n, 6, replace=False), 0] *= -1.0
    if noise:
        X[:, 1:] = (noise * rng.standard_normal((n, d - 1))).astype(np.float32)
    return X


@pytest.mark.parametrize("kind", ["i8", "bf16"])
@pytest.mark.parametrize("noise", [0.0, 1e-3], ids=["exactly_on_axis", "residual_1e-8"])
def test_query_on_the_mean_axis_of_a_centred_copy(kind, noise, oracle, lib_built):
    """A usable query whose residual r_q is 0 (or ~1e-8): before the fix of prep_queries_kernel's step (floored at kMinStep8 only for
    mx > 0) the centred int8 copy gave it the step 0 -- the mark of an unusable query -- and scan8_kernel scored every row 0 against
    cosines of +-1: the certificate was violated (measured on the parent commit: see tests/CERTIFICATE_ADVERSARY.md) and the answer
    came from the EXACT path."""
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(5)
    d = 384
    X = axis_corpus(rng, d, noise)
    if noise:
        q = M.unit_rows(X).sum(axis=0)[:d]
        Q = (q / np.linalg.norm(q)).astype(np.float32)[None, :]
    else:
        Q = np.zeros((1, d), dtype=np.float32)
        Q[0, 0] = 3.0                                                     # along +e0: a_q = -1, r_q = 0 exactly
    with FlatIndex(d) as idx:
        idx.add(X)
        idx.set_filter_copy("bf16" if kind == "i8" else False)
        idx.set_filter_copy(kind)
        st = idx.stats()
        assert st.filter_centred == 1 and st.filter_kind == (2 if kind == "i8" else 3)
        idx.set_profiling(True)
        idx.reset_stats()
        oi, od, os_, onf = oracle.search(X, Q, 3)
        ids, sc, di, nf = idx.search(Q, 3)
        np.testing.assert_array_equal(ids, oi)
        np.testing.assert_array_equal(bits(di), bits(od))
        np.testing.assert_array_equal(bits(sc), bits(os_))
        np.testing.assert_array_equal(nf, onf)
        st = idx.stats()
        print(f"{kind} noise {noise}: max_abs_err {st.max_abs_err:.3e} approx_err_bound {st.approx_err_bound:.3e} fallback {st.fallback_queries}")
        assert st.fallback_queries == 0
        assert st.max_abs_err <= st.approx_err_bound, (st.max_abs_err, st.approx_err_bound)
        D = oracle_dists(oracle, X, Q)
        t = np.full(1, 0.5, np.float32)
        same(idx.search_range(Q, t, CAP), range_oracle(D, np.ones(len(X), dtype=bool), t, CAP), f"{kind} on-axis range")
        assert idx.stats().fallback_queries == 0
