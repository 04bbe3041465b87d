"""What a script of tests/cpp/test_store_features.cpp must print, restated in NumPy over the oracle and the feature models -- TEST
INFRASTRUCTURE, not product code.  No library call is made: the state is (X, names, alive) and every answer is a statement over it.

Rows are numbered r = 1 .. n in insertion order.  ``S(q, allowed)`` is the oracle's full ranking of the live allowed rows, ordered by
(dist bits, id): the oracle's DistCosine over every allowed row (``COracle.all_dists``, the C function ``COracle.search`` runs; a test
holds the two to each other) and ``score_from_dist``.

    search / search_within / search_in   the first ``limit`` entries of S, as _ids (an _id with several rows may repeat); ``within``
                                         and a filter allow exactly the rows stored under the named _ids; COUNT = (rows in the set,
                                         live rows among them)
    search_above                         the entries of S whose score is >= the threshold as floats, the first ``limit`` of them
    search_diverse                       mmr_model, fetch 0 = min(max(4 * limit, 32), 1024)
    search_fused                         fused_model with rrf_c = 60; fetch 0 = limit (MAX) or min(max(4 * limit, 32), 256) (RRF); no
                                         weights = all ones
    more_like(_id, limit)                every live row under _id is a query; S without the rows under _id; the union by best dist,
                                         ordered (dist, id), the first ``limit``.  limit + rows under _id > 4095: Unsupported
    search_like                          like_model with weights beta / n_pos_rows and -gamma / n_neg_rows AS F32 DIVISIONS OF THE F32
                                         VALUES of beta and gamma (the C ABI takes float weights); more than 16 rows: invalid_argument
    rerank                               every row under the named _ids, once; S over them; each _id once, at its best row; cut to
                                         ``limit`` (0: all)
    find_duplicates(min_score, per_row)  row i lists the first per_row entries of S(row i, the other live rows) that reach min_score;
                                         a pair is reported when either end lists the other, in (smaller id, larger id) order; so a
                                         pair is left out only if BOTH ends have more than per_row rows in range.  truncated: the
                                         _ids of the rows with more than per_row in range, in id order
    remove / compact / reload            ``alive`` is updated; compaction renumbers; a filter made before a COMPACT that dropped a
                                         row, a RELOAD, a DELETE_ALL or a call through get_vector_storage (it attaches by a load)
                                         answers VectorStoreError SearchError
    errors                               a query of another dimension: SearchError; a limit / fetch the library does not take
                                         (range limit > 4096, MMR fetch > 1024, fused fetch > 256): Unsupported
"""
import numpy as np

from fused_model import fused_model
from like_model import drop_examples, like_combined
from mmr_model import mmr_model
from oracle.search_oracle import score_from_dist

SEARCH_ERROR = "VectorStoreError SearchError"
UNSUPPORTED = "VectorStoreError Unsupported"
INVALID = "std::invalid_argument -"


class ModelError(Exception):
    pass


def f32_of(tok):
    return np.array([int(tok, 16)], dtype=np.uint32).view(np.float32)[0]


def bits_of(x):
    return "%08x" % int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def rocchio_weights(beta, gamma, n_pos, n_neg):
    """the contract of search_like's weights: f32 divisions of the f32 parameters"""
    pos = [np.float32(beta) / np.float32(n_pos)] * n_pos if n_pos else []
    neg = [-np.float32(gamma) / np.float32(n_neg)] * n_neg if n_neg else []
    return np.array(pos + neg, dtype=np.float32)


def split_like(args):
    """LIKE's arguments -> (limit, vec token, (alpha, beta, gamma) f32, positive names, negative names)"""
    limit, vec = int(args[0]), args[1]
    if args[2] == "default":
        par, i = (np.float32(1.0), np.float32(0.75), np.float32(0.15)), 3
    else:
        par, i = tuple(f32_of(t) for t in args[2:5]), 5
    rest = args[i + 1:]
    cut = rest.index("-")
    return limit, vec, par, rest[:cut], rest[cut + 1:]


class StoreModel:
    def __init__(self, oracle, pool):
        self.oracle = oracle
        self.pool = np.ascontiguousarray(pool, dtype=np.float32)
        self.dim = self.pool.shape[1]
        self.X = np.zeros((0, self.dim), np.float32)
        self.names = []
        self.alive = np.zeros(0, bool)
        self.filters = {}                                     # name -> [set of 0-based rows, stale]
        self.records = []                                     # one dict per command: what the conditions of the tests look at

    # -- state ---------------------------------------------------------------------------------------------------------------------
    def vec(self, tok):
        if tok == "-":
            return None
        idx, _, n = tok.partition("/")
        v = self.pool[int(idx)]
        return v[:int(n)] if n else v

    def rows_under(self, ids, once=True):
        """0-based rows stored under the _ids, in the order named (an _id named twice counts once unless once=False)"""
        by = {}
        for r, nm in enumerate(self.names):
            by.setdefault(nm, []).append(r)
        ids = list(dict.fromkeys(ids)) if once else list(ids)
        return [r for nm in ids for r in by.get(nm, ())]

    def live(self):
        return np.flatnonzero(self.alive)

    def S(self, q, allowed):
        """-> (0-based rows, dists, scores) of the live rows among ``allowed`` in (dist, id) order"""
        rows = np.array(sorted(r for r in set(int(a) for a in allowed) if self.alive[r]), dtype=np.int64)
        if rows.size == 0:
            return rows, np.zeros(0, np.float32), np.zeros(0, np.float32)
        d = self.oracle.all_dists(self.X[rows], np.ascontiguousarray(q, dtype=np.float32))
        order = np.lexsort((rows, d))
        return rows[order], d[order], score_from_dist(d[order])

    def check_dim(self, q):
        if q is None or len(q) != self.dim:
            raise ModelError(SEARCH_ERROR)

    def listed(self, rows, dists, scores, limit=None):
        if limit is not None:
            rows, dists, scores = rows[:limit], dists[:limit], scores[:limit]
        self.rec["rows"] = [int(r) for r in rows]
        self.rec["dists"] = [bits_of(d) for d in dists]
        return [(self.names[int(r)], bits_of(s)) for r, s in zip(rows, scores)]

    def flt(self, name):
        f = self.filters[name]
        if f[1]:
            raise ModelError(SEARCH_ERROR)
        return f

    def stale_all(self):
        for f in self.filters.values():
            f[1] = True

    # -- the methods ---------------------------------------------------------------------------------------------------------------
    def do_SEARCH(self, a):
        q, limit = self.vec(a[0]), int(a[1])
        if limit == 0:
            return []
        self.check_dim(q)
        return self.listed(*self.S(q, self.live()), limit)

    def do_WITHIN(self, a):
        q, limit = self.vec(a[0]), int(a[1])
        if limit == 0 or not self.names:
            return []
        self.check_dim(q)
        allowed = self.rows_under(a[2:])
        self.rec["allowed"] = sorted(allowed)
        return self.listed(*self.S(q, allowed), limit)

    def do_FILTER(self, a):
        self.filters[a[0]] = [set(self.rows_under(a[1:])), False]
        return []

    def do_ALLOW(self, a):
        self.flt(a[0])[0].update(self.rows_under(a[1:]))
        return []

    def do_DENY(self, a):
        self.flt(a[0])[0].difference_update(self.rows_under(a[1:]))
        return []

    def do_COUNT(self, a):
        rows = self.flt(a[0])[0]
        return [("rows", "%08x" % len(rows)), ("live", "%08x" % sum(bool(self.alive[r]) for r in rows))]

    def do_IN(self, a):
        q, limit = self.vec(a[0]), int(a[1])
        if limit == 0:
            return []
        self.check_dim(q)
        return self.listed(*self.S(q, self.flt(a[2])[0]), limit)

    def do_ABOVE(self, a):
        q, thr, limit = self.vec(a[0]), f32_of(a[1]), int(a[2])
        if limit == 0:
            return []
        self.check_dim(q)
        if limit > 4096:
            raise ModelError(UNSUPPORTED)
        rows, d, s = self.S(q, self.live())
        keep = s >= thr
        return self.listed(rows[keep], d[keep], s[keep], limit)

    def do_DIVERSE(self, a):
        q, limit, fetch, lam = self.vec(a[0]), int(a[1]), int(a[2]), f32_of(a[3])
        if limit == 0:
            return []
        self.check_dim(q)
        fetch = fetch or min(max(4 * limit, 32), 1024)
        if fetch < limit:
            raise ModelError(SEARCH_ERROR)
        if fetch > 1024:
            raise ModelError(UNSUPPORTED)
        ids, sc, di, nf = mmr_model(self.oracle, self.X, q, limit, fetch, lam, alive=self.alive)
        n = int(nf[0])
        return self.listed(ids[0, :n].astype(np.int64) - 1, di[0, :n], sc[0, :n])

    def do_FUSED(self, a):
        mode, limit, fetch, m = a[0], int(a[1]), int(a[2]), int(a[3])
        vecs = [self.vec(t) for t in a[4:4 + m]]
        w = [f32_of(t) for t in a[4 + m:]]
        if limit == 0 or not vecs:
            return []
        for v in vecs:
            self.check_dim(v)
        fetch = fetch or (limit if mode == "max" else min(max(4 * limit, 32), 256))
        if fetch < limit:
            raise ModelError(SEARCH_ERROR)
        if m > 16 or fetch > 256:
            raise ModelError(UNSUPPORTED)
        ids, sc, di, nf, _, _ = fused_model(self.oracle, self.X, np.stack(vecs)[None], limit, mode, fetch,
                                            np.array(w, np.float32)[None] if w else None, 60.0, alive=self.alive)
        n = int(nf[0])
        return self.listed(ids[0, :n].astype(np.int64) - 1, di[0, :n], sc[0, :n])

    def do_MORE(self, a):
        limit = int(a[1])
        mine = self.rows_under([a[0]])
        if limit == 0 or not mine:
            return []
        if limit + len(mine) > 4095:
            raise ModelError(UNSUPPORTED)
        others = np.array(sorted(set(int(r) for r in self.live()) - set(mine)), dtype=np.int64)
        queries = [r for r in mine if self.alive[r]]
        if not queries or others.size == 0:
            return []
        best = np.min([self.oracle.all_dists(self.X[others], self.X[r]) for r in queries], axis=0)   # every S is over all of `others`
        order = np.lexsort((others, best))[:limit]
        return self.listed(others[order], best[order], score_from_dist(best[order]))

    def do_LIKE(self, a):
        limit, vtok, (alpha, beta, gamma), pos_names, neg_names = split_like(a)
        if limit == 0 or not self.names:
            return []
        pos, neg = self.rows_under(pos_names, once=False), self.rows_under(neg_names, once=False)
        if len(pos) + len(neg) > 16:
            raise ModelError(INVALID)
        q = self.vec(vtok)
        if q is not None:
            self.check_dim(q)
        if not pos and not neg and q is None:
            return []
        if pos or neg:
            ex = np.array([r + 1 for r in pos + neg], dtype=np.uint64)[None]
            w = rocchio_weights(beta, gamma, len(pos), len(neg))[None]
        else:
            ex, w = np.zeros((1, 1), np.uint64), np.zeros((1, 1), np.float32)
        self.rec["weights"] = [bits_of(x) for x in w[0]]
        self.rec["n_neg"] = len(neg)
        if limit + ex.shape[1] > 4096:
            raise ModelError(UNSUPPORTED)
        rows_of = lambda i: self.X[i - 1] if 1 <= i <= len(self.names) and self.alive[i - 1] else None  # noqa: E731
        comb, used, _ = like_combined(rows_of, ex, w, None if q is None else q[None], None if q is None else np.array([alpha], np.float32),
                                      dim=self.dim)
        rows, d, s = self.S(comb[0], self.live())
        lists = ((rows + 1).astype(np.uint64)[None], s[None], d[None], np.array([len(rows)], np.int32))
        ids, sc, di, nf = drop_examples(lists, ex, used, comb, limit, True)
        n = int(nf[0])
        return self.listed(ids[0, :n].astype(np.int64) - 1, di[0, :n], sc[0, :n])

    def do_VS_LIKE(self, a):
        self.stale_all()                                      # get_vector_storage attaches by a load
        return self.do_LIKE(a)

    def do_RERANK(self, a):
        q, limit = self.vec(a[0]), int(a[1])
        rows = self.rows_under(a[2:])
        self.rec["candidates"] = len(rows)
        if not rows:
            return []
        self.check_dim(q)
        out, seen = [], set()
        for r, d, s in zip(*self.S(q, rows)):
            if self.names[int(r)] in seen:
                continue
            seen.add(self.names[int(r)])
            out.append((int(r), d, s))
            if limit and len(out) >= limit:
                break
        return self.listed([o[0] for o in out], [o[1] for o in out], [o[2] for o in out])

    def do_VS_RERANK(self, a):
        self.stale_all()
        return self.do_RERANK(a)

    def do_DUPS(self, a):
        thr, per_row = f32_of(a[0]), int(a[1])
        live = self.live()
        pairs, full, cut = {}, set(), []
        Xl = self.X[live]
        for i in live:
            d = self.oracle.all_dists(Xl, self.X[i])
            s = score_from_dist(d)
            ok = (s >= thr) & (live != i)
            rows, dd, ss = live[ok], d[ok], s[ok]
            order = np.lexsort((rows, dd))
            if len(rows) > per_row:
                cut.append(int(i))
            for n, j in enumerate(order):
                key = (min(int(i), int(rows[j])), max(int(i), int(rows[j])))
                full.add(key)
                if n < per_row:
                    pairs[key] = ss[j]
        self.rec["pairs_lost"] = len(full) - len(pairs)
        self.rec["truncated"] = len(cut)
        self.rec["lost_with_a_listed_end"] = sum(1 for p in full - set(pairs) if p[0] not in cut or p[1] not in cut)
        return ([(self.names[a], self.names[b], bits_of(s)) for (a, b), s in sorted(pairs.items())], [self.names[r] for r in cut])

    def do_INSERT(self, a):
        ids, vecs = zip(*[(t.rpartition(":")[0], self.vec(t.rpartition(":")[2])) for t in a])
        self.X = np.ascontiguousarray(np.concatenate([self.X, np.stack(vecs)]))
        self.names += list(ids)
        self.alive = np.concatenate([self.alive, np.ones(len(ids), bool)])
        return []

    def do_REMOVE(self, a):
        rows = self.rows_under(a)
        n = int(sum(bool(self.alive[r]) for r in rows))
        self.alive[rows] = False
        return [("removed", "%08x" % n)]

    def do_COMPACT(self, a):
        if not self.names:
            return [("kept", "%08x" % 0)]
        if not self.alive.all():
            keep = self.live()
            self.X, self.names, self.alive = np.ascontiguousarray(self.X[keep]), [self.names[r] for r in keep], np.ones(len(keep), bool)
            self.stale_all()
        return [("kept", "%08x" % len(self.names))]

    def do_RELOAD(self, a):
        self.stale_all()
        return []

    def do_DELETE_ALL(self, a):
        self.X, self.names, self.alive = np.zeros((0, self.dim), np.float32), [], np.zeros(0, bool)
        self.stale_all()
        return []

    def do_OPEN(self, a):
        return []

    do_SAVE = do_OPEN

    # -- the script ----------------------------------------------------------------------------------------------------------------
    def replay(self, script):
        """script: the text of a script file -> the lines the driver must print"""
        out = []
        for no, ln in enumerate(script.splitlines(), 1):
            tok = ln.split()
            if not tok:
                continue
            self.rec = {"line": no, "op": tok[0], "args": tok[1:], "error": None, "rows": None}
            try:
                res = getattr(self, "do_" + tok[0])(tok[1:])
                out.append(format_result(no, tok[0], res))
                self.rec["n"] = len(res[0]) if tok[0] == "DUPS" else len(res)
            except ModelError as e:
                self.rec["error"] = str(e)
                out.append(f"E {no} {e}")
            self.records.append(self.rec)
        return out


def format_result(no, op, res):
    if op == "DUPS":
        pairs, cut_names = res
        return " ".join([f"R {no} {len(pairs)}"] + [f"{a} {b} {s}" for a, b, s in pairs] + [f"T {len(cut_names)}"] + list(cut_names))
    return " ".join([f"R {no} {len(res)}"] + [f"{nm} {val}" for nm, val in res])


def replay(oracle, pool, script):
    """-> (expected lines, records)"""
    m = StoreModel(oracle, pool)
    lines = m.replay(script)
    return lines, m.records
