"""Random operations over filters built from row attributes on one long-lived index: appends past capacity growths,
removals, id offsets, edits of a prior and a grouping, and -- on a pool of live filters -- set_where, set_keys, combine, invert and the
older set_ranges, in a seeded random order.  After every step every live filter is held against the NumPy model
(where_model.py: ranges, count, n_selected), and every few steps one of them is searched and held against the per-call filtered
search and the oracle.  The layouts are those of tests/random_walk.py (tests/RANDOM_WALK.md): its plain cases' first and its
three-shard case; the walk itself is this file's own, the model of random_walk.py knows no priors."""
import numpy as np
import pytest

import where_model as wm
from random_walk import ADD_SIZES, CASES, OFFSETS
from test_resident_filter_gpu import check_search, check_set

pytestmark = pytest.mark.gpu

STEPS = 60
MAX_ROWS = 7800
VALUES = np.array([0.0, -0.0, 0.5, 1.0, 1.0, 2.0, -3.0, 1e-40, 7.5], np.float32)
FORCED = {0: "new", 1: "where", 3: "keys", 5: "combine", 7: "invert", 9: "add"}
LAYOUTS = [c for c in CASES if c["name"] in ("int8-d384", "3shards-d100")]


class State:
    def __init__(self, idx, rng, d):
        self.idx, self.rng, self.d = idx, rng, d
        self.X = np.zeros((0, d), np.float32)
        self.alive = np.zeros(0, bool)
        self.vals = np.zeros(0, np.float32)
        self.keys = np.zeros(0, np.uint32)
        self.off = 0
        self.pri, self.grp = idx.make_prior(), idx.make_grouping()
        self.filters = []                                               # [handle, model]
        self.log = []

    @property
    def n(self):
        return self.X.shape[0]

    def grow(self, m):
        rows = (self.rng.standard_normal((m, self.d)) * self.rng.uniform(0.5, 2.0, (m, 1))).astype(np.float32)
        self.idx.add(rows)
        self.X = np.concatenate([self.X, rows])
        self.alive = np.r_[self.alive, np.ones(m, bool)]
        self.vals = np.r_[self.vals, np.zeros(m, np.float32)]           # new rows read 0 / key 0 until a call names them
        self.keys = np.r_[self.keys, np.zeros(m, np.uint32)]
        for f in self.filters:
            f[1] = wm.grown(f[1], self.n)                               # ... and are outside every filter

    def some_rows(self, m):
        return self.rng.choice(self.n, min(m, self.n), replace=False)

    def ids(self, rows):
        return np.asarray(rows, np.uint64) + np.uint64(1 + self.off)

    def bounds(self):
        lo, hi = np.sort(self.rng.choice(VALUES, 2))
        pick = self.rng.integers(5)
        return [(lo, hi), (-np.inf, hi), (lo, np.inf), (lo, lo), (hi, lo)][pick]

    def step(self, forced=None):
        rng, idx = self.rng, self.idx
        ops = ["where", "where", "keys", "keys", "combine", "invert", "prior", "group", "new", "ranges"]
        if self.n < MAX_ROWS:
            ops += ["add", "add"]
        if self.alive.sum() > 200:
            ops.append("remove")
        ops.append("offset")
        if len(self.filters) > 5:
            ops.append("drop")
        op = ops[rng.integers(len(ops))]
        if forced in ops:
            op = forced
        if not self.filters and op in ("where", "keys", "combine", "invert", "ranges", "drop"):
            op = "new"
        self.log.append(op)
        f = self.filters[rng.integers(len(self.filters))] if self.filters else None
        if op == "add":
            self.grow(int(rng.choice(ADD_SIZES)))
        elif op == "remove":
            rows = self.some_rows(int(rng.integers(1, 120)))
            idx.remove(self.ids(rows))
            self.alive[rows] = False
        elif op == "offset":
            self.off = int(rng.choice(OFFSETS))
            idx.set_id_offset(self.off)
        elif op == "prior":
            if rng.integers(2):
                rows = self.some_rows(int(rng.integers(1, 400)))
                v = rng.choice(VALUES, rows.size)
                self.pri.set_ids(self.ids(rows), v)
                self.vals[rows] = v
            else:
                a = int(rng.integers(self.n))
                b = min(self.n, a + int(rng.integers(1, 700)))
                v = rng.choice(VALUES)
                self.pri.set_ranges([[a + 1 + self.off, b + 1 + self.off]], [v])
                self.vals[a:b] = v
        elif op == "group":
            a = int(rng.integers(self.n))
            b = min(self.n, a + int(rng.integers(1, 300)))
            k = int(rng.choice([0, 1, 2, 3, 5, 0xFFFFFFFF, 77]))
            self.grp.set_ranges([[a + 1 + self.off, b + 1 + self.off]], [k])
            self.keys[a:b] = k
        elif op == "new":
            self.filters.append([idx.make_filter(), np.zeros(self.n, bool)])
        elif op == "drop":
            f[0].close()
            self.filters = [g for g in self.filters if g is not f]
        elif op == "ranges":
            a = int(rng.integers(self.n))
            b = min(self.n, a + int(rng.integers(1, 900)))
            allow = int(rng.integers(2))
            (f[0].allow if allow else f[0].deny)(ranges=[[a + 1 + self.off, b + 1 + self.off]])
            f[1][a:b] = bool(allow)
        elif op == "where":
            lo, hi = self.bounds()
            allow = int(rng.integers(3) > 0)
            got = (f[0].allow_where if allow else f[0].deny_where)(self.pri, float(lo), float(hi))
            f[1], want = wm.edit(f[1], wm.select_where(self.vals, self.n, lo, hi), allow)
            assert got == want, self.what(f"n_selected of [{lo}, {hi}]")
        elif op == "keys":
            wanted = rng.choice([0, 1, 2, 3, 5, 0xFFFFFFFF, 77, 12345], int(rng.integers(0, 6)))
            allow = int(rng.integers(3) > 0)
            got = (f[0].allow_keys if allow else f[0].deny_keys)(self.grp, wanted.astype(np.uint32))
            f[1], want = wm.edit(f[1], wm.select_keys(self.keys, self.n, wanted), allow)
            assert got == want, self.what(f"n_selected of keys {wanted.tolist()}")
        elif op == "invert":
            f[0].invert()
            f[1] = wm.invert(f[1])
        elif op == "combine":
            g = self.filters[rng.integers(len(self.filters))]
            h = self.filters[rng.integers(len(self.filters))]            # dst: any of them, the operands included
            code = int(rng.integers(4))
            assert idx.combine_filters(f[0], g[0], code, out=h[0]) is h[0]
            h[1] = wm.combine(f[1], g[1], code)

    def what(self, msg):
        return f"step {len(self.log)} ({' '.join(self.log[-8:])}): {msg}"

    def check(self):
        assert len(self.idx) == self.n
        for i, (flt, model) in enumerate(self.filters):
            check_set(flt, model, self.alive, self.what(f"filter {i}"), self.off)

    def close(self):
        for flt, _ in self.filters:
            flt.close()
        self.pri.close()
        self.grp.close()


@pytest.mark.parametrize("case", LAYOUTS, ids=[c["name"] for c in LAYOUTS])
def test_random_operations(case, oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(case["seed"] + 18)
    kw = dict(devices=case["devices"], block_rows=case["block_rows"]) if case["devices"] else {}
    with FlatIndex(case["d"], **kw) as idx:
        if case["copy"] == "i8":
            idx.set_filter_copy("i8")
        s = State(idx, rng, case["d"])
        try:
            s.grow(700)
            seen = set()
            for i in range(STEPS):
                s.step(FORCED.get(i % 12))                              # every kind of edit comes round, the rest is drawn
                s.check()
                seen.add(s.log[-1])
                if i % 6 == 5 and s.filters:
                    flt, model = s.filters[rng.integers(len(s.filters))]
                    Q = rng.standard_normal((4, case["d"])).astype(np.float32)
                    Q[3] = 0.0
                    check_search(idx, flt, oracle, s.X, model, s.alive, Q, 10, s.what("search"), s.off)
            assert {"where", "keys", "combine", "invert", "add"} <= seen, seen
            assert s.n > 1024 + 700                                     # rows were appended under live filters
        finally:
            s.close()
