"""The C++ store mirror's feature methods (include/memex_hip.hpp: search_within, filters, search_above, search_diverse, search_fused,
more_like, search_like, rerank, find_duplicates, remove / compact, the VectorStorage forwards) against tests/cpp_store_model.py.

One scripted driver process per scenario (tests/cpp/test_store_features.cpp); its stdout is compared line by line with the model's
lines: _id strings and f32 score bits must be equal, there is no tolerance anywhere.  The same script is replayed on the Python mirror
(memex_amd/storage.py) and held to the same lines.  tests/CPP_MIRROR.md maps methods to scenario lines and lists the mutants."""
import os
import subprocess

import numpy as np
import pytest

from cpp_store_model import bits_of, f32_of, replay, rocchio_weights, split_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STATE = {"dead": None}                                           # set by a driver that timed out or died by a signal
_BUILT = {}


def build_driver(tmp_path_factory):
    if "exe" not in _BUILT:
        exe = str(tmp_path_factory.mktemp("store_features") / "test_store_features")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "test_store_features.cpp"), "-o", exe,
                               "-L", os.path.join(ROOT, "memex_amd"), "-lmemex_hip", "-lpthread",
                               "-Wl,-rpath," + os.path.join(ROOT, "memex_amd")])
        _BUILT["exe"] = exe
    return _BUILT["exe"]


def hexf(x):
    return bits_of(np.float32(x))


# ---- scenarios: (pool f32 [count, d], script text) ------------------------------------------------------------------------------------
class Script:
    """collects the lines of a script while a model runs them, so a later line can be written from the state so far"""

    def __init__(self, oracle, pool):
        from cpp_store_model import StoreModel
        self.model = StoreModel(oracle, pool)
        self.lines = []

    def add(self, *tokens):
        ln = " ".join(str(t) for t in tokens)
        self.lines.append(ln)
        no = len(self.lines)
        self.model.replay("\n" * (no - 1) + ln)
        return self.model.records[-1]

    def text(self):
        return "\n".join(self.lines) + "\n"


def unit(v):
    return v / np.linalg.norm(v)


def segments(oracle, mode):
    """d = 40 (padded inside the library), about 600 rows under 150 _ids of 1 .. 6 rows; see tests/CPP_MIRROR.md"""
    d, n_ids = 40, 150
    rng = np.random.default_rng(4040)
    counts = rng.integers(1, 7, n_ids)
    perm = [int(i) for i in rng.permutation(n_ids)]
    copies = [[perm[g * 5 + c] for c in range(5)] for g in range(8)]           # 8 groups of 5 exact copies, each under another _id
    triple, zero, hub, leaves = perm[40:43], perm[43], perm[44], perm[45:48]
    doc6, near = perm[48], perm[49:52]
    between = sorted(perm[52:100])[10]                                          # a single-row _id between two others (WITHIN's gap)
    counts[doc6], counts[between] = 6, 1
    plain = [i for i in perm[52:] if i not in (between - 1, between, between + 1)]
    name = lambda i: f"s{i:03d}"  # noqa: E731
    vecs = {i: rng.standard_normal((counts[i], d)).astype(np.float32) for i in range(n_ids)}
    for g in copies:
        v = rng.standard_normal(d).astype(np.float32)
        for i in g:
            vecs[i][0] = v
    vecs[triple[0]][0] = vecs[triple[1]][0] = vecs[triple[2]][0] = rng.standard_normal(d).astype(np.float32)
    vecs[zero][0] = 0
    basis = np.linalg.qr(rng.standard_normal((d, 4)))[0].T                      # hub and three leaves at cos 0.99 of it, 0.98 of each other
    vecs[hub][0] = (3.0 * basis[0]).astype(np.float32)
    for j, i in enumerate(leaves):
        vecs[i][0] = (0.99 * basis[0] + np.sqrt(1 - 0.99 ** 2) * basis[j + 1]).astype(np.float32)
    centre = unit(rng.standard_normal(d))
    vecs[doc6] = np.stack([centre + 0.07 * rng.standard_normal(d) for _ in range(6)]).astype(np.float32)   # a tight cluster under one _id
    for i in near:
        vecs[i][0] = (centre + 0.2 * rng.standard_normal(d)).astype(np.float32)
    two_runs = [int(i) for i in rng.choice([i for i in range(n_ids) if counts[i] >= 2 and i != doc6], 20, replace=False)]
    # the pool: the rows in _id order, then the queries
    first, rows = {}, []
    for i in range(n_ids):
        first[i] = len(rows)
        rows += list(vecs[i])
    n_rows = len(rows)
    rand_q = [rng.standard_normal(d).astype(np.float32) for _ in range(6)]
    fuse_q = [(centre + 0.3 * rng.standard_normal(d)).astype(np.float32) for _ in range(3)]
    pool = np.stack(rows + rand_q + fuse_q + [np.float32(2.5) * vecs[copies[0][0]][0]])
    Q = list(range(n_rows, n_rows + 6))                                         # six random queries
    FQ = list(range(n_rows + 6, n_rows + 9))                                    # three phrasings near the cluster
    stored = [first[copies[1][2]], first[plain[0]]]                             # two stored rows as queries
    scaled = n_rows + 9                                                         # a scaled copy of a duplicated row
    s = Script(oracle, pool)
    s.add("OPEN", mode)

    def insert(ids, part):
        toks = []
        for i in ids:
            half = counts[i] // 2 if i in two_runs else counts[i]
            ks = range(half) if part == 0 else range(half, counts[i])
            toks += [f"{name(i)}:{first[i] + k}" for k in ks]
        s.add("INSERT", *toks)
    insert(range(0, 75), 0)
    insert(range(75, n_ids), 0)
    insert(sorted(two_runs), 1)                                                 # twenty _ids get their second run of rows

    def pick(total, avoid=()):
        """plain _ids whose row counts sum to `total`"""
        out, left = [], total
        for i in plain:
            if i not in avoid and i not in out and counts[i] <= left:
                out.append(i)
                left -= counts[i]
            if left == 0:
                return out
        raise AssertionError(total)

    pos1 = pick(2)
    pos2 = pick(4, pos1)
    neg = {n: pick(n, pos1 + pos2) for n in (1, 3, 5, 10)}
    seventeen = pick(17)
    removed = [g[3] for g in copies] + [g[4] for g in copies] + [zero, neg[3][0], plain[5]]
    within_ids = [two_runs[0], two_runs[1], plain[1], plain[2], removed[0], doc6]
    rerank_ids = [two_runs[2], copies[2][0], copies[2][1], plain[3], doc6, removed[1], hub]
    nm = lambda ids: [name(i) for i in ids]  # noqa: E731

    def battery(p):
        f = f"f{p}"
        for q in Q + stored + [scaled]:
            s.add("SEARCH", q, 10)
        s.add("SEARCH", Q[0], 700)
        s.add("SEARCH", Q[0], 0)
        s.add("SEARCH", f"{Q[0]}/39", 5)
        s.add("WITHIN", Q[1], 5, *nm(within_ids), "nobody", name(within_ids[0]))
        s.add("WITHIN", first[between], 3, name(between - 1), name(between + 1))     # the row between the two runs is the query
        s.add("WITHIN", stored[0], 4, *nm(copies[1]))
        s.add("WITHIN", f"{Q[1]}/41", 5, *nm(within_ids))
        s.add("WITHIN", Q[1], 5, "nobody")
        s.add("FILTER", f, *nm(within_ids[:4]))
        s.add("COUNT", f)
        s.add("IN", Q[2], 5, f)
        s.add("ALLOW", f, *nm(copies[3]), "nobody", name(removed[2]))
        s.add("DENY", f, name(within_ids[1]), name(plain[4]))
        s.add("COUNT", f)
        s.add("IN", Q[2], 8, f)
        s.add("IN", stored[0], 30, f)
        s.add("IN", f"{Q[2]}/39", 5, f)
        sc = s.model.S(pool[Q[3]], s.model.live())[2]
        for at, limit in ((0, 10), (6, 10), (len(sc) - 1, 700), (6, 3)):             # thresholds bit for bit at the oracle's scores
            s.add("ABOVE", Q[3], bits_of(sc[at]), limit)
        s.add("ABOVE", scaled, hexf(0.999), 10)
        s.add("ABOVE", Q[3], bits_of(sc[6]), 5000)
        s.add("ABOVE", f"{Q[3]}/39", bits_of(sc[6]), 10)
        s.add("DIVERSE", Q[4], 5, 0, hexf(0.5))
        s.add("DIVERSE", scaled, 6, 0, hexf(0.3))
        s.add("DIVERSE", FQ[0], 6, 40, hexf(0.7))
        s.add("DIVERSE", f"{Q[4]}/39", 5, 0, hexf(0.5))
        s.add("FUSED", "max", 5, 0, 3, Q[0], Q[1], Q[2])
        s.add("FUSED", "rrf", 8, 0, 3, *FQ)
        s.add("FUSED", "rrf", 5, 20, 3, *FQ, hexf(1.0), hexf(0.0), hexf(2.0))
        s.add("FUSED", "max", 5, 0, 2, scaled, Q[5], hexf(1.0), hexf(0.5))
        s.add("FUSED", "max", 5, 0, 2, Q[0], f"{Q[1]}/39")
        s.add("MORE", name(doc6), 3)
        s.add("MORE", name(copies[2][1]), 5)
        s.add("MORE", name(two_runs[3]), 4)
        s.add("MORE", "nobody", 5)
        s.add("MORE", name(removed[0]), 5)
        for n in (1, 3, 5, 10):
            s.add("LIKE", 5, "-", "default", "+", *nm(pos1), "-", *nm(neg[n]))
        s.add("LIKE", 5, Q[5], "default", "+", *nm(pos1), "-", *nm(neg[5]))          # vec + both
        s.add("LIKE", 5, "-", "default", "+", *nm(pos1 + pos2), "-")                 # positive only
        s.add("LIKE", 5, Q[0], "default", "+", "-")                                  # vec only
        s.add("LIKE", 6, stored[1], hexf(0.5), hexf(1.0), hexf(0.25), "+", name(doc6), "-", name(hub), "nobody")
        s.add("LIKE", 5, "-", "default", "+", "nobody", "-")
        s.add("LIKE", 5, "-", "default", "+", *nm(pos1), "nobody", "-", *nm(neg[1]))
        s.add("LIKE", 5, "-", "default", "+", *nm(seventeen), "-")
        s.add("LIKE", 5, f"{Q[5]}/39", "default", "+", *nm(pos1), "-")
        s.add("RERANK", Q[1], 0, *nm(rerank_ids), "nobody")
        s.add("RERANK", Q[1], 3, *nm(rerank_ids))
        s.add("RERANK", scaled, 0, *nm(copies[0]), name(copies[0][0]))
        s.add("RERANK", f"{Q[1]}/39", 0, *nm(rerank_ids))
        s.add("RERANK", Q[1], 0, "nobody")
        s.add("DUPS", hexf(0.985), 64)
        s.add("DUPS", hexf(0.985), 2)
        s.add("VS_LIKE", 5, Q[5], "default", "+", *nm(pos1), "-", *nm(neg[5]))
        s.add("VS_RERANK", Q[1], 3, *nm(rerank_ids))
        s.add("COUNT", f)                                                        # get_vector_storage attached by a load: stale

    battery(0)
    s.add("REMOVE", *nm(removed), "nobody", name(removed[0]))
    s.add("REMOVE", name(removed[0]))                                           # already gone: 0
    battery(1)
    s.add("FILTER", "r1", *nm(within_ids[:4]))
    s.add("RELOAD")                                                             # the removals come back from the files
    s.add("COUNT", "r1")
    s.add("SEARCH", Q[0], 10)
    s.add("FILTER", "c1", *nm(within_ids[:4]))
    s.add("COMPACT")
    s.add("COUNT", "c1")
    s.add("IN", Q[2], 5, "c1")
    s.add("ALLOW", "c1", name(plain[1]))
    battery(2)
    s.add("FILTER", "c2", *nm(within_ids[:4]))
    s.add("COMPACT")                                                            # nothing removed: a no-op, the filter stays
    s.add("COUNT", "c2")
    s.add("SAVE")
    s.add("RELOAD")
    s.add("DENY", "c2", name(plain[1]))
    battery(3)
    s.add("INSERT", f"late:{Q[0]}", f"{name(plain[1])}:{Q[1]}")                  # ids continue after the compacted rows
    s.add("SEARCH", Q[0], 3)
    s.add("WITHIN", Q[1], 3, name(plain[1]))
    s.add("FILTER", "d1", "late")
    s.add("COUNT", "d1")
    s.add("DELETE_ALL")
    s.add("COUNT", "d1")
    s.add("SEARCH", Q[0], 5)
    return pool, s.text()


def wide_lists(oracle, mode="plain"):
    """d = 8, 9000 rows under 3 _ids, a cluster of 300 rows under a fourth, six singles"""
    d = 8
    rng = np.random.default_rng(808)
    big = rng.standard_normal((9000, d)).astype(np.float32)
    centre = unit(rng.standard_normal(d))
    cluster = (centre + 0.05 * rng.standard_normal((300, d))).astype(np.float32)
    singles = rng.standard_normal((6, d)).astype(np.float32)
    big[10] = big[3500] = big[8000] = singles[0]                                # four exact copies, 512-row blocks apart
    big[8700] = np.float32(1.5) * big[700]                                      # and a scaled pair
    queries = np.stack([np.float32(2.0) * big[8500], big[5000], rng.standard_normal(d).astype(np.float32),
                        (centre + 0.1 * rng.standard_normal(d)).astype(np.float32)])
    pool = np.concatenate([big, cluster, singles, queries])
    QC, QB, QR, QM = range(9306, 9310)
    s = Script(oracle, pool)
    s.add("OPEN", mode)
    for j, nm in enumerate("ABC"):
        s.add("INSERT", *[f"{nm}:{r}" for r in range(3000 * j, 3000 * (j + 1))])
    s.add("INSERT", *[f"M:{r}" for r in range(9000, 9300)], *[f"x{j}:{9300 + j}" for j in range(6)])
    s.add("SEARCH", QR, 10)
    s.add("WITHIN", QR, 10, "B", "x3")
    s.add("FILTER", "f", "A", "C", "x1")
    s.add("COUNT", "f")
    s.add("IN", QB, 10, "f")
    s.add("RERANK", QC, 0, "C", "A", "B", "x0", "nobody")                       # 9001 candidate rows: three lists of one call
    s.add("RERANK", QC, 2, "A", "B", "C")
    s.add("RERANK", QB, 0, "A", "B", "C", "x2")
    s.add("VS_RERANK", QB, 2, "A", "B", "C")
    s.add("DUPS", hexf(0.9995), 64)
    s.add("DUPS", hexf(0.9995), 2)
    s.add("MORE", "M", 40)
    s.add("MORE", "x0", 5)
    s.add("MORE", "A", 2000)                                                    # 2000 + 3000 entries per list: more than the library lists
    s.add("MORE", "M", 3796)                                                    # 4096
    s.add("LIKE", 5, QM, "default", "+", "x1", "x2", "-", "x3")
    s.add("FUSED", "rrf", 5, 0, 2, QM, QR)
    s.add("DIVERSE", QM, 5, 0, hexf(0.5))
    s.add("REMOVE", "B", "x0")
    s.add("RERANK", QB, 0, "A", "B", "C", "x0")
    s.add("MORE", "M", 40)
    s.add("DUPS", hexf(0.9995), 2)
    s.add("COMPACT")
    s.add("RERANK", QC, 0, "A", "B", "C", "M")
    s.add("DELETE_ALL")
    return pool, s.text()


SCENARIOS = {"segments-plain": (segments, "plain"), "segments-sharded": (segments, "sharded"), "wide_lists": (wide_lists, "plain")}
_CASES = {}


def case(name, oracle):
    """-> (pool, script, expected lines, records): computed once per scenario and shared"""
    if name not in _CASES:
        fn, mode = SCENARIOS[name]
        if mode == "sharded":                                     # the same script behind another first line: the same answers
            pool, script, lines, records = case(name.replace("sharded", "plain"), oracle)
            assert script.startswith("OPEN plain\n")
            _CASES[name] = (pool, script.replace("OPEN plain", "OPEN sharded", 1), lines, records)
        else:
            pool, script = fn(oracle, mode)
            lines, records = replay(oracle, pool, script)
            _CASES[name] = (pool, script, lines, records)
    return _CASES[name]


# ---- conditions on the scenarios, from the model alone: a scenario cannot pass by being empty -----------------------------------------
RESULT_OPS = ("SEARCH", "WITHIN", "IN", "ABOVE", "DIVERSE", "FUSED", "MORE", "LIKE", "RERANK", "DUPS", "VS_LIKE", "VS_RERANK", "COUNT")


def runs(rows):
    rows = sorted(rows)
    return sum(1 for i, r in enumerate(rows) if i == 0 or r != rows[i - 1] + 1)


def check_conditions(name, records):
    by_op = {}
    for r in records:
        by_op.setdefault(r["op"], []).append(r)
    for op in RESULT_OPS:
        if name == "wide_lists" and op in ("ABOVE", "VS_LIKE"):
            continue
        assert any(r["error"] is None and r["n"] > 0 for r in by_op.get(op, [])), f"{name}: no non-empty {op}"
    assert any(r["rows"] and any(a == b for a, b in zip(r["dists"], r["dists"][1:])) for r in records), f"{name}: no tie"
    dups2 = [r for r in by_op["DUPS"] if r["args"][1] == "2"]
    assert all(r["lost_with_a_listed_end"] == 0 for r in by_op["DUPS"])
    assert any(r["truncated"] > 0 for r in dups2) and any(r["pairs_lost"] > 0 for r in dups2)
    if name == "wide_lists":                                      # (its DUPS are about crossing 512-row blocks)
        assert all(r["n"] > 0 for r in by_op["DUPS"]) and any(r.get("candidates", 0) > 2 * 4096 for r in by_op["RERANK"])
        return
    assert any(r["truncated"] > 0 and r["pairs_lost"] == 0 for r in dups2), f"{name}: DUPS per_row 2 that loses no pair"
    assert any(runs(r["allowed"]) >= 3 for r in by_op["WITHIN"] if r.get("allowed")), f"{name}: WITHIN runs"
    seen = set()
    for r in by_op["LIKE"]:
        if r["error"] is None and r.get("n_neg") in (5, 10) and r["args"][2] == "default":
            double = np.float32(-0.15 / r["n_neg"])
            assert r["weights"][-1] != bits_of(double), r
            seen.add(r["n_neg"])
    assert seen == {5, 10}
    assert {r.get("n_neg") for r in by_op["LIKE"] if r["error"] is None} >= {0, 1, 3, 5, 10}
    assert any(r["error"] == "std::invalid_argument -" for r in by_op["LIKE"])
    first_remove = next(i for i, r in enumerate(records) if r["op"] == "REMOVE")
    before = {tuple(r["args"]): r["rows"] for r in records[:first_remove] if r["op"] == "SEARCH"}
    after = [r for r in records[first_remove:] if r["op"] == "SEARCH" and tuple(r["args"]) in before]
    assert any(r["rows"] != before[tuple(r["args"])] for r in after[:12]), f"{name}: REMOVE changes no list"
    stale = [r for r in records if r["op"] in ("COUNT", "IN", "ALLOW", "DENY") and r["args"][-1 if r["op"] == "IN" else 0] in ("r1", "c1", "c2", "d1")]
    assert [r["error"] is None for r in stale] == [False, False, False, False, True, False, True, False], stale
    stale = [r for r in records if r["op"] == "COUNT" and r["error"]]
    assert len(stale) >= 7 and all(r["error"] == "VectorStoreError SearchError" for r in stale)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenarios_meet_their_conditions(name, oracle):
    """(CPU) the conditions of the scenarios, and the model's S against COracle.search with k = n"""
    pool, script, lines, records = case(name, oracle)
    check_conditions(name, records)
    assert len(lines) == len(script.splitlines())
    from cpp_store_model import StoreModel
    m = StoreModel(oracle, pool)
    m.replay("\n".join(script.splitlines()[:4]))
    n = len(m.names) if name != "wide_lists" else 600
    for q in pool[-3:]:
        ids, dists, scores, nf = oracle.search(m.X[:n], q, n)
        rows, d, s = m.S(q, range(n))
        assert nf[0] == n and np.array_equal(ids[0].astype(np.int64) - 1, rows)
        assert np.array_equal(dists[0].view(np.uint32), d.view(np.uint32)) and np.array_equal(scores[0].view(np.uint32), s.view(np.uint32))


# ---- CPU: the driver builds with -Wall and its parser round-trips the scripts ---------------------------------------------------------
def test_driver_compiles_and_links_with_wall(tmp_path_factory, lib_built):
    assert os.path.exists(build_driver(tmp_path_factory))


def test_parse_round_trips_the_scenario_scripts(tmp_path_factory, tmp_path, lib_built, oracle):
    exe = build_driver(tmp_path_factory)
    for name in ("segments-plain", "wide_lists"):
        script = case(name, oracle)[1]
        path = tmp_path / f"{name}.txt"
        path.write_text(script)
        r = subprocess.run([exe, "--parse", str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == script, r.stderr
    bad = tmp_path / "bad.txt"
    bad.write_text("OPEN plain\nABOVE 1 3f8 5\n")
    assert subprocess.run([exe, "--parse", str(bad)], capture_output=True, text=True, timeout=120).returncode == 2


def test_both_mirrors_send_the_same_rocchio_weights():
    """(CPU) memex_amd/storage.py's weights are the f32 divisions the C++ mirror computes from its float parameters, for every
    n_pos, n_neg <= 16 at the default parameters; the double division it used to compute differs for some of them"""
    import inspect
    from memex_amd import storage
    sig = inspect.signature(storage.HipFlatStore.search_like)
    beta, gamma = sig.parameters["beta"].default, sig.parameters["gamma"].default
    differs = set()
    for n_pos in range(0, 17):
        for n_neg in range(0, 17 - n_pos):
            if n_pos + n_neg == 0:
                continue
            w = storage._rocchio_weights(beta, gamma, n_pos, n_neg)
            want = rocchio_weights(np.float32(0.75), np.float32(0.15), n_pos, n_neg)
            assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), want.view(np.uint32)), (n_pos, n_neg)
            if n_neg and w[-1] != np.float32(-gamma / n_neg):
                differs.add(n_neg)
    assert {5, 10, 11, 15} <= differs


def test_python_search_like_hands_those_weights_to_the_index(tmp_path):
    """(CPU) the Python mirror with a stub index: the weights that reach FlatIndex.search_like"""
    from memex_amd import storage
    got = {}

    class StubIndex:
        def search_like(self, ex, k, w, q, qw):
            got["ex"], got["w"] = np.array(ex), np.array(w)
            return np.zeros((1, k), np.uint64), np.zeros((1, k), np.float32), None, np.zeros(1, np.int32), None, None

    st = storage.HipFlatStore(storage_path=str(tmp_path / "col"))
    st._index, st._dim = StubIndex(), 4
    st._id_map = {i + 1: ("p" if i < 2 else f"n{i}") for i in range(12)}
    assert st.search_like(["p"], [f"n{i}" for i in range(2, 12)], 5) == []
    assert got["ex"].tolist() == list(range(1, 13)) and got["w"].dtype == np.float32
    assert np.array_equal(got["w"].view(np.uint32), rocchio_weights(np.float32(0.75), np.float32(0.15), 2, 10).view(np.uint32))
    assert got["w"][-1] != np.float32(-0.15 / 10)


# ---- GPU: the C++ mirror and the Python mirror against the model ----------------------------------------------------------------------
def compare(got, want, what, script):
    src = script.splitlines()
    assert len(got) == len(want), f"{what}: {len(got)} lines for {len(want)} commands\n" + "\n".join(got[-3:])
    for g, w in zip(got, want):
        if g != w:
            no = int(w.split()[1])
            gt, wt = g.split(), w.split()
            at = next((i for i, (a, b) in enumerate(zip(gt, wt)) if a != b), min(len(gt), len(wt)))
            raise AssertionError(f"{what}: line {no}: {src[no - 1][:200]}\n  first difference at token {at}\n  got  {' '.join(gt[:3])} .. "
                                 f"{' '.join(gt[max(at - 2, 0):at + 6])}\n  want {' '.join(wt[:3])} .. {' '.join(wt[max(at - 2, 0):at + 6])}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_cpp_mirror_against_the_model(name, oracle, lib_built, tmp_path_factory, tmp_path):
    if _STATE["dead"]:
        pytest.fail(f"not run: the driver {_STATE['dead']}")
    pool, script, want, records = case(name, oracle)
    check_conditions(name, records)                               # from the model alone, before any GPU output is read
    exe = build_driver(tmp_path_factory)
    with open(tmp_path / "vectors.bin", "wb") as f:
        f.write(np.array(pool.shape[::-1], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(pool, dtype=np.float32).tobytes())
    (tmp_path / "script.txt").write_text(script)
    try:
        r = subprocess.run([exe, str(tmp_path / "work"), str(tmp_path / "vectors.bin"), str(tmp_path / "script.txt")],
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _STATE["dead"] = f"timed out on {name}"
        pytest.fail(_STATE["dead"])
    if r.returncode < 0 or r.returncode in (134, 139):
        _STATE["dead"] = f"died with {r.returncode} on {name}"
        pytest.fail(_STATE["dead"] + "\n" + r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    compare(r.stdout.splitlines(), want, f"C++ mirror, {name}", script)


ERRORS = {"SearchError": "VectorStoreError SearchError", "Unsupported": "VectorStoreError Unsupported", "ValueError": "std::invalid_argument -"}


def python_replay(pool, script, work):
    """the script on memex_amd.storage.HipFlatStore -> the driver's lines"""
    from memex_amd import storage
    from cpp_store_model import format_result
    path = os.path.join(work, "col")
    vec = lambda t: None if t == "-" else (pool[int(t.split("/")[0])][:int(t.split("/")[1])] if "/" in t else pool[int(t)])  # noqa: E731
    listed = lambda res: [(n, bits_of(s)) for n, s in res]  # noqa: E731
    st, devices, filters, out = None, None, {}, []
    for no, ln in enumerate(script.splitlines(), 1):
        op, a = ln.split()[0], ln.split()[1:]
        try:
            res = []
            if op == "OPEN":
                devices = [0, 0] if a[0] == "sharded" else None
                st = storage.HipFlatStore.new(path, devices=devices)
            elif op == "INSERT":
                st.bulk_insert([storage.VectorData(_id=t.rpartition(":")[0], document_id="doc", text="", vector=vec(t.rpartition(":")[2]))
                                for t in a])
            elif op == "REMOVE":
                res = [("removed", "%08x" % st.remove(a))]
            elif op == "COMPACT":
                res = [("kept", "%08x" % len(st.compact()))]
            elif op == "SAVE":
                st.save()
            elif op == "RELOAD":
                storage.evict_resident(path)
                st = storage.HipFlatStore.load(path, devices=devices)
            elif op == "DELETE_ALL":
                st.delete_all()
            elif op == "SEARCH":
                res = listed(st.search(vec(a[0]), int(a[1])))
            elif op == "WITHIN":
                res = listed(st.search_within(vec(a[0]), int(a[1]), a[2:]))
            elif op == "FILTER":
                filters[a[0]] = st.make_filter(a[1:])
            elif op == "ALLOW":
                filters[a[0]].allow(a[1:])
            elif op == "DENY":
                filters[a[0]].deny(a[1:])
            elif op == "COUNT":
                n = filters[a[0]].count()
                res = [("rows", "%08x" % n[0]), ("live", "%08x" % n[1])]
            elif op == "IN":
                res = listed(st.search_in(vec(a[0]), int(a[1]), filters[a[2]]))
            elif op == "ABOVE":
                res = listed(st.search_above(vec(a[0]), f32_of(a[1]), int(a[2])))
            elif op == "DIVERSE":
                res = listed(st.search_diverse(vec(a[0]), int(a[1]), int(a[2]) or None, f32_of(a[3])))
            elif op == "FUSED":
                m = int(a[3])
                w = [f32_of(t) for t in a[4 + m:]]
                res = listed(st.search_fused([vec(t) for t in a[4:4 + m]], int(a[1]), a[0], int(a[2]) or None, w or None))
            elif op == "MORE":
                res = listed(st.more_like(a[0], int(a[1])))
            elif op in ("LIKE", "VS_LIKE"):
                limit, vtok, par, pos, neg = split_like(a)
                target = st if op == "LIKE" else storage.get_vector_storage("hip://" + work, "col", devices=devices)
                kw = {} if a[2] == "default" else dict(alpha=float(par[0]), beta=float(par[1]), gamma=float(par[2]))
                res = listed(target.search_like(pos, neg, limit, vec(vtok), **kw))
            elif op in ("RERANK", "VS_RERANK"):
                target = st if op == "RERANK" else storage.get_vector_storage("hip://" + work, "col", devices=devices)
                res = listed(target.rerank(vec(a[0]), a[2:], int(a[1]) or None))
            elif op == "DUPS":
                pairs, cut = st.find_duplicates(f32_of(a[0]), int(a[1]))
                res = ([(x, y, bits_of(s)) for x, y, s in pairs], cut)
            out.append(format_result(no, op, res))
        except (storage.VectorStoreError, ValueError) as e:
            out.append(f"E {no} {ERRORS.get(type(e).__name__, 'other -')}")
    for f in filters.values():
        f.close()
    storage.evict_resident(path)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_python_mirror_against_the_model(name, oracle, lib_built, tmp_path):
    pool, script, want, records = case(name, oracle)
    check_conditions(name, records)
    compare(python_replay(pool, script, str(tmp_path)), want, f"Python mirror, {name}", script)
