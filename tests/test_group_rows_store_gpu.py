"""The store and task mirrors of grouped search with members (HipFlatStore.search_document_passages / search_spread, their VectorStorage
forwards, tasks.search_document_passages / search_docs_spread, and the same two methods of include/memex_hip.hpp) against
tests/group_rows_model.py.  One script runs on the C++ mirror (tests/cpp/test_store_group_rows.cpp, one driver process) and on the
Python mirror; both must print the model's lines: _id strings and f32 score bits equal, no tolerance anywhere."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import bits
from group_rows_model import capped_model, default_fetch_rows, group_rows_model
from grouped_model import default_fetch
from mmr_model import near_copy_corpus, queries_near_centres

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 64
_CACHE = {}


def hexf(x):
    return "%08x" % int(bits(np.float32(x)).reshape(-1)[0])


def corpus():
    """12 clusters of 8 near-copies: 96 segments; documents d0 .. d8 hold the rows of clusters 0 .. 8, d9 holds clusters 9 and 10 (16
    rows: more than a first list of 8 candidates), cluster 11 stays ungrouped; rows 5 and 29 are removed.  Queries: four near
    cluster centres 3, 9, 11 and 0, one far from everything"""
    if "corpus" not in _CACHE:
        rng = np.random.default_rng(3195)
        X, centres = near_copy_corpus(rng, clusters=12, per=8, d=D)
        Q = np.concatenate([queries_near_centres(rng, centres[[3, 9, 11, 0]], 4), rng.standard_normal((1, D))]).astype(np.float32)
        keys = np.zeros(96, np.uint32)
        keys[:80] = np.arange(80) // 8 + 1                              # keys 1, 2, ... in the order the names are first seen
        keys[80:88] = 10
        alive = np.ones(96, bool)
        alive[[5, 29]] = False
        _CACHE["corpus"] = (X, Q, keys, alive)
    return _CACHE["corpus"]


def doc(key):
    return f"d{int(key) - 1}" if key else None


def want_passages(oracle, q, limit, passages, fetch):
    """what search_document_passages returns: the model at the first fetch, once more at 4096 when that is not complete"""
    X, _, keys, alive = corpus()
    first = fetch or default_fetch_rows(limit, passages)
    for f in (first, 4096):
        ids, sc, _, gk, _, mem, mc, nf, done = group_rows_model(oracle, X, q, limit, passages, keys, fetch=f, alive=alive)
        if done[0] or f >= 4096:
            break
    hits = [(doc(gk[0, j]), [(f"s{int(ids[0, j, r]) - 1}", float(sc[0, j, r])) for r in range(int(mem[0, j]))], bool(mc[0, j]))
            for j in range(int(nf[0]))]
    return hits, bool(done[0]), f != first


def want_spread(oracle, q, limit, per_document, fetch):
    X, _, keys, alive = corpus()
    first = fetch or default_fetch(limit)
    for f in (first, 4096):
        ids, sc, _, gk, nf, done = capped_model(oracle, X, q, limit, per_document, keys, f, alive=alive)
        if done[0] or f >= 4096:
            break
    return [(doc(gk[0, j]), f"s{int(ids[0, j]) - 1}", float(sc[0, j])) for j in range(int(nf[0]))], bool(done[0]), f != first


def passages_line(hits, complete):
    out = [str(int(complete)), str(len(hits))]
    for d, rows, mc in hits:
        out += [d or "-", str(int(mc)), str(len(rows))] + [t for n, s in rows for t in (n, hexf(s))]
    return " ".join(out)


def spread_line(hits, complete):
    return " ".join([str(int(complete)), str(len(hits))] + [t for d, n, s in hits for t in (d or "-", n, hexf(s))])


# (query, limit, passages / per_document, fetch; 0: the default)
PASSAGES = [(0, 4, 3, 0), (0, 4, 3, 8), (1, 3, 16, 8), (1, 2, 5, 12), (2, 5, 2, 0), (3, 10, 1, 0), (4, 6, 4, 40), (1, 12, 8, 96), (0, 1, 1, 1),
            (2, 1, 16, 4)]
SPREAD = [(0, 6, 2, 0), (0, 6, 1, 6), (1, 10, 2, 12), (1, 4, 20, 4), (2, 8, 1, 0), (3, 5, 3, 5), (4, 10, 2, 0), (1, 40, 3, 64)]


def scenario(oracle, mode):
    X, Q, keys, alive = corpus()
    pool = np.ascontiguousarray(np.concatenate([X, Q]))
    lines, want, asked_again, open_groups = [f"OPEN {mode}"], {}, 0, 0
    lines.append("INSERT " + " ".join(f"s{i}:{i}" for i in range(80)))
    for d in range(9):
        lines.append(f"GROUP d{d} " + " ".join(f"s{i}" for i in range(8 * d, 8 * d + 8)))
    lines.append("INSERT " + " ".join(f"s{i}:{i}" for i in range(80, 96)))      # arrive later: ungrouped until assigned
    lines.append("GROUP d9 " + " ".join(f"s{i}" for i in range(72, 88)))
    lines.append("REMOVE s5 s29")
    for b, limit, n, fetch in PASSAGES:
        hits, complete, again = want_passages(oracle, Q[b], limit, n, fetch)
        lines.append(f"PASSAGES {96 + b} {limit} {n} {fetch}")
        want[len(lines)] = passages_line(hits, complete)
        asked_again += again
        open_groups += sum(not h[2] for h in hits)
    for b, limit, per, fetch in SPREAD:
        hits, complete, again = want_spread(oracle, Q[b], limit, per, fetch)
        lines.append(f"SPREAD {96 + b} {limit} {per} {fetch}")
        want[len(lines)] = spread_line(hits, complete)
        asked_again += again
    lines.append("PASSAGES 96 300 16 0")                                 # k * n > 4096: refused
    lines.append("PASSAGES 96 4 17 0")                                   # n > 16: refused
    assert asked_again >= 3 and open_groups >= 1                         # (conditions on the input: the second ask, an open group)
    return pool, "\n".join(lines) + "\n", want


def python_replay(pool, script, work):
    """the script on memex_amd.storage.HipFlatStore -> the driver's lines"""
    from memex_amd import storage
    st, grp, out = None, None, []
    for no, ln in enumerate(script.splitlines(), 1):
        op, a = ln.split()[0], ln.split()[1:]
        try:
            res = "0"
            if op == "OPEN":
                st = storage.HipFlatStore.new(os.path.join(work, "col"), devices=[0, 0] if a[0] == "sharded" else None)
            elif op == "INSERT":
                st.bulk_insert([storage.VectorData(_id=t.split(":")[0], document_id="d", text="", vector=pool[int(t.split(":")[1])].tolist())
                                for t in a])
                res = str(len(a))
            elif op == "REMOVE":
                res = str(st.remove(a))
            elif op == "GROUP":
                grp = grp or st.make_grouping()
                grp.assign(a[0], a[1:])
                res = str(len(a) - 1)
            elif op == "PASSAGES":
                res = passages_line(*st.search_document_passages(pool[int(a[0])], int(a[1]), grp, int(a[2]), int(a[3]) or None))
            elif op == "SPREAD":
                res = spread_line(*st.search_spread(pool[int(a[0])], int(a[1]), grp, int(a[2]), int(a[3]) or None))
            else:
                raise AssertionError(ln)
            out.append(f"R {no} {res}")
        except storage.Unsupported:
            out.append(f"E {no} Unsupported")
        except storage.SearchError:
            out.append(f"E {no} SearchError")
    if grp:
        grp.close()
    st.delete_all()
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory, lib_built):
    exe = str(tmp_path_factory.mktemp("store_group_rows") / "test_store_group_rows")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_store_group_rows.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "memex_amd"), "-lmemex_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "memex_amd")])
    return exe


@pytest.mark.parametrize("mode", ["plain", "sharded"])
def test_cpp_and_python_mirrors_against_the_model(mode, oracle, driver, tmp_path):
    pool, script, want = scenario(oracle, mode)
    (tmp_path / "cpp").mkdir()
    (tmp_path / "py").mkdir()
    with open(tmp_path / "vectors.bin", "wb") as f:
        f.write(struct.pack("<ii", pool.shape[1], pool.shape[0]))
        f.write(pool.tobytes())
    (tmp_path / "script.txt").write_text(script)
    r = subprocess.run([driver, str(tmp_path / "cpp"), str(tmp_path / "vectors.bin"), str(tmp_path / "script.txt")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    cpp = r.stdout.splitlines()
    py = python_replay(pool, script, str(tmp_path / "py"))
    src = script.splitlines()
    assert len(cpp) == len(py) == len(src)
    for no, (c, p) in enumerate(zip(cpp, py), 1):
        assert c == p, f"line {no}: {src[no - 1][:80]}\n  C++    {c[:300]}\n  Python {p[:300]}"
        if no in want:
            assert c == f"R {no} {want[no]}", f"line {no}: {src[no - 1][:80]}: the model says {want[no][:300]}"
    assert cpp[-2].startswith(f"E {len(src) - 1} ") and cpp[-1].startswith(f"E {len(src)} ")


def test_store_forwards_and_tasks(oracle, lib_built, tmp_path):
    from memex_amd import storage, tasks
    X, Q, keys, alive = corpus()
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    assert st.search_document_passages(Q[0], 4, None) == ([], True) and st.search_spread(Q[0], 4, None) == ([], True)   # no rows: no device
    st.bulk_insert([storage.VectorData(_id=f"s{i}", document_id="", text="", vector=list(map(float, v))) for i, v in enumerate(X)])
    docs = {f"d{d}": [f"s{i}" for i in range(8 * d, 8 * d + 8)] for d in range(9)}
    docs["d9"] = [f"s{i}" for i in range(72, 88)]
    with st.make_grouping(docs) as grp:
        st.remove(["s5", "s29"])
        hits, complete = st.search_document_passages(Q[0], 4, grp)
        assert (hits, complete) == want_passages(oracle, Q[0], 4, 3, 0)[:2] and complete
        assert hits[0][0] == "d3" and len(hits[0][1]) == 3 and hits[0][2] is True
        assert hits[0][1][0] == st.search(Q[0], 1)[0]                   # the first passage is the best segment
        assert [h[0] for h in hits] == [h[0] for h in st.search_documents(Q[0], 4, grp)[0]]
        assert st.search_document_passages(Q[1], 3, grp, 16, fetch=8) == want_passages(oracle, Q[1], 3, 16, 8)[:2]     # asks again by itself
        assert want_passages(oracle, Q[1], 3, 16, 8)[2]
        flat, complete = st.search_spread(Q[0], 6, grp)
        assert (flat, complete) == want_spread(oracle, Q[0], 6, 2, 0)[:2] and complete
        assert max(sum(1 for h in flat if h[0] == d) for d in docs) <= 2 and [h[0] for h in flat[:2]] == ["d3", "d3"]
        assert st.search_spread(Q[0], 6, grp, 1, fetch=6) == want_spread(oracle, Q[0], 6, 1, 6)[:2]
        assert st.search_document_passages(Q[0], 0, grp) == ([], True) and st.search_spread(Q[0], 3, grp, 0) == ([], True)
        vs = storage.VectorStorage(st)
        assert vs.search_document_passages(Q[0], 4, grp) == (hits, True) and vs.search_spread(Q[0], 6, grp) == (flat, True)
        with pytest.raises(storage.SearchError):
            st.search_document_passages(Q[0][:5], 4, grp)

        class Hit:
            def __init__(self, v):
                self.vector = v

        class Embedder:
            def encode_single(self, text):
                return Hit(list(map(float, Q[0]))) if text else None

        assert tasks.search_document_passages(vs, Embedder(), grp, "a question", limit=4) == (hits, True)
        assert tasks.search_document_passages(st, Embedder(), grp, "a question", limit=3, passages=16) == \
            want_passages(oracle, Q[0], 3, 16, 0)[:2]
        assert tasks.search_docs_spread(vs, Embedder(), grp, "a question", limit=6) == (flat, True)
        assert tasks.search_docs_spread(st, Embedder(), grp, "a question", limit=6, per_document=1) == want_spread(oracle, Q[0], 6, 1, 0)[:2]
        for call in (tasks.search_document_passages, tasks.search_docs_spread):
            with pytest.raises(ValueError, match="Invalid query"):
                call(st, Embedder(), grp, "")
        st.compact()                                                    # the rows were renumbered: the grouping says so
        with pytest.raises(storage.SearchError, match="stale"):
            st.search_document_passages(Q[0], 4, grp)
        with pytest.raises(storage.SearchError, match="stale"):
            st.search_spread(Q[0], 4, grp)
    st.delete_all()
