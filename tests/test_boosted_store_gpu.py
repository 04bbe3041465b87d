"""Boosted search in the store mirrors on the GPU: HipFlatStore.search_boosted and its 4096 ladder, VectorStorage.search_boosted, the
recency pair of memex_amd/tasks.py against the folded-weight statement in NumPy, and the C++ mirror (include/memex_hip.hpp) through
the scripted driver tests/cpp/test_store_boosted.cpp, whose output lines must equal the Python mirror's: _id strings, f32 and f64
bits."""
import os
import subprocess

import numpy as np
import pytest

from boosted_model import boosted_model, case_a, case_b
from conftest import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = 20                                                                # windows per document in Case A's corpus


def hexf(x):
    return "%08x" % int(bits(np.float32(x))[0])


def hits_of(got, b=0):
    ids, sc, _, pr, cb, nf, done = got
    n = int(nf[b])
    return [(f"s{int(i) - 1}", float(s), float(p), float(c)) for i, s, p, c in zip(ids[b, :n], sc[b, :n], pr[b, :n], cb[b, :n])], bool(done[b])


def fill(storage, path, X):
    st = storage.HipFlatStore.new(path)
    st.bulk_insert([storage.VectorData(_id=f"s{i}", document_id=f"d{i // PER}", text="", vector=v, segment_id=i % PER)
                    for i, v in enumerate(X)])
    return st


def test_store_search_boosted_and_its_ladder(oracle, lib_built, tmp_path):
    from memex_amd import storage
    X, Q, pv = case_a()
    st = fill(storage, str(tmp_path / "col"), X)
    with st.make_prior() as pri:
        assert st.search_boosted(Q[0], 5, pri, 0.05) == hits_of(boosted_model(oracle, X, Q[:1], 5, None, w=0.05, fetch=32))   # all 0
        pri.set([f"s{i}" for i in range(len(X))] + ["nobody"], np.concatenate([pv, [7.0]]))     # an unknown _id adds nothing
        assert pri.bound() == float(pv.max()), "the value of an unknown _id never reaches the index: the bound does not see it"
        pri.set(["s7"], [7.0])
        pri.set(["s7"], [pv[7]])
        assert pri.bound() == 7.0, "an overwritten large value still bounds"
        assert pri.bound(refresh=True) == float(pv.max())
        for b in range(len(Q)):                                         # Case A: complete at the first rung
            want = hits_of(boosted_model(oracle, X, Q[b:b + 1], 5, pv, w=0.05, fetch=32))
            assert want[1] and st.search_boosted(Q[b], 5, pri, 0.05) == want
        assert storage.VectorStorage(st).search_boosted(Q[0], 5, pri, 0.05) == st.search_boosted(Q[0], 5, pri, 0.05)
        assert st.search_boosted(Q[0], 5, pri, 0.05, fetch=64) == hits_of(boosted_model(oracle, X, Q[:1], 5, pv, w=0.05, fetch=64))
    X, Q, pb, far = case_b(oracle)
    with st.make_prior() as pri:                                        # Case B forces the second rung
        pri.set_document([f"s{far}"], 100.0)
        first = boosted_model(oracle, X, Q[:1], 5, pb, w=1.0, hi=np.float32(100.0), fetch=32)
        assert not first[6][0], "(condition on the input) 32 candidates must not be complete"
        hits, complete = st.search_boosted(Q[0], 5, pri, 1.0)
        assert (hits, complete) == hits_of(boosted_model(oracle, X, Q[:1], 5, pb, w=1.0, hi=np.float32(100.0), fetch=4096))
        assert complete and hits[0][0] == f"s{far}" and hits[0][2] == 100.0
        st.remove([f"s{far}"])                                          # the row is gone, its value still bounds: refresh lowers it
        assert st.search_boosted(Q[0], 5, pri, 1.0)[1] is True and pri.bound() == 100.0
        assert pri.bound(refresh=True) == 0.0
        alive = np.ones(len(X), bool)
        alive[far] = False
        assert st.search_boosted(Q[0], 5, pri, 1.0) == hits_of(boosted_model(oracle, X, Q[:1], 5, None, w=1.0, fetch=32, alive=alive))
        with pytest.raises(storage.SearchError):                        # one segment with two values in one edit
            pri.set(["s1", "s1"], [1.0, 2.0])
        with pytest.raises(storage.SearchError):
            pri.set(["s1"], [float("nan")])
        st.compact()                                                    # the rows were renumbered: the prior says so
        with pytest.raises(storage.SearchError, match="stale"):
            st.search_boosted(Q[0], 5, pri, 1.0)


def test_tasks_recency(oracle, lib_built, tmp_path):
    """documents stamped at different times; a query at `now` ranks a segment by score + weight * 2^-((now - t) / half_life): the stored
    value times the folded weight, both f32, combined in f64 -- the statement is boosted_model with those two.  Row i belongs to
    document i % 100, so the 20 near-copies of a cluster belong to 20 documents of different ages and recency has something to
    re-order"""
    from memex_amd import storage, tasks
    X, Q, _ = case_a()
    n_docs, t0, half = len(X) // PER, 1000.0, 30.0
    rng = np.random.default_rng(3176)
    t = t0 + rng.uniform(0.0, 300.0, n_docs)                            # up to ten half-lives after t0
    data = [storage.VectorData(_id=f"s{i}", document_id=f"d{i % n_docs}", text="", vector=v, segment_id=i // n_docs) for i, v in enumerate(X)]
    st = storage.HipFlatStore.new(str(tmp_path / "col"))
    st.bulk_insert(data)
    pv = np.tile(np.exp2((t - t0) / half).astype(np.float32), PER)

    class Hit:
        def __init__(self, v):
            self.vector = v

    class Embedder:
        def __init__(self, q):
            self.q = q

        def encode_single(self, text):
            return Hit(self.q) if text else None

    with st.make_prior() as pri:
        for d in range(n_docs):
            tasks.stamp_document(pri, data[d::n_docs], t[d], half, t0)
        assert pri.bound() == float(pv.max())
        changed = 0
        for now, weight in ((t0 + 300.0, 0.2), (t0 + 400.0, 0.2), (t0 + 300.0, 0.0)):
            w = np.float32(weight * np.exp2(-(now - t0) / half))
            assert tasks.recency_weight(weight, now, half, t0) == float(w)
            for b in range(len(Q)):
                first = boosted_model(oracle, X, Q[b:b + 1], 5, pv, w=w, fetch=32)
                want = hits_of(first if first[6][0] else boosted_model(oracle, X, Q[b:b + 1], 5, pv, w=w, fetch=4096))
                got = tasks.search_docs_recent(st, Embedder(Q[b]), pri, "a question", limit=5, now=now, half_life=half, t0=t0, weight=weight)
                assert got == want, (now, weight, b)
                assert tasks.search_docs_recent(storage.VectorStorage(st), Embedder(Q[b]), pri, "q", 5, now, half, t0, weight) == want
                # the boost of a hit is weight * 2^-((now - t) / half_life) of its document, to f32 rounding of the two factors
                for name, s, p, c in got[0]:
                    age = now - t[int(name[1:]) % n_docs]
                    assert abs((c - s) - weight * 2.0 ** (-age / half)) <= 2.0 ** -22 * weight
                changed += [h[0] for h in got[0]] != [n for n, _ in st.search(Q[b], 5)]
        assert changed > 0, "(condition on the input) recency re-orders some answer"
        with pytest.raises(ValueError, match="Invalid query"):
            tasks.search_docs_recent(st, Embedder(Q[0]), pri, "", 5, t0, half, t0, 1.0)


def script_for(X, pv, far):
    n = len(X)                                                          # the queries follow the rows in the pool
    lines = [f"INSERT 0 {n} {PER}", "PRIOR", "BOUND 0", f"BOOST {n} 5 {hexf(0.05)} 0"]
    lines.append("SETEACH " + " ".join(f"s{i}:{hexf(pv[i])}" for i in range(n)) + f" nobody:{hexf(3.0)}")
    lines += ["BOUND 0", "BOUND 1"]
    for b in range(6):
        lines.append(f"BOOST {n + b} 5 {hexf(0.05)} 0")
    lines += [f"BOOST {n} 10 {hexf(0.0)} 0", f"BOOST {n + 1} 10 {hexf(1.0)} 64", f"BOOST {n + 2} 3 {hexf(0.3)} 4096", f"BOOST {n} 0 {hexf(1.0)} 0",
              f"VS_BOOST {n + 3} 5 {hexf(0.05)} 0", f"BOOST {n} 5 {hexf(-1.0)} 0", f"BOOST {n} 5 7fc00000 0"]
    lines += ["SET " + hexf(0.0) + " " + " ".join(f"s{i}" for i in range(n)), f"SET {hexf(100.0)} s{far}", "BOUND 1",
              f"BOOST {n} 5 {hexf(1.0)} 0",                             # Case B: the ladder
              f"SETEACH s1:{hexf(1.0)} s1:{hexf(2.0)}", f"SET 7f800000 s2", f"REMOVE s{far}", f"BOOST {n} 5 {hexf(1.0)} 0", "BOUND 1",
              "DELETE_ALL", "BOUND 0", f"BOOST {n} 5 {hexf(1.0)} 0"]
    return "\n".join(lines) + "\n"


def python_replay(pool, script, work):
    """the script on memex_amd.storage.HipFlatStore -> the driver's lines"""
    from memex_amd import storage
    f32 = lambda t: float(np.asarray([int(t, 16)], np.uint32).view(np.float32)[0])  # noqa: E731
    st = storage.HipFlatStore.new(os.path.join(work, "col"))
    pri, out = None, []
    for no, ln in enumerate(script.splitlines(), 1):
        op, a = ln.split()[0], ln.split()[1:]
        try:
            if op == "INSERT":
                first, count, per = int(a[0]), int(a[1]), int(a[2])
                st.bulk_insert([storage.VectorData(_id=f"s{r}", document_id=f"d{r // per}", text="", vector=pool[r], segment_id=r % per)
                                for r in range(first, first + count)])
                out.append(f"R {no} 0")
            elif op == "PRIOR":
                pri = st.make_prior()
                out.append(f"R {no} 0")
            elif op == "SET":
                pri.set_document(a[1:], f32(a[0]))
                out.append(f"R {no} 0")
            elif op == "SETEACH":
                pri.set([t.rpartition(":")[0] for t in a], [f32(t.rpartition(":")[2]) for t in a])
                out.append(f"R {no} 0")
            elif op == "BOUND":
                out.append(f"R {no} 1 {hexf(pri.bound(a[0] == '1'))}")
            elif op in ("BOOST", "VS_BOOST"):
                target = st if op == "BOOST" else storage.VectorStorage(st)
                hits, done = target.search_boosted(pool[int(a[0])], int(a[1]), pri, f32(a[2]), int(a[3]) or None)
                body = "".join(" %s %s %s %016x" % (n, hexf(s), hexf(p), int(np.asarray([c], np.float64).view(np.uint64)[0])) for n, s, p, c in hits)
                out.append(f"R {no} {len(hits)}{body} complete {int(done)}")
            elif op == "REMOVE":
                out.append(f"R {no} 1 %08x" % st.remove(a))
            elif op == "DELETE_ALL":
                st.delete_all()
                out.append(f"R {no} 0")
        except storage.VectorStoreError:
            out.append(f"E {no} VectorStoreError")
    if pri is not None:
        pri.close()
    storage.evict_resident(os.path.join(work, "col"))
    return out


def test_cpp_mirror_equals_the_python_mirror(oracle, lib_built, tmp_path):
    X, Q, pv = case_a()
    far = case_b(oracle)[3]
    pool = np.ascontiguousarray(np.concatenate([X, Q]), dtype=np.float32)
    script = script_for(X, pv, far)
    exe = str(tmp_path / "test_store_boosted")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_store_boosted.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "memex_amd"), "-lmemex_hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "memex_amd")])
    with open(tmp_path / "vectors.bin", "wb") as f:
        f.write(np.array(pool.shape[::-1], dtype=np.int32).tobytes())
        f.write(pool.tobytes())
    (tmp_path / "script.txt").write_text(script)
    os.makedirs(tmp_path / "py")
    want = python_replay(pool, script, str(tmp_path / "py"))
    # (conditions on the script, from the Python mirror's lines) results, the ladder, and refused calls
    src = script.splitlines()
    res = {no: ln for no, ln in enumerate(want, 1)}
    boosts = [no for no, s in enumerate(src, 1) if s.split()[0] in ("BOOST", "VS_BOOST")]
    assert sum(res[no].startswith("R") and int(res[no].split()[2]) > 0 for no in boosts) >= 10
    assert sum(ln.startswith("E") for ln in want) == 6, "a negative and a NaN weight, two refused edits, two calls on a stale prior"
    ladder = next(no for no, s in enumerate(src, 1) if s.startswith("BOOST") and src[no - 2] == "BOUND 1" and src[no - 3].startswith("SET " + hexf(100.0)))
    assert res[ladder].split()[3] == f"s{far}" and res[ladder].endswith("complete 1")
    r = subprocess.run([exe, str(tmp_path / "cpp"), str(tmp_path / "vectors.bin"), str(tmp_path / "script.txt")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want) == len(src)
    for no, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, f"line {no}: {src[no - 1][:120]}\n  C++    {g[:300]}\n  Python {w[:300]}"
