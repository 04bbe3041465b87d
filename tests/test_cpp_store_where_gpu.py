"""The C++ store mirror's filters from row attributes (include/memex_hip.hpp: Filter::allow_where / deny_where / allow_documents /
deny_documents / invert, HipFlatStore::combine_filters) against the Python mirror and a dict model, as
tests/test_cpp_store_features_gpu.py holds the older methods.

One scripted driver process per scenario (tests/cpp/test_store_where.cpp).  The same script is replayed on memex_amd/storage.py; the
two outputs must be equal line by line -- _id strings and f32 score bits, no tolerance -- and the count lines (n_selected, allowed,
live) must be what a dict model of the store says."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 40                                                            # padded inside the library
OPS = ("and", "or", "andnot", "xor")


def hexf(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def scenario(mode):
    """-> (pool f32 [n, D], script, expected count lines {line number: text after "R <no>"})"""
    rng = np.random.default_rng(1800 + len(mode))
    n_docs = 40
    segs, doc_of, stamp = [], {}, {}
    for i in range(n_docs):
        for j in range(int(rng.integers(1, 7))):
            s = f"d{i:02d}s{j}"
            segs.append(s)
            doc_of[s] = f"doc{i:02d}"
    for i in range(n_docs):
        stamp[f"doc{i:02d}"] = float(rng.choice([0.0, -0.0, 0.25, 1.0, 1.0, 2.0, 4.0])) if i < 32 else None   # the last eight: never set
    pool = rng.standard_normal((len(segs) + 4, D)).astype(np.float32)
    value = {s: np.float32(stamp[doc_of[s]] or 0.0) for s in segs}
    lines, want = [], {}
    alive = set(segs)
    sets = {}

    def add(ln, expect=None):
        lines.append(ln)
        if expect is not None:
            want[len(lines)] = expect

    def count(name):
        add(f"COUNT {name}", f"{len(sets[name])} {len(sets[name] & alive)}")

    add(f"OPEN {mode}")
    add("INSERT " + " ".join(f"{s}:{i}" for i, s in enumerate(segs)), str(len(segs)))
    for doc, v in stamp.items():
        if v is not None:
            add(f"PRIOR {hexf(v)} " + " ".join(s for s in segs if doc_of[s] == doc))
    for i in range(n_docs - 4):                                   # the last four documents stay ungrouped
        doc = f"doc{i:02d}"
        add(f"GROUP {doc} " + " ".join(s for s in segs if doc_of[s] == doc))
    grouped = {f"doc{i:02d}" for i in range(n_docs - 4)}
    gone = [segs[3], segs[40], segs[41]]
    add("REMOVE " + " ".join(gone), "3")
    alive -= set(gone)

    def where(name, allow, lo, hi):
        sel = {s for s in segs if np.float32(lo) <= value[s] <= np.float32(hi)}
        sets[name] = (sets[name] | sel) if allow else (sets[name] - sel)
        add(f"WHERE {name} {'allow' if allow else 'deny'} {hexf(lo)} {hexf(hi)}", str(len(sel)))

    def docs(name, allow, names):
        sel = {s for s in segs if doc_of[s] in names and doc_of[s] in grouped}
        sets[name] = (sets[name] | sel) if allow else (sets[name] - sel)
        add(f"DOCS {name} {'allow' if allow else 'deny'} " + " ".join(names), str(len(sel)))

    for name in ("recent", "chosen", "out"):
        add(f"FILTER {name}", "0")
        sets[name] = set()
    where("recent", True, 1.0, np.inf)
    count("recent")
    add(f"IN {len(segs)} 200 recent")
    where("recent", False, 4.0, 4.0)
    where("recent", True, 0.0, 0.0)                              # +0.0, -0.0 and the segments nobody stamped
    where("recent", True, 3.0, 2.0)                              # lo > hi: nothing
    count("recent")
    add(f"IN {len(segs) + 1} 10 recent")
    docs("chosen", True, ["doc03", "doc17", "doc03", "nobody", "doc38", "doc20"])   # unknown, repeated, ungrouped names
    docs("chosen", True, ["nobody", "nothing"])
    docs("chosen", False, ["doc17"])
    count("chosen")
    add(f"IN {len(segs) + 2} 200 chosen")
    for code, op in enumerate(OPS):
        a, b = sets["recent"], sets["chosen"]
        sets["out"] = {"and": a & b, "or": a | b, "andnot": a - b, "xor": a ^ b}[op]
        add(f"COMBINE out recent chosen {code}", "0")
        count("out")
        add(f"IN {len(segs) + 3} 200 out")
        sets["n" + op] = set(sets["out"])
        add(f"COMBINE +n{op} recent chosen {code}", "0")
        count("n" + op)
    sets["chosen"] = sets["recent"] | sets["chosen"]
    add("COMBINE chosen recent chosen 1", "0")                    # out is b
    count("chosen")
    sets["chosen"] = set(segs) - sets["chosen"]
    add("INVERT chosen", "0")
    count("chosen")
    add(f"IN {len(segs)} 200 chosen")
    add("INVERT chosen", "0")
    sets["chosen"] = set(segs) - sets["chosen"]
    count("chosen")
    lines.append("COMBINE out recent chosen 7")                  # an op outside the enum
    lines.append(f"WHERE recent allow {hexf(np.nan)} {hexf(1.0)}")
    count("out")
    count("recent")
    return pool, "\n".join(lines) + "\n", want


def python_replay(pool, script, work):
    """the script on memex_amd.storage.HipFlatStore -> the driver's lines"""
    from memex_amd import storage
    st, pri, grp, filters, out = None, None, None, {}, []
    f32 = lambda t: float(np.array([int(t, 16)], np.uint32).view(np.float32)[0])  # noqa: E731
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
            elif op == "PRIOR":
                pri = pri or st.make_prior()
                pri.set_document(a[1:], f32(a[0]))
                res = str(len(a) - 1)
            elif op == "GROUP":
                grp = grp or st.make_grouping()
                grp.assign(a[0], a[1:])
                res = str(len(a) - 1)
            elif op == "FILTER":
                filters[a[0]] = st.make_filter()
            elif op == "WHERE":
                f = filters[a[0]]
                res = str((f.allow_where if a[1] == "allow" else f.deny_where)(pri, f32(a[2]), f32(a[3])))
            elif op == "DOCS":
                f = filters[a[0]]
                res = str((f.allow_documents if a[1] == "allow" else f.deny_documents)(grp, a[2:]))
            elif op == "INVERT":
                filters[a[0]].invert()
            elif op == "COMBINE":
                if a[0].startswith("+"):
                    filters[a[0][1:]] = st.combine_filters(filters[a[1]], filters[a[2]], int(a[3]))
                else:
                    st.combine_filters(filters[a[1]], filters[a[2]], int(a[3]), out=filters[a[0]])
            elif op == "COUNT":
                res = "%d %d" % filters[a[0]].count()
            elif op == "IN":
                hits = st.search_in(pool[int(a[0])], int(a[1]), filters[a[2]])
                res = " ".join([str(len(hits))] + [f"{n} {hexf(s)}" for n, s in hits])
            else:
                raise AssertionError(ln)
            out.append(f"R {no} {res}")
        except storage.SearchError:
            out.append(f"E {no} SearchError")
    for f in filters.values():
        f.close()
    for h in (pri, grp):
        if h:
            h.close()
    st.delete_all()
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory, lib_built):
    exe = str(tmp_path_factory.mktemp("store_where") / "test_store_where")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_store_where.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "memex_amd"), "-lmemex_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "memex_amd")])
    return exe


@pytest.mark.parametrize("mode", ["plain", "sharded"])
def test_cpp_filters_from_attributes_against_python_and_the_model(mode, driver, tmp_path):
    pool, script, want = scenario(mode)
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
            assert c == f"R {no} {want[no]}", f"line {no}: {src[no - 1][:80]}: the model says {want[no]}"
    assert cpp[-4] == f"E {len(src) - 3} SearchError" and cpp[-3] == f"E {len(src) - 2} SearchError"
    searched = [c for c, s in zip(cpp, src) if s.startswith("IN ")]
    assert len(searched) == 8 and sum(int(c.split()[2]) > 0 for c in searched) >= 5
