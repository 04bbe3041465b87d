"""Filters from row attributes (mx_filter_set_where / set_keys / combine / invert) on the headline corpus (bench.py's
10M x 384 Gaussian rows, int8 filter copy).  Every row carries a prior value uniform in [0, 1) and the key of its 70-row document.
Each predicate edit -- set_where selecting 1 %, 50 % and 100 % of the rows, set_keys with 300 and 100k keys -- is timed beside the
only route there was before for the same set, in the same run: the ids computed in NumPy from a HOST copy of the column (a copy the
library does not keep), handed to set_ids; the host-side selection and the set_ids call are timed separately.  Then combine (the
four ops) and invert, and a search through a predicate-built filter beside a search through the same set built by set_ranges, twice (two handles: what
equal bitmaps differ by): the bitmaps are identical, so all three must cost the same.  One JSON line per case; --out also writes them to a file.

  python scripts/bench_filter_where.py [--rows 10000000] [--dim 384] [--steps 10] [--warmup 2] [--out profiles/filter_where_10Mx384.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MEMEX_HIP_SPIN", "1")  # as bench.py: the benchmark owns its core

DOC = 70


def timed(call, steps, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    import numpy as np
    import torch
    from bench import fill_index, make_queries
    from memex_amd.index import FlatIndex
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, k = a.rows, a.k
    rng = np.random.default_rng(0)
    sink = open(a.out, "w") if a.out else None

    def report(case, ms, extra=None):
        rec = {"case": case, "dim": a.dim, "rows": n, "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
               "ms_mean": round(statistics.mean(ms), 4)}
        rec.update(extra or {})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    with FlatIndex(a.dim) as idx, idx.make_prior() as pri, idx.make_grouping() as grp:
        idx.set_filter_copy("i8")
        fill_index(idx, n, a.dim, 0, n, "gaussian")
        vals = rng.random(n, dtype=np.float32)                         # the host copy only the old route needs
        n_docs = (n + DOC - 1) // DOC
        keys = (np.arange(n, dtype=np.uint32) // DOC) + 1
        for lo in range(0, n, 1 << 20):
            hi = min(lo + (1 << 20), n)
            pri.set_ids(np.arange(lo + 1, hi + 1, dtype=np.uint64), vals[lo:hi])
        starts = np.arange(0, n, DOC, dtype=np.uint64)
        grp.set_ranges(np.stack([starts + 1, np.minimum(starts + DOC, n) + 1], 1), np.arange(1, n_docs + 1, dtype=np.uint32))

        def edits(case, device_edit, host_select, extra):
            with idx.make_filter() as flt:
                sel = device_edit(flt)
                want = flt.ranges()
                report(case + ": on the device", timed(lambda: device_edit(flt), a.steps, a.warmup), dict(extra, selected=sel))
            ids = host_select()
            assert ids.size == sel, (case, ids.size, sel)
            report(case + ": old route, host selection (NumPy on a host copy)", timed(host_select, max(a.steps // 2, 3), 1),
                   dict(extra, selected=sel))
            with idx.make_filter() as flt:
                report(case + ": old route, set_ids of the selected ids", timed(lambda: flt.allow(ids=ids), max(a.steps // 2, 3), 1),
                       dict(extra, selected=sel, id_bytes=int(ids.nbytes)))
                assert np.array_equal(flt.ranges(), want), case         # the two routes build the same set

        for share, lo in (("1%", 0.99), ("50%", 0.5), ("100%", 0.0)):
            edits(f"set_where {share}", lambda f, lo=lo: f.allow_where(pri, lo, 1.0),
                  lambda lo=lo: (np.flatnonzero((np.float32(lo) <= vals) & (vals <= np.float32(1.0))) + 1).astype(np.uint64), {"lo": lo})
        for m in (300, 100_000):
            wanted = (rng.choice(n_docs, m, replace=False) + 1).astype(np.uint32)
            edits(f"set_keys {m} keys", lambda f, w=wanted: f.allow_keys(grp, w),
                  lambda w=wanted: (np.flatnonzero(np.isin(keys, w)) + 1).astype(np.uint64), {"keys": m})

        with idx.make_filter() as fa, idx.make_filter() as fb, idx.make_filter() as out:
            fa.allow_where(pri, 0.25, 0.75)
            fb.allow_keys(grp, np.arange(1, n_docs + 1, 2, dtype=np.uint32))
            for op in ("and", "or", "andnot", "xor"):
                report(f"combine {op}", timed(lambda: idx.combine_filters(fa, fb, op, out=out), a.steps, a.warmup))
            report("invert", timed(out.invert, a.steps, a.warmup))

        # a search through a predicate-built filter against the same set built by set_ranges
        q256 = make_queries(256, a.dim, "gaussian")
        outs = {B: (torch.zeros((B, k), dtype=torch.int64, device="cuda"), torch.zeros((B, k), dtype=torch.float32, device="cuda"),
                    torch.zeros((B, k), dtype=torch.float32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"))
                for B in (1, 256)}

        def search_ms(flt, B):
            def call():
                idx.search_with_device(flt, q256[:B], k, *outs[B])
                torch.cuda.synchronize()
            return timed(call, 3 * a.steps, a.warmup)

        wanted = (rng.choice(n_docs, 300, replace=False) + 1).astype(np.uint32)
        for case, build in (("1% by set_where", lambda f: f.allow_where(pri, 0.99, 1.0)), ("300 documents by set_keys", lambda f: f.allow_keys(grp, wanted))):
            with idx.make_filter() as fw:
                build(fw)
                # two handles by set_ranges: what two filters of equal words differ by is the yardstick for the third
                with idx.make_filter(ranges=fw.ranges()) as fr, idx.make_filter(ranges=fw.ranges()) as fr2:
                    trio = [("predicate-built", fw), ("the same set by set_ranges", fr), ("the same set by set_ranges, a second handle", fr2)]
                    for rnd in range(3):  # the order rotates: whichever comes first after a change of batch size is timed on other clocks
                        for B in (256, 1):
                            for pos, (how, flt) in enumerate(trio[rnd:] + trio[:rnd]):
                                report(f"search, {case}, {how} (round {rnd + 1})", search_ms(flt, B), {"batch": B, "k": k, "timed": pos + 1})
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
