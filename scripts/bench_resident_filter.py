"""Per-call against resident filters (mx_filter) on the headline corpus (bench.py's 10M x 384 Gaussian rows, int8
filter copy, top-10).  The cases of the section 3.8 table -- 1 % of the rows contiguous, 1 % scattered (about 99k ranges), a 70-row
document, 16384 scattered rows -- each as a per-call filter (mx_index_search_filtered_device) and as a resident one
(mx_index_search_with_filter_device) at B = 1 and B = 256; beside them the unfiltered call and the filter covering every id
(the masked scan with no set-up: the yardstick of a resident scattered filter), twice each so that their spread shows; and what
building and editing cost: create + set_ranges of the 99k-range filter, set_ids of 100k ids, one allow of a 70-id document.
The last lines time the host stages of the per-call scattered filter on their own (sorting the ranges; uploading them from
pageable memory), to set beside the whole call.  One JSON line per case; --out also writes them to a file.

  python scripts/bench_resident_filter.py [--rows 10000000] [--dim 384] [--steps 30] [--warmup 5] [--out profiles/resident_filter_10Mx384.txt]
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


def timed(call, steps, warmup):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
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
    from memex_amd.index import FlatIndex, ids_to_ranges
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, k = a.rows, a.k
    rng = np.random.default_rng(0)
    q256 = make_queries(256, a.dim, "gaussian")
    out = {B: (torch.zeros((B, k), dtype=torch.int64, device="cuda"), torch.zeros((B, k), dtype=torch.float32, device="cuda"),
               torch.zeros((B, k), dtype=torch.float32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"))
           for B in (1, 256)}
    sink = open(a.out, "w") if a.out else None

    def report(case, B, ms, extra=None):
        med = statistics.median(ms)
        rec = {"case": case, "dim": a.dim, "rows": n, "batch": B, "k": k, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
               "ms_mean": round(statistics.mean(ms), 4)}
        rec.update(extra or {})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        return med

    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy("i8")
        fill_index(idx, n, a.dim, 0, n, "gaussian")
        one = n // 100
        lo = int(rng.integers(1, n - one))
        scattered = ids_to_ranges(rng.choice(n, one, replace=False) + 1)
        every = np.array([[1, n + 1]], dtype=np.uint64)
        cases = [("1% contiguous", np.array([[lo, lo + one]], dtype=np.uint64)),
                 ("1% scattered", scattered),
                 ("70-row document", np.array([[lo, lo + 70]], dtype=np.uint64)),
                 ("16384 scattered", ids_to_ranges(rng.choice(n, 16384, replace=False) + 1))]
        with idx.make_filter(ranges=every) as f_every:
            for rnd in range(3):  # the yardsticks, three times over the run: their spread is the noise a comparison has to clear
                for B in (256, 1):
                    q = q256[:B]
                    report(f"unfiltered (round {rnd + 1})", B, timed(lambda: idx.search_device(q, k, *out[B]), a.steps, a.warmup))
                    report(f"every id, per-call (round {rnd + 1})", B,
                           timed(lambda: idx.search_filtered_device(q, k, *out[B], ranges=every), a.steps, a.warmup))
                    report(f"every id, resident (round {rnd + 1})", B,
                           timed(lambda: idx.search_with_device(f_every, q, k, *out[B]), a.steps, a.warmup))
                if rnd == 0:
                    for name, r in cases:
                        with idx.make_filter(ranges=r) as flt:
                            for B in (256, 1):
                                q = q256[:B]
                                idx.reset_stats()
                                report(f"{name}, per-call", B,
                                       timed(lambda: idx.search_filtered_device(q, k, *out[B], ranges=r), a.steps, a.warmup),
                                       {"ranges": int(r.shape[0])})
                                idx.reset_stats()
                                report(f"{name}, resident", B, timed(lambda: idx.search_with_device(flt, q, k, *out[B]), a.steps, a.warmup),
                                       {"ranges": int(r.shape[0]),
                                        "subset_share": round(idx.stats().subset_queries / max(idx.stats().filtered_queries, 1), 3)})
        # building and editing
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            flt = idx.make_filter(ranges=scattered)
            ms.append((time.perf_counter() - t0) * 1e3)
            flt.close()
        report("create + set_ranges, 1% scattered", 0, ms, {"ranges": int(scattered.shape[0])})
        ids100k = (rng.choice(n, 100_000, replace=False) + 1).astype(np.uint64)
        doc = np.arange(lo, lo + 70, dtype=np.uint64)
        with idx.make_filter() as flt:
            report("set_ids, 100k ids", 0, timed(lambda: flt.allow(ids=ids100k), 5, 1), {"ids": 100_000})
            report("allow of a 70-id document", 0, timed(lambda: flt.allow(ids=doc), a.steps, a.warmup), {"ids": 70})
            report("count() after an edit", 0, timed(lambda: (flt.deny(ids=doc[:1]), flt.count()), 5, 1))
            report("ranges() of 100k scattered ids", 0, timed(flt.ranges, 5, 1))
        # the per-call scattered filter's host stages, timed apart from the call (what the library does before its first launch)
        flat = np.ascontiguousarray(scattered.reshape(-1))
        dev = torch.zeros(flat.size, dtype=torch.int64, device="cuda")

        def normalise():
            r = scattered[np.argsort(scattered[:, 0], kind="stable")]
            return r[r[:, 0] < r[:, 1]]

        def upload():
            dev.copy_(torch.from_numpy(flat.view(np.int64)))   # pageable host memory, as the library's upload
            torch.cuda.synchronize()

        report("stage: sort of 99k ranges (host, NumPy)", 0, timed(normalise, a.steps, a.warmup))
        report("stage: upload of 99k ranges from pageable memory", 0, timed(upload, a.steps, a.warmup), {"bytes": int(flat.nbytes)})
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
