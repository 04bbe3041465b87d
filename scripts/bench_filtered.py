"""Cost of a filtered search (mx_index_search_filtered) on the headline corpus (bench.py's 10M x 384 Gaussian rows, int8 filter
copy, top-10): unfiltered against a filter covering every id (the masked kernels' overhead), one contiguous range of 1 % of the
rows, 1 % of the rows scattered at random (the masked scan over the whole span), a 70-row document (the subset kernel) at B = 1
and B = 256, and the switch point between the two paths: m allowed rows (contiguous or scattered over the collection) at B = 1
and 256, each on the masked pipeline (MEMEX_HIP_DEBUG=filt_subset=0) and on the subset kernel (filt_subset=1).  Prints one JSON
line per case: median and mean milliseconds per call, queries per second and the ratio to the unfiltered step.

  python scripts/bench_filtered.py [--rows 10000000] [--dim 384] [--copy i8|bf16|none] [--steps 30] [--warmup 5]
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
    ap.add_argument("--copy", choices=["i8", "bf16", "none"], default="i8")
    a = ap.parse_args()
    n, k = a.rows, a.k
    rng = np.random.default_rng(0)
    q256 = make_queries(256, a.dim, "gaussian")
    out = {B: (torch.zeros((B, k), dtype=torch.int64, device="cuda"), torch.zeros((B, k), dtype=torch.float32, device="cuda"),
               torch.zeros((B, k), dtype=torch.float32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"))
           for B in (1, 256)}
    base = {}

    def report(case, B, ms, idx, extra=None):
        st = idx.stats()
        med = statistics.median(ms)
        rec = {"case": case, "copy": a.copy, "dim": a.dim, "rows": n, "batch": B, "k": k, "ms_median": round(med, 4),
               "ms_mean": round(statistics.mean(ms), 4), "qps": round(B / (med / 1e3), 1)}
        if B in base:
            rec["vs_unfiltered"] = round(med / base[B], 4)
        rec["subset_share"] = round(st.subset_queries / max(st.filtered_queries, 1), 3)
        rec.update(extra or {})
        print(json.dumps(rec), flush=True)
        return med

    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy(False if a.copy == "none" else a.copy)
        fill_index(idx, n, a.dim, 0, n, "gaussian")

        def plain(B):
            q = q256[:B]
            return lambda: idx.search_device(q, k, *out[B])

        def filt(B, r):
            q = q256[:B]
            return lambda: idx.search_filtered_device(q, k, *out[B], ranges=r)

        every = np.array([[1, n + 1]], dtype=np.uint64)
        # unfiltered and all-ids in alternating rounds (the scan runs at the package power cap: drift shows as the spread)
        for rnd in range(2):
            for B in (256, 1):
                idx.reset_stats()
                m = report(f"unfiltered (round {rnd + 1})", B, timed(plain(B), a.steps, a.warmup), idx)
                if rnd == 0:
                    base[B] = m
                idx.reset_stats()
                report(f"filter covering all ids (round {rnd + 1})", B, timed(filt(B, every), a.steps, a.warmup), idx)
        one = n // 100
        lo = int(rng.integers(1, n - one))
        cases = [("1% contiguous", np.array([[lo, lo + one]], dtype=np.uint64)),
                 ("1% scattered", ids_to_ranges(rng.choice(n, one, replace=False) + 1)),
                 ("70-row document", np.array([[lo, lo + 70]], dtype=np.uint64))]
        for name, r in cases:
            for B in (256, 1):
                idx.reset_stats()
                report(name, B, timed(filt(B, r), a.steps, a.warmup), idx, {"ranges": int(r.shape[0])})
        # switch point: the same filters forced onto either path
        for m in (70, 1024, 4096, 16384):
            layouts = [("contiguous", np.array([[lo, lo + m]], dtype=np.uint64)),
                       ("scattered", ids_to_ranges(rng.choice(n, m, replace=False) + 1))]
            for layout, r in layouts:
                for B in (1, 256):
                    for force in (0, 1):
                        os.environ["MEMEX_HIP_DEBUG"] = f"filt_subset={force}"
                        idx.reset_stats()
                        report(f"switch: {m} rows {layout}, {'subset kernel' if force else 'masked pipeline'}", B,
                               timed(filt(B, r), a.steps, a.warmup), idx, {"m": m})
                        del os.environ["MEMEX_HIP_DEBUG"]


if __name__ == "__main__":
    main()
