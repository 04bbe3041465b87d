"""Cost of a search by stored row (mx_index_search_by_id / mx_index_search_range_by_id) on the headline corpus (bench.py's 10M x 384
Gaussian rows, int8 filter copy), host-pointer calls throughout because the route it replaces is a host route:

  top-k   search_by_id(k = 10) at B = 1 and B = 256 against get_rows + search(k = 11) of the same run (a block of consecutive ids, so the
          old route fetches its rows in ONE get_rows call: its best case)
  range   search_range_by_id at each query's own 10th-best score against the plain search_range call on the fetched rows
  join    a near_duplicates pass over the first --dup-rows ids in blocks of 512: ms per block split into the device call and the host's
          pair handling, and the pass extrapolated to the collection

Prints one JSON line per case (median and mean milliseconds per call).

  python scripts/bench_by_id.py [--rows 10000000] [--dim 384] [--steps 30] [--warmup 5] [--dup-rows 1000000] [--dup-score 0.9]
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
    from bench import fill_index
    from memex_amd.index import FlatIndex
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dup-rows", type=int, default=1_000_000)
    ap.add_argument("--dup-score", type=float, default=0.9)
    a = ap.parse_args()

    def report(case, B, ms, extra=None):
        rec = {"case": case, "rows": a.rows, "dim": a.dim, "batch": B, "ms_median": round(statistics.median(ms), 4),
               "ms_mean": round(statistics.mean(ms), 4)}
        rec.update(extra or {})
        print(json.dumps(rec), flush=True)
        return statistics.median(ms)

    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy("i8")
        fill_index(idx, a.rows, a.dim, 0, a.rows, "gaussian")
        for B in (1, 256):
            first = a.rows // 3                                         # a block of consecutive ids in the middle of the corpus
            q = np.arange(first + 1, first + 1 + B, dtype=np.uint64)
            by_id = report("search_by_id k = 10", B, timed(lambda: idx.search_by_id(q, 10), a.steps, a.warmup))
            old = report("get_rows + search k = 11", B, timed(lambda: idx.search(idx.get_rows(first, B), 11), a.steps, a.warmup))
            print(json.dumps({"top_k_ratio_to_old_route": round(by_id / old, 4), "batch": B}), flush=True)
            thr = idx.search_by_id(q, 10)[1][:, 9].copy()               # the query's 10th-best other row: 10 rows in range
            by_id = report("search_range_by_id cap = 16", B, timed(lambda: idx.search_range_by_id(q, thr, 16), a.steps, a.warmup))
            rows = idx.get_rows(first, B)
            plain = report("search_range cap = 17 (rows on the host)", B, timed(lambda: idx.search_range(rows, thr, 17), a.steps, a.warmup))
            old = report("get_rows + search_range cap = 17", B, timed(lambda: idx.search_range(idx.get_rows(first, B), thr, 17), a.steps, a.warmup))
            print(json.dumps({"range_ratio_to_plain_call": round(by_id / plain, 4), "range_ratio_to_old_route": round(by_id / old, 4),
                              "batch": B}), flush=True)
        # the self-join, block by block as near_duplicates walks it, the device call and the host's pair handling timed apart
        n = min(a.dup_rows, a.rows)
        dev_ms, host_ms, pairs, cut = [], [], 0, 0
        t_all = time.perf_counter()
        for lo in range(0, n, 512):
            q = np.arange(lo + 1, min(lo + 512, n) + 1, dtype=np.uint64)
            t0 = time.perf_counter()
            ids, scores, _, nf, nr = idx.search_range_by_id(q, a.dup_score, 64)
            t1 = time.perf_counter()
            listed = np.arange(ids.shape[1])[None, :] < nf[:, None]
            own, other = np.broadcast_to(q[:, None], ids.shape)[listed], ids[listed]
            lo_id, hi_id, s = np.minimum(own, other), np.maximum(own, other), scores[listed]
            order = np.lexsort((hi_id, lo_id))
            pairs += int(s[order].size)
            cut += int((nr > 64).sum())
            t2 = time.perf_counter()
            dev_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
        total_s = time.perf_counter() - t_all
        blocks = len(dev_ms)
        print(json.dumps({"case": "near_duplicates pass", "ids": n, "min_score": a.dup_score, "per_row": 64, "blocks": blocks,
                          "ms_per_block_device_median": round(statistics.median(dev_ms), 4),
                          "ms_per_block_host_median": round(statistics.median(host_ms), 4),
                          "pass_s": round(total_s, 3), "listed_entries": pairs, "truncated": cut,
                          "collection_s_extrapolated": round(total_s * a.rows / n, 1)}), flush=True)


if __name__ == "__main__":
    main()
