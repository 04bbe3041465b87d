"""Cost of scoring named rows (mx_index_score_ids) on the headline corpus (bench.py's 10M x 384 Gaussian rows, int8 filter copy),
host-pointer calls throughout because the routes it replaces are host routes.  For B in {1, 256} queries and m in {64, 1024} ids per
query (each query its own random ids), in the same run:

  score_ids      the call itself
  search         search(k = m): what a caller pays who wants m scored rows and has no say in WHICH rows (m = 1024 is the EXACT path)
  filter         per query: make_filter(ids) + search_with(k = m) + the filter's release -- the only way to hand a per-query candidate
                 set to the search entry points
  get_rows       per query: get_rows for each candidate id (one call per id: the ids are scattered) plus a host dot product; B = 256
                 with m = 1024 is skipped unless --all (262144 single-row copies)

Prints one JSON line per case (median and mean milliseconds per call) and the ratios to score_ids.

  python scripts/bench_score_ids.py [--rows 10000000] [--dim 384] [--steps 10] [--warmup 2] [--all]
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()

    def report(case, B, m, ms):
        print(json.dumps({"case": case, "rows": a.rows, "dim": a.dim, "batch": B, "m": m, "ms_median": round(statistics.median(ms), 4),
                          "ms_mean": round(statistics.mean(ms), 4)}), flush=True)
        return statistics.median(ms)

    rng = np.random.default_rng(5)
    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy("i8")
        fill_index(idx, a.rows, a.dim, 0, a.rows, "gaussian")
        for B in (1, 256):
            q = rng.standard_normal((B, a.dim)).astype(np.float32)
            for m in (64, 1024):
                ids = (rng.integers(0, a.rows, (B, m)) + 1).astype(np.uint64)

                def by_filter():
                    for b in range(B):
                        with idx.make_filter(ids=ids[b]) as f:
                            idx.search_with(f, q[b], m)

                def by_rows():
                    for b in range(B):
                        rows = np.concatenate([idx.get_rows(int(i) - 1, 1) for i in ids[b]])
                        rows @ q[b]

                own = report("score_ids", B, m, timed(lambda: idx.score_ids(q, ids), a.steps, a.warmup))
                other = {"search k = m": report("search k = m", B, m, timed(lambda: idx.search(q, m), a.steps, a.warmup)),
                         "filter per query": report("make_filter + search_with per query", B, m, timed(by_filter, a.steps, a.warmup))}
                if a.all or B * m <= 65536:
                    other["get_rows + host dot"] = report("get_rows + host dot product", B, m, timed(by_rows, max(a.steps // 5, 1), 1))
                print(json.dumps({"batch": B, "m": m, "ratio_to_score_ids": {k: round(v / own, 2) for k, v in other.items()}}), flush=True)


if __name__ == "__main__":
    main()
