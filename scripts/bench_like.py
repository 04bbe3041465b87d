"""Cost of a search by examples (mx_index_search_like) on the headline corpus (bench.py's 10M x 384 Gaussian rows, int8 filter copy):
R requests of m = 8 examples each (five positive, three negative, ids spread over the corpus), k = 10, against the plain
search(k + m) call over the requests' own combined vectors in the same run -- the pass search_like runs inside, so the difference is what
the gather, the blend, the drop kernel and their uploads add.  Host-pointer calls throughout.  Cases: R = 1 and R = 32.

Prints one JSON line per case (median and mean milliseconds per call).

  python scripts/bench_like.py [--rows 10000000] [--dim 384] [--steps 30] [--warmup 5] [--m 8] [--k 10]
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
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args()

    def report(case, R, ms):
        print(json.dumps({"case": case, "rows": a.rows, "dim": a.dim, "requests": R, "m": a.m, "k": a.k,
                          "ms_median": round(statistics.median(ms), 4), "ms_mean": round(statistics.mean(ms), 4)}), flush=True)
        return statistics.median(ms)

    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy("i8")
        fill_index(idx, a.rows, a.dim, 0, a.rows, "gaussian")
        rng = np.random.default_rng(77)
        n_pos = a.m - a.m * 3 // 8
        w = np.array([0.75 / n_pos] * n_pos + [-0.15 / max(a.m - n_pos, 1)] * (a.m - n_pos), dtype=np.float32)
        for R in (1, 32):
            ex = rng.choice(np.arange(1, a.rows + 1, dtype=np.uint64), (R, a.m), replace=False)
            got = idx.search_like(ex, a.k, w)
            assert (got[4] == a.m).all() and (got[3] == a.k).all()
            comb = got[5]
            like = report("search_like", R, timed(lambda: idx.search_like(ex, a.k, w), a.steps, a.warmup))
            plain = report("search k + m (the combined vectors on the host)", R, timed(lambda: idx.search(comb, a.k + a.m), a.steps, a.warmup))
            print(json.dumps({"ratio_to_plain_call": round(like / plain, 4), "added_ms": round(like - plain, 4), "requests": R}), flush=True)


if __name__ == "__main__":
    main()
