"""Cost of the dead-row mask on the headline search (bench.py's 10M x 384 Gaussian corpus, batches of 256 queries, top-10,
int8 filter copy; --copy / --dim / --rows measure the other scans): the same index with nothing removed (the kernels without the mask), with 1 % of the rows removed at
random, and with 10 % removed in contiguous runs of 1000 rows (the masked scan8_kernel / finish_kernel), then with nothing removed
once more.  Prints one JSON line
per case: median and mean milliseconds per 256-query step, queries per second, and the slowdown against the first unmasked run.

  python scripts/bench_removed.py [--rows 10000000] [--dim 384] [--copy i8|bf16|none] [--steps 50] [--warmup 10]
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


def run(idx, q, k, steps, warmup):
    import torch
    B = q.shape[0]
    ids = torch.zeros((B, k), dtype=torch.int64, device="cuda")
    sc = torch.zeros((B, k), dtype=torch.float32, device="cuda")
    di = torch.zeros((B, k), dtype=torch.float32, device="cuda")
    nf = torch.zeros(B, dtype=torch.int32, device="cuda")
    for _ in range(warmup):
        idx.search_device(q, k, ids, sc, di, nf)
    torch.cuda.synchronize()
    idx.reset_stats()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        idx.search_device(q, k, ids, sc, di, nf)
        ms.append((time.perf_counter() - t0) * 1e3)
    st = idx.stats()
    return ms, st, ids.cpu().numpy().astype("uint64")


def main():
    import numpy as np
    from bench import fill_index, make_queries
    from memex_amd.index import FlatIndex
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--copy", choices=["i8", "bf16", "none"], default="i8",
                    help="filter copy the scan streams: int8 (scan8_kernel), bf16 (scan16_kernel; scan16w_kernel above 768 dims), none (scan_kernel)")
    a = ap.parse_args()
    q = make_queries(a.batch, a.dim, "gaussian")
    rng = np.random.default_rng(0)
    n = a.rows
    cases = [("none", None), ("1% random", lambda: rng.choice(n, n // 100, replace=False)),
             ("10% in runs of 1000", lambda: (rng.choice(n // 1000, n // 10000, replace=False)[:, None] * 1000 + np.arange(1000)).ravel()),
             ("none, again", None)]  # (the scan runs at the package power cap: a second unmasked run after the masked ones shows the drift)
    base = None
    for name, pick in cases:
        with FlatIndex(a.dim) as idx:
            idx.set_filter_copy(False if a.copy == "none" else a.copy)
            fill_index(idx, n, a.dim, 0, n, "gaussian")
            removed = np.zeros(0, dtype=np.int64)
            if pick is not None:
                removed = np.asarray(pick(), dtype=np.int64)
                idx.remove(removed + 1)
            ms, st, ids = run(idx, q, a.k, a.steps, a.warmup)
            assert not np.isin(ids, removed + 1).any(), "a removed id was returned"
            med = statistics.median(ms)
            base = med if base is None else base
            print(json.dumps({"case": name, "copy": a.copy, "dim": a.dim, "rows": n, "removed": int(idx.removed), "batch": a.batch, "k": a.k,
                              "ms_median": round(med, 4), "ms_mean": round(statistics.mean(ms), 4),
                              "qps": round(a.batch / (med / 1e3), 1), "vs_none": round(med / base, 4),
                              "fallback_queries": int(st.fallback_queries), "retry_queries": int(st.retry_queries),
                              "candidates_per_query": round(st.candidates / max(st.queries, 1), 1)}), flush=True)


if __name__ == "__main__":
    main()
