"""Cost of a range search (mx_index_search_range) on the headline corpus (bench.py's 10M x 384 Gaussian rows, int8 filter copy,
B = 256).  Each query's threshold is its own 10th-, 100th- or 1000th-best score, taken from top-k runs in the same process; the
top-10 and top-1000 calls of that run are timed beside the range calls.  Also: a cone-shaped corpus (rows around a common
direction, as an encoder produces; its int8 copy is centred) at the 10th-best threshold, and the all-rows threshold -1, which
takes the EXACT range path.  Prints one JSON line per case: median and mean milliseconds per call, f32-rescored candidates per
query, quartiles of n_in_range, EXACT fallbacks; and the ratios to the top-k calls.

  python scripts/bench_range.py [--rows 10000000] [--dim 384] [--batch 256] [--steps 30] [--warmup 5] [--cone-rows 10000000]
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


def cone_rows(n: int, dim: int, seed: int):
    """rows around one unit axis: axis + Gaussian noise of norm ~0.6, times a random length"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    axis = torch.randn(dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(77))
    axis /= axis.norm()
    x = axis + torch.randn((n, dim), device="cuda", generator=g) * (0.6 / dim ** 0.5)
    return x * torch.empty((n, 1), device="cuda").uniform_(0.5, 2.0, generator=g)


def main():
    import numpy as np
    import torch
    from bench import BLOCK, fill_index, make_queries
    from memex_amd.index import FlatIndex
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cone-rows", type=int, default=10_000_000)
    a = ap.parse_args()
    B, n = a.batch, a.rows

    def zeros(*shape, dt=torch.float32):
        return torch.zeros(shape, dtype=dt, device="cuda")

    def report(case, idx, ms, extra=None, nr=None):
        st = idx.stats()
        med = statistics.median(ms)
        rec = {"case": case, "rows": int(len(idx)), "dim": a.dim, "batch": B, "ms_median": round(med, 4),
               "ms_mean": round(statistics.mean(ms), 4), "candidates_per_query": round(st.candidates / max(st.queries, 1), 1),
               "fallback_queries": int(st.fallback_queries), "queries": int(st.queries)}
        if nr is not None:
            qs = np.percentile(nr.cpu().numpy().astype(np.float64), [0, 25, 50, 75, 100])
            rec["n_in_range_quartiles"] = [int(v) for v in qs]
        rec.update(extra or {})
        print(json.dumps(rec), flush=True)
        return med

    def ratio(what, v):
        print(json.dumps({"ratio": what, "value": round(v, 4)}), flush=True)

    def topk(idx, q, k, steps, warmup, case):
        o = (zeros(B, k, dt=torch.int64), zeros(B, k), zeros(B, k), zeros(B, dt=torch.int32))
        idx.reset_stats()
        ms = timed(lambda: idx.search_device(q, k, *o), steps, warmup)
        return report(case, idx, ms, {"k": k}), o[1].cpu().numpy()

    def range_call(idx, q, t, cap, steps, warmup, case, extra=None):
        o = (zeros(B, cap, dt=torch.int64), zeros(B, cap), zeros(B, cap), zeros(B, dt=torch.int32), zeros(B, dt=torch.int64))
        idx.reset_stats()
        ms = timed(lambda: idx.search_range_device(q, t, cap, *o), steps, warmup)
        e = {"cap": cap}
        e.update(extra or {})
        return report(case, idx, ms, e, nr=o[4])

    q = make_queries(B, a.dim, "gaussian")
    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy("i8")
        fill_index(idx, n, a.dim, 0, n, "gaussian")
        k10, s10 = topk(idx, q, 10, a.steps, a.warmup, "search k = 10")
        k1000, s1000 = topk(idx, q, 1000, 3, 1, "search k = 1000 (EXACT path)")
        t10, t100, t1000 = s10[:, 9].copy(), s1000[:, 99].copy(), s1000[:, 999].copy()
        for cap in (10, 1024):
            m = range_call(idx, q, t10, cap, a.steps, a.warmup, "range at each query's 10th-best score")
            ratio(f"range (10th-best, cap {cap}) / search k = 10", m / k10)
        range_call(idx, q, t100, 1024, a.steps, a.warmup, "range at each query's 100th-best score")
        m = range_call(idx, q, t1000, 1024, a.steps, a.warmup, "range at each query's 1000th-best score")
        ratio("range (1000th-best, cap 1024) / search k = 1000", m / k1000)
        m = range_call(idx, q, np.full(B, -1.0, np.float32), 1024, 2, 1, "range at -1: every row (EXACT range path)")
        ratio("range (all rows) / search k = 10", m / k10)
    torch.cuda.empty_cache()
    if a.cone_rows > 0:
        with FlatIndex(a.dim) as idx:
            idx.reserve(a.cone_rows)
            for b0 in range(0, a.cone_rows, BLOCK):
                idx.add_device(cone_rows(min(BLOCK, a.cone_rows - b0), a.dim, 300 + b0 // BLOCK).contiguous())
            idx.set_filter_copy(False)
            idx.set_filter_copy("i8")                          # rebuilt from a populated cone: centred
            centred = int(idx.stats().filter_centred)
            qc = cone_rows(B, a.dim, 9).contiguous()
            kc10, sc10 = topk(idx, qc, 10, a.steps, a.warmup, "cone corpus: search k = 10")
            m = range_call(idx, qc, sc10[:, 9].copy(), 10, a.steps, a.warmup, "cone corpus: range at each query's 10th-best score",
                           {"centred": centred})
            ratio("cone corpus: range (10th-best, cap 10) / search k = 10", m / kc10)


if __name__ == "__main__":
    main()
