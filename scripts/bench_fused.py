"""Cost of a fused search (mx_index_search_fused) on the headline corpus (bench.py's 10M x 384 Gaussian rows, int8 filter copy): R = 32
requests of m = 8 sub-queries, k = 10, with fetch = 10 and fetch = 64, both modes.  Each fused call is timed against the plain
search(k = fetch) call over the same R * m = 256 queries in the same run: the difference is what the fusion adds (the weights' upload
and fuse_kernel).  Prints one JSON line per case (median and mean milliseconds per call) and one per difference.

  python scripts/bench_fused.py [--rows 10000000] [--dim 384] [--requests 32] [--sub 8] [--steps 30] [--warmup 5]
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
    import torch
    from bench import fill_index, make_queries
    from memex_amd.index import FlatIndex
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--sub", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    R, m, k = a.requests, a.sub, 10

    def zeros(*shape, dt=torch.float32):
        return torch.zeros(shape, dtype=dt, device="cuda")

    def report(case, ms, extra):
        rec = {"case": case, "rows": a.rows, "dim": a.dim, "requests": R, "sub_queries": m, "ms_median": round(statistics.median(ms), 4),
               "ms_mean": round(statistics.mean(ms), 4)}
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        return statistics.median(ms)

    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy("i8")
        fill_index(idx, a.rows, a.dim, 0, a.rows, "gaussian")
        q = make_queries(R * m, a.dim, "gaussian")                        # [R * m, dim]; the fused call reads it as [R, m, dim]
        for fetch in (10, 64):
            o = (zeros(R * m, fetch, dt=torch.int64), zeros(R * m, fetch), zeros(R * m, fetch), zeros(R * m, dt=torch.int32))
            plain = report(f"search k = {fetch}", timed(lambda: idx.search_device(q, fetch, *o), a.steps, a.warmup), {"k": fetch})
            for mode in ("max", "rrf"):
                f = (zeros(R, k, dt=torch.int64), zeros(R, k), zeros(R, k), zeros(R, dt=torch.int32), zeros(R, k, dt=torch.int32),
                     zeros(R, k, dt=torch.float64))
                fused = report(f"fused {mode} k = {k}, fetch = {fetch}",
                               timed(lambda: idx.search_fused_device(q.view(R, m, a.dim), k, *f, mode=mode, fetch=fetch), a.steps, a.warmup),
                               {"k": k, "fetch": fetch, "mode": mode})
                print(json.dumps({"fusion_ms": round(fused - plain, 4), "mode": mode, "k": k, "fetch": fetch,
                                  "ratio_to_plain": round(fused / plain, 4)}), flush=True)


if __name__ == "__main__":
    main()
