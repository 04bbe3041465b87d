"""Cost of a diversified search (mx_index_search_mmr) on the headline corpus (bench.py's 10M x 384 Gaussian rows, int8 filter copy), at
B = 256 and B = 1, k = 10.  For fetch in {32, 100, 256} the MMR call is timed against the plain search(k = fetch) call of the same run:
the difference is what the selection stage costs (candidate lists to the host, the gather of the candidates' rows, mmr_select_kernel).
Also fetch = 1024 with k = 64, whose candidate stage runs on the EXACT path.  Prints one JSON line per case (median and mean
milliseconds per call) and one per difference.

  python scripts/bench_mmr.py [--rows 10000000] [--dim 384] [--steps 30] [--warmup 5] [--lam 0.5]
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lam", type=float, default=0.5)
    a = ap.parse_args()

    def zeros(*shape, dt=torch.float32):
        return torch.zeros(shape, dtype=dt, device="cuda")

    def outs(B, k):
        return zeros(B, k, dt=torch.int64), zeros(B, k), zeros(B, k), zeros(B, dt=torch.int32)

    def report(case, B, ms, extra):
        rec = {"case": case, "rows": a.rows, "dim": a.dim, "batch": B, "ms_median": round(statistics.median(ms), 4),
               "ms_mean": round(statistics.mean(ms), 4)}
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        return statistics.median(ms)

    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy("i8")
        fill_index(idx, a.rows, a.dim, 0, a.rows, "gaussian")
        for B in (256, 1):
            q = make_queries(B, a.dim, "gaussian")
            for k, fetch, steps, warmup in ((10, 32, a.steps, a.warmup), (10, 100, a.steps, a.warmup), (10, 256, a.steps, a.warmup),
                                            (64, 1024, 3, 1)):
                o = outs(B, fetch)
                plain = report(f"search k = {fetch}", B, timed(lambda: idx.search_device(q, fetch, *o), steps, warmup), {"k": fetch})
                o = outs(B, k)
                mmr = report(f"mmr k = {k}, fetch = {fetch}", B,
                             timed(lambda: idx.search_mmr_device(q, k, *o, fetch=fetch, lam=a.lam), steps, warmup),
                             {"k": k, "fetch": fetch, "lam": a.lam})
                print(json.dumps({"selection_ms": round(mmr - plain, 4), "batch": B, "k": k, "fetch": fetch,
                                  "ratio_to_plain": round(mmr / plain, 4)}), flush=True)


if __name__ == "__main__":
    main()
