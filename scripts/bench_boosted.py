"""Cost of a boosted search (mx_index_search_boosted) and of building its prior on the headline corpus (bench.py's 10M x 384 Gaussian
rows, int8 filter copy): priors uniform in [0, 1) set by ranges of 70 consecutive rows (142858 of them), 256 queries, k = 10, w = 0.05,
with fetch = 40 and fetch = 256.  Each boosted call is timed between two timings of the plain search(k = fetch) call over the same
queries in the same run: the difference to their mean is what the re-ranking adds (one H2D copy of the weights, one boost_rank_kernel
launch and a stream synchronise), and the difference between the two plain medians is the spread to read it against.  Also timed:
make_prior + set_ranges of all the ranges, and one set_ids of a document's 70 ids.  Prints one JSON line per case (median and mean
milliseconds per call) and the share of queries that came back complete.

  python scripts/bench_boosted.py [--rows 10000000] [--dim 384] [--queries 256] [--per-doc 70] [--weight 0.05] [--steps 30] [--warmup 5]
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
    from memex_amd.index import FlatIndex
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--per-doc", type=int, default=70)
    ap.add_argument("--weight", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    B, k = a.queries, 10

    def zeros(*shape, dt=torch.float32):
        return torch.zeros(shape, dtype=dt, device="cuda")

    def report(case, ms, extra):
        rec = {"case": case, "rows": a.rows, "dim": a.dim, "queries": B, "ms_median": round(statistics.median(ms), 4),
               "ms_mean": round(statistics.mean(ms), 4)}
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        return statistics.median(ms)

    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy("i8")
        fill_index(idx, a.rows, a.dim, 0, a.rows, "gaussian")
        starts = np.arange(1, a.rows + 1, a.per_doc, dtype=np.uint64)
        ranges = np.ascontiguousarray(np.stack([starts, np.minimum(starts + np.uint64(a.per_doc), np.uint64(a.rows + 1))], axis=1))
        values = np.random.default_rng(317).random(len(ranges)).astype(np.float32)

        def build():
            with idx.make_prior() as p:
                p.set_ranges(ranges, values)

        report("make_prior + set_ranges", timed(build, a.steps, a.warmup), {"ranges": len(ranges), "per_doc": a.per_doc})
        with idx.make_prior() as pri:
            pri.set_ranges(ranges, values)
            assert pri.bound() == float(values.max()) == pri.bound(refresh=True)
            doc = np.arange(1, a.per_doc + 1, dtype=np.uint64) + np.uint64((len(ranges) // 2) * a.per_doc)
            report(f"set_ids of {a.per_doc} ids", timed(lambda: pri.set_ids(doc, 0.5), a.steps, a.warmup), {"ids": a.per_doc})
            report("bound(refresh=True)", timed(lambda: pri.bound(refresh=True), a.steps, a.warmup), {})
            q = make_queries(B, a.dim, "gaussian")
            for fetch in (40, 256):
                o = (zeros(B, fetch, dt=torch.int64), zeros(B, fetch), zeros(B, fetch), zeros(B, dt=torch.int32))
                g = (zeros(B, k, dt=torch.int64), zeros(B, k), zeros(B, k), zeros(B, k), zeros(B, k, dt=torch.float64),
                     zeros(B, dt=torch.int32), zeros(B, dt=torch.uint8))
                plain_a = report(f"search k = {fetch} (before)", timed(lambda: idx.search_device(q, fetch, *o), a.steps, a.warmup), {"k": fetch})
                boosted = report(f"boosted k = {k}, fetch = {fetch}",
                                 timed(lambda: idx.search_boosted_device(pri, q, k, *g, weight=a.weight, fetch=fetch), a.steps, a.warmup),
                                 {"k": k, "fetch": fetch, "weight": a.weight, "complete_share": round(float(g[6].float().mean().item()), 4),
                                  "n_found_min": int(g[5].min().item())})
                plain_b = report(f"search k = {fetch} (after)", timed(lambda: idx.search_device(q, fetch, *o), a.steps, a.warmup), {"k": fetch})
                plain = 0.5 * (plain_a + plain_b)
                print(json.dumps({"boost_ms": round(boosted - plain, 4), "plain_spread_ms": round(abs(plain_a - plain_b), 4), "k": k,
                                  "fetch": fetch, "ratio_to_plain": round(boosted / plain, 4)}), flush=True)


if __name__ == "__main__":
    main()
