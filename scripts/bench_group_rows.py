"""Cost of grouped search with members (mx_index_search_group_rows, mx_index_search_capped, mx_grouping_key_counts) on
the headline corpus (bench.py's 10M x 384 Gaussian rows, int8 filter copy): documents of 70 consecutive rows set by ranges, 256 queries
and 1 query, fetch = 40 and fetch = 256.  Device-pointer calls.  Per batch size and fetch, in one run and in this order:

  search k = fetch (before)   grouped k = 10   group rows k = 10, n = 3   capped k = 10, per_key = 2   search k = fetch (after)

The plain and grouped calls are the yardstick: the three grouped forms run the same candidate stage, so the difference of each to the
mean of the two plain medians is what its list kernel and stream synchronise add, and `ratio_to_grouped` is the figure DESIGN.md 3.19
quotes.  Also timed: one key_counts of 2560 distinct keys (a pass over the keys of all rows).  Prints one JSON line per case (median
and mean milliseconds per call).

  python scripts/bench_group_rows.py [--rows 10000000] [--dim 384] [--per-doc 70] [--steps 30] [--warmup 5]
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
    ap.add_argument("--per-doc", type=int, default=70)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    k, n, per_key = 10, 3, 2

    def zeros(*shape, dt=torch.float32):
        return torch.zeros(shape, dtype=dt, device="cuda")

    def report(case, ms, extra):
        rec = {"case": case, "rows": a.rows, "dim": a.dim, "ms_median": round(statistics.median(ms), 4), "ms_mean": round(statistics.mean(ms), 4)}
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        return statistics.median(ms)

    with FlatIndex(a.dim) as idx:
        idx.set_filter_copy("i8")
        fill_index(idx, a.rows, a.dim, 0, a.rows, "gaussian")
        starts = np.arange(1, a.rows + 1, a.per_doc, dtype=np.uint64)
        ranges = np.ascontiguousarray(np.stack([starts, np.minimum(starts + np.uint64(a.per_doc), np.uint64(a.rows + 1))], axis=1))
        with idx.make_grouping() as grp:
            grp.set_ranges(ranges, np.arange(1, len(ranges) + 1, dtype=np.uint32))
            asked = np.arange(1, min(2560, len(ranges)) + 1, dtype=np.uint32) * np.uint32(max(len(ranges) // 2560, 1))
            r, l = grp.key_counts(asked)
            assert int(r.min()) >= 1 and int(r.max()) <= a.per_doc and (r == l).all()
            report(f"key_counts of {asked.size} keys", timed(lambda: grp.key_counts(asked), a.steps, a.warmup), {"keys": int(asked.size)})
            for B in (256, 1):
                q = make_queries(B, a.dim, "gaussian")
                for fetch in (40, 256):
                    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
                    o = (zeros(B, fetch, dt=i64), zeros(B, fetch), zeros(B, fetch), zeros(B, dt=i32))
                    g = (zeros(B, k, dt=i64), zeros(B, k), zeros(B, k), zeros(B, k, dt=i32), zeros(B, k, dt=i32), zeros(B, dt=i32), zeros(B, dt=u8))
                    m = (zeros(B, k, n, dt=i64), zeros(B, k, n), zeros(B, k, n), zeros(B, k, dt=i32), zeros(B, k, dt=i32), zeros(B, k, dt=i32),
                         zeros(B, k, dt=u8), zeros(B, dt=i32), zeros(B, dt=u8))
                    c = (zeros(B, k, dt=i64), zeros(B, k), zeros(B, k), zeros(B, k, dt=i32), zeros(B, dt=i32), zeros(B, dt=u8))
                    tag = {"queries": B, "k": k, "fetch": fetch}
                    plain_a = report(f"search k = {fetch} (before)", timed(lambda: idx.search_device(q, fetch, *o), a.steps, a.warmup),
                                     {"queries": B, "k": fetch})
                    grouped = report("grouped", timed(lambda: idx.search_grouped_device(grp, q, k, *g, fetch=fetch), a.steps, a.warmup), tag)
                    rows = report(f"group rows n = {n}",
                                  timed(lambda: idx.search_group_rows_device(grp, q, k, n, *m, fetch=fetch), a.steps, a.warmup),
                                  dict(tag, n=n, complete=int(m[8].sum().item()), members_complete=int(m[6].sum().item())))
                    capped = report(f"capped per_key = {per_key}",
                                    timed(lambda: idx.search_capped_device(grp, q, k, per_key, *c, fetch=fetch), a.steps, a.warmup),
                                    dict(tag, per_key=per_key, complete=int(c[5].sum().item())))
                    plain_b = report(f"search k = {fetch} (after)", timed(lambda: idx.search_device(q, fetch, *o), a.steps, a.warmup),
                                     {"queries": B, "k": fetch})
                    plain = 0.5 * (plain_a + plain_b)
                    print(json.dumps(dict(tag, plain_spread_ms=round(abs(plain_a - plain_b), 4), grouped_over_plain_ms=round(grouped - plain, 4),
                                          group_rows_over_plain_ms=round(rows - plain, 4), capped_over_plain_ms=round(capped - plain, 4),
                                          group_rows_ratio_to_grouped=round(rows / grouped, 4),
                                          capped_ratio_to_grouped=round(capped / grouped, 4))), flush=True)


if __name__ == "__main__":
    main()
