"""Compaction (mx_index_compact) on the headline corpus (bench.py's 10M x 384 Gaussian rows, int8 filter copy, batches of 256
queries, top-10).

Default: the search step of three resident indexes, measured in alternating rounds -- one that never had removals, one with 1 %
of its rows removed at random (the masked kernels), and the same after compaction -- then the wall-clock time of compactions at
1 % and 50 % removed and the device memory each released.  One JSON line per result.
--only-compact FRAC: build, remove FRAC of the rows at random and compact once (for a kernel trace of the compaction alone).

  python scripts/bench_compact.py [--rows 10000000] [--dim 384] [--rounds 5] [--steps 30] [--warmup 5] [--only-compact 0.5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
os.environ.setdefault("MEMEX_HIP_SPIN", "1")  # as bench.py: the benchmark owns its core


def build(n, dim, frac, seed):
    import numpy as np
    from bench import fill_index
    from memex_amd.index import FlatIndex
    idx = FlatIndex(dim)
    idx.set_filter_copy("i8")
    fill_index(idx, n, dim, 0, n, "gaussian")
    if frac > 0:
        rng = np.random.default_rng(seed)
        idx.remove(rng.choice(n, int(n * frac), replace=False).astype(np.uint64) + 1)
    return idx


def timed_compact(idx):
    import torch
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    t0 = time.perf_counter()
    kept = idx.compact()
    ms = (time.perf_counter() - t0) * 1e3
    free1, _ = torch.cuda.mem_get_info()
    return ms, (free1 - free0) / 2**30, kept.size


def main():
    from bench_removed import run
    from bench import make_queries
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only-compact", type=float, default=None)
    a = ap.parse_args()
    n = a.rows
    if a.only_compact is not None:
        idx = build(n, a.dim, a.only_compact, 1)
        ms, gib, live = timed_compact(idx)
        print(json.dumps({"case": f"compact {a.only_compact:.0%} removed", "rows": n, "live": live, "wall_ms": round(ms, 2), "released_gib": round(gib, 3)}))
        return
    q = make_queries(a.batch, a.dim, "gaussian")
    import torch
    idx = {"never removed": build(n, a.dim, 0.0, 0), "1% removed": build(n, a.dim, 0.01, 0), "1% removed, compacted": build(n, a.dim, 0.01, 0)}
    ms, gib, live = timed_compact(idx["1% removed, compacted"])
    compact_1 = {"case": "compact 1% removed", "rows": n, "live": live, "wall_ms": round(ms, 2), "released_gib": round(gib, 3)}
    per = {k: [] for k in idx}
    for _ in range(a.rounds):  # old and new alternated: the package's power state drifts between runs
        for name, ix in idx.items():
            times, _, _ = run(ix, q, a.k, a.steps, a.warmup)
            per[name].append(statistics.median(times))
    base = statistics.median(per["never removed"])
    for name, meds in per.items():
        med = statistics.median(meds)
        print(json.dumps({"case": name, "rows": n, "dim": a.dim, "batch": a.batch, "k": a.k, "ms_median": round(med, 4),
                          "round_medians": [round(m, 4) for m in meds], "qps": round(a.batch / (med / 1e3), 1),
                          "vs_never_removed": round(med / base, 4)}), flush=True)
    print(json.dumps(compact_1), flush=True)
    for ix in idx.values():
        ix.close()
    torch.cuda.empty_cache()
    for frac in (0.5, 0.01):
        walls = []
        for r in range(3):
            ix = build(n, a.dim, frac, 10 + r)
            ms, gib, live = timed_compact(ix)
            walls.append(ms)
            ix.close()
        print(json.dumps({"case": f"compact {frac:.0%} removed", "rows": n, "live": live, "wall_ms_median": round(statistics.median(walls), 2),
                          "wall_ms": [round(w, 2) for w in walls], "released_gib": round(gib, 3)}), flush=True)


if __name__ == "__main__":
    main()
