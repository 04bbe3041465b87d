"""Grouped search with members on one long-lived index: a short random walk that mixes appends, removals, grouping edits, compaction
and the two new searches, with the host model (tests/group_rows_model.py over tests/grouped_model.py) beside it, compared exactly
after every search.  The walk is its own: the long walk of tests/test_feature_random_ops_gpu.py stays what it is."""
import numpy as np
import pytest

from conftest import bits
from group_rows_model import capped_model, group_rows_model, key_counts_model
from grouped_model import GroupingModel
from mmr_model import near_copy_corpus, queries_near_centres

pytestmark = pytest.mark.gpu

D, STEPS = 32, 70
ROWS_NAMES = ("ids", "scores", "dists", "keys", "group_rows", "n_members", "members_complete", "n_found", "complete")
CAPPED_NAMES = ("ids", "scores", "dists", "keys", "n_found", "complete")


def same(got, want, names, what):
    for name, g, w in zip(names, got, want):
        if name in ("scores", "dists"):
            g, w = bits(g), bits(w)
        np.testing.assert_array_equal(np.asarray(g), np.asarray(w), err_msg=f"{what}: {name}")


@pytest.mark.parametrize("devices,block_rows,seed", [(None, 0, 3196), ([0, 0], 64, 3197)], ids=["plain", "2-shards"])
def test_group_rows_random_ops(devices, block_rows, seed, oracle, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(seed)
    pool, centres = near_copy_corpus(rng, clusters=150, per=10, d=D)    # 1500 rows to draw from, in cluster order
    kw = dict(devices=devices, block_rows=block_rows) if devices else {}
    seen = dict(add=0, remove=0, edit=0, compact=0, rows=0, capped=0, counts=0, open=0, short=0)
    with FlatIndex(D, **kw) as idx:
        idx.add(pool[:400])
        rows, alive, at = pool[:400].copy(), np.ones(400, bool), 400
        grp, keys = idx.make_grouping(), GroupingModel()
        try:
            for step in range(STEPS):
                op = rng.choice(["add", "remove", "ranges", "ids", "compact", "rows", "capped", "counts"],
                                p=[0.1, 0.12, 0.12, 0.1, 0.06, 0.2, 0.2, 0.1])
                what = f"seed {seed} step {step} {op}"
                n = rows.shape[0]
                if op == "add" and at < len(pool):
                    m = int(rng.integers(1, 120))
                    idx.add(pool[at:at + m])
                    rows = np.concatenate([rows, pool[at:at + m]])
                    alive = np.concatenate([alive, np.ones(rows.shape[0] - n, bool)])
                    at += m
                    seen["add"] += 1
                elif op == "remove" and alive.sum() > 100:
                    gone = rng.choice(np.flatnonzero(alive), int(rng.integers(1, 40)), replace=False)
                    idx.remove(gone.astype(np.uint64) + np.uint64(1))
                    alive[gone] = False
                    seen["remove"] += 1
                elif op == "ranges":                                    # documents of consecutive rows, some ranges past the rows
                    cuts = np.sort(rng.choice(np.arange(1, n + 30), 12, replace=False))
                    r = np.stack([cuts[0::2], cuts[1::2]], axis=1).astype(np.uint64)
                    k = rng.integers(0, 9, len(r)).astype(np.uint32)    # few keys: groups grow large; key 0 un-groups
                    grp.set_ranges(r, k)
                    keys.set_ranges(r, k, 0, n)
                    seen["edit"] += 1
                elif op == "ids":
                    i = rng.integers(1, n + 10, 60).astype(np.uint64)
                    k = (i % np.uint64(5)).astype(np.uint32) * np.uint32(1 + step % 3)
                    grp.set_ids(i, k)
                    keys.set_ids(i, k, 0, n)
                    seen["edit"] += 1
                elif op == "compact":
                    dropped = not alive.all()
                    idx.compact()
                    if dropped:                                         # the rows were renumbered: the grouping is stale
                        with pytest.raises(Exception, match="stale"):
                            idx.search_capped(grp, pool[:1], 3, 1)
                        grp.close()
                        old = keys.keys_of(np.flatnonzero(alive).astype(np.uint64) + np.uint64(1), 0, n)
                        rows, alive = np.ascontiguousarray(rows[alive]), np.ones(int(alive.sum()), bool)
                        grp, keys = idx.make_grouping(), GroupingModel()
                        ids = np.arange(1, rows.shape[0] + 1, dtype=np.uint64)
                        grp.set_ids(ids, old)                           # the host puts its documents back
                        keys.set_ids(ids, old, 0, rows.shape[0])
                        seen["compact"] += 1
                elif op in ("rows", "capped"):
                    B = int(rng.integers(1, 6))
                    Q = queries_near_centres(rng, centres[rng.integers(0, 150, B)], B).astype(np.float32)
                    k = int(rng.choice([1, 3, 10]))
                    fetch = int(rng.choice([k, 17, 64, 300, 4096]))
                    if op == "rows":
                        m = int(rng.choice([1, 2, 5, 16]))
                        want = group_rows_model(oracle, rows, Q, k, m, keys, fetch=fetch, alive=alive)
                        same(idx.search_group_rows(grp, Q, k, m, fetch=fetch), want, ROWS_NAMES, f"{what} k {k} n {m} fetch {fetch}")
                        seen["open"] += int((~want[6] & (want[5] > 0)).any())
                        seen["short"] += int((~want[8]).any())
                    else:
                        per = int(rng.choice([1, 2, 7, fetch]))
                        want = capped_model(oracle, rows, Q, k, per, keys, fetch, alive=alive)
                        same(idx.search_capped(grp, Q, k, per, fetch=fetch), want, CAPPED_NAMES, f"{what} k {k} per_key {per} fetch {fetch}")
                        seen["short"] += int((~want[5]).any())
                    seen[op] += 1
                elif op == "counts":
                    asked = rng.integers(0, 12, 20).astype(np.uint32)
                    r, l = grp.key_counts(asked)
                    wr, wl = key_counts_model(keys.keys, n, asked, alive)
                    np.testing.assert_array_equal(r, wr, err_msg=what)
                    np.testing.assert_array_equal(l, wl, err_msg=what)
                    seen["counts"] += 1
        finally:
            grp.close()
    assert all(v > 0 for v in seen.values()), seen                      # (condition on the seeds: every event occurs)
