"""Random sequences of appends, removals (single ids, runs, whole tiles, ids already removed), filter-copy switches, clears
and save + load, each followed by a search that must be bit-identical to the oracle on the live rows.  Seeded, in the style
of test_random_ops_gpu.py."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d,seed", [(384, 1), (100, 2), (1024, 3), (1536, 4), (384, -5), (256, 6)])
def test_random_sequences_with_removals(d, seed, oracle, lib_built, tmp_path):
    from memex_amd.index import FlatIndex
    cone = seed < 0
    rng = np.random.default_rng(abs(seed) + 500)
    axis = rng.standard_normal(d).astype(np.float32)
    axis /= np.linalg.norm(axis)
    rows = np.zeros((0, d), dtype=np.float32)
    alive = np.zeros(0, dtype=bool)
    kinds = ["i8", "bf16", False, True]
    idx = FlatIndex(d)
    try:
        for step in range(30):
            op = rng.choice(["add", "remove", "remove", "kind", "clear", "saveload"], p=[.3, .3, .15, .1, .03, .12])
            if op == "add" or rows.shape[0] == 0:
                n = int(rng.choice([1, 31, 64, 65, 1000, 4097, 20000]))
                X = rng.standard_normal((n, d))
                if cone:
                    X = axis + X * (0.5 / np.sqrt(d))
                X = (X * rng.uniform(0.1, 10.0, (n, 1))).astype(np.float32)
                if n > 2 and rng.random() < 0.3:
                    X[rng.integers(0, n)] = 0
                if n > 40 and rng.random() < 0.3:
                    X[1:8] = X[0]
                assert idx.add(X) == rows.shape[0] + 1
                rows = np.concatenate([rows, X])
                alive = np.concatenate([alive, np.ones(n, dtype=bool)])
            elif op == "remove":
                n = rows.shape[0]
                how = rng.integers(0, 4)
                if how == 0:
                    r = rng.choice(n, max(1, n // 50), replace=True)          # random, repeats and already-removed ones too
                elif how == 1:
                    a = int(rng.integers(0, n))
                    r = np.arange(a, min(n, a + int(rng.integers(1, 3000))))  # a run
                elif how == 2:
                    t = int(rng.integers(0, (n + 63) // 64))
                    r = np.arange(64 * t, min(n, 64 * t + 64))                # a whole scan tile
                else:
                    r = np.array([int(rng.integers(0, n))])                   # one row
                expect = int(np.unique(r[alive[r]]).size)
                assert idx.remove(r + 1) == expect
                alive[r] = False
            elif op == "kind":
                idx.set_filter_copy(kinds[int(rng.integers(0, len(kinds)))])
            elif op == "clear" and rows.shape[0] > 20000:
                idx.clear()
                rows = np.zeros((0, d), dtype=np.float32)
                alive = np.zeros(0, dtype=bool)
                continue
            elif op == "saveload":
                idx.save(str(tmp_path))
                idx.close()
                idx = FlatIndex(d)
                if rng.random() < 0.5:
                    idx.set_filter_copy(kinds[int(rng.integers(0, len(kinds)))])
                idx.load(str(tmp_path))
            assert len(idx) == rows.shape[0] and idx.removed == int((~alive).sum())
            if rows.shape[0] == 0:
                continue
            B = int(rng.choice([1, 5, 33, 130, 256, 300]))
            k = int(rng.choice([1, 10, 40]))
            Q = rng.standard_normal((B, d)).astype(np.float32)
            if cone:
                Q[::2] = axis + Q[::2] * (0.7 / np.sqrt(d))
            Q[0] = rows[int(rng.integers(0, rows.shape[0]))] * 2.0   # a query that is a row, perhaps a removed one
            ids, sc, di, nf = idx.search(Q, k)
            live_ids = np.flatnonzero(alive).astype(np.uint64) + 1
            oi, od, os_, onf = oracle.search(rows[alive], Q, k)
            oi = np.where(oi > 0, live_ids[np.maximum(oi.astype(np.int64) - 1, 0)] if live_ids.size else 0, 0).astype(np.uint64)
            msg = f"step {step} op {op} n {rows.shape[0]} live {int(alive.sum())}"
            np.testing.assert_array_equal(nf, onf, err_msg=msg)
            np.testing.assert_array_equal(ids, oi, err_msg=msg)
            np.testing.assert_array_equal(bits(di), bits(od), err_msg=msg)
            np.testing.assert_array_equal(bits(sc), bits(os_), err_msg=msg)
    finally:
        idx.close()
