"""Seeded random sequences of add, remove, compact, save and load, checked against a host model after every step: the model
holds the rows behind ids 1 .. len and which of them are removed; a compaction renumbers it the way kept_ids says."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,kind", [(1, "i8"), (2, "bf16"), (3, "compressed"), (4, "i8")])
def test_random_ops_with_compaction(seed, kind, oracle, lib_built, tmp_path):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(seed)
    d = 72
    rows = np.zeros((0, d), dtype=np.float32)                  # the model: rows behind ids 1 .. len
    alive = np.zeros(0, dtype=bool)
    Q = rng.standard_normal((6, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        if kind == "compressed":
            idx.set_corpus_mode("bf16")
        else:
            idx.set_filter_copy(kind)
        for step in range(40):
            op = rng.choice(["add", "add", "remove", "remove", "compact", "save", "load"])
            what = f"seed {seed} step {step}: {op}"
            if op == "add":
                m = int(rng.integers(1, 1500))
                Y = (rng.standard_normal((m, d)) * rng.uniform(0.5, 3.0, (m, 1))).astype(np.float32)
                if rng.random() < 0.3:
                    Y[0] = 0.0                                 # a zero-norm row
                first = idx.add(Y)
                assert first == len(rows) + 1, what
                if kind == "compressed":
                    Y = idx.get_rows(len(rows), m)
                rows = np.concatenate([rows, Y])
                alive = np.concatenate([alive, np.ones(m, dtype=bool)])
            elif op == "remove" and len(rows):
                r = rng.choice(len(rows), int(rng.integers(1, max(2, len(rows) // 4))), replace=True)
                idx.remove(r.astype(np.uint64) + 1)
                alive[r] = False
            elif op == "compact":
                kept = idx.compact()
                np.testing.assert_array_equal(kept, np.flatnonzero(alive).astype(np.uint64) + 1, err_msg=what)
                rows, alive = rows[alive], np.ones(int(alive.sum()), dtype=bool)
            elif op == "save":
                idx.save(str(tmp_path))
            elif op == "load":
                idx.save(str(tmp_path))
                with FlatIndex(d) as other:
                    if kind == "compressed":
                        other.set_corpus_mode("bf16")
                    other.load(str(tmp_path))
                    assert len(other) == len(rows) and other.removed == int((~alive).sum()), what
                idx.load(str(tmp_path))
            assert len(idx) == len(rows) and idx.removed == int((~alive).sum()), what
            if alive.any():
                live_ids = np.flatnonzero(alive).astype(np.uint64) + 1
                ids, sc, di, nf = idx.search(Q, 10)
                oi, od, os_, onf = oracle.search(rows[alive], Q, 10)
                np.testing.assert_array_equal(nf, onf, err_msg=what)
                np.testing.assert_array_equal(ids, np.where(oi > 0, live_ids[np.maximum(oi.astype(np.int64) - 1, 0)], 0), err_msg=what)
                np.testing.assert_array_equal(bits(di), bits(od), err_msg=what)
                np.testing.assert_array_equal(bits(sc), bits(os_), err_msg=what)
