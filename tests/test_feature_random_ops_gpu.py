"""Every search form on one long-lived index: the random walk of tests/random_walk.py with FlatIndex as its target and the host model
of tests/index_model.py beside it, compared exactly after every step (tests/RANDOM_WALK.md).  tests/test_random_walk_model.py shows on
the CPU that these seeds meet every event the walk exists for and that the comparison catches each of twelve named defects.

MEMEX_TEST_SOAK=<n> walks n further seeds per layout (off by default)."""
import os
import time

import numpy as np
import pytest

from index_model import IndexModel
from random_walk import CASES, STEPS, run

pytestmark = pytest.mark.gpu

SOAK = int(os.environ.get("MEMEX_TEST_SOAK", "0"))


def walk(case, seed, oracle, store_dir):
    from memex_amd.index import FlatIndex
    model = IndexModel(case["d"], oracle, case["compressed"])
    t0 = time.perf_counter()
    with FlatIndex(case["d"], devices=case["devices"], block_rows=case["block_rows"]) as idx:
        if case["compressed"]:
            idx.set_corpus_mode("bf16")
        if case["copy"]:
            idx.set_filter_copy(case["copy"])
            model.set_filter_copy(case["copy"])
        run(idx, model, np.random.default_rng(seed), STEPS, store_dir=store_dir, cone=case["cone"], tag=f"{case['name']} seed {seed}",
            shards=len(case["devices"] or [0]), block_rows=case["block_rows"])
    print(f"{case['name']} seed {seed}: {STEPS} steps in {time.perf_counter() - t0:.2f} s")


# MEMEX_TEST_SOAK=n: n more seeds per layout (a one-off soak run, not part of the default suite)
_WALKS = [(c, c["seed"]) for c in CASES] + [(c, 7000 + i) for i in range(SOAK) for c in CASES]


@pytest.mark.parametrize("case,seed", _WALKS, ids=[c["name"] if s == c["seed"] else f"{c['name']}-soak{s}" for c, s in _WALKS])
def test_feature_random_ops(case, seed, oracle, lib_built, tmp_path):
    walk(case, seed, oracle, tmp_path)
