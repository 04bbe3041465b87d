"""Proof, without a GPU, that the random walk of tests/test_feature_random_ops_gpu.py reaches what it is for (tests/RANDOM_WALK.md):
for every seed the GPU test uses, the clean model walks against itself without a difference and meets every event, and each defective
model (tests/index_model.py: DEFECTS) is caught within the same step budget."""
import collections

import numpy as np
import pytest

from index_model import DEFECTS, DefectiveModel, IndexModel
from random_walk import CASES, EVENTS, STEPS, run

_CLEAN = {}


def layout(case):
    """how the case's target deals its rows to shards: the walk's growth events are about each shard's own storage"""
    return dict(shards=len(case["devices"] or [0]), block_rows=case["block_rows"])


def clean_walk(case, oracle):
    """the clean model as its own target, once per case -> (the tape of its answers, the events it met).  The target is a second
    model that computes every answer itself (no tape), so the comparison is of two computations, mutation by mutation"""
    if case["name"] not in _CLEAN:
        tape, events = [], collections.Counter()
        model = IndexModel(case["d"], oracle, case["compressed"], tape=tape, tape_mode="record")
        target = IndexModel(case["d"], oracle, case["compressed"])
        for idx in (model, target):
            if case["copy"]:
                idx.set_filter_copy(case["copy"])
        run(target, model, np.random.default_rng(case["seed"]), STEPS, lambda name: events.update([name]), cone=case["cone"],
            tag=f"{case['name']} seed {case['seed']}", **layout(case))
        _CLEAN[case["name"]] = (tape, events)
    return _CLEAN[case["name"]]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_clean_walk_meets_every_event(case, oracle):
    tape, events = clean_walk(case, oracle)
    missing = [e for e in EVENTS if not events[e]]
    assert not missing, f"{case['name']} seed {case['seed']}: {STEPS} steps never reach {missing}"
    names = collections.Counter(name for name, _ in tape)
    assert len(names) == 11 and min(names.values()) >= 3, names       # every search method ran, more than once or twice


@pytest.mark.parametrize("defect", list(DEFECTS))
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_walk_catches_defect(case, defect, oracle):
    tape, _ = clean_walk(case, oracle)
    model = IndexModel(case["d"], oracle, case["compressed"], tape=tape, tape_mode="replay")
    target = DefectiveModel(defect, case["d"], oracle, case["compressed"], tape=tape, tape_mode="replay", **layout(case))
    for idx in (model, target):
        if case["copy"]:
            idx.set_filter_copy(case["copy"])
    tag = f"{case['name']} seed {case['seed']}"
    with pytest.raises(AssertionError, match=f"{tag} step [0-9]+: ") as e:
        run(target, model, np.random.default_rng(case["seed"]), STEPS, cone=case["cone"], tag=tag, **layout(case))
    print(defect, "->", str(e.value)[:300])


def test_failure_names_seed_step_and_operation(oracle):
    case = CASES[3]
    tape, _ = clean_walk(case, oracle)
    model = IndexModel(case["d"], oracle, case["compressed"], tape=tape, tape_mode="replay")
    target = DefectiveModel("mmr_candidate_order", case["d"], oracle, case["compressed"], tape=tape, tape_mode="replay", **layout(case))
    with pytest.raises(AssertionError) as e:
        run(target, model, np.random.default_rng(case["seed"]), STEPS, cone=case["cone"], tag=f"{case['name']} seed {case['seed']}",
            **layout(case))
    msg = str(e.value)
    assert f"seed {case['seed']} step " in msg and "mmr(" in msg and "differs" in msg, msg
