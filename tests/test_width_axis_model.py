"""Proof, without a GPU, that the lattice of tests/width_axis_cases.py is what tests/test_width_axis_gpu.py needs (tests/WIDTH_AXIS.md):
every switch point has a width on each side, the expected-route table is total, the oracle alone answers every corpus with the edge
rows among the answers the GPU test compares, the range thresholds admit exactly 5 rows and every row, and the clean model walks the
`wide-d1540` layout of the random walk against itself without a difference."""
import numpy as np
import pytest

import width_axis_cases as W
from index_model import IndexModel
from oracle.search_oracle import score_from_dist
from random_walk import EVENTS, STEPS, run


def test_every_switch_has_a_width_on_each_side():
    accepted, refused = set(W.LATTICE), set(W.REFUSED)
    for near, what in W.SWITCHES:
        assert near in accepted | refused and near + 1 in accepted | refused, (near, what)
        assert (near in accepted) or (near + 1 in accepted), (near, what)
    assert all(1 <= d <= W.MAX_DIM for d in accepted) and not any(1 <= d <= W.MAX_DIM for d in refused)
    for sub in (W.REDUCED, W.MOVERS, W.COMPRESSED, W.LISTS_ONLY):
        assert set(sub) <= accepted | {130}                               # (130: the reduced lattice's own dim & 3 != 0 width)
    assert {d & 3 == 0 for d in W.REDUCED} == {True, False} and {d & 3 == 0 for d in W.MOVERS} == {True, False}
    # the padded widths: 128-rounding up to 768, 256-rounding above
    assert [W.ds_of(d) for d in (1, 128, 129, 768, 769, 1025, 1281, 1537, 1793, 65535)] == [128, 128, 256, 768, 1024, 1280, 1536,
                                                                                           1792, 2048, 65536]
    # the query preparation above 1536 padded dims: one chunk exactly, whole chunks, and a last chunk of 1 and of chunk - 1 floats
    rest = {d % W.PREP_CHUNK for d in accepted if W.ds_of(d) > W.MAX_KC16 * W.CHUNK}
    assert {0, 1, W.PREP_CHUNK - 1} <= rest and W.PREP_CHUNK in accepted
    assert any(d >= W.PREP_LDS_DIMS for d in accepted)


def test_the_route_table_is_total():
    for dim in W.LATTICE:
        ds = W.ds_of(dim)
        for kind in W.KINDS:
            r = W.route(dim, kind)
            if r is None:
                assert kind == "compressed" and ds > 1536
                continue
            assert set(r) == {"filter_kind", "elem_bytes", "scan", "scan_elem_bytes", "wide", "subset"}
            assert r["filter_kind"] in (0, 2, 3) and r["elem_bytes"] == {0: 0, 2: 1, 3: 2}[r["filter_kind"]]
            assert r["scan"] == (r["scan_elem_bytes"] > 0)
            assert (ds > 1536) <= (r["filter_kind"] == 0 and not r["scan"] and not r["subset"])
            for B in W.batch_sizes(dim):
                assert W.passes(dim, kind, B) == (2 if r["wide"] and B > 128 else 1)
    # one width per regime, spelled out
    assert W.route(512, "auto")["filter_kind"] == 2 and W.route(1024, "auto")["filter_kind"] == 2
    assert W.route(1025, "auto") == dict(filter_kind=3, elem_bytes=2, scan=True, scan_elem_bytes=2, wide=True, subset=True)
    assert W.route(1281, "i8")["filter_kind"] == 2 and not W.route(1281, "i8")["wide"]
    assert W.route(768, "none")["scan"] and not W.route(769, "none")["scan"]
    assert W.route(1536, "compressed")["filter_kind"] == 3 and W.route(1537, "compressed") is None
    assert W.route(1537, "i8")["filter_kind"] == 0
    assert W.batch_sizes(1536) == (1, 33, 129) and W.batch_sizes(1537) == (1, 40)
    assert W.n_rows(8192) == 700 and W.n_rows(8193) == 300


@pytest.mark.parametrize("dim", W.LATTICE)
def test_the_oracle_answers_with_the_edge_rows(dim, oracle):
    X, Q = W.corpus(dim)
    n = W.n_rows(dim)
    assert X.shape == (n, dim) and Q.shape == (129, dim) and np.isfinite(X).all()
    assert not X[W.ZERO_ROW].any() and (X[W.DUP_FIRST:W.DUP_FIRST + W.DUP_COUNT] == X[W.DUP_FIRST]).all()
    assert set(np.flatnonzero(X[W.ENDS_ROW])) == {0, dim - 1}
    norms = np.linalg.norm(X.astype(np.float64), axis=1)
    assert 0.5e-22 < norms[W.TINY_ROW] < 2e-22 and 0.5e18 < norms[W.HUGE_ROW] < 2e18
    assert (Q[W.Q_DOUBLE] == 2 * X[W.DUP_FIRST]).all() and not Q[W.Q_ZERO].any() and set(np.flatnonzero(Q[W.Q_LAST])) == {dim - 1}
    dups = set(range(W.DUP_FIRST + 1, W.DUP_FIRST + W.DUP_COUNT + 1))
    ids10, d10, _, nf10 = oracle.search(X, Q[:3], 10)
    ids300, d300, _, nf300 = oracle.search(X, Q[:3], 300)
    assert (nf10 == 10).all() and (nf300 == 300).all()
    assert W.ZERO_ROW + 1 in ids10[W.Q_DOUBLE] and W.ZERO_ROW + 1 in ids10[W.Q_ZERO] and W.ZERO_ROW + 1 in ids10[W.Q_LAST]
    if dim > 1:      # (one dim: half of the rows are at dist 0 of any query, and the lists are those rows in row order)
        assert len(dups & set(ids10[W.Q_DOUBLE].tolist())) >= 5, "the top-10 of the doubled row holds duplicates, ordered by row"
        assert W.ENDS_ROW + 1 in ids10[W.Q_LAST], "the two-element row is among the best rows of the last-element query"
    assert dups <= set(ids300[W.Q_DOUBLE].tolist()), "the top-300 of the doubled row holds the whole run"
    at = [ids300[W.Q_DOUBLE].tolist().index(i) for i in sorted(dups)]
    assert at == list(range(at[0], at[0] + W.DUP_COUNT)) and len(set(d300[W.Q_DOUBLE, at].tolist())) == 1
    assert list(ids10[W.Q_ZERO]) == list(range(1, 11)) and not d10[W.Q_ZERO].any()      # a zero query: dist 0 to all, ordered by row


@pytest.mark.parametrize("dim", W.REDUCED)
def test_the_range_thresholds_admit_five_rows_and_every_row(dim, oracle):
    X, Q = W.corpus(dim)
    alive = np.ones(len(X), bool)
    alive[W.REMOVED_ROW] = False
    for live in (None, alive):
        t5, t_all = W.range_thresholds(oracle, dim, live)
        s = score_from_dist(oracle.all_dists(X, Q[W.Q_RANGE]))
        if live is not None:
            s = s[live]
        assert int((s >= t5).sum()) == 5 and int((s >= t_all).sum()) == len(s)


def test_the_wide_walk_completes_on_the_model(oracle):
    """the seed tests/test_width_axis_gpu.py walks: the clean model against a second clean model, every step compared, and every
    event the walk exists for (random_walk.EVENTS) met within its 40 steps"""
    import collections
    events = collections.Counter()
    model = IndexModel(W.WALK["d"], oracle)
    target = IndexModel(W.WALK["d"], oracle)
    run(target, model, np.random.default_rng(W.WALK["seed"]), STEPS, lambda name: events.update([name]), cone=False,
        tag=f"{W.WALK['name']} seed {W.WALK['seed']}")
    missing = [e for e in EVENTS if not events[e]]         # growth under live handles, every form after a compaction, loads, ...
    assert not missing, f"seed {W.WALK['seed']}: {STEPS} steps never reach {missing}"
