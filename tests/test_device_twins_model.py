"""The tools of the device-pointer twin tests, checked without a GPU (tests/DEVICE_TWINS.md): the table of forms is complete, the
guard zones notice a write one element outside a view, every section A case names a branch the counters can prove, the corpora have
the sizes the branches need, and the model that cuts the oracle's distances into top-k lists is oracle.search."""
import inspect

import numpy as np
import pytest

import device_twins as DT
from conftest import bits
from filtered_model import allowed_mask, subset_oracle
from range_model import oracle_dists


def test_every_device_method_has_a_row():
    from memex_amd.index import FlatIndex
    methods = sorted(n for n in dir(FlatIndex) if n.endswith("_device"))
    rows = sorted(f.name for f in DT.FORMS)
    assert rows == methods, f"FORMS and FlatIndex disagree: {sorted(set(rows) ^ set(methods))}"
    assert len(set(rows)) == len(rows)
    assert [f.name for f in DT.FORMS if not f.search] == ["add_device"]
    for f in DT.SEARCH_FORMS:
        assert hasattr(FlatIndex, f.host), f.host
        assert f.name == f.host + "_device", f.name
        names = [o[0] for o in f.outs]
        assert set(f.optional) <= set(names) and set(f.host_order) == set(names), f.name
        assert callable(f.call_device) and callable(f.call_host), f.name
        # every output of the row is a parameter of the method (out_ids: the by-id forms' name for ids)
        params = set(inspect.signature(getattr(FlatIndex, f.name)).parameters)
        assert {("out_ids" if n == "ids" and "out_ids" in params else n) for n in names} <= params, f.name


@pytest.mark.parametrize("kind", sorted(DT.KINDS))
def test_guards_catch_one_element_either_side(kind):
    import torch
    for shape in ((3, 5), (7,), (2, 3, 4)):
        view, check = DT.out(kind, shape, device="cpu")
        size = view.element_size()
        assert view.is_contiguous() and tuple(view.shape) == shape
        assert view.data_ptr() % (2 * size) == size % (2 * size) or size == 1, "the view is aligned beyond its element type"
        assert bool((view == DT.KINDS[kind][1]).all())
        check("untouched")
        view.fill_(1)                                                       # writing the whole view is what a kernel does
        check("view written")
        n = view.numel()
        for at, where in ((-1, "in front of"), (n, "behind")):
            v, chk = DT.out(kind, shape, device="cpu")
            torch.as_strided(v, (1,), (1,), v.storage_offset() + at).fill_(3)
            with pytest.raises(AssertionError, match=f"written 1 element.* {where}"):
                chk("one element outside")
        for at, where in ((-DT.LEAD, "in front of"), (n + DT.TAIL - 1, "behind")):   # the far ends of the zones
            v, chk = DT.out(kind, shape, device="cpu")
            torch.as_strided(v, (1,), (1,), v.storage_offset() + at).fill_(3)
            with pytest.raises(AssertionError, match=where):
                chk("far end")
    assert DT.LEAD % 2 == 1 and DT.LEAD >= 64 and DT.TAIL >= 64


def test_every_case_names_a_branch_and_the_corpora_reach_it():
    cap = 16384                                                            # kCandCap = kSubsetCap (index_kernels.h)
    X, gone = DT.corpus(72)
    assert X.shape[0] == DT.N_ROWS and DT.N_ROWS % 64 != 0 and DT.N_ROWS > cap
    assert not X[DT.ZERO_ROW].any() and (X[DT.DUP_FIRST:DT.DUP_FIRST + DT.DUP_COUNT] == X[DT.DUP_FIRST]).all()
    alive = np.ones(DT.N_ROWS, bool)
    alive[gone] = False
    flt = DT.filters()
    live = {n: int((alive & allowed_mask(DT.N_ROWS, r, DT.ID_OFFSET)).sum()) for n, r in flt.items()}
    assert 0 < live["small"] < 100 and 0 < live["scattered"] <= cap < live["big"] and live["empty"] == 0 and live["all"] == alive.sum()
    assert DT.N_COPIES > cap
    names = set()
    for c in DT.TOPK_CASES + DT.RANGE_CASES:
        assert c.branch in DT.BRANCHES, c.name
        assert c.handle in ("plain", "sharded", "compressed", "copies"), c.name
        assert (type(c).__name__, c.name) not in names, c.name
        names.add((type(c).__name__, c.name))
    for c in DT.TOPK_CASES:
        assert c.flt == "copies" or c.flt in flt, c.name
        n = DT.N_COPIES if c.flt == "copies" else live[c.flt]
        if c.branch == "subset":
            assert n <= cap and c.k <= 256 and c.mode == 0, c.name         # (the subset kernel serves every k; run_exact only k > 256 at force=0)
        if c.branch in ("masked", "overflow"):
            assert n > 0 and c.k <= 256 and c.mode == 0 and (n > cap or c.force == 0), c.name
        if c.branch == "exact":
            assert (c.k > 256 or c.mode == DT.EXACT) and (n > cap or c.force == 0), c.name
        if c.branch == "nothing":
            assert n == 0, c.name
    for branch in DT.BRANCHES:
        assert any(c.branch == branch for c in DT.TOPK_CASES + DT.RANGE_CASES), f"no case claims {branch}"
    for handle in ("plain", "sharded", "compressed", "copies"):
        assert any(c.handle == handle for c in DT.TOPK_CASES) and any(c.handle == handle for c in DT.RANGE_CASES), handle
    assert {c.cap for c in DT.RANGE_CASES} >= {1, 10, 4096}
    assert set(DT.B_AXIS) >= {1, 255, 256, 257, 512, 513, 600, 1025}


def test_prove_tells_the_branches_apart():
    from memex_amd._lib import IndexStats
    def st(**kw):
        s = IndexStats()
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    B = 12
    shown = {
        "subset": st(queries=B, filtered_queries=B, subset_queries=B),
        "masked": st(queries=B, filtered_queries=B, scan_launches=1),
        "nothing": st(queries=B, filtered_queries=B),
        "overflow": st(queries=B, filtered_queries=B, scan_launches=1, retry_queries=1, fallback_queries=1),
        "range-scan": st(queries=B, scan_launches=1),
        "range-overflow": st(queries=B, scan_launches=1, fallback_queries=2),
        "range-exact": st(queries=B),
    }
    topk = ("subset", "masked", "nothing", "overflow")
    ranges = ("range-scan", "range-overflow", "range-exact")
    for family in (topk, ranges):
        for branch in family:
            DT.prove(branch, shown[branch], B)
            for other in family:
                if other != branch:
                    with pytest.raises(AssertionError):
                        DT.prove(other, shown[branch], B)
    DT.prove("exact", shown["nothing"], B)                                  # (run_exact and the blanks: both without a scan)
    for branch in ("subset", "masked", "overflow"):
        with pytest.raises(AssertionError):
            DT.prove("exact", shown[branch], B)
    with pytest.raises(AssertionError):
        DT.prove("masked", shown["masked"], B + 1)
    with pytest.raises(AssertionError):
        DT.prove("masked", st(queries=B, filtered_queries=B, scan_launches=4), B, G=3)
    DT.prove("masked", st(queries=B, filtered_queries=B, scan_launches=3), B, G=3)


def test_topk_from_dists_is_the_oracles_search(oracle):
    X, gone = DT.corpus(72)
    Q = DT.queries(X, 9)
    alive = np.ones(DT.N_ROWS, bool)
    alive[gone] = False
    D = oracle_dists(oracle, X, Q)
    for name, r in DT.filters().items():
        keep = alive & allowed_mask(DT.N_ROWS, r, DT.ID_OFFSET)
        for k in (1, 10, 100, 300):
            got = DT.topk_from_dists(D, keep, k, DT.ID_OFFSET)
            want = subset_oracle(oracle, X, keep, Q, k, DT.ID_OFFSET)
            for g, w, what in zip(got, want, ("ids", "scores", "dists", "n_found")):
                g, w = (bits(g), bits(w)) if w.dtype == np.float32 else (g, w)
                np.testing.assert_array_equal(g, w, err_msg=f"{name}, k = {k}: {what}")
    # the zero row (dist 0 to everything) leads, then the duplicated row's live copies tie and come in id order; query 5 is all zeros
    ids = DT.topk_from_dists(D, alive, DT.DUP_COUNT, DT.ID_OFFSET)[0][4].astype(np.int64) - DT.ID_OFFSET - 1
    dups = [r for r in range(DT.DUP_FIRST, DT.DUP_FIRST + DT.DUP_COUNT) if alive[r]]
    assert ids[0] == DT.ZERO_ROW and list(ids[1:]) == dups and len(dups) == DT.DUP_COUNT - 1
    assert not Q[5].any()
