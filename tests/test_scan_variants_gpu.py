"""Every entry of the four scans' variant tables (scan_common.h: one table per kernel family drives both set-up and launch) is
launched at least once: every slot count kc = dim_pad / 128 of scan_kernel (f32 rows, no filter copy), scan16_kernel / scan16w_kernel
(bf16 copy) and scan8_kernel (int8 copy: one query group, two query groups, the two-workgroup form, the centred copy), as built and
with a row removed (the DEAD instances).  An instance that set-up missed fails its launch with an LDS-size error, for that one
kc / geometry / removed-rows combination only.  Bar: ids, scores, dists and n_found bit-equal to the same index in SEARCH_EXACT
mode, and the scan did run.  (fallback_queries is not looked at: at these sizes a query may take the fallback, behind the scan.)"""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

K = 10
BATCHES = (3, 200, 300)   # a few waves | the two-workgroup form up to kc 4 | two query groups up to kc 4, split passes above


def _kinds(kc):
    """copy kinds that have a scan at this width: the f32 scan up to 6 slots; scan16_kernel up to 6, scan16w_kernel above; int8: all"""
    return (("none",) if kc <= 6 else ()) + ("bf16", "i8")


def _exact(idx, Q):
    from memex_amd.index import SEARCH_AUTO, SEARCH_EXACT
    idx.set_search_mode(SEARCH_EXACT)
    try:
        return idx.search(Q, K)
    finally:
        idx.set_search_mode(SEARCH_AUTO)


def _check(idx, Q, what):
    """every batch size through the fast path against the EXACT answers of the same index (a query's answer does not depend on its batch)"""
    ref = _exact(idx, Q)
    for B in BATCHES:
        idx.reset_stats()
        ids, sc, di, nf = idx.search(Q[:B], K)
        assert idx.stats().scan_launches > 0, (what, B)
        np.testing.assert_array_equal(ids, ref[0][:B], err_msg=f"{what} B={B}: ids")
        np.testing.assert_array_equal(bits(sc), bits(ref[1][:B]), err_msg=f"{what} B={B}: scores")
        np.testing.assert_array_equal(bits(di), bits(ref[2][:B]), err_msg=f"{what} B={B}: dists")
        np.testing.assert_array_equal(nf, ref[3][:B], err_msg=f"{what} B={B}: n_found")
    return ref


# n = 3003: no multiple of 32 or 64, and most workgroups get no tile; 70019: a workgroup of every geometry wraps its ring over several tiles
@pytest.mark.parametrize("kc,n", [(kc, 3003) for kc in range(1, 13)] + [(3, 70019), (4, 70019), (8, 70019)])
def test_every_slot_count_of_every_scan(kc, n, lib_built):
    from memex_amd.index import FlatIndex
    d = 128 * kc - 5
    rng = np.random.default_rng(1000 * kc + n % 7)
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((max(BATCHES), d), dtype=np.float32)
    with FlatIndex(d) as idx:
        idx.add(X)
        for kind in _kinds(kc):
            idx.set_filter_copy(kind)
            ref = _check(idx, Q, f"kc={kc} n={n} {kind}")
        assert idx.remove([int(ref[0][0, 0])]) == 1           # the best row of query 0: a removed row the masked kernels must hide
        for kind in _kinds(kc):
            idx.set_filter_copy(kind)
            _check(idx, Q, f"kc={kc} n={n} {kind}, one row removed")


@pytest.mark.parametrize("kc", range(1, 7))
def test_every_slot_count_of_the_centred_scans(kc, lib_built):
    """rows in a cone (a fixed unit direction + 0.3 x noise): copies rebuilt from the populated index are centred (test_centred_gpu.py)"""
    from memex_amd.index import FlatIndex
    d, n = 128 * kc - 5, 3003
    rng = np.random.default_rng(77 + kc)
    axis = rng.standard_normal(d).astype(np.float32)
    axis /= np.linalg.norm(axis)

    def cone(m):
        return (axis[None, :] + (0.3 / np.sqrt(d)) * rng.standard_normal((m, d), dtype=np.float32)).astype(np.float32)

    X, Q = cone(n), cone(max(BATCHES))
    with FlatIndex(d) as idx:
        idx.add(X)
        for removed in (False, True):
            for kind in ("bf16", "i8"):                            # bf16 first: the int8 copy is then rebuilt from resident rows, centred
                idx.set_filter_copy(kind)
                assert idx.stats().filter_centred == 1, (kc, kind, removed)
                ref = _check(idx, Q, f"centred kc={kc} {kind} removed={removed}")
            if not removed:
                assert idx.remove([int(ref[0][0, 0])]) == 1
