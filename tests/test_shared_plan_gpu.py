"""Top-k and range search take the same scan.  Both derive their batch geometry (which scan kernel, how many queries per pass, how
many workgroups, where a batch splits) from one plan, so for the same index and the same B the first collect launch of every pass
must be the same launch: `scan_launches` and `scan_bytes` count exactly those, over all tiles, whatever a retry pass adds.  A
threshold of 2.0 is above every score: the range call selects nothing and cannot overflow.  One top-k call runs before the two
that are compared: where the library chooses the filter copy itself, a top-k batch that overflows rebuilds the copy and answers again
on the new one (two counted launches on two copies in that one call), which a range call never does."""
import numpy as np
import pytest

from test_range_gpu import _KINDS
from test_remove_gpu import corpus

pytestmark = pytest.mark.gpu


def scan_of(idx, call):
    idx.reset_stats()
    call()
    st = idx.stats()
    return int(st.scan_launches), int(st.scan_bytes)


def same_scan(idx, Q, what):
    idx.search(Q, 10)       # an automatic copy may be rebuilt inside a top-k call (centred, or demoted to bf16): let it settle first
    topk = scan_of(idx, lambda: idx.search(Q, 10))
    rng_ = scan_of(idx, lambda: idx.search_range(Q, 2.0, 10))
    print(f"{what}: top-k (scan_launches, scan_bytes) = {topk}, range = {rng_}")
    assert topk[0] >= 1, f"{what}: the top-k call did not scan"
    assert topk == rng_, f"{what}: top-k scanned {topk}, range scanned {rng_} (scan_launches, scan_bytes)"


@pytest.mark.parametrize("name,d,n,setup,cone", _KINDS, ids=[c[0] for c in _KINDS])
def test_every_copy_kind_scans_alike(name, d, n, setup, cone, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    X = corpus(rng, n, d, cone=cone)
    if name == "compressed" or d == 3:  # (as test_range_gpu: no rows that send the batch to the EXACT path)
        X[[11, n - 100]] = rng.standard_normal((2, d)).astype(np.float32)
    with FlatIndex(d) as idx:
        if name == "compressed":
            setup(idx)
        idx.add(X)
        if setup == "centre_i8":
            idx.set_filter_copy(False)
            idx.set_filter_copy("i8")                          # rebuilt from a populated cone: centred
        elif setup is not None and name != "compressed":
            setup(idx)
        if name in ("centred_int8", "centred_bf16"):
            assert idx.stats().filter_centred == 1
        same_scan(idx, rng.standard_normal((24, d)).astype(np.float32), name)


@pytest.mark.parametrize("B", [1, 100, 200, 300, 512, 700])
def test_every_batch_geometry_scans_alike(B, lib_built):
    from memex_amd.index import FlatIndex
    rng = np.random.default_rng(42 + B)
    d, n = 384, 20000
    X = corpus(rng, n, d)
    with FlatIndex(d) as idx:
        idx.set_filter_copy("i8")
        idx.add(X)
        same_scan(idx, rng.standard_normal((B, d)).astype(np.float32), f"int8, B = {B}")
