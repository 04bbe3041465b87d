"""Who owns the device and pinned buffers of the index and encoder hosts (memex_amd/csrc/mx_owned.h).
The index scenarios run in a child process bound to libmemex_hip_testing.so, whose policies count live buffers
(mx_testing_live_buffers) and can fail the n-th next allocation without calling HIP (mx_testing_fail_alloc)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PRELUDE = r'''
import ctypes, os, sys, numpy as np
sys.path.insert(0, os.getcwd())
from memex_amd import _lib
_lib.use_testing_library()
from memex_amd.index import FlatIndex
from oracle.search_oracle import COracle
L = _lib.lib()
L.mx_testing_live_buffers.restype = ctypes.c_long
L.mx_testing_fail_alloc.restype = ctypes.c_long
L.mx_testing_fail_alloc.argtypes = [ctypes.c_long]
live = L.mx_testing_live_buffers
rng = np.random.default_rng(11)
X = rng.standard_normal((3000, 128), dtype=np.float32)
Q = rng.standard_normal((4, 128), dtype=np.float32)
K = 5
oi, od, osc, onf = COracle().search(X, Q, K)
def same_as_oracle(res):
    ids, sc, di, nf = res
    assert np.array_equal(ids, oi) and np.array_equal(di.view(np.uint32), od.view(np.uint32))
    assert np.array_equal(sc.view(np.uint32), osc.view(np.uint32)) and np.array_equal(nf, onf)
'''

_CYCLE = _PRELUDE + r'''
def cycle(make, plain, store):
    idx = make()
    idx.add(X)
    same_as_oracle(idx.search(Q, K))
    assert live() > 0
    other = FlatIndex(128)                       # a second index, opened and closed while the first is open
    other.add(X[:100])
    other.search(Q, K)
    other.close()
    before = idx.stats().subset_queries
    idx.search_filtered(Q, K, ranges=[[10, 30]])         # few rows: the subset kernel
    if plain:
        assert idx.stats().subset_queries == before + len(Q)
    idx.search_filtered(Q, K, ranges=[[1, 3001]])        # every row: the masked pass
    if plain:
        assert idx.stats().subset_queries == before + len(Q)
    idx.search_range(Q, 0.2, 16)
    idx.search_mmr(Q, K)
    idx.search_fused(Q.reshape(2, 2, 128), K)
    idx.search_fused(Q.reshape(2, 2, 128), K, mode="rrf")
    idx.search_by_id([1, 7, 2999], K)
    idx.search_range_by_id([1, 7, 2999], 0.2, 16)
    flt = idx.make_filter(ranges=[[1, 200]])
    flt.deny(ids=[5, 6])
    flt.allow(ranges=[[1000, 2500]])
    idx.search_with(flt, Q, K)
    flt.close()
    grp, pri = idx.make_grouping(), idx.make_prior()
    kept = [idx.make_grouping(), idx.make_prior()]       # these two stay open across idx.close()
    for g in (grp, kept[0]):
        g.set_ranges([[1, 700]], 7)                      # rows below 1,024, then rows above 2,048
        g.set_ids([2500, 2600], [8, 9])
    assert list(grp.keys_of([1, 699, 700, 2500, 2600, 4000])) == [7, 7, 0, 8, 9, 0]
    assert grp.count() == (701, 701)
    assert [list(c) for c in grp.key_counts([7, 9, 5])] == [[699, 1, 0], [699, 1, 0]]
    for p in (pri, kept[1]):
        p.set_ranges([[1, 700]], 0.5)
        p.set_ids([2500, 2600], [0.25, -1.0])
    assert list(pri.values_of([1, 700, 2500, 2600, 4000])) == [0.5, 0.0, 0.25, -1.0, 0.0]
    assert pri.bound() == 0.5 and pri.bound(refresh=True) == 0.5
    flt = idx.make_filter(ranges=[[1, 2000]])
    for f in (None, flt):
        assert (idx.search_grouped(grp, Q, K, flt=f)[5] == K).all()
        assert (idx.search_group_rows(grp, Q, K, 3, flt=f)[7] == K).all()
        assert (idx.search_capped(grp, Q, K, 2, flt=f)[4] == K).all()
        assert (idx.search_boosted(pri, Q, K, flt=f)[5] == K).all()
    assert flt.allow_where(pri, 0.2, 1.0) == 700 and flt.allow_keys(grp, [8, 9]) == 2
    for h in (flt, grp, pri):
        h.close()
    grow = make()                                # a grouping and a prior made at 1,000 rows and edited at 3,000: their arrays grow
    grow.add(X[:1000])
    grp, pri = grow.make_grouping(), grow.make_prior()
    grp.set_ids([10], 4)
    pri.set_ids([10], 2.0)
    grow.add(X[1000:])
    grp.set_ids([2500], 5)
    pri.set_ranges([[2400, 2600]], 3.0)
    assert list(grp.keys_of([10, 2500])) == [4, 5] and list(pri.values_of([10, 2500])) == [2.0, 3.0]
    for h in (grow, grp, pri):
        h.close()
    assert idx.remove(np.arange(1, 600, 3)) == 200
    idx.search(Q, K)
    assert len(idx.compact()) == 2800
    idx.set_filter_copy(0)
    idx.search(Q, K)
    idx.set_filter_copy(3)
    idx.search(Q, K)
    idx.save(store)
    idx.load(store)
    ids, _, _, nf = idx.search(Q, 300)           # k > 256: the EXACT path
    assert (nf == 300).all()
    idx.close()
    assert live() > 0                            # the grouping and the prior left open keep the index
    for h in kept:
        h.close()
    assert live() == 0, live()                   # exact: every buffer of the index, its scratch and its handles is gone

assert live() == 0
cycle(lambda: FlatIndex(128), True, os.path.join(sys.argv[1], "plain"))
cycle(lambda: FlatIndex(128, devices=[0, 0], block_rows=512), False, os.path.join(sys.argv[1], "sharded"))
print("OWNERSHIP_OK")
'''

_FAILED_ALLOCS = _PRELUDE + r'''
def armed(n, call):
    """call() with the n-th next allocation failing -> (its mx_status, allocations it asked for); disarmed on the way out"""
    L.mx_testing_fail_alloc(n)
    try:
        call()
        rc = _lib.MX_OK
    except _lib.MemexHipError as e:
        rc = e.code
    return rc, L.mx_testing_fail_alloc(0)

# ---- mx_index_open: allocation and memset only
box = []
rc, n_open = armed(0, lambda: box.append(FlatIndex(128)))
assert rc == _lib.MX_OK and n_open >= 3
box.pop().close()
assert live() == 0
for n in range(1, n_open + 1):
    rc, _ = armed(n, lambda: box.append(FlatIndex(128)))
    assert rc == _lib.MX_ENOMEM and not box, (n, rc)
    assert live() == 0, (n, live())
# ---- reserve() on an empty index: allocation, memset and copy only
idx = FlatIndex(128)
rc, n_res = armed(0, lambda: idx.reserve(4096))
assert rc == _lib.MX_OK and n_res >= 3
idx.close()
assert live() == 0
soft = 0
for n in range(1, n_res + 1):
    idx = FlatIndex(128)
    rc, _ = armed(n, lambda: idx.reserve(4096))
    assert rc in (_lib.MX_OK, _lib.MX_ENOMEM), (n, rc)
    if rc == _lib.MX_OK:                         # the filter copy did not fit: the index goes on without it
        soft += 1
        idx.add(X)
        same_as_oracle(idx.search(Q, K))
        assert idx.stats().filter_kind == 0
    idx.close()
    assert live() == 0, (n, live())
assert soft >= 1 and n_res - soft == 2           # the f32 rows and their norms are required, the filter copy is not
with FlatIndex(128) as idx:                      # ... and nothing of the sweep lingers
    idx.add(X)
    same_as_oracle(idx.search(Q, K))
    assert idx.stats().filter_kind != 0
assert live() == 0
# ---- mx_grouping_create, mx_prior_create on a populated index: allocation, memset and copy only
idx = FlatIndex(128)
idx.add(X)
base = live()
for make in (idx.make_grouping, idx.make_prior):
    rc, n_make = armed(0, lambda: box.append(make()))
    assert rc == _lib.MX_OK and n_make >= 1
    box.pop().close()
    assert live() == base
    for n in range(1, n_make + 1):
        rc, _ = armed(n, lambda: box.append(make()))
        assert rc == _lib.MX_ENOMEM and not box, (n, rc)
        assert live() == base, (n, live(), base)
same_as_oracle(idx.search(Q, K))
idx.close()
assert live() == 0
print("OWNERSHIP_OK")
'''


def _child(code, *args):
    env = dict(os.environ, MEMEX_HIP_EXCHANGE="p2p")   # (the testing build's one-off all-gather injection plays no part)
    r = subprocess.run([sys.executable, "-c", code, *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OWNERSHIP_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_every_buffer_is_released_with_its_owner(lib_built, tmp_path):
    """One cycle through every feature that allocates -- open, add, each kind of search, a resident filter, a grouping and a prior
    (edited, read, grown, named in the grouped, group-rows, capped and boosted searches and in filters by predicate), remove,
    compact, both filter-copy switches, save, load, the EXACT path, close -- on a plain index and on two logical shards, a second
    index opened and closed meanwhile, a grouping and a prior closed only after their index: after the last close the testing
    library counts exactly 0 live buffers.  The first search is compared bit for bit with the oracle, so the scenario cannot pass
    by doing nothing."""
    _child(_CYCLE, str(tmp_path))


def test_failed_allocations_leak_nothing(lib_built):
    """Every allocation of mx_index_open, of reserve() on an empty index, and of mx_grouping_create and mx_prior_create on a
    populated one fails in turn (the hook is armed across those calls only: none launches a kernel).  The call returns MX_OK or
    MX_ENOMEM, and after closing whatever was opened nothing is live; a failed create leaves the live count where it was and the
    index answering like the oracle.  A failed filter-copy allocation stays soft: reserve() returns MX_OK and the index answers
    like the oracle from its f32 rows (filter_kind 0)."""
    _child(_FAILED_ALLOCS)


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_encoder_cycles_return_their_memory(precision, lib_built):
    """Create / encode / close of a small encoder, four times: free device memory after cycles 2 and 3 equals that after cycle 1
    (the first cycle warms the runtime up) within SLACK.  The testing library does not count the encoder's buffers, so this
    check is coarse: it sees a leak of the weights or the workspace (6 MiB and up per cycle here), not of a small buffer.  The
    fine net is the owning type itself (tests/cpp/test_owned_buf.cpp): the encoder has no free list left to forget a name in.
    SLACK: twice the largest cycle-to-cycle difference at the parent commit, not less than two 2 MiB granules.  Measured at the
    parent commit with this same test: 0 bytes between any two cycles in both modes (an open encoder of this shape holds
    52 MiB of device memory in bf16 and 28 MiB in bf16x3, all of it back after close), so SLACK is the floor, 4 MiB."""
    from memex_amd.encoder import Encoder
    from memex_amd.weights import EncoderConfig, synthetic_weights
    SLACK = 2 * (2 << 20)
    cfg = EncoderConfig(layers=1, hidden=384, heads=12, ffn=1536, vocab=2000, precision=precision)
    w = synthetic_weights(cfg, 3)
    rng = np.random.default_rng(3)
    ids = rng.integers(1000, cfg.vocab, size=(4, 48)).astype(np.int32)
    lens = np.array([48, 1, 17, 33], dtype=np.int32)
    free = []
    for _ in range(4):
        with Encoder(cfg, w) as enc:
            assert np.isfinite(enc.encode(ids, lens)).all()
        free.append(_free_bytes())
    print("free bytes after each cycle, relative to the first:", [f - free[0] for f in free])
    assert abs(free[2] - free[1]) <= SLACK and abs(free[3] - free[1]) <= SLACK, [f - free[1] for f in free]
