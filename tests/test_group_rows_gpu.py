"""Grouped search with members (mx_index_search_group_rows, mx_index_search_capped, mx_grouping_key_counts) on
the GPU against its statement in NumPy (tests/group_rows_model.py).  Every case compares every output, blanks included: integers by
equality, scores and dists by their bits.  The shapes are small: the kernel never looks past the top-`fetch` list."""
import numpy as np
import pytest

from conftest import bits
from group_rows_model import capped_lists, group_rows_lists, key_counts_model, settle_model
from grouped_model import candidate_lists, random_keys, row_keys
from mmr_model import near_copy_corpus, queries_near_centres

pytestmark = pytest.mark.gpu

N, D = 2000, 64
FETCHES = (17, 64, 256, 300, 1025, 4096)       # not a multiple of 4; AUTO; the EXACT path; two numbering rounds; more than the rows
ROWS_NAMES = ("ids", "scores", "dists", "keys", "group_rows", "n_members", "members_complete", "n_found", "complete")
CAPPED_NAMES = ("ids", "scores", "dists", "keys", "n_found", "complete")
_CACHE = {}


def small():
    """the near-copy corpus (200 clusters x 10 rows x 64 dims), 33 queries near cluster centres, and two key arrays.  `many`: groups
    of 1 - 40 rows, a fifth of the rows at key 0; the first 1000 rows are cut into groups in cluster order (the rows of a group meet
    at the head of a list), the rest in a random order (the rows of a group lie anywhere in a list of all rows: on both sides of entry
    1023 / 1024).  `one`: a fifth at key 0, every other row under key 5."""
    if "small" not in _CACHE:
        rng = np.random.default_rng(3190)
        X, centres = near_copy_corpus(rng, clusters=N // 10, per=10, d=D)
        Q = queries_near_centres(rng, centres[rng.choice(len(centres), 33, replace=False)], 33).astype(np.float32)
        many = random_keys(rng, N, biggest=40, order=np.concatenate([np.arange(1000), 1000 + rng.permutation(1000)]))
        one = np.where(rng.random(N) < 0.2, 0, 5).astype(np.uint32)
        _CACHE["small"] = (X, centres, Q, many, one)
    return _CACHE["small"]


def lists(oracle, name, rows, Q, fetch, **kw):
    """the oracle's candidate lists, computed once per named case"""
    if (name, fetch) not in _CACHE:
        _CACHE[name, fetch] = candidate_lists(oracle, rows, Q, fetch, **kw)
    return _CACHE[name, fetch]


def same(got, want, names, what):
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        if name in ("scores", "dists"):
            g, w = bits(g), bits(w)
        np.testing.assert_array_equal(np.asarray(g), np.asarray(w), err_msg=f"{what}: {name}")


def own_lists(idx, Q, fetch, flt=None):
    return idx.search(Q, fetch) if flt is None else idx.search_with(flt, Q, fetch)


def set_keys(grp, keys, id_offset=0):
    grp.set_ids(np.arange(1, len(keys) + 1, dtype=np.uint64) + np.uint64(id_offset), keys)


def check_both(idx, grp, oracle, name, rows, Q, keys, k, n, per_key, fetch, flt=None, id_offset=0, **kw):
    """both forms at one fetch against the model over the oracle's lists"""
    L = lists(oracle, name, rows, Q, fetch, id_offset=id_offset, **kw)
    rk = row_keys(keys, len(rows))
    same(idx.search_group_rows(grp, Q, k, n, fetch=fetch, flt=flt), group_rows_lists(*L, rk, k, n, fetch, id_offset), ROWS_NAMES,
         f"{name}: group rows k {k} n {n} fetch {fetch}")
    same(idx.search_capped(grp, Q, k, per_key, fetch=fetch, flt=flt), capped_lists(*L, rk, k, per_key, fetch, id_offset), CAPPED_NAMES,
         f"{name}: capped k {k} per_key {per_key} fetch {fetch}")


@pytest.fixture(scope="module")
def plain(lib_built):
    """one index with the rows of small() and a grouping per key array, shared by the tests that change neither"""
    from memex_amd.index import FlatIndex
    X, _, _, many, one = small()
    with FlatIndex(D) as idx, idx.make_grouping() as gm, idx.make_grouping() as go:
        idx.add(X)
        set_keys(gm, many)
        set_keys(go, one)
        yield idx, gm, go


# ---- both forms against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 10])
def test_group_rows_equals_the_model(k, oracle, plain):
    idx, gm, go = plain
    X, _, Q, many, one = small()
    Q = Q[:5]
    seen = dict(short=False, beyond=False, partial=False, open=False)
    for fetch in sorted({k} | set(FETCHES)):
        L = lists(oracle, "small5", X, Q, fetch)
        for n in (1, 2, 5, 16):
            for grp, keys, tag in ((gm, many, "many"), (go, one, "one")):
                if tag == "one" and n in (2, 5) and fetch not in (k, 300):
                    continue
                got = idx.search_group_rows(grp, Q, k, n, fetch=fetch)
                want = group_rows_lists(*L, keys, k, n, fetch)
                same(got, want, ROWS_NAMES, f"{tag} k {k} n {n} fetch {fetch}")
                seen["short"] |= bool((want[7] < k).any())
                seen["partial"] |= bool(((want[5] > 1) & (want[5] < n)).any())
                seen["open"] |= bool((~want[6] & (want[5] > 0)).any())
                seen["beyond"] |= bool((L[3] > want[4].sum(axis=1)).any())           # entries under heads behind the first k
        own = own_lists(idx, Q, fetch)                                  # the lists of this run are the oracle's
        same(own, (L[0], L[1], L[2], L[3]), ("ids", "scores", "dists", "n_found"), f"lists at fetch {fetch}")
    assert seen["partial"] and seen["open"] and seen["beyond"], seen     # (conditions on the input)
    assert seen["short"] or k == 1, seen


@pytest.mark.parametrize("k", [1, 3, 10])
def test_capped_equals_the_model(k, oracle, plain):
    idx, gm, go = plain
    X, _, Q, many, one = small()
    Q = Q[:5]
    short = False
    for fetch in sorted({k} | set(FETCHES)):
        L = lists(oracle, "small5", X, Q, fetch)
        for per_key in (1, 2, 7, fetch):
            for grp, keys, tag in ((gm, many, "many"), (go, one, "one")):
                want = capped_lists(*L, keys, k, per_key, fetch)
                same(idx.search_capped(grp, Q, k, per_key, fetch=fetch), want, CAPPED_NAMES, f"{tag} k {k} per_key {per_key} fetch {fetch}")
                short |= bool((want[4] < k).any())
    assert short or k == 1                                              # (condition on the input)


@pytest.mark.parametrize("B", [1, 33])
def test_other_batch_sizes(B, oracle, plain):
    idx, gm, _ = plain
    X, _, Q, many, _ = small()
    for k, n, per_key, fetch in ((3, 5, 2, 17), (10, 2, 7, 300), (10, 16, 1, 1025)):
        check_both(idx, gm, oracle, f"small{B}", X, Q[:B], many, k, n, per_key, fetch)
    one = idx.search_group_rows(gm, Q[0], 3, 2)                         # [dim]: one query, the default fetch 32
    same(one, idx.search_group_rows(gm, Q[:1], 3, 2, fetch=32), ROWS_NAMES, "default fetch")
    same(idx.search_capped(gm, Q[0], 10, 2), idx.search_capped(gm, Q[:1], 10, 2, fetch=40), CAPPED_NAMES, "default fetch, capped")


def test_two_batches(plain):
    """600 queries: batches of 512 and 88, against the model over the lists of this run"""
    idx, gm, _ = plain
    X, centres, _, many, _ = small()
    Q = queries_near_centres(np.random.default_rng(3191), centres, 600).astype(np.float32)
    L = own_lists(idx, Q, 12)
    got = idx.search_group_rows(gm, Q, 4, 3, fetch=12)
    same(got, group_rows_lists(*L, many, 4, 3, 12), ROWS_NAMES, "600 queries")
    assert (~got[8]).any() and got[8].any() and (~got[6][got[5] > 0]).any()                   # (conditions on the input)
    got = idx.search_capped(gm, Q, 8, 2, fetch=12)
    same(got, capped_lists(*L, many, 8, 2, 12), CAPPED_NAMES, "600 queries, capped")
    assert (~got[5]).any() and got[5].any()


def test_the_limits(oracle, plain):
    idx, gm, go = plain
    X, _, Q, many, one = small()
    Q = Q[:3]
    L = lists(oracle, "small3", X, Q, 4096)
    got = idx.search_group_rows(gm, Q, 256, 16, fetch=4096)             # k * n = 4096: the widest staging
    same(got, group_rows_lists(*L, many, 256, 16, 4096), ROWS_NAMES, "k 256 n 16")
    assert (got[7] == 256).all() and (got[4] > 16).any() and got[6].all()
    got = idx.search_group_rows(gm, Q, 4096, 1, fetch=4096)             # 2000 rows: fewer heads than k, a short list: complete
    same(got, group_rows_lists(*L, many, 4096, 1, 4096), ROWS_NAMES, "k 4096 n 1")
    assert (got[7] < 2000).all() and got[8].all()
    got = idx.search_group_rows(go, Q, 10, 16, fetch=64)                # one large group: sixteen members of many more
    same(got, group_rows_lists(*lists(oracle, "small3", X, Q, 64), one, 10, 16, 64), ROWS_NAMES, "one large group")
    assert (got[4] > 16).any() and (got[5] == 16).any()
    got = idx.search_capped(go, Q, 4096, 7, fetch=4096)
    same(got, capped_lists(*L, one, 4096, 7, 4096), CAPPED_NAMES, "capped k 4096")
    assert got[5].all() and (got[4] == int((one == 0).sum()) + 7).all()
    e = idx.search_group_rows(gm, np.zeros((0, D), np.float32), 5, 3)   # B = 0
    assert e[0].shape == (0, 5, 3) and e[3].shape == (0, 5) and e[7].shape == (0,)
    assert idx.search_capped(gm, np.zeros((0, D), np.float32), 5, 2)[0].shape == (0, 5)


def test_an_index_without_rows_and_an_empty_grouping(lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q, _, _ = small()
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        got = idx.search_group_rows(grp, Q[:3], 5, 4)
        assert (got[7] == 0).all() and got[8].all() and (got[0] == 0).all() and np.isposinf(got[2]).all() and not got[6].any()
        got = idx.search_capped(grp, Q[:3], 5, 2)
        assert (got[4] == 0).all() and got[5].all() and (got[0] == 0).all() and np.isposinf(got[2]).all()
        r, l = grp.key_counts([0, 3])
        assert r.tolist() == [0, 0] and l.tolist() == [0, 0]
        idx.add(X[:500])                                                # key 0 everywhere: every row heads a group of one
        ids, sc, di, nf = idx.search(Q[:3], 10)
        got = idx.search_group_rows(grp, Q[:3], 10, 3, fetch=10)
        np.testing.assert_array_equal(got[0][:, :, 0], ids)
        np.testing.assert_array_equal(bits(got[1][:, :, 0]), bits(sc))
        assert (got[0][:, :, 1:] == 0).all() and (got[5] == 1).all() and got[6].all() and got[8].all()
        r, l = grp.key_counts([0])
        assert r.tolist() == [500] and l.tolist() == [500]


# ---- the identities -------------------------------------------------------------------------------------------------------------------
def test_identities(plain):
    idx, gm, go = plain
    _, _, Q, _, _ = small()
    for grp in (gm, go):
        for k, fetch in ((1, 1), (3, 17), (10, 64), (10, 300), (10, 1025), (300, 4096)):
            g = idx.search_grouped(grp, Q, k, fetch=fetch)
            r = idx.search_group_rows(grp, Q, k, 1, fetch=fetch)
            same((r[0][:, :, 0], r[1][:, :, 0], r[2][:, :, 0], r[3], r[4], r[7], r[8]), g,
                 ("ids", "scores", "dists", "keys", "group_rows", "n_found", "complete"), f"n = 1 vs grouped, k {k} fetch {fetch}")
            c = idx.search_capped(grp, Q, k, 1, fetch=fetch)
            same(c, (g[0], g[1], g[2], g[3], g[5], g[6]), CAPPED_NAMES, f"per_key = 1 vs grouped, k {k} fetch {fetch}")
            c = idx.search_capped(grp, Q, k, fetch, fetch=fetch)
            p = idx.search(Q, k)
            same(c[:3] + (c[4],), p, ("ids", "scores", "dists", "n_found"), f"per_key = fetch vs search, k {k} fetch {fetch}")
            assert c[5].all()


def test_device_pointer_variants_equal_the_host_variants(lib_built):
    import torch
    from memex_amd.index import FlatIndex
    X, _, Q, many, _ = small()
    Q = Q[:6]
    with FlatIndex(D) as pl, FlatIndex(D, devices=[0, 0], block_rows=64) as sh:
        for idx in (pl, sh):
            idx.add(X)
            with idx.make_grouping() as grp, idx.make_filter(ranges=[[301, 1501]]) as flt:
                set_keys(grp, many)
                for k, n, fetch, extras, f in ((10, 3, None, True, None), (7, 16, 300, True, flt), (7, 2, 12, False, None)):
                    B = len(Q)
                    new = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")  # noqa: E731
                    q = torch.from_numpy(Q).cuda()
                    ids, sc, nf = new((B, k, n), torch.int64, -1), new((B, k, n), torch.float32, -1.0), new((B,), torch.int32, -1)
                    di = new((B, k, n), torch.float32, -1.0) if extras else None
                    gk, rows, mem = (new((B, k), torch.int32, -7) if extras else None for _ in range(3))
                    mc = new((B, k), torch.uint8, 9) if extras else None
                    done = new((B,), torch.uint8, 9) if extras else None
                    idx.search_group_rows_device(grp, q, k, n, ids, sc, di, gk, rows, mem, mc, nf, done, fetch=fetch, flt=f)
                    h = idx.search_group_rows(grp, Q, k, n, fetch=fetch, flt=f)
                    np.testing.assert_array_equal(ids.cpu().numpy().astype(np.uint64), h[0])
                    np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(h[1]))
                    np.testing.assert_array_equal(nf.cpu().numpy(), h[7])
                    if extras:
                        np.testing.assert_array_equal(bits(di.cpu().numpy()), bits(h[2]))
                        np.testing.assert_array_equal(gk.cpu().numpy().view(np.uint32), h[3])
                        np.testing.assert_array_equal(rows.cpu().numpy(), h[4])
                        np.testing.assert_array_equal(mem.cpu().numpy(), h[5])
                        np.testing.assert_array_equal(mc.cpu().numpy().astype(bool), h[6])
                        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), h[8])
                    ids, sc = new((B, k), torch.int64, -1), new((B, k), torch.float32, -1.0)
                    di = new((B, k), torch.float32, -1.0) if extras else None
                    gk = new((B, k), torch.int32, -7) if extras else None
                    cfetch = 40 if fetch is None else fetch
                    idx.search_capped_device(grp, q, k, n, ids, sc, di, gk, nf, done, fetch=cfetch, flt=f)
                    h = idx.search_capped(grp, Q, k, n, fetch=cfetch, flt=f)
                    np.testing.assert_array_equal(ids.cpu().numpy().astype(np.uint64), h[0])
                    np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(h[1]))
                    np.testing.assert_array_equal(nf.cpu().numpy(), h[4])
                    if extras:
                        np.testing.assert_array_equal(bits(di.cpu().numpy()), bits(h[2]))
                        np.testing.assert_array_equal(gk.cpu().numpy().view(np.uint32), h[3])
                        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), h[5])


# ---- removed rows, an id offset, a filter, the copy kinds, shards -------------------------------------------------------------------
CASES = ((3, 5, 2, 17), (10, 2, 7, 64), (10, 16, 1, 300), (3, 2, 2, 1025), (10, 5, 4096, 4096))


def test_removed_rows_an_id_offset_and_a_filter(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q, many, _ = small()
    Q = Q[:5]
    rng = np.random.default_rng(3192)
    gone = rng.choice(N, 300, replace=False)
    alive = np.ones(N, bool)
    alive[gone] = False
    allowed = np.zeros(N, bool)
    allowed[300:1500] = True
    off = 7000
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(X)
        idx.set_id_offset(off)
        set_keys(grp, many, off)
        idx.remove(gone.astype(np.uint64) + np.uint64(off + 1))
        with idx.make_filter(ranges=[[off + 301, off + 1501]]) as flt:
            for k, n, per_key, fetch in CASES:
                check_both(idx, grp, oracle, "removed", X, Q, many, k, n, per_key, fetch, id_offset=off, alive=alive)
                check_both(idx, grp, oracle, "filtered", X, Q, many, k, n, per_key, fetch, flt=flt, id_offset=off, alive=alive,
                           allowed=allowed)
            got = idx.search_group_rows(grp, Q, 10, 5, fetch=64, flt=flt)
            rows = got[0][got[0] != 0].astype(np.int64) - 1 - off
            assert allowed[rows].all() and alive[rows].all()
        # key_counts after removals, with repeated keys, key 0 and a key nobody has
        asked = np.concatenate([[0, 1, 1, 0, 4000000000], rng.integers(0, int(many.max()) + 3, 200)]).astype(np.uint32)
        r, l = grp.key_counts(asked)
        wr, wl = key_counts_model(many, N, asked, alive)
        np.testing.assert_array_equal(r, wr)
        np.testing.assert_array_equal(l, wl)
        assert (l < r).any() and r[4] == 0 and r[0] == r[3] == int((many == 0).sum())
        assert grp.key_counts([])[0].shape == (0,)
        # settle raises exactly the flags the group sizes allow
        Q = small()[2]                                                  # 33 queries: a few small groups lie whole in their lists
        got = idx.search_group_rows(grp, Q, 10, 16, fetch=64)
        assert (~got[6][got[5] > 0]).any()                              # (condition on the input)
        want = settle_model(got[3], got[5], got[6], got[7], many, N, alive)
        settled = idx.search_group_rows(grp, Q, 10, 16, fetch=64, settle=True)
        same(settled[:6] + settled[7:], got[:6] + got[7:], ROWS_NAMES[:6] + ROWS_NAMES[7:], "settle changes the flags only")
        np.testing.assert_array_equal(settled[6], want)
        assert (want != got[6]).any() and not want[got[5] > 0].all()    # (conditions on the input)


def test_key_counts_on_a_grouping_shorter_than_the_index(lib_built):
    from memex_amd.index import FlatIndex
    X, _, _, many, _ = small()
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        idx.add(X[:1000])
        set_keys(grp, many[:1000])
        idx.add(X[1000:])                                               # appended after the last edit: key 0
        idx.remove(np.arange(990, 1100, dtype=np.uint64))
        alive = np.ones(N, bool)
        alive[989:1099] = False
        asked = np.arange(0, int(many[:1000].max()) + 2, dtype=np.uint32)
        r, l = grp.key_counts(asked)
        wr, wl = key_counts_model(many[:1000], N, asked, alive)
        np.testing.assert_array_equal(r, wr)
        np.testing.assert_array_equal(l, wl)
        assert r[0] >= 1000 and int(r.sum()) == N and int(l.sum()) == int(alive.sum())


# (name, setup)
_KINDS = [("int8", lambda idx: idx.set_filter_copy("i8")), ("bf16", lambda idx: idx.set_filter_copy("bf16")), ("compressed", "compressed")]


@pytest.mark.parametrize("name,setup", _KINDS, ids=[c[0] for c in _KINDS])
def test_every_copy_kind_matches_the_model(name, setup, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q, many, _ = small()
    with FlatIndex(D) as idx, idx.make_grouping() as grp:
        if setup == "compressed":
            idx.set_corpus_mode("bf16")
        idx.add(X)
        if callable(setup):
            setup(idx)
        set_keys(grp, many)
        rows = idx.get_rows(0, len(X)) if setup == "compressed" else X
        assert setup != "compressed" or (rows != X).any()              # the model is fed what the index stores
        for k, n, per_key, fetch in CASES[:3]:
            check_both(idx, grp, oracle, "compressed" if setup == "compressed" else "small3k", rows, Q[:3], many, k, n, per_key, fetch)


@pytest.mark.parametrize("shards,block", [(3, 96), (2, 64)], ids=["3-shards", "2-shards"])
def test_sharded_equals_plain(shards, block, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, _, Q, many, _ = small()
    Q = Q[:5]
    gone = np.concatenate([np.arange(block, block + 30), np.arange(2 * block + 5, 2 * block + 25)])   # rows of the second and third block
    alive = np.ones(N, bool)
    alive[gone] = False
    with FlatIndex(D) as pl, FlatIndex(D, devices=[0] * shards, block_rows=block) as sh:
        grps = []
        for idx in (pl, sh):
            idx.add(X)
            idx.remove(gone.astype(np.uint64) + np.uint64(1))
            grps.append(idx.make_grouping())
            set_keys(grps[-1], many)
        try:
            for k, n, per_key, fetch in CASES:
                check_both(sh, grps[1], oracle, ("sharded", block), X, Q, many, k, n, per_key, fetch, alive=alive)
                same(sh.search_group_rows(grps[1], Q, k, n, fetch=fetch), pl.search_group_rows(grps[0], Q, k, n, fetch=fetch), ROWS_NAMES,
                     f"{shards} shards vs plain")
                same(sh.search_capped(grps[1], Q, k, per_key, fetch=fetch), pl.search_capped(grps[0], Q, k, per_key, fetch=fetch),
                     CAPPED_NAMES, f"{shards} shards vs plain, capped")
            asked = np.arange(0, 60, dtype=np.uint32)
            wr, wl = key_counts_model(many, N, asked, alive)
            for g in grps:
                r, l = g.key_counts(asked)
                np.testing.assert_array_equal(r, wr)
                np.testing.assert_array_equal(l, wl)
            assert (wl < wr).any()                                      # (condition on the input)
            with sh.make_filter(ranges=[[301, 1501]]) as fs, pl.make_filter(ranges=[[301, 1501]]) as fp:
                same(sh.search_group_rows(grps[1], Q, 10, 5, fetch=64, flt=fs), pl.search_group_rows(grps[0], Q, 10, 5, fetch=64, flt=fp),
                     ROWS_NAMES, f"{shards} shards vs plain, filtered")
        finally:
            for g in grps:
                g.close()


# ---- stale and foreign handles --------------------------------------------------------------------------------------------------------
def test_staleness_and_foreign_handles(lib_built, tmp_path):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    X, _, Q, many, _ = small()
    Q = Q[:3]

    def stale(idx, grp):
        for call in (lambda: idx.search_group_rows(grp, Q, 5, 3), lambda: idx.search_capped(grp, Q, 5, 2), lambda: grp.key_counts([1, 2])):
            with pytest.raises(_lib.MemexHipError, match="stale") as e:
                call()
            assert e.value.code == _lib.MX_EINVAL
        grp.close()

    with FlatIndex(D) as idx, FlatIndex(D) as other:
        idx.add(X)
        other.add(X[:100])
        grp = idx.make_grouping()
        set_keys(grp, many)
        for call in (lambda: other.search_group_rows(grp, Q, 5, 3), lambda: other.search_capped(grp, Q, 5, 2)):
            with pytest.raises(_lib.MemexHipError, match="another index") as e:
                call()
            assert e.value.code == _lib.MX_EINVAL
        with other.make_filter(ranges=[[1, 50]]) as foreign:
            for call in (lambda: idx.search_group_rows(grp, Q, 5, 3, flt=foreign), lambda: idx.search_capped(grp, Q, 5, 2, flt=foreign)):
                with pytest.raises(_lib.MemexHipError, match="another index") as e:
                    call()
                assert e.value.code == _lib.MX_EINVAL
        bad = Q.copy()
        bad[1, 3] = np.nan
        with pytest.raises(_lib.MemexHipError, match="non-finite"):
            idx.search_group_rows(grp, bad, 5, 3)
        with pytest.raises(_lib.MemexHipError, match="non-finite"):
            idx.search_capped(grp, bad, 5, 2)
        idx.remove([5, 150])
        idx.compact()
        stale(idx, grp)
        grp = idx.make_grouping()
        idx.save(str(tmp_path))
        idx.load(str(tmp_path))
        stale(idx, grp)
        grp = idx.make_grouping()
        idx.clear()
        stale(idx, grp)
