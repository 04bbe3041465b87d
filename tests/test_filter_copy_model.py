"""The CPU model of the filter copies (tests/filter_copy_model.py) checked against itself and against what the kernels' comments
claim: the rotation of mx_rotate.h is orthonormal and spreads one-hot vectors and Hadamard rows, the bound prep_queries_kernel
computes covers the under-score the model predicts, and the adversarial query uses several times the share of that bound a
random query does -- which is why tests/test_certificate_adversary_gpu.py exists."""
import numpy as np
import pytest

import filter_copy_model as M


def cone_rows(rng, n, d, spread=0.2, axis_seed=1):       # (tests/test_centred_gpu.py's corpus; that module needs a GPU mark)
    axis = np.random.default_rng(axis_seed).standard_normal(d).astype(np.float32)
    axis /= np.linalg.norm(axis)
    x = axis[None, :] + (spread / np.sqrt(d)) * rng.standard_normal((n, d), dtype=np.float32)
    return (x * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("m", range(1, 13))
def test_rotation_is_orthonormal_and_spreads(m):
    ds = 128 * m
    T = M.rotation(ds)
    assert np.abs(T @ T.T - np.eye(ds)).max() <= 1e-12
    assert np.abs(T.T @ T - np.eye(ds)).max() <= 1e-12
    lim = 4.0 / np.sqrt(ds)
    assert np.abs(T).max() < lim                                         # every one-hot vector (the columns of T)
    # a Hadamard row over the whole width (H_128 rows side by side): the sign diagonal keeps it from collapsing into one element
    i = np.arange(128)
    H = np.where(np.array([[bin(a & b).count("1") & 1 for b in i] for a in i]), -1.0, 1.0) / np.sqrt(128.0)
    W = np.tile(H, (1, m)) / np.sqrt(m)
    assert np.abs(W @ T.T).max() < lim, m
    # a Hadamard row inside ONE block (zeros elsewhere) is spread over its block by H D, and over the blocks by one COLUMN of the
    # DCT-II matrix, whose entries reach sqrt(2 / m), not 1 / sqrt(m): the limit that follows is sqrt(2) times the header's
    # (measured: 4.5 / sqrt(ds) at m = 3)
    for blk in range(m):
        V = np.zeros((128, ds))
        V[:, 128 * blk: 128 * blk + 128] = H
        assert np.abs(V @ T.T).max() < (lim if m == 1 else np.sqrt(2.0) * lim), (m, blk)


def test_rotation_matches_a_direct_restatement():
    """T x for one vector, written as the three factors of the header's formula (D, H_128 by its closed form, DCT-II across blocks)"""
    ds, m = 384, 3
    rng = np.random.default_rng(0)
    x = rng.standard_normal(ds)
    i = np.arange(128)
    H = np.where(np.array([[bin(a & b).count("1") & 1 for b in i] for a in i]), -1.0, 1.0) / np.sqrt(128.0)
    y = (x * M.rot_sign(np.arange(ds))).reshape(m, 128) @ H.T
    k = np.arange(m)[:, None]
    j = np.arange(m)[None, :]
    C = np.sqrt(np.where(k > 0, 2.0, 1.0) / m) * np.cos(np.pi * (2 * j + 1) * k / (2.0 * m))
    np.testing.assert_allclose(M.rotation(ds) @ x, (C @ y).reshape(ds), atol=1e-13)
    assert M.rot_sign(0) == -1.0 or M.rot_sign(0) == 1.0
    assert {float(v) for v in M.rot_sign(np.arange(4096))} == {-1.0, 1.0}


def _kinds(rng, n, d):
    G = rng.standard_normal((n, d)).astype(np.float32)
    C = cone_rows(rng, n, d)
    yield "i8", M.int8_copy(G), None, G
    yield "i8 centred", M.int8_copy(C, M.mean_direction(C)), M.mean_direction(C), C
    yield "bf16", M.bf16_copy(G), None, G
    yield "bf16 centred", M.bf16_copy(C, M.mean_direction(C)), M.mean_direction(C), C


def _queries(name, cp, mean, X, rng, victims):
    d = X.shape[1]
    for q in rng.standard_normal((4, d)).astype(np.float32):
        yield "random", None, q
    for q in X[:3]:
        yield "a row", None, q
    for v in victims:
        q = M.adversary(cp, v, 0.3)
        yield "adversary", v, q
        if cp.kind == "i8":
            yield "sharpened", v, M.sharpen(cp, v, q)
        elif mean is None:
            yield "sharpened", v, M.sharpen_bf16(cp, v, q)
        if mean is not None:
            q = M.adversary(cp, v, 0.3, a_q=0.0)
            yield "off the cone", v, q
            if cp.kind == "i8":
                yield "off the cone, sharpened", v, M.sharpen(cp, v, q)


@pytest.mark.parametrize("d", [128, 384, 640])
def test_predicted_error_stays_within_the_models_own_bound(d):
    rng = np.random.default_rng(d)
    for name, cp, mean, X in _kinds(rng, 512, d):
        victims = M.pick_victims(cp, np.arange(cp.n), 6)
        for what, v, q in _queries(name, cp, mean, X, rng, victims):
            qs = M.query_side(q, cp.kind, mean, cp)
            score, under, bound = M.predict(cp, qs)
            assert (np.abs(under) <= bound).all(), (name, what, float((np.abs(under) / bound).max()))
            assert bound.max() <= qs.e1 * (1 + 1e-6), (name, what)
            if v is not None:                                                # the victim is the row the query under-scores most
                assert int(np.argmax(under)) == v and under[v] > 0, (name, what)


def test_adversary_uses_most_of_the_int8_bound_and_random_queries_do_not():
    """Gaussian rows, d = 384, 4096 rows: a random query's worst row uses 0.14 of qa + qb * e_h; the adversary 0.58-0.67 (measured
    with this model; the first draft of it, with victims taken as they came, gave 0.51 at the low end); with the query's own
    residual aimed as well, 0.85-0.87.  A bound several times too small passes every random test."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((4096, 384)).astype(np.float32)
    cp = M.int8_copy(X)
    worst = 0.0
    for q in rng.standard_normal((8, 384)).astype(np.float32):
        _, under, bound = M.predict(cp, M.query_side(q, "i8", None, cp))
        worst = max(worst, float((np.abs(under) / bound).max()))
    assert worst < 0.2, worst
    plain, sharp = [], []
    for v in M.pick_victims(cp, np.arange(cp.n), 43):
        q = M.adversary(cp, v, 0.3)
        _, under, bound = M.predict(cp, M.query_side(q, "i8", None, cp))
        plain.append(under[v] / bound[v])
        _, under, bound = M.predict(cp, M.query_side(M.sharpen(cp, v, q), "i8", None, cp))
        sharp.append(under[v] / bound[v])
    assert min(plain) >= 0.5, min(plain)
    assert min(sharp) >= 0.8, min(sharp)
    print(f"random {worst:.3f}  adversary {min(plain):.3f}-{max(plain):.3f}  sharpened {min(sharp):.3f}-{max(sharp):.3f}")


def test_adversary_shares_of_the_other_kinds():
    """What the adversary reaches on the other three kinds (d = 384, 2048 rows), as floors: centred copies carry kAccSlack = 2.7e-4
    in a bound that is itself below 1e-3, so their shares are lower."""
    rng = np.random.default_rng(1)
    floors = {"i8 centred": 0.45, "bf16": 0.6, "bf16 centred": 0.05}
    for name, cp, mean, X in _kinds(rng, 2048, 384):
        if name == "i8":
            continue
        best = []
        for v in M.pick_victims(cp, np.arange(cp.n), 12):
            shares = []
            for what, _, q in _queries(name, cp, mean, X[:0], rng, [v]):
                if what in ("random", "a row"):
                    continue
                _, under, bound = M.predict(cp, M.query_side(q, cp.kind, mean, cp))
                shares.append(under[v] / bound[v])
            best.append(max(shares))
        print(name, f"{min(best):.3f}-{max(best):.3f}")
        assert min(best) >= floors[name], (name, min(best))


def test_unit_rows_and_bf16_rounding():
    X = np.array([[3.0, 4.0], [0.0, 0.0], [1e-20, 0.0], [1e20, 1e20]], dtype=np.float32)
    u = M.unit_rows(X)
    np.testing.assert_allclose(u[0, :2], [0.6, 0.8], rtol=1e-7)
    assert not u[1].any() and not u[2].any() and not u[3].any()      # zero norm, norm below 1e-15, norm above 1e15
    v = np.array([1.0, 1.00390625, 1.001953125, 1.005859375, -0.3333333], dtype=np.float32)
    np.testing.assert_array_equal(M.to_bf16(v), [1.0, 1.0, 1.0, 1.0078125, -0.333984375])   # ties to even
