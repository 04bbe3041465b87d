"""The encoder parity bars are reference-derived and separate what they claim (no GPU).

For every (case, precision) of tests/encoder_bars_cases.py: the floor f is what a NumPy restatement of the mode's rounding
points reaches against the f64 oracle on the case's own inputs, the bar is 4 f, and every deviation D the case claims lies at
d_D >= 2 x bar from the oracle -- so a kernel route that passes tests/test_encoder_bars_gpu.py cannot have made mistake D.
This is a condition on the test design; nothing here is measured on a GPU.  Also: the oracle without a deviation is, bit for
bit, what it was before it learnt to deviate."""
import numpy as np
import pytest

import encoder_bars_cases as C
import encoder_rounding_model as M
from oracle import bert_oracle


def test_oracle_without_a_deviation_is_bit_identical():
    """against the committed golden vectors (the bound of test_encoder_oracle.py), against a second call, and against the
    spellings of "no deviation"; every deviation moves the output."""
    from test_encoder_oracle import golden_cases
    second = 0
    for name, cfg, w, ids, lens, gold in golden_cases():
        a = bert_oracle.encode(w, cfg.as_dict(), ids, lens)
        assert np.abs(a - gold).max() < 1e-9, name
        if ids.size <= 1024:                                                                                        # a second call
            np.testing.assert_array_equal(a, bert_oracle.encode(w, cfg.as_dict(), ids, lens, deviate={}), err_msg=name)
            second += 1
    assert second > 0
    case = C.CASES[0]
    ids, lens = C.inputs(case)
    base = bert_oracle.encode(C.weights(case), case.cfg().as_dict(), ids, lens)
    np.testing.assert_array_equal(base, C.oracle(case))
    np.testing.assert_array_equal(base, bert_oracle.encode(C.weights(case), case.cfg().as_dict(), ids, lens, deviate=None))
    # the oracle's statements in the order they had before `deviate=` existed, restated here once: the same bits
    np.testing.assert_array_equal(base, _oracle_as_it_was(C.weights(case), case.cfg().as_dict(), ids, lens))
    for name in C.DEVIATIONS:
        if C.applicable(case, name) and name != "pool_div":
            assert C.distance(case, name) > 0.0, name
    with pytest.raises(ValueError):
        bert_oracle.encode(C.weights(case), case.cfg().as_dict(), ids, lens, deviate=dict(scale=1.01, gelu="tanh"))
    with pytest.raises(ValueError):
        bert_oracle.encode(C.weights(case), case.cfg().as_dict(), ids, lens, deviate=dict(key_bias=1))


def _oracle_as_it_was(weights, cfg, ids, lens):
    import math
    W = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}
    B, S = ids.shape
    H, nh, L = cfg["hidden"], cfg["heads"], cfg["layers"]
    dh = H // nh
    eps = cfg.get("ln_eps", 1e-12)
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.float64)
    x = (W["embeddings.word_embeddings.weight"][ids]
         + W["embeddings.position_embeddings.weight"][None, cfg.get("pos_offset", 0):cfg.get("pos_offset", 0) + S]
         + W["embeddings.token_type_embeddings.weight"][0][None, None, :])
    x = bert_oracle.layer_norm(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], eps)
    add_mask = (1.0 - mask)[:, None, None, :] * -10000.0
    for l in range(L):
        p = f"encoder.layer.{l}."

        def lin(t, name):
            w = W[p + name + ".weight"]
            return (t.reshape(-1, t.shape[-1]) @ w.T + W[p + name + ".bias"]).reshape(t.shape[:-1] + (w.shape[0],))

        def heads(t):
            return np.ascontiguousarray(t.reshape(B, S, nh, dh).transpose(0, 2, 1, 3))

        q, k, v = heads(lin(x, "attention.self.query")), heads(lin(x, "attention.self.key")), heads(lin(x, "attention.self.value"))
        s = q @ np.ascontiguousarray(k.transpose(0, 1, 3, 2)) / math.sqrt(dh) + add_mask
        s = s - s.max(axis=-1, keepdims=True)
        pr = np.exp(s)
        pr = pr / pr.sum(axis=-1, keepdims=True)
        ctx = (pr @ v).transpose(0, 2, 1, 3).reshape(B, S, H)
        x = bert_oracle.layer_norm(lin(ctx, "attention.output.dense") + x, W[p + "attention.output.LayerNorm.weight"],
                                   W[p + "attention.output.LayerNorm.bias"], eps)
        o = lin(bert_oracle.gelu_erf(lin(x, "intermediate.dense")), "output.dense")
        x = bert_oracle.layer_norm(o + x, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
    pooled = (x * mask[:, :, None]).sum(axis=1) / np.maximum(mask.sum(axis=1, keepdims=True), 1e-9)
    return pooled / np.maximum(np.linalg.norm(pooled, axis=1, keepdims=True), 1e-12)


@pytest.mark.parametrize("case", [c for c in C.CASES if c.name in ("m384_s33", "b768_cls_s77", "roberta768_s77", "m384_raw")],
                         ids=lambda c: c.name)
def test_model_without_rounding_is_the_oracle(case):
    """every rounding function on `ident`: f32 products only -- CLS and mean pooling, shifted position rows, un-normalised output"""
    d = C.floor(case, "exact")
    print(f"{case.name}: exact model vs oracle 1 - cos = {d:.2e}")
    assert d <= 1e-12
    if not case.cfg().normalize:
        assert C.floor_rel(case, "exact") <= 1e-5       # f32 products: 2^-24 x a few


@pytest.mark.parametrize("case,precision", C.pairs(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_bar_separates_every_claimed_deviation(case, precision):
    f, b = C.floor(case, precision), C.bar(case, precision)
    assert 0.0 < f < 1e-3
    claimed = case.claimed(precision)
    assert claimed, "a case without a claim has a bar that means nothing"
    lines = []
    for name in claimed:
        assert C.applicable(case, name), name
        if name == "pool_div":                                     # a row's length, not its direction: the element-wise measure
            fr, br, d = C.floor_rel(case, precision), C.bar_rel(case, precision), C.distance_rel(case, name)
            lines.append(f"  {name:10s} d_rel {d:.2e}  bar_rel {br:.2e}  ratio {d / 2 / br:.1f}")
            assert br <= d / 2, (case.name, precision, name, fr, br, d)
            continue
        d = C.distance(case, name)
        lines.append(f"  {name:10s} d {d:.2e}  ratio {d / 2 / b:.1f}")
        assert b <= d / 2, (case.name, precision, name, f, b, d)
    print(f"{case.name} {precision}: floor {f:.2e}  bar {b:.2e}\n" + "\n".join(lines))


def test_every_family_is_covered_on_every_precision():
    """the caps: per precision mode every deviation is claimed by at least one case that runs a route of that mode, except the
    pairs listed as not visible -- and those are at most eps / gelu / scale, never on the split-operand mode"""
    for precision in C.PRECISIONS:
        claimed = set()
        for case in C.CASES:
            if case.routed(precision):
                claimed |= set(case.claimed(precision))
        missing = set(C.DEVIATIONS) - claimed
        assert missing == set(C.NOT_VISIBLE[precision]), (precision, sorted(missing))
        assert missing <= set(C.SUBTLE)
        for fam in C.FAMILIES:
            assert any(fam in C.DEVIATIONS[n][1] for n in claimed), (precision, fam)
    assert not C.NOT_VISIBLE["bf16x3"]
    for case in C.CASES:
        for precision in C.PRECISIONS:
            assert set(case.routed(precision)) <= set(C.ROUTES)
            assert bool(case.routed(precision)) == bool(case.claimed(precision)), (case.name, precision)


def test_shape_cases_claim_the_shape_deviations():
    """every case of the shape axis claims a dropped last ffn chunk and an unscheduled last head on every precision it routes
    (test_bar_separates_every_claimed_deviation then proves the 2 x), and follows the file's rule for the rest: the members of
    _COARSE and _BIASES with a ratio of at least 1.5 are claimed, the others are not"""
    assert len(C.SHAPE_CASES) == 16 and set(C.SHAPE_CASES) <= set(C.CASES)
    for case in C.SHAPE_CASES:
        assert dict(case.kw)["layers"] == 2 and dict(case.kw)["vocab"] == 3000
        ids, lens = C.inputs(case)
        assert lens[:case.held or case.B].min() < case.S, "ragged"
        for precision in C.PRECISIONS:
            if not case.routed(precision):
                continue
            claimed = set(case.claimed(precision))
            assert {"ffn_tail", "head_last"} <= claimed, (case.name, precision)
            b = C.bar(case, precision)
            for name in C._COARSE + C._BIASES:
                ratio = C.distance(case, name) / 2 / b            # (another BLAS moves a floor in its second digit: 20 % either way)
                assert ratio >= 1.5 / 1.2 if name in claimed else ratio < 1.5 * 1.2, (case.name, precision, name, ratio)
    for name in ("ffn_tail", "head_last"):
        assert C.deviation(C.SHAPE_CASES[0], name) == {name: 128 if name == "ffn_tail" else 1}


def test_rounding_functions():
    x = np.float32([1.0, 1.00390625, 1.0 + 2.0 ** -9, 3.14159274, -2.71828175, 65504.0, 1e-3])
    np.testing.assert_array_equal(M.bf(x)[:2], np.float32([1.0, 1.0]))           # 1 + 2^-8 is a tie: to even
    assert np.all(np.abs(M.bf(x) - x) <= np.abs(x) * 2.0 ** -8)
    assert np.all(np.abs(M.r16(x) - x) <= np.abs(x) * 2.0 ** -16)
    assert np.all(np.abs(M.hf(x) - x) <= np.abs(x) * 2.0 ** -11)
    assert np.all(np.abs(M.r22(x) - x)[:-1] <= np.abs(x[:-1]) * 2.0 ** -22)          # (1e-3: its lo half is an fp16 subnormal)
    np.testing.assert_array_equal(M.ident(x), x)
    assert set(M.MODES) == set(C.PRECISIONS)
