"""The contract of mx_encoder_create over the whole lattice of shapes it accepts (include/memex_hip.h, next to mx_encoder_cfg).

Whatever `create` accepts encodes: hidden 384 / 768, head dim 32 / 64, every ffn width 384, 768, ... 3840 and every precision
mode build an encoder that takes a batch of lengths (1, S - 1, S) at S = 33, 130 and 300 -- one length per attention form -- and
answers within the bar of tests/encoder_bars_cases.py (4 x the floor of the mode's rounding model on these very inputs, nothing
measured) of the f64 oracle; the full-length row encoded alone lies within the same bar of itself in the batch.  What `create`
does not accept it refuses with the code the header names, and a refusal leaves the library usable."""
import numpy as np
import pytest

import encoder_bars_cases as C
import encoder_rounding_model as M

pytestmark = pytest.mark.gpu

HEADS = {(384, 32): 12, (384, 64): 6, (768, 32): 24, (768, 64): 12}
FFNS = tuple(range(384, 3840 + 1, 384))
LENGTHS = (33, 130, 300)


def _case(hidden, dh, ffn, S, lens, layers=1):
    kw = C._kw(layers=layers, hidden=hidden, heads=HEADS[hidden, dh], ffn=ffn, vocab=200, max_pos=512)
    return C.Case(f"lattice_{hidden}_{dh}_{ffn}_{S}", kw, len(lens), S, 77, lens=tuple(lens))


def _hold(enc, case, precision, what):
    """one encode of the case's inputs within the bar of the oracle, then its last row alone within the bar of the batch's"""
    ids, lens = C.inputs(case)
    ref, bar = C.oracle(case), C.bar(case, precision)
    out = enc.encode(ids, lens)
    assert np.isfinite(out).all(), what
    got = float(M.one_minus_cos(out, ref).max())
    print(f"LATTICE | {what} | 1-cos {got:.2e} | bar {bar:.2e}")
    assert 0.0 < bar < 1e-3 and got <= bar, (what, got, bar)
    n = int(lens[-1])
    alone = enc.encode(np.ascontiguousarray(ids[-1:, :n]), lens[-1:])
    assert np.isfinite(alone).all(), what
    apart = float(M.one_minus_cos(alone, out[-1:]).max())
    assert apart <= bar, (what, "alone against the batch", apart, bar)
    assert float(M.one_minus_cos(alone, ref[-1:]).max()) <= bar, (what, "alone against the oracle")


@pytest.mark.parametrize("ffn", FFNS)
@pytest.mark.parametrize("hidden,dh", sorted(HEADS))
def test_every_accepted_shape_encodes_within_its_bar(hidden, dh, ffn, lib_built):
    from memex_amd.encoder import Encoder
    from memex_amd.weights import pack_weights
    cases = [_case(hidden, dh, ffn, S, (1, S - 1, S)) for S in LENGTHS]
    for precision in C.PRECISIONS:
        cfg = cases[0].cfg(precision)
        with Encoder(cfg, pack_weights(C.weights(cases[0]), cfg)) as enc:      # (the weights depend on the seed alone)
            for case in cases:
                _hold(enc, case, precision, f"{hidden} / {cfg.heads} heads / ffn {ffn} / {precision} / S {case.S}")
    C.weights.cache_clear()                                                    # (a hundred sets of weights would stay otherwise)


@pytest.mark.parametrize("precision", C.PRECISIONS)
def test_24_heads_encode_at_every_length(precision, lib_built):
    """hidden 768 with 24 heads of 32: 24 head groups per sequence.  One short query (the short attention kernel), one
    sequence of the full 512 tokens and a batch of ragged ones in between, on one encoder"""
    from memex_amd.encoder import Encoder
    from memex_amd.weights import pack_weights
    cases = [_case(768, 32, 3072, S, lens) for S, lens in ((16, (16,)), (512, (512,)), (200, (1, 129, 200, 77)))]
    cfg = cases[0].cfg(precision)
    with Encoder(cfg, pack_weights(C.weights(cases[0]), cfg)) as enc:
        for case in cases:
            _hold(enc, case, precision, f"768 / 24 heads / {precision} / lens {case.lens}")
    C.weights.cache_clear()


def _cfg(**over):
    from memex_amd.weights import EncoderConfig
    kw = dict(layers=1, hidden=384, heads=12, ffn=384, vocab=200, max_pos=512)
    kw.update(over)
    return EncoderConfig(**kw)


REJECTED = (
    [("MX_EUNSUPPORTED", dict(hidden=h, heads=h // 32, ffn=384)) for h in (256, 512, 1024)]
    + [("MX_EUNSUPPORTED", dict(hidden=h, heads=h // d)) for d in (16, 48, 96, 128) for h in (384, 768)]
    + [("MX_EUNSUPPORTED", dict(hidden=h, heads=h // 32, ffn=f)) for f in (0, 192, 256, 400, 1664) for h in (384, 768)]
    + [("MX_EUNSUPPORTED", dict(layers=n)) for n in (0, 49)]
    + [("MX_EINVAL", dict(hidden=h, heads=n)) for h in (384, 768) for n in (5, 7, 9 if h == 384 else 11)]
)


@pytest.mark.parametrize("code,over", REJECTED, ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_what_create_refuses_and_with_which_code(code, over, lib_built):
    from memex_amd import _lib
    from memex_amd.encoder import Encoder
    from memex_amd.weights import synthetic_weights
    bad = _cfg(**over)
    blob = np.zeros(Encoder.weight_bytes(bad) // 4, dtype=np.float32)         # of the size the configuration asks for
    for precision in C.PRECISIONS:
        with pytest.raises(_lib.MemexHipError) as ei:
            Encoder(_cfg(**over, precision=precision), blob)
        assert ei.value.code == getattr(_lib, code), (precision, ei.value.code, ei.value.msg)
    good = _cfg()
    with Encoder(good, synthetic_weights(good, 0)) as enc:                     # the refusal left nothing behind
        out = enc.encode(np.arange(10, dtype=np.int32).reshape(2, 5), np.array([5, 3], np.int32))
    assert np.isfinite(out).all()
    np.testing.assert_allclose(np.linalg.norm(out, axis=1), 1.0, atol=1e-5)
