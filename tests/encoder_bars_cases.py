"""The cases of the encoder parity bars -- TEST INFRASTRUCTURE shared by tests/test_encoder_bars_model.py (no GPU: proves that
each bar separates the deviations the case claims) and tests/test_encoder_bars_gpu.py (holds every kernel route to that bar).

A case is a small configuration with its inputs; per precision mode it has
    floor f   max over rows of 1 - cos( rounding model of the mode , f64 oracle )        (encoder_rounding_model.MODES)
    bar   b = 4 f     a factor 2 in relative error for what the model does not state: summation order, the un-shifted exp2
                      fast path, split-k, where P is rounded
    d_D       max over rows of 1 - cos( f64 oracle with the named deviation D , f64 oracle )   (bert_oracle.encode(deviate=))
and it CLAIMS the deviations with b <= d_D / 2.  Nothing here comes from a GPU run.  tests/ENCODER_BARS.md is the record.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import encoder_rounding_model as M
from memex_amd.weights import EncoderConfig, synthetic_weights
from oracle import bert_oracle

FACTOR = 4.0          # bar = FACTOR * floor, in 1 - cos
FACTOR_REL = 2.0      # ... = a factor 2 in relative error: the element-wise bar of un-normalised outputs
PRECISIONS = ("bf16", "bf16x3", "mixed", "mixed1")

# name -> (deviate dict, the kernel families it touches)
DEVIATIONS = {
    "bias_q":     (dict(drop_bias=(-1, "query")), ("qkv",)),
    "bias_v":     (dict(drop_bias=(-1, "value")), ("qkv",)),
    "bias_ao":    (dict(drop_bias=(-1, "attn_out")), ("out_ln",)),
    "bias_int":   (dict(drop_bias=(-1, "intermediate")), ("mlp",)),
    "bias_mlp":   (dict(drop_bias=(-1, "mlp_out")), ("mlp",)),
    "scale":      (dict(scale=1.01), ("attention",)),
    "eps":        (None, ("embed_ln", "out_ln", "mlp")),          # the other of 1e-12 / 1e-5: see deviation()
    "gelu":       (dict(gelu="tanh"), ("mlp",)),
    "keys_extra": (dict(keys_extra=1), ("attention",)),
    "pool_extra": (dict(pool_extra=1), ("pooling",)),
    "pos+1":      (dict(pos_shift=1), ("embed_ln",)),
    "pos-1":      (dict(pos_shift=-1), ("embed_ln",)),
    "type1":      (dict(token_type=1), ("embed_ln",)),
    "swap_v":     (dict(swap_v_heads=(-1, 0, 1)), ("qkv", "attention")),
    "ln_gain":    (dict(drop_ln="gain"), ("mlp",)),
    "ln_bias":    (dict(drop_ln="bias"), ("mlp",)),
    "pool_div":   (dict(pool_div="S"), ("pooling",)),
    "ffn_tail":   (dict(ffn_tail=128), ("mlp",)),            # the last 128-feature chunk of the last layer's MLP dropped
    "head_last":  (dict(head_last=1), ("attention",)),       # the last head of the last layer never scheduled
}
SUBTLE = ("eps", "gelu", "scale")     # at most these may stay unseen on routes with bf16 operands
FAMILIES = ("embed_ln", "qkv", "attention", "out_ln", "mlp", "pooling")


@dataclass(frozen=True)
class Case:
    name: str
    kw: tuple                      # EncoderConfig arguments without the precision, as sorted items
    B: int
    S: int
    seed: int
    tweak: str = ""                # "" | "emb_small": the three embedding tables x 1e-2 | "q_bias": the query biases x 16
    held: int = 0                  # > 0: only the first `held` sequences are held to the oracle (large passes); they are ragged
    claims: tuple = ()             # ((precision, (deviation, ...)), ...): what test_encoder_bars_model.py proves separable
    routes: tuple = ()             # ((precision, (route, ...)), ...): see test_encoder_bars_gpu.ROUTES
    lens: tuple = ()               # the lengths themselves instead of drawn ones (tests/test_encoder_lattice_gpu.py)

    def cfg(self, precision="bf16"):
        return EncoderConfig(**dict(self.kw), precision=precision)

    def claimed(self, precision):
        return dict(self.claims).get(precision, ())

    def routed(self, precision):
        return dict(self.routes).get(precision, ())


def _kw(**kw):
    return tuple(sorted(kw.items()))


@lru_cache(maxsize=None)
def weights(case):
    cfg = case.cfg()
    w = synthetic_weights(cfg, case.seed)
    if case.tweak == "emb_small":
        # the embedding LayerNorm then sees a variance of ~1e-4 x 3 x 0.05^2: eps = 1e-5 against 1e-12 moves its output by percents
        for n in ("word_embeddings", "position_embeddings", "token_type_embeddings"):
            w[f"embeddings.{n}.weight"] = (w[f"embeddings.{n}.weight"] * np.float32(1e-2)).astype(np.float32)
    elif case.tweak == "q_bias":
        # query biases of the size of the projected queries themselves (x 16: 0.32 against ~1)
        for l in range(cfg.layers):
            n = f"encoder.layer.{l}.attention.self.query.bias"
            w[n] = (w[n] * np.float32(16.0)).astype(np.float32)
    elif case.tweak:
        raise ValueError(case.tweak)
    for v in w.values():
        v.setflags(write=False)
    return w


@lru_cache(maxsize=None)
def inputs(case):
    """-> ids [B, S], lens [B].  The first rows carry the deviations' weight: ragged, shorter than S (a padding key / padding
    token exists), the first one longer than one token; large passes fill up with full-length rows behind them."""
    cfg = case.cfg()
    rng = np.random.default_rng(case.seed)
    ids = rng.integers(1000 if cfg.vocab > 1000 else 0, cfg.vocab, size=(case.B, case.S)).astype(np.int32)
    if case.lens:
        lens = np.asarray(case.lens, dtype=np.int32)
        assert lens.shape == (case.B,) and not case.held
        ids.setflags(write=False)
        lens.setflags(write=False)
        return ids, lens
    n = case.held or case.B
    lens = np.full(case.B, case.S, dtype=np.int32)
    lens[:n] = rng.integers(max(2, case.S // 3), case.S, size=n)
    if not case.held:
        lens[-1] = case.S                                           # one full-length row
    ids.setflags(write=False)
    lens.setflags(write=False)
    return ids, lens


def _sub(case):
    ids, lens = inputs(case)
    n = case.held or case.B
    smax = int(lens[:n].max())
    return ids[:n, :smax], lens[:n]


def deviation(case, name):
    if name == "eps":
        return dict(ln_eps=1e-5 if case.cfg().ln_eps < 1e-8 else 1e-12)
    return DEVIATIONS[name][0]


def applicable(case, name):
    cfg = case.cfg()
    if name in ("pool_extra", "pool_div") and cfg.pooling != "mean":
        return False
    if name == "pool_div" and cfg.normalize:
        return False
    if name == "pos-1" and cfg.pos_offset < 1:
        return False
    if name == "type1" and cfg.type_vocab < 2:
        return False
    return True


@lru_cache(maxsize=None)
def oracle(case, dev_name=None):
    """the f64 oracle on the held rows (with one named deviation)"""
    ids, lens = _sub(case)
    out = bert_oracle.encode(weights(case), case.cfg().as_dict(), ids, lens, deviate=deviation(case, dev_name) if dev_name else None)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def model(case, precision):
    ids, lens = _sub(case)
    out = M.run(weights(case), case.cfg(), ids, lens, M.MODES[precision] if precision != "exact" else M.EXACT)
    out.setflags(write=False)
    return out


def floor(case, precision):
    return float(M.one_minus_cos(model(case, precision), oracle(case)).max())


def bar(case, precision):
    return FACTOR * floor(case, precision)


def distance(case, dev_name):
    return float(M.one_minus_cos(oracle(case, dev_name), oracle(case)).max())


# un-normalised outputs: the element-wise measure (the pooling divisor changes a row's length, not its direction)
def floor_rel(case, precision):
    return float(M.rel_err(model(case, precision), oracle(case)).max())


def bar_rel(case, precision):
    return FACTOR_REL * floor_rel(case, precision)


def distance_rel(case, dev_name):
    return float(M.rel_err(oracle(case, dev_name), oracle(case)).max())


_M384 = dict(layers=2, hidden=384, heads=12, ffn=1536, vocab=3000)
_M768 = dict(layers=2, hidden=768, heads=12, ffn=3072, vocab=3000)
_ROBERTA = dict(max_pos=514, type_vocab=1, ln_eps=1e-5, pos_offset=2)

# What a case claims per precision.  The sets below were chosen from the distances and floors measured on a CPU (the ratio
# (d / 2) / b in tests/ENCODER_BARS.md); only pairs with a ratio of at least 1.5 are claimed, so that another BLAS's summation
# order inside the model cannot turn a claim over.  test_encoder_bars_model.py proves every one of them.
_COARSE = ("keys_extra", "pos+1", "type1", "swap_v", "ln_gain", "ln_bias")        # seen by every mode on every generic input
_BIASES = ("bias_v", "bias_ao", "bias_int", "bias_mlp")
_FINE = ("bias_q", "scale")                                                         # need 16-bit operands on generic inputs
_X3 = _COARSE + _BIASES + _FINE + ("eps", "gelu")


def _claims(bf16, bf16x3=None, mixed=None, mixed1=None):
    out = [("bf16", tuple(bf16))]
    for name, c in (("bf16x3", bf16x3), ("mixed", mixed), ("mixed1", mixed1)):
        if c is not None:
            out.append((name, tuple(c)))
    return tuple(out)


def _routes(**kw):
    return tuple((k, tuple(v)) for k, v in kw.items())


# the routes of a hidden-384 / hidden-768 small pass with head dim 32 (see test_encoder_bars_gpu.ROUTES)
_R384 = ("default", "small=0", "unfused_tail", "attn_short=0", "attn_short_lds=0", "attn_pair=1", "attn_pair=0", "attn_safe=1")
_R768 = ("default", "splitk=0", "small=0", "attn_short=0", "attn_safe=1")
_RX3 = ("default", "attn_f32=1")

CASES = (
    # hidden 384, one small pass of short sequences: every route of the hidden-384 layer and of the short attention
    Case("m384_s33", _kw(**_M384), 5, 33, 5,
         claims=_claims(_COARSE + _BIASES + ("pool_extra",), _X3 + ("pool_extra",), _COARSE + _BIASES + _FINE + ("pool_extra",),
                        _COARSE + _BIASES + _FINE + ("pool_extra",)),
         routes=_routes(bf16=_R384, bf16x3=_RX3, mixed=("default",), mixed1=("default",))),
    # head dim 64 at hidden 384 (attention_kernel<64, 1> at every length), a narrow MLP
    Case("m384_d64_s77", _kw(layers=2, hidden=384, heads=6, ffn=768, vocab=3000), 5, 77, 10,
         claims=_claims(_COARSE + _BIASES + ("pool_extra",), _X3 + ("pool_extra",), _COARSE + _BIASES + _FINE, _COARSE + _BIASES + _FINE),
         routes=_routes(bf16=("default", "small=0", "unfused_tail", "attn_safe=1"), bf16x3=_RX3, mixed=("default",), mixed1=("default",))),
    # 130 tokens: past the short attention kernel, the staged kernel with one stage
    Case("m384_s130", _kw(**_M384), 6, 130, 11,
         claims=_claims(("keys_extra", "swap_v", "bias_v", "bias_mlp", "pool_extra"), ("keys_extra", "swap_v", "scale", "bias_q")),
         routes=_routes(bf16=("default", "small=0", "attn_pair=1", "attn_safe=1"), bf16x3=_RX3)),
    # 300 tokens: two stages of keys
    Case("m384_s300", _kw(**_M384), 4, 300, 12,
         claims=_claims(("swap_v", "bias_v", "bias_ao", "bias_mlp", "pos+1"), ("keys_extra", "swap_v", "scale", "bias_q"), ("keys_extra", "swap_v")),
         routes=_routes(bf16=("default", "small=0", "attn_pair=1", "attn_safe=1"), bf16x3=_RX3, mixed=("default",))),
    # un-normalised output: the pooling divisor
    Case("m384_raw", _kw(**_M384, normalize=False), 5, 33, 13,
         claims=_claims(("pool_div", "pool_extra", "ln_gain", "bias_mlp"), ("pool_div", "pool_extra", "ln_gain", "gelu"),
                        ("pool_div", "pool_extra"), ("pool_div", "pool_extra")),
         routes=_routes(bf16=("default", "small=0"), bf16x3=("default",), mixed=("default",), mixed1=("default",))),
    # hidden 768, CLS pooling: the split-k small pass with the fused Q/K/V product
    Case("b768_cls_s77", _kw(**_M768, pooling="cls"), 4, 77, 6,
         claims=_claims(_COARSE, _X3, _COARSE + _BIASES, _COARSE + _BIASES),
         routes=_routes(bf16=_R768, bf16x3=_RX3, mixed=("default",), mixed1=("default",))),
    # hidden 768, mean pooling
    Case("b768_mean_s33", _kw(**_M768), 5, 33, 7,
         claims=_claims(_COARSE + ("bias_v", "bias_ao", "bias_mlp", "pool_extra"), _X3 + ("pool_extra",), _COARSE + _BIASES + _FINE,
                        _COARSE + _BIASES + _FINE),
         routes=_routes(bf16=("default", "splitk=0", "attn_safe=1"), bf16x3=("default",), mixed=("default",), mixed1=("default",))),
    # hidden 768 past 512 packed rows: split-k Add&Norm GEMMs behind gemm_kernel's Q/K/V; the staged attention at 300 tokens
    Case("b768_mean_s300", _kw(**_M768), 4, 300, 23,
         claims=_claims(("swap_v", "bias_v", "bias_ao", "bias_int", "bias_mlp"), ("keys_extra", "swap_v", "scale")),
         routes=_routes(bf16=("default", "splitk=0", "attn_safe=1"), bf16x3=("default",))),
    # RoBERTa-style tables: positions from row 2, one token type, eps 1e-5
    Case("roberta768_s77", _kw(**_M768, **_ROBERTA), 4, 77, 9,
         claims=_claims(("pos+1", "pos-1", "keys_extra", "swap_v", "bias_v", "bias_ao", "bias_mlp", "pool_extra"),
                        ("pos+1", "pos-1", "eps", "gelu", "scale", "bias_q"), ("pos+1", "pos-1", "scale")),
         routes=_routes(bf16=("default", "splitk=0"), bf16x3=("default",), mixed=("default",))),
    Case("roberta384_s33", _kw(**_M384, **_ROBERTA), 5, 33, 19,
         claims=_claims(("pos+1", "pos-1", "pool_extra"), None, None, ("pos+1", "pos-1", "scale")),
         routes=_routes(bf16=("default", "small=0"), mixed1=("default",))),
    # purpose-built: embedding tables x 1e-2, so that the embedding LayerNorm's eps decides percents of its output; both values
    # of cfg.ln_eps, each against its own oracle
    Case("eps_1e-12", _kw(**_M384), 5, 33, 14, tweak="emb_small",
         claims=_claims(("eps", "pos+1"), ("eps",), ("eps",), ("eps",)),
         routes=_routes(bf16=("default", "small=0"), bf16x3=("default",), mixed=("default",), mixed1=("default",))),
    Case("eps_1e-5", _kw(**_M384, ln_eps=1e-5), 5, 33, 14, tweak="emb_small",
         claims=_claims(("eps", "pos+1"), ("eps",), ("eps",), ("eps",)),
         routes=_routes(bf16=("default", "small=0"), bf16x3=("default",), mixed=("default",), mixed1=("default",))),
    Case("eps768_1e-5", _kw(**_M768, ln_eps=1e-5), 5, 33, 14, tweak="emb_small",
         claims=_claims(("eps",)), routes=_routes(bf16=("default", "splitk=0"))),
    # purpose-built: query biases x 16, so that a bf16 route sees a dropped one
    Case("qbias384", _kw(**_M384), 5, 33, 21, tweak="q_bias",
         claims=_claims(("bias_q",), ("bias_q",), ("bias_q",), ("bias_q",)),
         routes=_routes(bf16=("default", "small=0", "unfused_tail"), bf16x3=("default",), mixed=("default",), mixed1=("default",))),
    Case("qbias768", _kw(**_M768), 5, 33, 21, tweak="q_bias",
         claims=_claims(("bias_q",)), routes=_routes(bf16=("default", "splitk=0"))),
    # large passes (>= 32768 packed rows with their padding): the GEMMs on pgemm_kernel, head pairs chosen by the pass itself.
    # The four ragged rows in front are held to the oracle; 240 full-length rows behind them fill the pass.
    Case("big384_s130", _kw(**_M384), 244, 130, 16, held=4,
         claims=_claims(_COARSE + _BIASES + ("pool_extra",), _X3 + ("pool_extra",), _COARSE + _BIASES + _FINE, _COARSE + _BIASES + _FINE),
         routes=_routes(bf16=("default", "pgemm=0", "unfused_tail", "unfused_tail,pgemm=0"), bf16x3=("default", "pgemm=0"),
                        mixed=("default", "pgemm=0"), mixed1=("default", "pgemm=0"))),
    Case("big768_mean_s130", _kw(**_M768), 244, 130, 18, held=4,
         claims=_claims(_COARSE + _BIASES + ("pool_extra",), _X3 + ("pool_extra",), _COARSE + _BIASES + _FINE, _COARSE + _BIASES + _FINE),
         routes=_routes(bf16=("default", "pgemm=0"), bf16x3=("default", "pgemm=0"), mixed=("default", "pgemm=0"), mixed1=("default", "pgemm=0"))),
    Case("big768_cls_s130", _kw(**_M768, pooling="cls"), 244, 130, 17, held=4,
         claims=_claims(("pos+1", "type1", "swap_v", "ln_gain", "ln_bias"), _X3),
         routes=_routes(bf16=("default", "pgemm=0"), bf16x3=("default",))),
)

# ---- the shape axis: every kind of ffn width and head count that mx_encoder_create accepts and the cases above do not reach.
# Each claims ffn_tail and head_last (the mistakes a chunk count or a head-group count invites) on every precision it routes,
# and the members of _COARSE and _BIASES that reach the 1.5 ratio there.
_SHAPE = ("ffn_tail", "head_last")


def _m384(ffn, heads=12):
    return _kw(layers=2, hidden=384, heads=heads, ffn=ffn, vocab=3000)


def _b768(ffn, heads=12):
    return _kw(layers=2, hidden=768, heads=heads, ffn=ffn, vocab=3000)


_BIG = ("default", "pgemm=0")
_ALL = _SHAPE + _COARSE + _BIASES


def _all(*precisions, bf16_not=()):
    """_SHAPE, _COARSE and _BIASES on bf16 and the named further precisions; `bf16_not`: the members below the 1.5 ratio on bf16
    (tests/ENCODER_BARS.md has every ratio; on the other precisions the smallest ratio of these cases is 138)"""
    return _claims(tuple(n for n in _ALL if n not in bf16_not), **{p: _ALL for p in precisions})


SHAPE_CASES = (
    # hidden 384, the fused tail and the small-pass MLP at odd chunk counts: 3 and 9 chunks of 128 ffn features
    Case("m384_f384_s33", _m384(384), 5, 33, 31, claims=_all("bf16x3", "mixed", "mixed1"),
         routes=_routes(bf16=("default", "small=0", "unfused_tail"), bf16x3=("default",), mixed=("default",), mixed1=("default",))),
    Case("m384_f1152_s33", _m384(1152), 5, 33, 32, claims=_all("bf16x3", "mixed", "mixed1", bf16_not=("bias_int",)),
         routes=_routes(bf16=("default", "small=0", "unfused_tail"), bf16x3=("default",), mixed=("default",), mixed1=("default",))),
    # hidden 384 past the fused tail (ffn > 1536): gemm_kernel serves the small pass; 1920 = 7 x 256 + 128
    Case("m384_f1920_s33", _m384(1920), 5, 33, 33, claims=_all("bf16x3", "mixed", "mixed1"),
         routes=_routes(bf16=("default", "attn_safe=1"), bf16x3=("default",), mixed=("default",), mixed1=("default",))),
    Case("m384_f3072_s33", _m384(3072), 5, 33, 34, claims=_all("bf16x3"), routes=_routes(bf16=("default",), bf16x3=("default",))),
    # head dim 64 at hidden 384 on the staged attention kernel with two stages of keys
    Case("m384_d64_s300", _m384(1536, heads=6), 4, 300, 35, claims=_all("bf16x3"),
         routes=_routes(bf16=("default", "small=0", "attn_safe=1"), bf16x3=_RX3)),
    # hidden 768, split-k over ns_2 = min(8, ffn / 384) chunks: 1 (W2 not split, the out-projection is), 3, 5, 8 chunks that do
    # not divide into k-tiles (3456 / 8 = 432: the fused GEMM instead), 8 chunks of 480 columns
    Case("b768_f384_s33", _b768(384), 5, 33, 36, claims=_all("bf16x3", bf16_not=("bias_int",)), routes=_routes(bf16=("default", "splitk=0"), bf16x3=("default",))),
    Case("b768_f1152_s33", _b768(1152), 5, 33, 37, claims=_all("bf16x3", "mixed", bf16_not=("bias_int",)),
         routes=_routes(bf16=("default", "splitk=0"), bf16x3=("default",), mixed=("default",))),
    Case("b768_f1920_s33", _b768(1920), 5, 33, 38, claims=_all("mixed1", bf16_not=("bias_int",)), routes=_routes(bf16=("default", "splitk=0"), mixed1=("default",))),
    Case("b768_f3456_s33", _b768(3456), 5, 33, 39, claims=_all("bf16x3"), routes=_routes(bf16=("default", "splitk=0"), bf16x3=("default",))),
    Case("b768_f3840_s33", _b768(3840), 5, 33, 40, claims=_all(), routes=_routes(bf16=("default", "splitk=0"))),
    # hidden 768 with 24 heads of 32: 24 head groups per sequence in the short and the one-head form, 12 in the paired one
    Case("b768_h24_s33", _b768(3072, heads=24), 5, 33, 41, claims=_all("bf16x3"),
         routes=_routes(bf16=("default", "attn_short=0", "attn_safe=1"), bf16x3=_RX3)),
    Case("b768_h24_s130", _b768(3072, heads=24), 6, 130, 42, claims=_all("bf16x3"),
         routes=_routes(bf16=("default", "attn_pair=1", "attn_pair=0"), bf16x3=("default",))),
    Case("b768_h24_s300", _b768(3072, heads=24), 4, 300, 43, claims=_all("mixed", bf16_not=("keys_extra",)), routes=_routes(bf16=("default",), mixed=("default",))),
    # large passes: N = 1152 / 1920 end in a half tile of pgemm_kernel (the f32 epilogues take it, the bf16 W1 goes to gemm_kernel)
    Case("big384_f1152_s130", _m384(1152), 244, 130, 44, held=4, claims=_all("bf16x3", "mixed"),
         routes=_routes(bf16=_BIG + ("unfused_tail",), bf16x3=_BIG, mixed=_BIG)),
    Case("big384_f1920_s130", _m384(1920), 244, 130, 45, held=4, claims=_all("bf16x3", "mixed1"), routes=_routes(bf16=_BIG, bf16x3=_BIG, mixed1=_BIG)),
    Case("big768_h24_s130", _b768(3072, heads=24), 244, 130, 46, held=4, claims=_all("bf16x3"), routes=_routes(bf16=_BIG, bf16x3=("default",))),
)
CASES = CASES + SHAPE_CASES

# The pairs no case claims, with the reason (tests/ENCODER_BARS.md repeats them).  The cap of the issue: at most eps, gelu and
# the 1 % scale, and only on routes with a bf16 operand -- the mixed modes keep P as one bf16 value and their MLP operands as
# one fp16 value (11 bits), so the GELU variant stays below their floor as well.
NOT_VISIBLE = {
    "bf16": {"scale": "d = 1e-6 on generic inputs, 1e-6 with logits x 3 as well; the bf16 floor is 5e-6",
             "gelu": "d = 5e-9 (4e-9 with pre-activations x 2); the bf16 floor is 5e-6"},
    "bf16x3": {},
    "mixed": {"gelu": "d = 5e-9; the floor of a bf16 P and fp16 MLP weights is 2e-8"},
    "mixed1": {"gelu": "d = 5e-9; the floor of a bf16 P and one fp16 MLP product is 2e-8"},
}

# The routes: MEMEX_HIP_DEBUG keys (memex_amd/csrc/mx_debug.h) set before the encoder is created, and how a route shows that it
# ran -- its bits against another route's on the same input: "differs" where the two forms sum or round in another order,
# "same" where the library promises the same bits (then only the promise is checked: the interface has no counter that would
# tell the two apart, see tests/ENCODER_BARS.md).
ROUTES = {
    "default":              {},
    "small=0":              dict(small=0),                     # hidden 384: the bulk kernels; hidden 768: no split-k
    "unfused_tail":         dict(small=0, unfused_tail=1),     # out-projection / W1 / W2 as three GEMMs
    "unfused_tail,pgemm=0": dict(small=0, unfused_tail=1, pgemm=0),
    "pgemm=0":              dict(pgemm=0),
    "splitk=0":             dict(splitk=0),
    "attn_short=0":         dict(attn_short=0),
    "attn_short_lds=0":     dict(attn_short_lds=0),
    "attn_pair=1":          dict(attn_short=0, attn_pair=1),
    "attn_pair=0":          dict(attn_short=0, attn_pair=0),
    "attn_safe=1":          dict(attn_safe=1),
    "attn_f32=1":           dict(attn_f32=1),
    "held_alone":           {},                                # large passes: the held rows in a call of their own (a small pass)
}


def relation(case, precision, route):
    """-> (other route, "differs" | "same") or None for the route the others are compared with"""
    cfg = case.cfg(precision)
    big = case.held > 0
    if route == "default":
        return None
    if route == "held_alone":
        # bf16 only: small-pass kernels / split-k against the large pass's.  Hidden 384 past the fused tail (ffn > 1536) has no
        # small-pass kernels: gemm_kernel at every pass size, and pgemm_kernel's Q / K of the large pass carry gemm_kernel's bits
        return ("default", "differs" if cfg.hidden == 768 or cfg.ffn <= 1536 else "same")
    if route == "small=0":
        return ("default", "differs")
    if route == "unfused_tail":
        return ("default", "same") if big else ("small=0", "same")
    if route == "unfused_tail,pgemm=0":
        return ("default", "same")
    if route == "pgemm=0":                  # hidden 768, bf16: the large pass moves the LayerNorms behind the GEMM
        return ("default", "differs" if precision == "bf16" and cfg.hidden == 768 else "same")
    if route in ("splitk=0", "attn_safe=1", "attn_f32=1"):
        return ("default", "differs")
    if route in ("attn_short=0", "attn_short_lds=0", "attn_pair=1", "attn_pair=0"):
        return ("default", "same")
    raise KeyError(route)


def pairs():
    """every (case, precision) with routes"""
    return [(c, p) for c in CASES for p in PRECISIONS if c.routed(p)]
