"""The rounding points of the HIP encoder (memex_amd/csrc/encoder*.hip) restated in NumPy -- TEST INFRASTRUCTURE, not product code.

``run`` is the encoder forward with a rounding function per operand class: products in f32 (numpy), softmax in f64, every
operand of a product passed through the function its class names.  With every class on ``ident`` it is the f64 oracle up to
the f32 products (1 - cos of 1e-13 to 2e-13); with the table of a precision mode (``MODES``) it reaches what a kernel that
rounds where that mode rounds can reach, however it orders its sums.  tests/test_encoder_bars_model.py turns that floor
into the bars of tests/test_encoder_bars_gpu.py; scripts/encoder_rounding_sim.py prints the tables the modes were chosen from.

Operand classes (the keys of ``R``; a missing key rounds to bf16):
    res     the hidden state as the residual of an Add&Norm         gout    a GEMM result before the residual is added
    x_qk    the hidden state into the Q / K projections             w_qk    their weights          qk (q, k)  Q, K as stored
    x_v     the hidden state into the V projection                  w_v     its weights            v          V as stored
    p       the un-normalised softmax weights into P.V              ctx     the attention output
    w_o     out-projection weights     x_f  the hidden state into W1     w_1, w_2  MLP weights     h   gelu(..) into W2
    final   the last hidden state into the pooling
"""
import math

import numpy as np
from scipy.special import erf


def bf(x):  # round to nearest even bf16, returned as f32
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).reshape(x.shape)


def hf(x):  # fp16
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def ident(x):
    return np.asarray(x, dtype=np.float32)


def r16(x):  # hi + lo bf16 split: 16 significant bits
    x = np.asarray(x, np.float32)
    hi = bf(x)
    return hi + bf(x - hi)


def r22(x):  # fp16 hi + fp16 lo split: 22 significant bits (inside fp16's exponent range)
    x = np.asarray(x, np.float32)
    hi = hf(x)
    return hi + hf(x - hi)


def ln(x, g, b, eps):
    x = x.astype(np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return ((x - mu) / np.sqrt(var + eps) * g + b).astype(np.float32)


ALL = ['res', 'gout', 'x_qk', 'w_qk', 'qk', 'x_v', 'w_v', 'v', 'p', 'ctx', 'w_o', 'x_f', 'w_1', 'h', 'w_2', 'final']
F32 = dict(res=ident, gout=ident, final=ident)       # hidden state / GEMM results / output in f32
WEIGHTS = ['w_qk', 'w_v', 'w_o', 'w_1', 'w_2']
ACTS = ['x_qk', 'x_v', 'ctx', 'x_f', 'h']


def allof(fn, **over):
    d = {k: fn for k in ALL}
    d.update(over)
    return d


def mode(wfn, afn, **attn):  # f32 state, one function for every weight, one for every activation operand
    d = dict(F32)
    d.update({k: wfn for k in WEIGHTS})
    d.update({k: afn for k in ACTS})
    d.update(attn)
    return d


# MX_PREC_MIXED as first drafted: three bf16 products on the attention block, two fp16 ones in the MLP
MIXED = dict(qk=r16, p=r16, v=r16, w_1=hf, w_2=hf, x_f=r22, h=r22)


def mixed(**over):
    d = mode(r16, r16, **MIXED)
    d.update(over)
    return d


# the four precision modes of the library (include/memex_hip.h MX_PREC_*), as built
MODES = {
    "bf16": allof(bf),                                                   # every operand and the hidden state one bf16 value
    "bf16x3": allof(r16, res=ident, gout=ident, final=ident),          # 16-bit split operands, f32 state
    "mixed": mixed(p=bf),                                                # ... P one bf16 value, the MLP on two fp16 products
    "mixed1": mixed(p=bf, x_f=hf, h=hf),                                 # ... the MLP on ONE fp16 product
}
EXACT = allof(ident)


def run(w, cfg, ids, lens, R):
    """``cfg``: an EncoderConfig (layers, hidden, heads, ln_eps, pooling, normalize, pos_offset are read; token type 0 always, as
    in the oracle and the library).  -> [B, hidden] f64, L2-normalised iff cfg.normalize."""
    g = lambda k: R.get(k, bf)
    H, nh, L = cfg.hidden, cfg.heads, cfg.layers
    dh = H // nh
    ids = np.asarray(ids)
    lens = np.asarray(lens)
    B, S = ids.shape
    W = {k: np.asarray(v, np.float32) for k, v in w.items()}
    mask = (np.arange(S)[None, :] < lens[:, None])
    p0 = getattr(cfg, "pos_offset", 0)
    x = (W["embeddings.word_embeddings.weight"][ids] + W["embeddings.position_embeddings.weight"][None, p0:p0 + S]
         + W["embeddings.token_type_embeddings.weight"][0])
    x = ln(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], cfg.ln_eps)
    for l in range(L):
        p = f"encoder.layer.{l}."

        def lin(t, name, rw):
            return (t.reshape(-1, t.shape[-1]).astype(np.float32) @ rw(W[p + name + ".weight"]).T + W[p + name + ".bias"]).reshape(t.shape[:-1] + (-1,))

        def heads(t):
            return t.reshape(B, S, nh, dh).transpose(0, 2, 1, 3)

        xr = g('res')(x)
        q = heads(R.get('q', g('qk'))(lin(g('x_qk')(x), "attention.self.query", g('w_qk')) / math.sqrt(dh)))
        k = heads(R.get('k', g('qk'))(lin(g('x_qk')(x), "attention.self.key", g('w_qk'))))
        v = heads(g('v')(lin(g('x_v')(x), "attention.self.value", g('w_v'))))
        s = (q.astype(np.float64) @ k.transpose(0, 1, 3, 2).astype(np.float64))
        s = np.where(mask[:, None, None, :], s, -1e30)
        s = s - s.max(-1, keepdims=True)
        pr = np.exp(s)
        lsum = pr.sum(-1, keepdims=True)
        ctx = (g('p')(pr.astype(np.float32)) @ v) / lsum
        ctx = g('ctx')(ctx.transpose(0, 2, 1, 3).reshape(B, S, H))
        a = g('gout')(lin(ctx, "attention.output.dense", g('w_o')))
        x1 = ln(a.astype(np.float32) + xr, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], cfg.ln_eps)
        x1r = g('res')(x1)
        h = lin(g('x_f')(x1), "intermediate.dense", g('w_1')).astype(np.float64)
        h = g('h')((0.5 * h * (1 + erf(h / math.sqrt(2)))).astype(np.float32))
        o = g('gout')(lin(h, "output.dense", g('w_2')))
        x = ln(o + x1r, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], cfg.ln_eps)
    x = g('final')(x)
    if cfg.pooling == "cls":
        pooled = x[:, 0, :].astype(np.float64)
    else:
        pooled = (x.astype(np.float64) * mask[:, :, None]).sum(1) / lens[:, None]
    if not getattr(cfg, "normalize", True):
        return pooled
    return pooled / np.linalg.norm(pooled, axis=1, keepdims=True)


def one_minus_cos(a, b):
    """[B] : 1 - cos of matching rows, in f64"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


def rel_err(a, b):
    """[B] : max |a - b| of a row over the largest |b| of that row -- the element-wise measure of un-normalised outputs"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b).max(1) / np.abs(b).max(1)
