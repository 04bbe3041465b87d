"""A CPU model of the scan's filter copies -- TEST INFRASTRUCTURE, plain numpy, float64 where the kernels are float32.

Written from memex_amd/csrc/mx_rotate.h (the rotation T), scan8.hip's shadow8_kernel (int8 copy: one step per 32-row half
tile, e_h = 1.01 * worst residual of the half tile + 1e-6), scan16.hip's shadow_kernel (bf16 copy) and index_kernels.hip's
prep_queries_kernel (query codes, Eq, |r_q|, a_q and the bound  |filter score - cosine| <= qa + qb * e_h,  e1 for the worst row).

What it is for: the certificate is a Cauchy-Schwarz bound, and a random query uses a seventh of it.  `adversary` builds the
query that uses most of it against one chosen row: it points along MINUS that row's quantisation error, stored - true (so the
stored row scores below the true one by as much as its residual allows), and `sharpen` moves the query's own elements to 0.45 of a
step beside their codes, on the side of the row's sign (so the query's residual points along the row).  `predict` says what
the kernel will then score.  tests/test_certificate_adversary_gpu.py runs these queries with a range threshold that sits
exactly on the victim's score: the scan keeps the row only if the bound it computed really covers the under-score.

Nothing here reads the library; the GPU tests use it as the reference of their liveness assertion."""
from dataclasses import dataclass

import numpy as np

K_ACC_SLACK = float(np.float32(2.7e-4))          # index_kernels.h: kAccSlack
K_APPROX_ERR = float(np.float32(0.0081))         # index_kernels.h: kApproxErr
K_MIN_STEP8 = 1.0 / 32768.0                      # index_kernels.h: kMinStep8
HALF = 32                                        # rows per quantisation step (scan8.hip: a half tile)
f32 = np.float32


# ---------------------------------------------------------------------------------------------
# mx_rotate.h
# ---------------------------------------------------------------------------------------------
def rot_sign(j):
    """+-1 per dimension: the 32-bit hash of mx_rotate.h::rot_sign"""
    j = np.asarray(j, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = (j * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m
    h ^= h >> np.uint64(13)
    return np.where(h & np.uint64(1), -1.0, 1.0)


def _hadamard128(v):
    """H_128 / sqrt(128) along the last axis, in rot_wave's butterfly order: stride 64 first, then strides 1, 2, ... 32"""
    shape = v.shape
    for bit in (64, 1, 2, 4, 8, 16, 32):
        w = v.reshape(shape[:-1] + (128 // (2 * bit), 2, bit))
        lo, hi = w[..., 0, :], w[..., 1, :]
        v = np.stack([lo + hi, lo - hi], axis=-2).reshape(shape)
    return v * 0.08838834764831845


def dct_mix(m):
    """M_m of rot_fill_mix: the orthonormal DCT-II matrix, M[k][j] = sqrt((k ? 2 : 1) / m) cos(pi (2j + 1) k / (2m))"""
    k = np.arange(m)[:, None]
    j = np.arange(m)[None, :]
    return np.sqrt(np.where(k > 0, 2.0, 1.0) / m) * np.cos(np.pi * ((2 * j + 1) * k) / (2.0 * m))


_ROT = {}


def rotation(ds):
    """T [ds, ds] of mx_rotate.h for ds = 128 m, m = 1 .. 12: rotated = T @ x"""
    m, rem = divmod(int(ds), 128)
    assert rem == 0 and 1 <= m <= 12, ds
    if ds not in _ROT:
        e = np.eye(ds) * rot_sign(np.arange(ds))[None, :]                  # columns of D
        hd = _hadamard128(e.T.reshape(ds, m, 128)).reshape(ds, m, 128)     # row i: (I (x) H) D e_i, by block
        t = np.einsum("kj,ijp->ikp", dct_mix(m), hd) if m > 1 else hd      # out[128 k + p] = sum_j M[k][j] in[128 j + p]
        _ROT[ds] = np.ascontiguousarray(t.reshape(ds, ds).T)
    return _ROT[ds]


def pad128(d):
    return (int(d) + 127) // 128 * 128


# ---------------------------------------------------------------------------------------------
# the rows' side
# ---------------------------------------------------------------------------------------------
@dataclass
class Copy:
    kind: str                 # "i8" or "bf16"
    d: int
    ds: int
    mean: object              # f64 [ds] (the f32 values, zero padded) or None
    unit: np.ndarray          # f64 [n, ds]: the f32 unit rows c / |c| (zeros for a zero-norm or wide-norm row)
    a_c: np.ndarray           # f64 [n]: the f32 a_c = (c/|c|) . mean (0 when not centred)
    target: np.ndarray        # f64 [n, ds]: what the quantiser sees: r_c = unit - a_c mean, rotated for "i8"
    stored: np.ndarray        # f64 [n, ds]: what the copy holds, in the units of `target`: step * codes, or the bf16 values
    codes: object             # int32 [n, ds] ("i8")
    step: object              # f64 [n]: the f32 s_h of the row's half tile ("i8")
    e_row: np.ndarray         # f64 [n]: |target - stored| per row
    e_h: np.ndarray           # f64 [n]: the residual bound the scan uses for the row: 1.01 max over its half tile + 1e-6
                              #          ("bf16": 1.01 ec_max + 1e-6 for every row)
    ec_max: float             # largest row residual of the copy
    rc_max: float             # largest |r_c| (centred) or 1

    @property
    def resid(self):
        return self.target - self.stored

    @property
    def n(self):
        return self.unit.shape[0]


def unit_rows(X, ds=None):
    """ingest_kernel: 1/|c| = f32(1 / sqrt(f64 sum of squares)), 0 for a zero norm and for a norm outside [1e-15, 1e15];
    the scaled row as the builders compute it, c * (1/|c|) rounded to f32; zero padded to ds"""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    ds = pad128(d) if ds is None else ds
    acc = (X.astype(np.float64) ** 2).sum(axis=1)
    ok = (acc >= 1e-30) & (acc <= 1e30) & np.isfinite(acc)
    sc = np.zeros(n, dtype=np.float32)
    sc[ok] = (1.0 / np.sqrt(acc[ok])).astype(np.float32)
    out = np.zeros((n, ds))
    out[:, :d] = (X * sc[:, None]).astype(np.float32)
    return out


def mean_direction(X):
    """mean_sum_kernel + mean_norm_kernel: the normalised sum of the unit rows as f32 (the kernel sums in f32 in an order that is
    not fixed; this sums in f64 -- the two agree to ~1e-6, which the model's users must allow for)"""
    s = unit_rows(X).sum(axis=0)
    return (s / np.linalg.norm(s)).astype(np.float32)


def _centre(unit, mean, ds):
    n = unit.shape[0]
    if mean is None:
        return None, np.zeros(n), unit
    m = np.zeros(ds)
    m[: len(mean)] = np.asarray(mean, dtype=np.float32)
    a_c = (unit @ m).astype(np.float32).astype(np.float64)             # f64 sum, stored as f32
    a_c[~unit.any(axis=1)] = 0.0
    return m, a_c, (unit - a_c[:, None] * m[None, :]).astype(np.float32).astype(np.float64)   # one fma per element


def int8_copy(X, mean=None, groups=None):
    """shadow8_kernel.  groups: the row count at which each half-tile step was (re)computed is irrelevant to the final state --
    a half tile is always requantised as a whole from all its rows -- so the model quantises the final rows."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    ds = pad128(d)
    unit = unit_rows(X, ds)
    m, a_c, r = _centre(unit, mean, ds)
    target = r @ rotation(ds).T
    live = unit.any(axis=1)
    codes = np.zeros((n, ds), dtype=np.int32)
    step = np.zeros(n)
    e_row = np.zeros(n)
    e_h = np.zeros(n)
    for h0 in range(0, n, HALF):
        sl = slice(h0, min(h0 + HALF, n))
        blk = target[sl] * live[sl, None]
        mx = f32(np.abs(blk).max())
        if mean is not None:
            sh = max(f32(mx / f32(127.0)), f32(K_MIN_STEP8))
            inv = f32(1.0) / sh
        else:
            sh = f32(mx / f32(127.0))
            inv = f32(127.0) / mx if mx > 0 else f32(0.0)
        c = np.clip(np.rint(blk * float(inv)), -127, 127)
        codes[sl] = c.astype(np.int32)
        step[sl] = float(sh)
        er = np.linalg.norm(blk - c * float(sh), axis=1)
        e_row[sl] = er
        e_h[sl] = er.max() * 1.01 + 1e-6
    target = target * live[:, None]
    rc = float(np.linalg.norm(r, axis=1).max()) if mean is not None else 1.0
    return Copy("i8", d, ds, m, unit, a_c, target, codes * step[:, None], codes, step, e_row, e_h, float(e_row.max()), rc)


def to_bf16(v):
    """round to nearest even bf16, returned as f64"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_copy(X, mean=None):
    """shadow_kernel: bf16(c/|c|), or bf16(r_c) when centred; the worst row residual (and, uncentred, the worst ||stored| - 1|)
    is the one Ec of every row"""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    ds = pad128(d)
    unit = unit_rows(X, ds)
    m, a_c, r = _centre(unit, mean, ds)
    stored = to_bf16(r)
    e_row = np.linalg.norm(r - stored, axis=1)
    worst = e_row.copy()
    if mean is None:
        n2 = np.linalg.norm(stored, axis=1)
        worst = np.maximum(worst, np.where(n2 > 0, np.abs(n2 - 1.0), 0.0))
    ec = float(worst.max())
    rc = float(np.linalg.norm(r, axis=1).max()) if mean is not None else 1.0
    return Copy("bf16", d, ds, m, unit, a_c, r, stored, None, None, e_row, np.full(n, ec * 1.01 + 1e-6), ec, rc)


# ---------------------------------------------------------------------------------------------
# the query's side
# ---------------------------------------------------------------------------------------------
@dataclass
class Query:
    kind: str
    unit: np.ndarray          # f64 [ds]: q / |q| as f32
    a_q: float                # the f32 a_q (0 when not centred)
    target: np.ndarray        # f64 [ds]: r_q = unit - a_q mean, rotated for "i8"
    stored: np.ndarray        # f64 [ds]: s_q * codes or the bf16 values
    codes: object
    step: float               # s_q ("i8")
    eq: float                 # 1.01 |target - stored| + 1e-6
    rq: float                 # 1.001 |r_q| + 1e-6 (centred)
    qa: float
    qb: float
    e1: float                 # the bound of a row of the worst half tile: stats().approx_err_bound is the batch's largest


def query_side(q, kind, mean=None, copy=None):
    """prep_queries_kernel for one usable query.  copy: where ec_max / rc_max come from (without one e1 is NaN and, centred int8,
    |r_c| is bounded by 1 + 1e-6 as the kernel does without the builder's measurement)"""
    q = np.asarray(q, dtype=np.float32)
    d = q.shape[0]
    ds = pad128(d)
    na = float(np.sum((q * q).astype(np.float32).astype(np.float64)))
    assert na > 0.0 and np.isfinite(na)
    inv = f32(1.0 / np.sqrt(na))
    unit = np.zeros(ds)
    unit[:d] = (q * inv).astype(np.float32)
    a_q, r = 0.0, unit
    if mean is not None:
        m = np.zeros(ds)
        m[: len(mean)] = np.asarray(mean, dtype=np.float32)
        a_q = float(f32(unit @ m))
        r = (unit - a_q * m).astype(np.float32).astype(np.float64)
    rq = float(f32(np.linalg.norm(r))) * 1.001 + 1e-6
    ec = copy.ec_max * 1.01 + 1e-6 if copy is not None else float("nan")
    if kind == "i8":
        target = r @ rotation(ds).T
        mx = f32(np.abs(target).max())
        if mean is not None:
            sq = max(f32(mx / f32(127.0)), f32(K_MIN_STEP8))      # (with the floor also for mx == 0: the fixed kernel)
            qinv = f32(1.0) / sq
        else:
            sq = f32(mx / f32(127.0))
            qinv = f32(127.0) / mx
        codes = np.clip(np.rint(target * float(qinv)), -127, 127).astype(np.int32)
        stored = codes * float(sq)
        eq = float(np.linalg.norm(stored - target)) * 1.01 + 1e-6
        if mean is None:
            qa, qb = eq + K_ACC_SLACK, 1.0 + eq
            e1 = ec + eq + ec * eq + K_ACC_SLACK
        else:
            rc = min(copy.rc_max * 1.001 + 1e-6, 1.0 + 1e-6) if copy is not None else 1.0 + 1e-6
            qa, qb = eq * rc * 1.0001 + K_ACC_SLACK, rq + eq
            e1 = qa + qb * ec
        return Query(kind, unit, a_q, target, stored, codes, float(sq), eq, rq, qa, qb, e1)
    stored = to_bf16(r)
    eq = float(np.linalg.norm(stored - r)) * 1.01 + 1e-6
    e1 = min(K_APPROX_ERR + ec * ec, ec + eq + ec * eq + K_ACC_SLACK)
    if mean is not None:
        e1 = min(e1, rq * ec + eq * 1.0001 + ec * eq + K_ACC_SLACK)
    return Query(kind, unit, a_q, r, stored, None, 0.0, eq, rq, e1, 0.0, e1)


def predict(copy, query):
    """-> (filter score [n], cosine - filter score [n], qa + qb * e_h [n]).  The score is the kernel's up to its f32 roundings
    (int8: the integer sum is exact, two f32 multiplications; centred: the accumulator start truncates a_q a_c to a whole number of
    s_h s_q units; bf16: f32 accumulation of exact products) -- all inside kAccSlack."""
    cos = copy.unit @ query.unit
    if copy.kind == "i8":
        acc = (copy.codes.astype(np.int64) @ query.codes.astype(np.int64)).astype(np.float64)
        if copy.mean is not None:
            unit_s = copy.step * query.step
            acc = acc + np.trunc(copy.a_c * query.a_q / unit_s)
        score = acc * copy.step * query.step
    else:
        score = copy.stored @ query.stored + copy.a_c * query.a_q
    return score, cos - score, query.qa + query.qb * copy.e_h


# ---------------------------------------------------------------------------------------------
# the adversary
# ---------------------------------------------------------------------------------------------
def _back(copy, t):
    """a vector of the quantiser's space -> the rows' space (T^T for "i8"), cut to the index's dims"""
    return (t @ rotation(copy.ds) if copy.kind == "i8" else t)[: copy.d]


def adversary(copy, victim, a, a_q=None):
    """The unit query  a * (victim direction) - sqrt(1 - a^2) * (residual / |residual|)  in the quantiser's space (residual = stored
    - true, the error the copy made; `Copy.resid` is its negative; its component across the row), so that the stored row scores BELOW
    the true one; mapped back
    through T^T for int8.  Centred copies: that vector, made orthogonal to the mean, is the query's r_q direction, and the query is
    a_q * mean + sqrt(1 - a_q^2) * r_q with a_q = the victim's a_c (the query sits in the cone like the row) unless given."""
    v = copy.target[victim]
    r = copy.resid[victim]
    v = v / np.linalg.norm(v)
    r = r - (r @ v) * v            # (the part of the residual across the row: the cosine with the victim is then a, whatever v . r is --
    #                                bf16 rounding errors follow the elements' sizes, and v . r / |r| wanders by +-0.2 at 384 dims)
    t = a * v + np.sqrt(1.0 - a * a) * r / np.linalg.norm(r)   # r = true - stored: minus the stored row's error
    if copy.mean is None:
        q = _back(copy, t)
        return (q / np.linalg.norm(q)).astype(np.float32)
    w = np.zeros(copy.ds)
    w[: copy.d] = _back(copy, t)
    w -= (w @ copy.mean) * copy.mean
    w /= np.linalg.norm(w)
    a_q = float(copy.a_c[victim]) if a_q is None else a_q
    q = a_q * copy.mean + np.sqrt(1.0 - a_q * a_q) * w
    return q[: copy.d].astype(np.float32)


def sharpen(copy, victim, q, frac=0.45):
    """int8 only.  The same codes as q's, every element moved to frac of a step beside its code on the side of the victim's sign:
    the query's residual then points along the stored row and r_q-residual . c reaches ~0.8 Eq |c| (a random query: ~0), on top
    of what the row's residual gives.  Quantisation is scale free (the step is max / 127), so the construction survives the
    kernel's normalisation; elements at the extreme codes stay where they are, so the step does."""
    assert copy.kind == "i8"
    qs = query_side(q, "i8", None if copy.mean is None else copy.mean[: copy.d])
    k = qs.codes.astype(np.float64)
    move = frac * np.sign(copy.target[victim]) * (np.abs(k) < 126)
    t = qs.step * (k + move)
    if copy.mean is None:
        out = _back(copy, t)
        return (out / np.linalg.norm(out)).astype(np.float32)
    tm = copy.mean @ rotation(copy.ds).T
    p = t - qs.target
    t = qs.target + p - (p @ tm) * tm                                  # r_q stays orthogonal to the mean: a_q, and so r_q, as planned
    w = np.zeros(copy.ds)
    w[: copy.d] = _back(copy, t)
    out = qs.a_q * copy.mean + w
    return (out[: copy.d] / np.linalg.norm(out[: copy.d])).astype(np.float32)


def sharpen_bf16(copy, victim, q, frac=0.45, free=8):
    """Plain bf16 copy.  Every element of the unit query moved to frac of a bf16 spacing beside its bf16 value, on the side of the
    victim's sign; the `free` largest elements are scaled instead, so that the query has unit length to f32 precision (rounding to
    bf16 is not scale free: the kernel's q * (1/|q|) must leave the elements where they were put, to ~1e-7 of their value)."""
    assert copy.kind == "bf16" and copy.mean is None
    u = query_side(q, "bf16").unit[: copy.d].copy()
    b = to_bf16(u)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(b), 1e-300))) - 7)
    moved = b + frac * ulp * np.sign(copy.stored[victim][: copy.d])
    moved = np.where((to_bf16(moved) == b) & (b != 0), moved, u)
    keep = np.argsort(-np.abs(u))[:free]
    moved[keep] = 0.0
    t2 = (1.0 - moved @ moved) / (u[keep] @ u[keep])
    assert 0.5 < t2 < 2.0
    moved[keep] = u[keep] * np.sqrt(t2)
    return moved.astype(np.float32)


def pick_victims(copy, rows, count):
    """of `rows`, the `count` whose own residual is the largest share of their half tile's e_h (the rows the bound is tight for)"""
    rows = np.asarray(rows)
    rows = rows[copy.e_row[rows] > 0]
    share = copy.e_row[rows] / copy.e_h[rows]
    return rows[np.argsort(-share, kind="stable")[:count]]
