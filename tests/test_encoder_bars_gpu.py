"""Every kernel route of the HIP encoder against the f64 oracle, at bars that come from a rounding model and catch named mistakes.

tests/encoder_bars_cases.py states the cases; tests/test_encoder_bars_model.py proves on a CPU that each bar b = 4 x (what the
mode's rounding points allow) lies at most half-way to every deviation the case claims -- a dropped bias, a padding key
attended, positions shifted, ...  Here each route (MEMEX_HIP_DEBUG, memex_amd/csrc/mx_debug.h) of each precision mode encodes the
case's inputs once through `Encoder(cfg, w).encode(ids, lens)` and must stay within b of the oracle: max(1 - cos) <= b, and for
un-normalised outputs the element-wise error within twice the model's as well (the pooling divisor).  Oracle, model and bar are
computed here from the inputs, never from a GPU run.  A route also has to show that it ran: bits that differ from the route it
replaces where the two sum or round in another order, the same bits where the library promises them.
Measured values: tests/ENCODER_BARS.md."""
import numpy as np
import pytest

import encoder_bars_cases as C
import encoder_rounding_model as M

pytestmark = pytest.mark.gpu

# (case, precision, route) -> reason: routes whose excess over 4 f could not be settled; their bar is min d_D / 2 over the
# deviations the case claims (still reference-derived), the excess an open finding in tests/ENCODER_BARS.md
OPEN_FINDINGS = {}


@pytest.fixture(scope="module")
def reference():
    """oracle, model floor and bar of a (case, precision): computed once per module (encoder_bars_cases caches them)"""
    def get(case, precision):
        out = dict(ref=C.oracle(case), floor=C.floor(case, precision), bar=C.bar(case, precision))
        if not case.cfg().normalize:
            out.update(floor_rel=C.floor_rel(case, precision), bar_rel=C.bar_rel(case, precision))
        return out
    return get


def _encode(monkeypatch, cfg, blob, ids, lens, env):
    from memex_amd.encoder import Encoder
    if env:
        monkeypatch.setenv("MEMEX_HIP_DEBUG", ",".join(f"{k}={v}" for k, v in env.items()))
    else:
        monkeypatch.delenv("MEMEX_HIP_DEBUG", raising=False)
    try:
        with Encoder(cfg, blob) as enc:          # (the keys an encoder reads when it is created, and those its passes read)
            return enc.encode(ids, lens)
    finally:
        monkeypatch.delenv("MEMEX_HIP_DEBUG", raising=False)


@pytest.mark.parametrize("case,precision", C.pairs(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_every_route_holds_the_bar(case, precision, reference, lib_built, monkeypatch):
    from memex_amd.weights import pack_weights
    cfg = case.cfg(precision)
    blob = pack_weights(C.weights(case), cfg)
    ids, lens = C.inputs(case)
    n = case.held or case.B
    r = reference(case, precision)
    ref = r["ref"]
    routes = list(case.routed(precision))
    if case.held and precision == "bf16":
        routes.append("held_alone")
    outs, failures = {}, []
    for route in routes:
        if route == "held_alone":
            smax = int(lens[:n].max())
            out = _encode(monkeypatch, cfg, blob, np.ascontiguousarray(ids[:n, :smax]), lens[:n], {})
        else:
            out = _encode(monkeypatch, cfg, blob, ids, lens, C.ROUTES[route])[:n]
        outs[route] = out
        if not np.isfinite(out).all():
            failures.append(f"{route}: non-finite output")
            continue
        got = float(M.one_minus_cos(out, ref).max())
        bar = r["bar"]
        if (case.name, precision, route) in OPEN_FINDINGS:
            bar = min(C.distance(case, d) for d in case.claimed(precision) if d != "pool_div") / 2
        rel = C.relation(case, precision, route)
        ran = "reference route"
        if rel is not None:
            other, how = rel
            equal = np.array_equal(out, outs[other])
            ran = f"bits {'==' if equal else '!='} {other} (expected {how})"
            if equal != (how == "same"):
                failures.append(f"{route}: {ran}" + ("" if equal else f", max |diff| {np.abs(out - outs[other]).max():.2e}")
                                + (": the route did not run" if equal else ""))
        line = f"BARS | {case.name} | {precision} | {route} | 1-cos {got:.2e} | floor {r['floor']:.2e} | bar {bar:.2e} | {ran}"
        if got > bar:
            failures.append(f"{route}: 1 - cos = {got:.2e} > bar {bar:.2e} (floor {r['floor']:.2e})")
        if not cfg.normalize:
            got_rel = float(M.rel_err(out, ref).max())
            line += f" | rel {got_rel:.2e} | floor_rel {r['floor_rel']:.2e} | bar_rel {r['bar_rel']:.2e}"
            if got_rel > r["bar_rel"]:
                failures.append(f"{route}: element-wise error {got_rel:.2e} > bar {r['bar_rel']:.2e} (floor {r['floor_rel']:.2e})")
        else:
            np.testing.assert_allclose(np.linalg.norm(out, axis=1), 1.0, atol=1e-5)
        print(line)
    assert not failures, f"{case.name} {precision}:\n  " + "\n  ".join(failures)
