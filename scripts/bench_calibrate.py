"""What the calibrated open costs (mx_encoder_open_calibrated, include/memex_hip.h) against the plain creates it replaces.

For the all-MiniLM-L6-v2, all-MiniLM-L12-v2 and bge-base-en shapes (full vocabulary) under checkpoint_like_weights:
  * one plain mx_encoder_create per precision mode -- the host route: every matrix re-laid on one host thread and uploaded;
    a naive calibration would pay all four;
  * one mx_encoder_open_calibrated with MX_CALIBRATE_ALL (all four modes built from one upload, on the device) and one
    without (stops at the chosen mode), with the library's own calibration time out of the report;
  * the chosen mode and the deviations that decided it.
The first open of a process also loads the kernels: a throw-away encoder is opened before anything is timed.
usage: bench_calibrate.py [seed]"""
import dataclasses, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from memex_amd.encoder import Encoder
from memex_amd import weights as W

seed = int(sys.argv[1]) if len(sys.argv) > 1 else 52
MODES = ("bf16", "mixed1", "mixed", "bf16x3")
warm = dataclasses.replace(W.ALL_MINILM_L6_V2, layers=1, vocab=1000)
Encoder(warm, W.pack_weights(W.synthetic_weights(warm, 0), warm)).close()
Encoder(dataclasses.replace(warm, precision="auto"), W.pack_weights(W.synthetic_weights(warm, 0), warm)).close()
for name, base in (("all-MiniLM-L6-v2", W.ALL_MINILM_L6_V2), ("all-MiniLM-L12-v2", W.ALL_MINILM_L12_V2), ("bge-base-en", W.BGE_BASE_EN)):
    blob = W.pack_weights(W.checkpoint_like_weights(base, seed), base)
    plain = {}
    for mode in MODES:
        t0 = time.perf_counter()
        enc = Encoder(dataclasses.replace(base, precision=mode), blob)
        plain[mode] = (time.perf_counter() - t0) * 1e3
        enc.close()
    auto = dataclasses.replace(base, precision="auto")
    t0 = time.perf_counter()
    enc = Encoder(auto, blob, measure_all=True)
    t_all = (time.perf_counter() - t0) * 1e3
    rep_all = enc.calibration
    enc.close()
    t0 = time.perf_counter()
    enc = Encoder(auto, blob)
    t_open = (time.perf_counter() - t0) * 1e3
    rep = enc.calibration
    enc.close()
    print(f"{name} (blob {blob.nbytes / 2**20:.0f} MiB, checkpoint_like_weights seed {seed}):")
    print("  plain mx_encoder_create  " + "  ".join(f"{m} {t:.0f} ms" for m, t in plain.items()) + f"  | all four {sum(plain.values()):.0f} ms")
    print(f"  mx_encoder_open_calibrated  {t_open:.0f} ms (library {rep.ms:.0f} ms; tried {', '.join(rep.tried)}) -> {rep.chosen}"
          f"  | with MX_CALIBRATE_ALL {t_all:.0f} ms (library {rep_all.ms:.0f} ms)")
    print("  pair_dev  " + "  ".join(f"{m} {rep_all.pair_dev[m]:.2e}" for m in MODES) + f"  | bar {rep_all.bar:.1e}", flush=True)
