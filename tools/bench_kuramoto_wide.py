#!/usr/bin/env python3
"""tools/bench_kuramoto_wide.py -- the wide coupled-phase kernel (kuramoto_wide.hip, K26, mxg_kuramoto_wide_render) at S x N =
256 x 1024, 1024 x 256, 16 x 1024 and 1 x 1024 oscillators x 512 samples at 44 100 Hz, each in the exact and the mean-field form,
mix only and with phases_out, with K17's exact form (mxg_kuramoto_render, 16 384 sets of 64, mix only) timed alternately in the
same process as the yardstick: both evaluate N * N sines per set and sample on the FP64 VALU with the same step functions, K26
with two workgroup barriers per sample.  Device events, one pair per launch, median of --reps blocks after a warm-up.  Prints one
JSON line and writes it to --out:

  * us per block; for the exact form T sines per second and their ratio to the yardstick's of the same run ("vs_k17": 1.0 = K17's
    sine rate);
  * for the mean-field form us per sample, against the 22.7 us a sample lasts at 44.1 kHz ("realtime_x": above 1 = faster than
    real time).  The exact form gets the same figure.

No pass mark: nothing is asserted on time.

    python tools/bench_kuramoto_wide.py [--reps 10] [--warmup 2] [--out profiles/kuramoto_wide_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maximilian_amd as mx  # noqa: E402

B = 512
SR = 44100
SHAPES = [(256, 1024), (1024, 256), (16, 1024), (1, 1024)]
K17_S, K17_N = 16384, 64


def bench(L, S, N, a, yard):
    D = mx.DeviceBuffer
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    rng = np.random.default_rng(S + N)
    freq = D.from_numpy(rng.uniform(0.5, 20.0, S))
    K = D.from_numpy(rng.uniform(0.0, 50.0, S))
    mix = D((B, S), zero=False)
    pout = D((B, S, N), zero=False)
    phase = {m: D.from_numpy(rng.uniform(0, 2 * np.pi, (S, N))) for m in (0, 1)}

    def kura(mode, want):
        return L.mxg_kuramoto_wide_render(mode, S, N, B, freq.ptr, 0, K.ptr, 0, phase[mode].ptr, None, None, want, mix.ptr,
                                          pout.ptr if want & 2 else None, None)

    yfreq, yK, yphase, ymix = yard
    runs = {
        "exact_mix": lambda: kura(0, 1),
        "exact_phases": lambda: kura(0, 3),
        "meanfield_mix": lambda: kura(1, 1),
        "meanfield_phases": lambda: kura(1, 3),
        "k17_exact_mix": lambda: L.mxg_kuramoto_render(0, K17_S, K17_N, B, yfreq.ptr, 0, yK.ptr, 0, yphase.ptr, None, None, 1, ymix.ptr,
                                                       None, None),
    }
    tot = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):  # alternating, one event pair per launch
        for k, f in runs.items():
            L.mxg_event_record(e0, None)
            mx._lib.check(f(), k)
            L.mxg_event_record(e1, None)
            L.mxg_event_sync(e1)
            L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            if i >= a.warmup:
                tot[k].append(ms.value * 1e3)
    res = {"S": S, "N": N, "B": B}
    for k, t in tot.items():
        res[k] = {"us": round(float(np.median(t)), 1), "min_us": round(float(np.min(t)), 1), "max_us": round(float(np.max(t)), 1)}
    yard_rate = K17_S * K17_N * K17_N * B / res["k17_exact_mix"]["us"]            # sines per us
    res["k17_exact_mix"]["Tsines_s"] = round(yard_rate / 1e6, 4)
    for k in ("exact_mix", "exact_phases"):
        rate = S * N * N * B / res[k]["us"]
        res[k]["Tsines_s"] = round(rate / 1e6, 4)
        res[k]["vs_k17"] = round(rate / yard_rate, 3)
    for k in ("exact_mix", "exact_phases", "meanfield_mix", "meanfield_phases"):
        res[k]["us_per_sample"] = round(res[k]["us"] / B, 3)
        res[k]["realtime_x"] = round(1e6 / SR / (res[k]["us"] / B), 3)
    for d in (freq, K, mix, pout, phase[0], phase[1]):
        d.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kuramoto_wide_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(SR, 2, 1024)
    D = mx.DeviceBuffer
    rng = np.random.default_rng(17)
    yard = (D.from_numpy(rng.uniform(0.5, 20.0, K17_S)), D.from_numpy(rng.uniform(0.0, 50.0, K17_S)),
            D.from_numpy(rng.uniform(0, 2 * np.pi, (K17_S, K17_N))), D((B, K17_S), zero=False))
    res = {"sample_rate": SR, "reps": a.reps, "us_per_sample_realtime": round(1e6 / SR, 2),
           "shapes": [bench(L, S, N, a, yard) for S, N in SHAPES]}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
