#!/usr/bin/env python3
"""tools/bench_kuramoto.py -- the coupled-phase kernel (kuramoto.hip, K17, mxg_kuramoto_render) at 1024, 4096 and 16 384 sets of
N = 64 and N = 8 oscillators x 512 samples at 44 100 Hz, each in the exact and the mean-field form, mix only and with phases_out,
with the `sinewave` oscillator bank (65 536 voices x 512) timed alternately in the same process as the yardstick.  K17 is the
library's one kernel whose cost is not bytes: the exact form evaluates N * N sines per set and sample on the FP64 VALU, and
sinewave is the library's VALU-bound sine (README: 57-59 us for 33.5 M sines).  Device events, one pair per launch, median of
--reps blocks after a warm-up.  Prints one JSON line and writes it to --out:

  * us per block; for the exact form sines per second and their ratio to sinewave's ("sines_vs_sinewave": 1.0 = the same sine
    rate; the kernel's sine has no table and computes both fdlibm kernels, so well below 1 is expected);
  * the mean-field / exact time ratio per shape ("meanfield_over_exact");
  * for the phases_out form the algorithmic bytes (8 B per set and sample of mix + 8 N B of phases) and the fraction of 8 TB/s.

No pass mark: no number exists yet.

    python tools/bench_kuramoto.py [--reps 10] [--warmup 2] [--out profiles/kuramoto_bench.json]
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
SINE_V = 65536


def bench(L, S, N, a, sine):
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
        return L.mxg_kuramoto_render(mode, S, N, B, freq.ptr, 0, K.ptr, 0, phase[mode].ptr, None, None, want, mix.ptr,
                                     pout.ptr if want & 2 else None, None)

    sbank, sfreq, sout = sine
    runs = {
        "exact_mix": lambda: kura(0, 1),
        "exact_phases": lambda: kura(0, 3),
        "meanfield_mix": lambda: kura(1, 1),
        "meanfield_phases": lambda: kura(1, 3),
        "sinewave": lambda: (sbank.sinewave(sfreq, B, out=sout), 0)[1],
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
    sine_rate = SINE_V * B / res["sinewave"]["us"]            # sines per us
    for k in ("exact_mix", "exact_phases"):
        rate = S * N * N * B / res[k]["us"]
        res[k]["Gsines_s"] = round(rate / 1e3, 2)
        res[k]["sines_vs_sinewave"] = round(rate / sine_rate, 3)
    res["sinewave"]["Gsines_s"] = round(sine_rate / 1e3, 2)
    for w in ("mix", "phases"):
        res["meanfield_over_exact_" + w] = round(res["meanfield_" + w]["us"] / res["exact_" + w]["us"], 4)
    for k in ("exact_phases", "meanfield_phases"):
        by = 8.0 * (1 + N)
        res[k]["bytes_per_set_sample"] = by
        res[k]["frac_of_8TBs"] = round(by * S * B / res[k]["us"] / 1e3 / 8000, 4)
    for d in (freq, K, mix, pout, phase[0], phase[1]):
        d.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--n", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kuramoto_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    sbank = mx.maxiOscBank(SINE_V)
    sine = (sbank, mx.DeviceBuffer.from_numpy(20.0 + np.arange(SINE_V) * 0.3), mx.DeviceBuffer((B, SINE_V), zero=False))
    res = {"sample_rate": 44100, "reps": a.reps, "shapes": [bench(L, S, N, a, sine) for N in a.n for S in a.sets]}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
