#!/usr/bin/env python3
"""tools/bench_polyblep.py -- the K20 kernel (polyblep.hip) at 65 536 and 1024 voices x 512 samples: SAWTOOTH, SQUARE, TRIANGLE,
SINE and TRAPEZOID_VARIABLE with one frequency per voice, and mxg_osc_render's saw and sinewave -- the same write-only 8 B per
sample stream -- timed alternately in the same process as the yardsticks.  Frequencies are spread over 20 Hz .. 8 kHz at 44.1 kHz,
so dt reaches 0.18 and the blep / blamp arms are taken on a good share of the samples; nothing reaches the sine fallback.
Device events, one pair per launch, median of --reps blocks after a warm-up; the output blocks rotate through --rot buffers so
that no launch finds its block in the caches from the launch before.  Prints one JSON line and writes it to --out: us per block,
G samples/s, the fraction of 8 TB/s on 8 B per sample, and each waveform's ratio to `saw` (the arithmetic ones) or to `sinewave`
(SINE) from the same run.

    python tools/bench_polyblep.py [--reps 20] [--warmup 5] [--rot 3] [--out profiles/polyblep_bench.json]
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

WAVES = ["SAWTOOTH", "SQUARE", "TRIANGLE", "SINE", "TRAPEZOID_VARIABLE"]
YARD = {"SAWTOOTH": "saw", "SQUARE": "saw", "TRIANGLE": "saw", "TRAPEZOID_VARIABLE": "saw", "SINE": "sinewave"}


def bench(L, V, N, a):
    D = mx.DeviceBuffer
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    rng = np.random.default_rng(20)
    freq = D.from_numpy(np.exp(rng.uniform(np.log(20.0), np.log(8000.0), V)))
    pw = D.from_numpy(rng.uniform(0.1, 0.9, V))
    outs = [D((N, V), zero=False) for _ in range(a.rot)]
    t = D(V)
    osc = mx.maxiOscBank(V)

    def pb(wf):
        return lambda i: L.mxg_polyblep_render(mx.POLYBLEP_WAVEFORMS[wf], V, N, freq.ptr, 0, pw.ptr, 44100.0, t.ptr, outs[i % a.rot].ptr, None)

    def yard(wf):
        return lambda i: L.mxg_osc_render(mx.OSC_WAVEFORMS[wf], V, N, freq.ptr, 0, None, None, osc.phase.ptr, osc.output.ptr, outs[i % a.rot].ptr, None)

    runs = {wf: pb(wf) for wf in WAVES}
    runs.update({"saw": yard("saw"), "sinewave": yard("sinewave")})
    tot = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):  # alternating, one event pair per launch
        for k, f in runs.items():
            L.mxg_event_record(e0, None)
            mx._lib.check(f(i), k)
            L.mxg_event_record(e1, None)
            L.mxg_event_sync(e1)
            L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            if i >= a.warmup:
                tot[k].append(ms.value * 1e3)
    res = {"V": V, "N": N}
    for k, x in tot.items():
        us = float(np.median(x))
        res[k] = {"us": round(us, 1), "min_us": round(float(np.min(x)), 1), "max_us": round(float(np.max(x)), 1),
                  "Gsamples_s": round(V * N / us / 1e3, 2), "frac_of_8TBs": round(8 * V * N / us / 1e3 / 8000, 4)}
    for k in WAVES:
        res[k]["ratio_to_" + YARD[k]] = round(res[k]["us"] / res[YARD[k]]["us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--voices", type=int, nargs="+", default=[65536, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polyblep_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    res = {"sample_rate": 44100, "reps": a.reps, "rot": a.rot, "banks": [bench(L, V, 512, a) for V in a.voices]}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
