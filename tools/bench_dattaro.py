#!/usr/bin/env python3
"""tools/bench_dattaro.py -- the maxiDattaroReverb bank (dattaro.hip, K14) at 16 384 and 1 024 voices x 512 samples at 44 100 Hz
(4.2 GB of rings at the larger size), with K13's maxiFreeVerbStereo form (mxg_reverb_render, the path of tools/bench_reverb.py) timed
alternately in the same process as the yardstick.  Device events, one pair per launch, median of --reps blocks after a warm-up; the
input / output blocks rotate through --rot sets so that no launch finds its block in the caches from the launch before.  Prints
one JSON line and writes it to --out: us per block, G samples/s, the algorithmic bytes per sample and the fraction of 8 TB/s on
them.

Algorithmic bytes per sample: K14 328 (12 ring steps x 16 + 14 taps x 8 + 8 in + 16 out, the header of dattaro.hip); K13 stereo 280.

    python tools/bench_dattaro.py [--reps 20] [--warmup 5] [--rot 3] [--out profiles/dattaro_bench.json]
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

BYTES = {"dattaro": 328, "freeverb_stereo": 280}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dattaro_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    N, rate = 512, 44100
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    res = {"N": N, "sample_rate": rate, "reps": a.reps, "rot": a.rot}
    rng = np.random.default_rng(1)
    for V in (16384, 1024):
        xs = [mx.DeviceBuffer.from_numpy(rng.uniform(-1, 1, (N, V))) for _ in range(a.rot)]
        outs = [mx.DeviceBuffer((2, N, V), zero=False) for _ in range(a.rot)]
        dt = mx.maxiDattaroReverbBank(V, rate)
        fv = mx.maxiFreeVerbStereoBank(V)
        runs = {
            "dattaro": lambda i: L.mxg_dattaro_render(rate, V, N, xs[i % a.rot].ptr, dt.rings.ptr, dt.idx.ptr, dt.state.ptr,
                                                      outs[i % a.rot].ptr, None),
            "freeverb_stereo": lambda i: L.mxg_reverb_render(fv.KIND, 0, V, N, xs[i % a.rot].ptr, None, None, 0, fv.rings.ptr,
                                                             fv.idx.ptr, None, None, outs[i % a.rot].ptr, None),
        }
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
        for k, t in tot.items():
            us = float(np.median(t))
            res["V%d_%s" % (V, k)] = {
                "us": round(us, 1), "min_us": round(float(np.min(t)), 1), "max_us": round(float(np.max(t)), 1),
                "Gsamples_s": round(V * N / us / 1e3, 2), "bytes_per_sample": BYTES[k],
                "frac_of_8TBs": round(BYTES[k] * V * N / us / 1e3 / 8000, 4)}
        dt.rings.free()
        fv.rings.free()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
