#!/usr/bin/env python3
"""tools/bench_reverb.py -- the reverb banks (reverb.hip, K13) at 65 536 and 1024 voices x 512 samples in their four forms:
maxiSatReverb, maxiFreeVerb play(x) (4 allpasses), play(x, roomsize, absorbtion) (31 allpasses) and maxiFreeVerbStereo.
Device events, one pair per launch, median of --reps blocks after a warm-up; the input / output blocks rotate through --rot
sets so that no launch finds its block in the caches from the launch before; K4 (mxg_delay_render, ring of 1024 slots) is timed
alternately in the same process as the yardstick tools/bench_fx.py uses.  Prints one JSON line: us per block, G samples/s, the
algorithmic bytes per sample and the fraction of 8 TB/s on them.

Algorithmic bytes per sample: 16 per ring step (read + write) + 8 in + 8 out per channel:
Sat 7 steps -> 128; FreeVerb play(x) 12 -> 208; play(x, r, a) 39 -> 640; Stereo 8 + 2 * 4 = 16 steps, two outputs -> 280.

    python tools/bench_reverb.py [--reps 20] [--warmup 5] [--rot 3]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maximilian_amd as mx  # noqa: E402

BYTES = {"sat": 128, "freeverb4": 208, "freeverb31": 640, "stereo": 280, "delay": 32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    N, cap = 512, 2048
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    res = {"N": N, "reps": a.reps, "rot": a.rot}
    rng = np.random.default_rng(1)
    for V in (65536, 1024):
        xs = [mx.DeviceBuffer.from_numpy(rng.uniform(-1, 1, (N, V))) for _ in range(a.rot)]
        outs = [mx.DeviceBuffer((2, N, V), zero=False) for _ in range(a.rot)]
        room = mx.DeviceBuffer.from_numpy(rng.uniform(-2.0, 1.0, V))
        absorb = mx.DeviceBuffer.from_numpy(rng.uniform(0.1, 0.9, V))
        size = mx.DeviceBuffer.from_numpy(np.full(V, 1024, np.int32))
        fb = mx.DeviceBuffer.from_numpy(np.full(V, 0.5))
        dlb = mx.maxiDelaylineBank(V, cap)
        for form in ("sat", "freeverb4", "freeverb31", "stereo"):
            bank = {"sat": mx.maxiSatReverbBank, "stereo": mx.maxiFreeVerbStereoBank}.get(form, mx.maxiFreeVerbBank)(V)
            lp = bank.lp.ptr if bank.lp is not None else None
            wc = bank.wc.ptr if bank.wc is not None else None
            mode = 1 if form == "freeverb31" else 0
            runs = {
                form: lambda i: L.mxg_reverb_render(bank.KIND, mode, V, N, xs[i % a.rot].ptr, room.ptr, absorb.ptr, 0, bank.rings.ptr,
                                                    bank.idx.ptr, lp, wc, outs[i % a.rot].ptr, None),
                "delay": lambda i: L.mxg_delay_render(0, V, N, xs[i % a.rot].ptr, size.ptr, fb.ptr, None, dlb.memory.ptr, cap,
                                                      dlb.phase.ptr, outs[i % a.rot].ptr, None),
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
                res["V%d_%s%s" % (V, k, "" if k == form else "_beside_" + form)] = {
                    "us": round(us, 1), "min_us": round(float(np.min(t)), 1), "Gsamples_s": round(V * N / us / 1e3, 2),
                    "bytes_per_sample": BYTES[k], "frac_of_8TBs": round(BYTES[k] * V * N / us / 1e3 / 8000, 4)}
            bank.rings.free()
        dlb.memory.free()
    for form in ("sat", "freeverb4", "freeverb31", "stereo"):
        res["%s_1024_over_65536" % form] = round(res["V1024_" + form]["us"] / res["V65536_" + form]["us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
