#!/usr/bin/env python3
"""tools/bench_fx.py -- maxiFlanger / maxiChorus banks (fx.hip, K11) at 65 536 voices x 512 samples, timed with device
events after a warm-up, alternating with mxg_delay_render (K4, static size 1024) at the same V, N and ring size in the
same process.  Prints one JSON line: us per block, algorithmic bytes and the fraction of 8 TB/s.

Regimes: large (delay 800, depth 0.5: sizes 400-1201, cap 2048, conflict-free tiles) and short (delay 20, depth 0.5:
sizes below the 64-sample tile, every tile walked serially; no bar, it must finish).

    python tools/bench_fx.py [--reps 20] [--warmup 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maximilian_amd as mx  # noqa: E402
from maximilian_amd.banks import chorus_coeffs  # noqa: E402

BYTES = {"delay": 32, "flanger": 32, "chorus": 52}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--voices", type=int, default=65536)
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    V, N, cap = a.voices, 512, 2048
    rng = np.random.default_rng(1)
    x = mx.DeviceBuffer.from_numpy(rng.uniform(-1, 1, (N, V)))
    out = mx.DeviceBuffer((N, V), zero=False)
    speed = rng.uniform(0.1, 10.0, V)
    rand = mx.DeviceBuffer.from_numpy(rng.integers(0, 2 ** 31 - 1, (N, V), dtype=np.int32))
    coef = mx.DeviceBuffer.from_numpy(chorus_coeffs(speed))
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    res = {"V": V, "N": N, "cap": cap}
    for regime, delay in (("large", 800), ("short", 20)):
        dl = mx.DeviceBuffer.from_numpy(np.full(V, delay, np.uint32))
        fb = mx.DeviceBuffer.from_numpy(np.full(V, 0.5))
        dp = mx.DeviceBuffer.from_numpy(np.full(V, 0.5))
        sp = mx.DeviceBuffer.from_numpy(speed)
        size = mx.DeviceBuffer.from_numpy(np.full(V, 1024 if regime == "large" else delay, np.int32))
        dlb = mx.maxiDelaylineBank(V, cap)
        fl = mx.maxiFlangerBank(V, cap)
        ch = mx.maxiChorusBank(V, cap)
        runs = {
            "delay": lambda: L.mxg_delay_render(0, V, N, x.ptr, size.ptr, fb.ptr, None, dlb.memory.ptr, cap,
                                                dlb.phase.ptr, out.ptr, None),
            "flanger": lambda: L.mxg_flanger_render(V, N, x.ptr, dl.ptr, fb.ptr, sp.ptr, dp.ptr, 0, fl.memory.ptr, cap,
                                                    fl.phase.ptr, fl.lfo_phase.ptr, None, out.ptr, None),
            "chorus": lambda: L.mxg_chorus_render(V, N, x.ptr, dl.ptr, fb.ptr, dp.ptr, 0, rand.ptr, coef.ptr, 0,
                                                  ch.memory.ptr, cap, ch.phase.ptr, ch.lp.ptr, None, out.ptr, None),
        }
        for f in runs.values():
            for _ in range(a.warmup):
                mx._lib.check(f(), "warm-up")
        tot = {k: [] for k in runs}
        for _ in range(a.reps):  # alternating, one event pair per launch
            for k, f in runs.items():
                L.mxg_event_record(e0, None)
                mx._lib.check(f(), k)
                L.mxg_event_record(e1, None)
                L.mxg_event_sync(e1)
                L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
                tot[k].append(ms.value * 1e3)
        for k, t in tot.items():
            us = float(np.median(t))
            gbs = BYTES[k] * V * N / us / 1e3
            res["%s_%s" % (regime, k)] = {"us": round(us, 1), "algorithmic_bytes": BYTES[k] * V * N,
                                          "frac_of_8TBs": round(gbs / 8000, 3)}
        res["%s_flanger_over_delay" % regime] = round(res["%s_flanger" % regime]["us"] / res["%s_delay" % regime]["us"], 3)
        for b in (dlb, fl, ch):
            b.memory.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
