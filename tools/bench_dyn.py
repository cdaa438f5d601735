#!/usr/bin/env python3
"""tools/bench_dyn.py -- maxiDynamicsBank (dyn.hip, K12) at 65 536 and 1024 voices x 512 samples, RMS and PEAK detector, with and
without look-ahead, timed with device events (median of --reps launches after a warm-up).  The input / output blocks rotate through
--rot sets so that no launch finds its block in the caches from the launch before.  Prints one JSON line: us per block, G samples/s,
algorithmic bytes per sample and the fraction of 8 TB/s on them.

Algorithmic bytes per sample (compress(): the control is the input): 8 in + 8 out; RMS detector + 8 ring write + 8 tail read;
look-ahead + 8 ring write + 8 ring read.

    python tools/bench_dyn.py [--reps 20] [--warmup 5] [--rot 3]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maximilian_amd as mx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    N = 512
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    res = {"N": N, "reps": a.reps, "rot": a.rot}
    rng = np.random.default_rng(1)
    for V in (65536, 1024):
        n = np.arange(N)[:, None]
        xs = []
        for r in range(a.rot):  # amplitude-modulated noise: the level crosses the threshold inside every block
            amp = 10.0 ** ((-40.0 + 40.0 * (0.5 - 0.5 * np.cos(n * 0.02 + rng.uniform(0, 6.28, V)[None, :]))) / 20.0)
            xs.append(mx.DeviceBuffer.from_numpy(rng.uniform(-1, 1, (N, V)) * amp))
        outs = [mx.DeviceBuffer((N, V), zero=False) for _ in range(a.rot)]
        for analyser in ("RMS", "PEAK"):
            for look in (0, 88):
                bank = mx.maxiDynamicsBank(V, cap_rms=1024, cap_lookahead=256)
                bank.setInputAnalyser(getattr(bank, analyser))
                bank.setRMSWindowSize(10.0)           # 441 samples
                bank.lookahead[:] = look              # 2 ms
                bank.invalidate()
                # the parameters as device arrays, so that no launch uploads anything
                th, ra, kn, z = (mx.DeviceBuffer.from_numpy(np.full(V, c)) for c in (-20.0, 4.0, 6.0, 0.0))
                bank._upload_control()
                t = []
                for i in range(a.warmup + a.reps):
                    x, o = xs[i % a.rot], outs[i % a.rot]
                    L.mxg_event_record(e0, None)
                    bank.play(x, None, th, ra, kn, z, z, z, out=o)
                    L.mxg_event_record(e1, None)
                    L.mxg_event_sync(e1)
                    L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
                    if i >= a.warmup:
                        t.append(ms.value * 1e3)
                us = float(np.median(t))
                b = 16 + (16 if analyser == "RMS" else 0) + (16 if look else 0)
                res["V%d_%s_look%d" % (V, analyser, look)] = {
                    "us": round(us, 1), "min_us": round(float(np.min(t)), 1), "Gsamples_s": round(V * N / us / 1e3, 2),
                    "bytes_per_sample": b, "frac_of_8TBs": round(b * V * N / us / 1e3 / 8000, 4)}
                for buf in (bank.rms_ring, bank.la_ring):
                    buf.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
