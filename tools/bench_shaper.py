#!/usr/bin/env python3
"""tools/bench_shaper.py -- the K18 kernels (shaper.hip) at 65 536 and 1024 voices x 512 samples: every maxiNonlinearity mode
(per-voice parameters), the cross-fade at C = 1 and C = 2 with an xfader per sample, maxiSelectX at K = 4 with signal values, and
the line on a trigger block -- with the maxiDCBlocker form of mxg_filter2_render (the plain 8 B in / 8 B out stream of the "one
lane per voice, samples serial" shape) timed alternately in the same process as the yardstick.  The three stateless kernels are
flat over the N * V elements with 16-byte accesses, so the design expectation is: hardclip, fastatan and fastAtanDist at or
below the DC blocker at the same 16 B per sample, the cross-fade at C = 1 (32 B per sample) no worse than 32 / 16 of it,
atanDist and asymclip possibly VALU-bound.  Device events, one pair per launch, median of --reps blocks after a warm-up; the
blocks rotate through --rot sets so that no launch finds its blocks in the caches from the launch before.  Prints one JSON line
and writes it to --out: us per block, G samples/s, the algorithmic bytes per sample, the fraction of 8 TB/s on them and the
ratio to the DC blocker's step ("ratio_to_dcblock", and per byte "ratio_per_byte").

Algorithmic bytes per sample: shaping 8 in + 8 out; xfade 8 (xfader) + C * 24; SelectX 8 (index) + 2 * 8 (the two values read)
+ 8 out; the line 8 in + 8 out.

    python tools/bench_shaper.py [--reps 20] [--warmup 5] [--rot 3] [--out profiles/shaper_bench.json]
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

BYTES = {"hardclip": 16, "softclip": 16, "fastatan": 16, "fastAtanDist": 16, "atanDist": 16, "asymclip": 16, "xfade_c1": 32, "xfade_c2": 56,
         "selectx_k4": 32, "line": 16, "dcblock": 16}


def bench(L, V, N, a):
    D = mx.DeviceBuffer
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    rng = np.random.default_rng(18)
    K = 4
    ins = [D.from_numpy(rng.uniform(-1.5, 1.5, (K, N, V))) for _ in range(a.rot)]   # 4 blocks per set: inputs, channels, select values
    idx = [D.from_numpy(rng.uniform(-0.5, K + 0.5, (N, V))) for _ in range(a.rot)]
    outs = [D((2, N, V), zero=False) for _ in range(a.rot)]
    E = N * V * 8
    shape = D.from_numpy(rng.uniform(0.5, 50.0, V))
    norm = D.from_numpy(mx.atan_norm(shape.numpy()))
    ea, eb = D.from_numpy(rng.uniform(0.25, 8.0, V)), D.from_numpy(rng.uniform(0.25, 8.0, V))
    line = mx.maxiLineBank(V)
    line.prepare(0.0, 1.0, rng.uniform(1.0, 8.0, V), False)
    line.triggerEnable(1)
    dcb = mx.maxiDCBlockerBank(V)
    dcb.coef = D.from_numpy(np.full(V, 0.995))

    def shaper(mode, pa=None, pb=None):
        return lambda i: L.mxg_shape_render(mx.SHAPE_MODES[mode], V, N, ins[i % a.rot].ptr, pa and pa.ptr, pb and pb.ptr, 0, outs[i % a.rot].ptr, None)

    runs = {
        "hardclip": shaper("hardclip"), "softclip": shaper("softclip"), "fastatan": shaper("fastatan"),
        "fastAtanDist": shaper("fastAtanDist", shape), "atanDist": shaper("atanDist", shape, norm), "asymclip": shaper("asymclip", ea, eb),
        "xfade_c1": lambda i: L.mxg_xfade_render(1, V, N, ins[i % a.rot].ptr, ins[i % a.rot].ptr + E, idx[i % a.rot].ptr, 1, outs[i % a.rot].ptr, None),
        "xfade_c2": lambda i: L.mxg_xfade_render(2, V, N, ins[i % a.rot].ptr, ins[i % a.rot].ptr + 2 * E, idx[i % a.rot].ptr, 1, outs[i % a.rot].ptr, None),
        "selectx_k4": lambda i: L.mxg_select_render(1, K, V, N, idx[i % a.rot].ptr, ins[i % a.rot].ptr, 1, 0, None, outs[i % a.rot].ptr, None),
        "line": lambda i: L.mxg_line_render(V, N, ins[i % a.rot].ptr, 0.0, line.par.ptr, line.state.ptr, outs[i % a.rot].ptr, None),
        "dcblock": lambda i: L.mxg_filter2_render(0, V, N, ins[i % a.rot].ptr, dcb.coef.ptr, dcb.state.ptr, outs[i % a.rot].ptr, None),
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
    res = {"V": V, "N": N}
    for k, t in tot.items():
        us = float(np.median(t))
        res[k] = {"us": round(us, 1), "min_us": round(float(np.min(t)), 1), "max_us": round(float(np.max(t)), 1),
                  "Gsamples_s": round(V * N / us / 1e3, 2), "bytes_per_sample": BYTES[k],
                  "frac_of_8TBs": round(BYTES[k] * V * N / us / 1e3 / 8000, 4)}
    for k in runs:
        if k != "dcblock":
            res[k]["ratio_to_dcblock"] = round(res[k]["us"] / res["dcblock"]["us"], 3)
            res[k]["ratio_per_byte"] = round(res[k]["us"] / res["dcblock"]["us"] * BYTES["dcblock"] / BYTES[k], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--voices", type=int, nargs="+", default=[65536, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shaper_bench.json"))
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
