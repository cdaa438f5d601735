#!/usr/bin/env python3
"""tools/bench_analysis.py -- the fused analysis kernel (analysis.hip, K16, mxg_analysis_render) at 65 536 and 1024 voices x 512
samples at 44 100 Hz in three forms -- the zero-crossing rate alone, the envelope follower alone, all four outputs -- with two of
the parent kernels on the same shape timed alternately in the same process as the yardsticks: mxg_rms_render at
window = cap = 44 100 (the closest kernel with a ring of DOUBLES: 16 B of ring traffic per sample) and the maxiDCBlocker form of
mxg_filter2_render (the plain 8 B in / 8 B out stream).  The rate keeps its window as a ring of BITS (one word read and one
written per 64 samples), so the design expectation is that it sits with the DC blocker ("ratio_to_dcblock"), not with the RMS
ring ("ratio_to_rms").  Device events, one pair per launch, median of --reps blocks after a warm-up; the input and output blocks
rotate through --rot sets so that no launch finds its blocks in the caches from the launch before.  Prints one JSON line and
writes it to --out: us per block, G samples/s, the algorithmic bytes per sample and the fraction of 8 TB/s on them.

Algorithmic bytes per sample: 8 in + 8 per output block; the RMS ring adds 8 written + 8 read, the ring of bits 16 / 64.

    python tools/bench_analysis.py [--reps 20] [--warmup 5] [--rot 3] [--out profiles/analysis_bench.json]
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

BYTES = {"ana_zcr": 16.25, "ana_env": 16, "ana_all": 40.25, "rms_ring": 32, "dcblock": 16}
CAP = 44100


def bench(L, V, N, a):
    D = mx.DeviceBuffer
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    rng = np.random.default_rng(1)
    # audio-like input: a few hundred crossings per voice and second
    n = np.arange(N)[:, None]
    ins = []
    for r in range(a.rot):
        f = rng.uniform(50.0, 2000.0, V)[None, :]
        ins.append(D.from_numpy(np.sin(2 * np.pi * n * f / 44100.0 + rng.uniform(0, 6, V)[None, :]) * rng.uniform(0.1, 1.0, V)[None, :]))
    outs = [[D((N, V), zero=False) for _ in range(4)] for _ in range(a.rot)]
    ana = mx.maxiAnalysisBank(V, cap=CAP)
    ana.hold_ms.upload(rng.choice([1.0, 2.5, 37.0, 300.0], V))
    win = D.from_numpy(ana.window)
    rms = mx.maxiRMSBank(V, CAP)
    rms.window[:] = CAP
    rwin = D.from_numpy(rms.window)
    dcb = mx.maxiDCBlockerBank(V)
    dcb.coef = D.from_numpy(np.full(V, 0.995))

    def ana_call(i, want):
        o, x = outs[i % a.rot], ins[i % a.rot]
        return L.mxg_analysis_render(V, N, x.ptr, want, ana.prev_x.ptr, win.ptr, ana.zring.ptr, CAP, ana.zpos.ptr, ana.zcount.ptr,
                                     ana.overflow.ptr, ana.attack.ptr, ana.release.ptr, ana.env.ptr, ana.hold_ms.ptr, 0, ana.sah_phase.ptr,
                                     ana.sah_value.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, None)

    runs = {
        "ana_zcr": lambda i: ana_call(i, 2),
        "ana_env": lambda i: ana_call(i, 4),
        "ana_all": lambda i: ana_call(i, 15),
        "rms_ring": lambda i: L.mxg_rms_render(V, N, ins[i % a.rot].ptr, rwin.ptr, rms.ring.ptr, CAP, rms.pos.ptr, rms.running.ptr,
                                               rms.overflow.ptr, outs[i % a.rot][0].ptr, None),
        "dcblock": lambda i: L.mxg_filter2_render(0, V, N, ins[i % a.rot].ptr, dcb.coef.ptr, dcb.state.ptr, outs[i % a.rot][1].ptr, None),
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
    res = {"V": V, "N": N, "cap": CAP}
    for k, t in tot.items():
        us = float(np.median(t))
        res[k] = {"us": round(us, 1), "min_us": round(float(np.min(t)), 1), "max_us": round(float(np.max(t)), 1),
                  "Gsamples_s": round(V * N / us / 1e3, 2), "bytes_per_sample": BYTES[k],
                  "frac_of_8TBs": round(BYTES[k] * V * N / us / 1e3 / 8000, 4)}
    for k in ("ana_zcr", "ana_env", "ana_all"):
        res[k]["ratio_to_dcblock"] = round(res[k]["us"] / res["dcblock"]["us"], 3)
        res[k]["ratio_to_rms"] = round(res[k]["us"] / res["rms_ring"]["us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--voices", type=int, nargs="+", default=[65536, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analysis_bench.json"))
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
