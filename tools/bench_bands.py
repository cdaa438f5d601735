#!/usr/bin/env python3
"""tools/bench_bands.py -- the K19 kernels (bands.hip) on config 4's workload: 2^20 frames x 512 bins of magnitudes from
mxg_fft_batch.  Times mxg_bark_batch (specific only, then all four outputs) and mxg_octave_batch for (44100, 512, 12) (averages
only, then with the peak pass at 2048 streams x 512 frames), alternated in the same process with the two existing passes over the
same rows: mxg_fft_features (centroid) and mxg_mfcc_batch method 0 (512 bins, 42 filters, 13 coefficients).  Device events, one
pair per call, median of --reps after a warm-up.  Reports the algorithmic bytes (bins * 4 in, outputs out) over time.  The design
expectation to confirm or refute: a lane-per-frame walk costs 8 adds per frame per lane-slot and therefore sits on the row read,
like the centroid pass.  Prints one JSON line and writes it to --out.

    python tools/bench_bands.py [--frames 1048576] [--reps 10] [--warmup 3] [--out profiles/bands_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bands_bench.json"))
    a = ap.parse_args()
    L, D = mx.lib(), mx.DeviceBuffer
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    F, B, hop = a.frames, 512, 64   # frames 64 samples apart over one noise signal: every row differs
    fft = mx.maxiFFT()
    fft.setup(1024, 512, 1024)
    sig = D.from_numpy(np.random.default_rng(19).uniform(-1, 1, (F - 1) * hop + 1024).astype(np.float32))
    fft.process_frames(sig, hop, F)
    mags = fft.getMagnitudes()
    bark = mx.maxiBarkBatch()
    bark.setup(44100, 1024)
    oc = mx.maxiOctaveBatch()
    oc.setup(44100.0, B, 12)
    nA = oc.nAverages
    mf = mx.maxiMFCC()
    mf.setup(B, 42, 13, 20.0, 20000.0)
    b3 = [D((F, 24), np.float64, zero=False) for _ in range(3)]
    tot, cen = D(F, np.float64, zero=False), D(F, np.float32, zero=False)
    avg, pk = D((F, nA), np.float32, zero=False), D((F, nA), np.float32, zero=False)
    S = 2048 if F % 2048 == 0 else 1
    ps, hs = D((S, nA), np.float32), D((S, nA), np.int32)
    co = D((F, 13), np.float64, zero=False)
    runs = {
        "bark_specific": (lambda: L.mxg_bark_batch(bark.plan, mags.ptr, B, F, None, b3[1].ptr, None, None, None), B * 4 + 192),
        "bark_all": (lambda: L.mxg_bark_batch(bark.plan, mags.ptr, B, F, b3[0].ptr, b3[1].ptr, b3[2].ptr, tot.ptr, None), B * 4 + 3 * 192 + 8),
        "octave_averages": (lambda: L.mxg_octave_batch(oc.plan, mags.ptr, B, F, 1, 1.0, 0.0, 0, 0.9, avg.ptr, None, None, None, None), B * 4 + nA * 4),
        "octave_with_peaks": (lambda: L.mxg_octave_batch(oc.plan, mags.ptr, B, S, F // S, 1.0, 0.0, 2, 0.9, avg.ptr, pk.ptr, ps.ptr, hs.ptr, None),
                              B * 4 + nA * 4 * 3),
        "centroid": (lambda: L.mxg_fft_features(fft.plan, mags.ptr, F, None, None, cen.ptr, None), B * 4 + 4),
        "mfcc_method0": (lambda: L.mxg_mfcc_batch(mf.plan, mags.ptr, B, F, None, None, co.ptr, 0, None), B * 4 + 13 * 8),
    }
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    t = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):   # alternating, one event pair per call
        for k, (f, _) in runs.items():
            L.mxg_event_record(e0, None)
            mx._lib.check(f(), k)
            L.mxg_event_record(e1, None)
            L.mxg_event_sync(e1)
            L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            if i >= a.warmup:
                t[k].append(ms.value)
    res = {"frames": F, "bins": B, "nAverages": nA, "peak_streams": S, "reps": a.reps}
    for k, (_, nbytes) in runs.items():
        med = float(np.median(t[k]))
        res[k] = {"ms": round(med, 4), "min_ms": round(float(np.min(t[k])), 4), "bytes_per_frame": nbytes,
                  "TB_s": round(nbytes * F / med / 1e9, 3), "ratio_to_centroid": 0.0}
    for k in runs:
        res[k]["ratio_to_centroid"] = round(res[k]["ms"] / res["centroid"]["ms"], 3)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
