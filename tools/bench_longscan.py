#!/usr/bin/env python3
"""tools/bench_longscan.py -- K28 (csrc/scan_long.hip, mxg_scan_long_render): every kind at V in {1, 8, 64} voices and N in
{2^16, 2^20, 2^24} samples (V * N capped at 2^26), beside two yardsticks from the same run:
  sequential   the sequential entry point of the kind at the same V and N (mxg_filter2_render / mxg_filter_render /
               mxg_lag_render, knob time_parallel = 0): the only path for that shape before K28 -- one lane per voice;
  k10_looped   K10 (knob time_parallel = 1) called once per 2048-sample block, N / 2048 launches (kinds 0-4; the lag has no K10).
Device events round each call on the default stream, median of --reps calls after --warmup; the input and output blocks rotate
through --rot sets.  K28's three launches are also timed one by one through the library's per-kernel timers (mxg_prof_*), in a
pass of their own.  Algorithmic bytes: 24 per voice-sample (8 read by the summaries, 8 read and 8 written by the render); the
fraction of 8 TB/s is taken on those -- with --rot 2 the blocks of the shapes below 2^26 bytes stay in the L2 / Infinity Cache from
one repetition to the next, for K28 and for the yardsticks alike: an HBM figure only for the largest shapes.  Prints one JSON line
and writes it to --out.

    python tools/bench_longscan.py [--reps 10] [--warmup 3] [--rot 2] [--out profiles/longscan_bench.json]
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

KINDS = ["dc", "svf", "biquad", "lores", "hires", "lag"]
T = 2048
LAUNCHES = ["scan_long_summary_kernel", "scan_long_chunks_kernel", "scan_long_render_kernel"]


def timed(L, f, a, reps=None):
    reps = a.reps if reps is None else reps
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    t = []
    for i in range(a.warmup + reps):
        L.mxg_event_record(e0, None)
        f(i)
        L.mxg_event_record(e1, None)
        L.mxg_event_sync(e1)
        L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
        if i >= a.warmup:
            t.append(ms.value * 1e3)
    L.mxg_event_destroy(e0)
    L.mxg_event_destroy(e1)
    return round(float(np.median(t)), 1)


def coefficients(kind, V):
    b = mx.maxiLongScanBank(V, kind)
    v = np.arange(V)
    {"dc": lambda: b.setDC(0.995), "svf": lambda: b.setSVF(300.0 + 10.0 * v, 2.0, (0.5, 0.25, 0.125, 0.6)),
     "biquad": lambda: b.setBiquad(0, 800.0 + 10.0 * v, 0.7, 0.0), "lores": lambda: b.setLores(800.0 + 10.0 * v, 3.0),
     "hires": lambda: b.setHires(800.0 + 10.0 * v, 3.0), "lag": lambda: b.setLag(0.01)}[kind]()
    return b.coef


def per_launch(L, call, a):
    """K28's launches one by one: the library's per-kernel timers over a.reps calls (a pass of its own: the timers add events)."""
    out = {}
    prev = L.mxg_prof_enable(1)
    try:
        L.mxg_prof_reset()
        for i in range(a.reps):
            call(i)
        mx._lib.check(L.mxg_sync(), "mxg_sync")
        for idx in range(L.mxg_prof_count()):
            label, ms, n = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_size_t()
            if L.mxg_prof_read(idx, ctypes.byref(label), ctypes.byref(ms), ctypes.byref(n)) == 0 and n.value and label.value.decode() in LAUNCHES:
                out[label.value.decode()] = round(ms.value * 1e3 / n.value, 1)
    finally:
        L.mxg_prof_reset()
        L.mxg_prof_enable(prev)
    return out


def bench(L, kind, V, N, a):
    D = mx.DeviceBuffer
    k = KINDS.index(kind)
    rng = np.random.default_rng(28)
    xs = [D.from_numpy(rng.uniform(-1, 1, (N, V))) for _ in range(a.rot)]
    outs = [D((N, V), zero=False) for _ in range(a.rot)]
    coef = coefficients(kind, V)
    rows = {"dc": 3, "svf": 3, "biquad": 3, "lores": 5, "hires": 5, "lag": 1}[kind]
    dcoef = D.from_numpy(np.concatenate([coef, np.zeros((1, V))]) if kind in ("lores", "hires") else coef)
    st = D((rows, V))
    dummy = D(V)

    def long_call(i):
        j = i % a.rot
        mx._lib.check(L.mxg_scan_long_render(k, V, N, xs[j].ptr, dcoef.ptr, st.ptr, outs[j].ptr, None), "mxg_scan_long_render")

    def seq_block(xp, op, n):
        if k <= 2:
            rc = L.mxg_filter2_render(k, V, n, xp, dcoef.ptr, st.ptr, op, None)
        elif k == 5:
            rc = L.mxg_lag_render(V, n, xp, dcoef.ptr, dcoef.ptr + 8 * V, 0, st.ptr, op, None)
        else:
            rc = L.mxg_filter_render(k - 3, V, n, xp, dummy.ptr, 0, dummy.ptr, 0, dcoef.ptr, st.ptr, op, None)
        mx._lib.check(rc, "sequential entry point")

    def seq_call(i):
        j = i % a.rot
        seq_block(xs[j].ptr, outs[j].ptr, N)

    def k10_call(i):
        j = i % a.rot
        for b in range(N // T):
            seq_block(xs[j].ptr + 8 * b * T * V, outs[j].ptr + 8 * b * T * V, T)

    r = {"kind": kind, "V": V, "N": N}
    r["k28_us"] = timed(L, long_call, a)
    pl = per_launch(L, long_call, a)
    if pl:
        r["k28_launch_us"] = pl
    nbytes = 24 * V * N
    r["algorithmic_bytes"] = nbytes
    r["frac_of_8TBs"] = round(nbytes / (r["k28_us"] * 1e-6) / 8e12, 4)
    L.mxg_tune(b"time_parallel", 0)
    r["sequential_us"] = timed(L, seq_call, a, reps=max(2, a.reps // 3 if N >= 1 << 24 else a.reps))
    if k != 5:
        L.mxg_tune(b"time_parallel", 1)
        try:
            r["k10_looped_us"] = timed(L, k10_call, a, reps=max(2, a.reps // 3 if N >= 1 << 24 else a.reps))
        finally:
            L.mxg_tune(b"time_parallel", 0)
    r["sequential_over_k28"] = round(r["sequential_us"] / r["k28_us"], 1)
    if "k10_looped_us" in r:
        r["k10_looped_over_k28"] = round(r["k10_looped_us"] / r["k28_us"], 1)
    for b in xs + outs + [dcoef, st, dummy]:
        b.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rot", type=int, default=2)
    ap.add_argument("--kinds", nargs="*", default=KINDS)
    ap.add_argument("--voices", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20, 24])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longscan_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    runs = []
    for kind in a.kinds:
        for V in a.voices:
            for ln in a.log2n:
                if V << ln > 1 << 26:
                    continue
                runs.append(bench(L, kind, V, 1 << ln, a))
                print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    res = {"chunk": T, "reps": a.reps, "warmup": a.warmup, "rot": a.rot, "runs": runs}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
