#!/usr/bin/env python3
"""tools/bench_longsweep.py -- K31 (csrc/scan_long_swept.hip, mxg_scan_long_render_swept): lores, hires and the lag with per-sample
coefficients at the shapes of K28's table (1 x 2^16, 1 x 2^20, 1 x 2^24, 8 x 2^20, 64 x 2^20), coef_rows 2 (packed) and 3 (the array
mxg_filter_render_coefs takes), beside two yardsticks from the same run:
  sequential   the sequential per-sample entry point at the same V and N (mxg_filter_render_coefs; mxg_lag_render with
               alpha_per_sample = 1): the only path for a sweep before K31 -- one lane per voice;
  k28_const    mxg_scan_long_render (block-constant coefficients) at the same shape: what the sweep costs over K28.
Device events round each call on the default stream, median of --reps calls after --warmup (the sequential path at 2^24: 2 after
1, a call is over a second); input, coefficient and output blocks rotate through --rot sets.  K31's three launches are also timed
one by one through the library's per-kernel timers (mxg_prof_*), in a pass of their own.  Algorithmic bytes per voice-sample:
8 (1 + rows) read in A, the same read in C, 8 written; the fraction of 8 TB/s is taken on those -- with --rot 2 the blocks of the
small shapes stay in the L2 / Infinity Cache from one repetition to the next: an HBM figure only for the largest shapes.  Prints
one JSON line and writes it to --out.

    python tools/bench_longsweep.py [--reps 10] [--warmup 3] [--rot 2] [--out profiles/longsweep_bench.json]
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

KINDS = {"lores": 3, "hires": 4, "lag": 5}
TS = 1024
LAUNCHES = ["scan_long_swept_summary_kernel", "scan_long_swept_chunks_kernel", "scan_long_swept_render_kernel"]
SHAPES = [(1, 16), (1, 20), (1, 24), (8, 20), (64, 20)]


def timed(L, f, warmup, reps):
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    t = []
    for i in range(warmup + reps):
        L.mxg_event_record(e0, None)
        f(i)
        L.mxg_event_record(e1, None)
        L.mxg_event_sync(e1)
        L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
        if i >= warmup:
            t.append(ms.value * 1e3)
    L.mxg_event_destroy(e0)
    L.mxg_event_destroy(e1)
    return round(float(np.median(t)), 1)


def per_launch(L, call, reps):
    out = {}
    prev = L.mxg_prof_enable(1)
    try:
        L.mxg_prof_reset()
        for i in range(reps):
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


def sweep(kind, V, N, rows, phase):
    """[N][rows][V]: any stable moving coefficients do for a timing -- c on a slow LFO 0.01 ... 0.2 with r = 0.95; alpha on one 0.001 ... 0.5."""
    n = np.arange(N, dtype=np.float64)
    lfo = 0.5 + 0.5 * np.sin(2.0 * np.pi * 2.0 * n / 44100.0 + phase)
    c = np.zeros((N, rows, V))
    if kind == "lag":
        c[:, 0] = (0.001 + 0.499 * lfo)[:, None]
        c[:, 1] = 1.0 - c[:, 0]
    else:
        c[:, 0] = (0.01 + 0.19 * lfo)[:, None]
        c[:, 1] = 0.95
    return c


def bench(L, kind, V, N, a):
    D = mx.DeviceBuffer
    k = KINDS[kind]
    rng = np.random.default_rng(31)
    xs = [D.from_numpy(rng.uniform(-1, 1, (N, V))) for _ in range(a.rot)]
    outs = [D((N, V), zero=False) for _ in range(a.rot)]
    c3 = [sweep(kind, V, N, 3, float(j)) for j in range(a.rot)]
    coefs = {3: [D.from_numpy(c) for c in c3], 2: [D.from_numpy(np.ascontiguousarray(c[:, :2])) for c in c3]}
    lag_rows = [(D.from_numpy(np.ascontiguousarray(c[:, 0])), D.from_numpy(np.ascontiguousarray(c[:, 1]))) for c in c3] if kind == "lag" else None
    dconst = D.from_numpy(np.ascontiguousarray(c3[0][0, :2]))
    del c3
    st = D((1 if kind == "lag" else 5, V))
    big = N >= 1 << 24
    r = {"kind": kind, "V": V, "N": N}

    for rows in a.rows:
        def swept_call(i, rows=rows):
            j = i % a.rot
            mx._lib.check(L.mxg_scan_long_render_swept(k, V, N, xs[j].ptr, coefs[rows][j].ptr, rows, st.ptr, outs[j].ptr, None), "mxg_scan_long_render_swept")

        us = timed(L, swept_call, a.warmup, a.reps)
        nbytes = (2 * 8 * (1 + rows) + 8) * V * N
        r["rows%d" % rows] = {"k31_us": us, "k31_launch_us": per_launch(L, swept_call, a.reps), "algorithmic_bytes": nbytes,
                              "frac_of_8TBs": round(nbytes / (us * 1e-6) / 8e12, 4)}

    def seq_call(i):
        j = i % a.rot
        if kind == "lag":
            rc = L.mxg_lag_render(V, N, xs[j].ptr, lag_rows[j][0].ptr, lag_rows[j][1].ptr, 1, st.ptr, outs[j].ptr, None)
        else:
            rc = L.mxg_filter_render_coefs(k - 3, V, N, xs[j].ptr, coefs[3][j].ptr, st.ptr, outs[j].ptr, None)
        mx._lib.check(rc, "sequential per-sample entry point")

    def const_call(i):
        j = i % a.rot
        mx._lib.check(L.mxg_scan_long_render(k, V, N, xs[j].ptr, dconst.ptr, st.ptr, outs[j].ptr, None), "mxg_scan_long_render")

    r["sequential_us"] = timed(L, seq_call, 1 if big else a.warmup, 2 if big else a.reps)
    r["k28_const_us"] = timed(L, const_call, a.warmup, a.reps)
    for rows in a.rows:
        e = r["rows%d" % rows]
        e["sequential_over_k31"] = round(r["sequential_us"] / e["k31_us"], 1)
        e["k31_over_k28_const"] = round(e["k31_us"] / r["k28_const_us"], 2)
    for b in xs + outs + coefs[2] + coefs[3] + [dconst, st] + ([t for p in lag_rows for t in p] if lag_rows else []):
        b.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rot", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="*", default=[2, 3])
    ap.add_argument("--kinds", nargs="*", default=list(KINDS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longsweep_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    runs = []
    for kind in a.kinds:
        for V, ln in SHAPES:
            runs.append(bench(L, kind, V, 1 << ln, a))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    res = {"chunk": TS, "reps": a.reps, "warmup": a.warmup, "rot": a.rot, "runs": runs}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
