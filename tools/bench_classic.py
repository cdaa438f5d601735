#!/usr/bin/env python3
"""tools/bench_classic.py -- the K23 kernels (classic.hip) at 65 536 and 1024 voices x 512 samples: the gate, the compressor, the
envelope's line (without and with a trigger block), the lag, and the maps linlin / linexp / explin -- each beside its yardstick,
timed alternately in the same process: the maxiDCBlocker form of mxg_filter2_render (8 B in + 8 B out per sample) for the gate,
the compressor and the lag; maxiOsc::saw (8 B out) for the line; hardclip (the flat 16 B stream) for the maps.  The design
expectation, not a bar: the three 16-byte state machines sit with the DC blocker, linlin with hardclip, linexp and explin are
VALU-bound like asymclip.  Device events, one pair per launch, median of --reps blocks after a warm-up; the blocks rotate through
--rot sets so that no launch finds its blocks in the caches from the launch before.  Prints one JSON line and writes it to
--out: us per block, G samples/s, the algorithmic bytes per sample, the fraction of 8 TB/s on them and the ratio to the
yardstick ("ratio", and per byte "ratio_per_byte").

    python tools/bench_classic.py [--reps 20] [--warmup 5] [--rot 3] [--out profiles/classic_bench.json]
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

BYTES = {"gate": 16, "compressor": 16, "lag": 16, "dcblock": 16, "line": 8, "line_trig": 16, "saw": 8, "linlin": 16, "linexp": 16, "explin": 16,
         "hardclip": 16}
YARDSTICK = {"gate": "dcblock", "compressor": "dcblock", "lag": "dcblock", "line": "saw", "line_trig": "saw", "linlin": "hardclip",
             "linexp": "hardclip", "explin": "hardclip"}


def bench(L, V, N, a):
    D = mx.DeviceBuffer
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    rng = np.random.default_rng(23)
    n = np.arange(N)[:, None]
    bursts = np.where((n % 128) < 48, 1.3, 0.2) * rng.uniform(-1.0, 1.0, (N, V))   # passes the thresholds in every period
    ins = [D.from_numpy(bursts * s) for s in np.linspace(1.0, 0.9, a.rot)]
    trig = [D.from_numpy((rng.uniform(0, 1, (N, V)) < 0.01).astype(np.float64)) for _ in range(a.rot)]
    outs = [D((N, V), zero=False) for _ in range(a.rot)]
    par = {k: D.from_numpy(rng.uniform(lo, hi, V)) for k, (lo, hi) in dict(thr=(0.3, 0.7), att=(0.1, 0.9), rel=(0.99, 0.9999), ratio=(2.5, 8.0),
                                                                               alpha=(0.01, 0.5)).items()}
    makeup = D.from_numpy(mx.dyn_makeup(par["ratio"].numpy()))
    recip = D.from_numpy(1.0 - par["alpha"].numpy())
    hold = D.from_numpy(rng.integers(0, 64, V).astype(np.int64))
    gate, comp = mx.maxiDynBank(V), mx.maxiDynBank(V)
    k = 44100 * 0.0011
    env = mx.maxiEnvelopeBank(V, [1.0, 100 / k, 0.25, 150 / k, 0.75, 60 / k, 0.0, 120 / k])
    env.trigger(0, 0.0)
    lagv = D(V)
    rng4 = np.stack([rng.uniform(0.05, 0.3, V), rng.uniform(0.6, 1.2, V), rng.uniform(20.0, 100.0, V), rng.uniform(1000.0, 8000.0, V)])
    d_range = D.from_numpy(rng4)
    aux = np.zeros(V)
    mx._lib.check(L.mxg_map_range_host(mx.MAP_MODES["explin"], V, rng4.ctypes.data, aux.ctypes.data), "mxg_map_range_host")
    d_aux = D.from_numpy(aux)
    dcb = mx.maxiDCBlockerBank(V)
    dcb.coef = D.from_numpy(np.full(V, 0.995))
    osc = mx.maxiOscBank(V)
    freq = D.from_numpy(rng.uniform(50.0, 2000.0, V))

    def mapper(mode):
        return lambda i: L.mxg_map_render(mx.MAP_MODES[mode], V, N, ins[i % a.rot].ptr, d_range.ptr, d_aux.ptr, outs[i % a.rot].ptr, None)

    def line(i, tb):
        return L.mxg_envelope_line_render(V, N, env.S, env.segments.ptr, env.count.ptr, trig[i % a.rot].ptr if tb else None, env.trig_index.ptr,
                                          env.trig_amp.ptr, env.dst.ptr, env.ist.ptr, outs[i % a.rot].ptr, None)

    runs = {
        "gate": lambda i: L.mxg_dyn_gate_render(V, N, ins[i % a.rot].ptr, par["thr"].ptr, par["att"].ptr, par["rel"].ptr, 0, hold.ptr, gate.dst.ptr,
                                                gate.ist.ptr, outs[i % a.rot].ptr, None),
        "compressor": lambda i: L.mxg_dyn_compress_render(V, N, ins[i % a.rot].ptr, par["ratio"].ptr, makeup.ptr, par["thr"].ptr, par["att"].ptr,
                                                          par["rel"].ptr, 0, comp.dst.ptr, comp.ist.ptr, outs[i % a.rot].ptr, None),
        "lag": lambda i: L.mxg_lag_render(V, N, ins[i % a.rot].ptr, par["alpha"].ptr, recip.ptr, 0, lagv.ptr, outs[i % a.rot].ptr, None),
        "dcblock": lambda i: L.mxg_filter2_render(0, V, N, ins[i % a.rot].ptr, dcb.coef.ptr, dcb.state.ptr, outs[i % a.rot].ptr, None),
        "line": lambda i: line(i, False),
        "line_trig": lambda i: line(i, True),
        "saw": lambda i: L.mxg_osc_render(mx.OSC_WAVEFORMS["saw"], V, N, freq.ptr, 0, None, None, osc.phase.ptr, osc.output.ptr, outs[i % a.rot].ptr, None),
        "linlin": mapper("linlin"), "linexp": mapper("linexp"), "explin": mapper("explin"),
        "hardclip": lambda i: L.mxg_shape_render(mx.SHAPE_MODES["hardclip"], V, N, ins[i % a.rot].ptr, None, None, 0, outs[i % a.rot].ptr, None),
    }
    tot = {k_: [] for k_ in runs}
    for i in range(a.warmup + a.reps):  # alternating, one event pair per launch
        for k_, f in runs.items():
            L.mxg_event_record(e0, None)
            mx._lib.check(f(i), k_)
            L.mxg_event_record(e1, None)
            L.mxg_event_sync(e1)
            L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            if i >= a.warmup:
                tot[k_].append(ms.value * 1e3)
    res = {"V": V, "N": N}
    for k_, t in tot.items():
        us = float(np.median(t))
        res[k_] = {"us": round(us, 1), "min_us": round(float(np.min(t)), 1), "max_us": round(float(np.max(t)), 1),
                   "Gsamples_s": round(V * N / us / 1e3, 2), "bytes_per_sample": BYTES[k_],
                   "frac_of_8TBs": round(BYTES[k_] * V * N / us / 1e3 / 8000, 4)}
    for k_, y in YARDSTICK.items():
        res[k_]["yardstick"] = y
        res[k_]["ratio"] = round(res[k_]["us"] / res[y]["us"], 3)
        res[k_]["ratio_per_byte"] = round(res[k_]["us"] / res[y]["us"] * BYTES[y] / BYTES[k_], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--voices", type=int, nargs="+", default=[65536, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classic_bench.json"))
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
