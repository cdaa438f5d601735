#!/usr/bin/env python3
"""tools/bench_seq.py -- the fused sequencer (seq.hip, K15, mxg_seq_render) at 65 536 voices x 512 samples at 44 100 Hz in three
forms -- trigger only, trigger + value (maxiStep::pull), all three outputs -- with mxg_osc_render(MXG_OSC_PHASOR) and
mxg_envgen_render (per-voice triggers) on the same shape timed alternately in the same process as the yardsticks.  The
trigger-only form stores the same 8 B per sample as the phasor render and does a handful of compares more, so the phasor
render's time in the same run is what it is measured against ("ratio_to_phasor").  Device events, one pair per launch, median
of --reps blocks after a warm-up; the output blocks rotate through --rot sets so that no launch finds its block in the caches
from the launch before.  Prints one JSON line and writes it to --out: us per block, G samples/s, the algorithmic bytes per
sample and the fraction of 8 TB/s on them.

Algorithmic bytes per sample: 8 per output block (the internal clock reads nothing per sample); phasor 8; maxiEnvGen 16 (trigger
in, value out).

    python tools/bench_seq.py [--reps 20] [--warmup 5] [--rot 3] [--out profiles/seq_bench.json]
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

BYTES = {"seq_trig": 8, "seq_trig_val": 16, "seq_all": 24, "phasor": 8, "envgen": 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--voices", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    V, N = a.voices, 512
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    rng = np.random.default_rng(1)
    D = mx.DeviceBuffer
    outs = [[D((N, V), zero=False) for _ in range(3)] for _ in range(a.rot)]
    seq = mx.maxiSeqBank(V, times=[[3, 3, 2], [1], [4, 4, 4, 1, 1, 1, 1], [33, 991, 13, 153]],
                         values=[[40.0, 80.0, 170.0, 350.0, 900.0, 3888.0], [60.0, 62.0, 65.0]])
    seq.setPattern(rng.integers(0, 4, V))
    seq.setValueList(rng.integers(0, 2, V))
    seq.setStep(rng.choice([1.0, 2.0, -1.0], V))
    seq.setHold(rng.choice([100.0, 300.0, 1000.0], V))
    freq = D.from_numpy(rng.uniform(20.0, 400.0, V))  # a few triggers per voice and block, as a sequencer's clock has them
    osc = mx.maxiOscBank(V)
    env = mx.maxiEnvGenBank(V)
    env.setup([0, 1, 0.2, 0], [5, 4, 2], [1, 1, 1], False, True)
    # the envelope's trigger block: one render of the sequencer itself
    trig = seq.render(N, freq=freq)[0]

    def seq_call(i, t, x, g):
        o = outs[i % a.rot]
        return L.mxg_seq_render(V, N, freq.ptr, seq.clock.ptr, None, 0, seq.norm.ptr, seq.len.ptr, seq.host_norm.shape[0],
                                seq.host_norm.shape[1], seq.pattern.ptr, 1, seq.values.ptr, seq.vlen.ptr, seq.values_shape[0],
                                seq.values_shape[1], seq.value_list.ptr, seq.step.ptr, seq.hold.ptr, seq.dstate.ptr, seq.istate.ptr,
                                o[0].ptr if t else None, o[1].ptr if x else None, o[2].ptr if g else None, None)

    runs = {
        "seq_trig": lambda i: seq_call(i, True, False, False),
        "seq_trig_val": lambda i: seq_call(i, True, True, False),
        "seq_all": lambda i: seq_call(i, True, True, True),
        "phasor": lambda i: L.mxg_osc_render(2, V, N, freq.ptr, 0, None, None, osc.phase.ptr, osc.output.ptr, outs[i % a.rot][0].ptr, None),
        "envgen": lambda i: L.mxg_envgen_render(V, N, trig.ptr, 1, env.stages.ptr, env.host_stages.shape[0], 0, 1, env.dstate.ptr,
                                                env.istate.ptr, outs[i % a.rot][1].ptr, None),
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
    res = {"V": V, "N": N, "sample_rate": 44100, "reps": a.reps, "rot": a.rot}
    for k, t in tot.items():
        us = float(np.median(t))
        res[k] = {"us": round(us, 1), "min_us": round(float(np.min(t)), 1), "max_us": round(float(np.max(t)), 1),
                  "Gsamples_s": round(V * N / us / 1e3, 2), "bytes_per_sample": BYTES[k],
                  "frac_of_8TBs": round(BYTES[k] * V * N / us / 1e3 / 8000, 4)}
    for k in ("seq_trig", "seq_trig_val", "seq_all"):
        res[k]["ratio_to_phasor"] = round(res[k]["us"] / res["phasor"]["us"], 3)
        res[k]["ratio_to_envgen"] = round(res[k]["us"] / res["envgen"]["us"], 3)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
