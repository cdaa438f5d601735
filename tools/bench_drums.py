#!/usr/bin/env python3
"""tools/bench_drums.py -- the K21 kernels (drums.hip) at 65 536 and 1024 voices x 512 samples: each drum `plain` (the class's
default switches) and `full` (distortion, filter and limiter on), triggered by a per-voice trigger block with a trigger every 128
samples, and the clock; in the same run, timed alternately in the same process as the yardsticks, mxg_osc_render's sinewave,
triangle and sinebuf (the drums' oscillators alone, the same write-only 8 B per sample stream) and the fused saw -> lores -> adsr
voice of config 3 (mxg_voice_render mode 0).  Device events, one pair per launch, median of --reps blocks after a warm-up; the
output blocks rotate through --rot buffers so that no launch finds its block in the caches from the launch before.  Prints one
JSON line and writes it to --out: us per block, G samples/s, and each drum's ratio to its oscillator and to the fused voice.

    python tools/bench_drums.py [--reps 20] [--warmup 5] [--rot 3] [--out profiles/drums_bench.json]
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

OSC_OF = {"kick": "sinewave", "snare": "triangle", "hats": "sinebuf"}


def bench(L, V, N, a):
    D = mx.DeviceBuffer
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    rng = np.random.default_rng(21)
    outs = [D((N, V), zero=False) for _ in range(a.rot)]
    trig_h = np.zeros((N, V))
    trig_h[(np.arange(N)[:, None] + rng.integers(0, 128, V)[None, :]) % 128 == 0] = 1.0
    trig = D.from_numpy(trig_h)
    itrig = D.from_numpy(trig_h.astype(np.int32))
    draws = D.from_numpy(rng.integers(0, 2 ** 31 - 1, (N, V)).astype(np.int32))
    freq = D.from_numpy(np.exp(rng.uniform(np.log(20.0), np.log(8000.0), V)))
    osc = mx.maxiOscBank(V)
    runs = {}
    for kind, cls in (("kick", mx.maxiKickBank), ("snare", mx.maxiSnareBank), ("hats", mx.maxiHatsBank)):
        for variant in ("plain", "full"):
            b = cls(V)
            b.setRelease(20), b.setCutoff(2000.0), b.setResonance(2.0), b.setDistortion(2.0)
            if variant == "full":
                b.useDistortion = b.useFilter = b.useLimiter = True
            rand = None if kind == "kick" else draws
            runs[kind + "/" + variant] = (lambda b, rand: lambda i: b.render(N, trig=trig, rand=rand, out=outs[i % a.rot]) and 0)(b, rand)
    clock = mx.maxiClockBank(V)
    clock.setTicksPerBeat(4), clock.setTempo(9000)
    runs["clock"] = lambda i: clock.render(N, out=outs[i % a.rot]) and 0
    for wf in ("sinewave", "triangle", "sinebuf"):
        runs[wf] = (lambda wf: lambda i: L.mxg_osc_render(mx.OSC_WAVEFORMS[wf], V, N, freq.ptr, 0, None, None, osc.phase.ptr, osc.output.ptr,
                                                          outs[i % a.rot].ptr, None))(wf)
    voice = mx.maxiVoiceBank(V)
    voice.env.setAttack(0), voice.env.setDecay(20), voice.env.setSustain(0.1), voice.env.setRelease(20)
    cut, res = np.full(V, 2000.0), np.full(V, 2.0)
    dpar, dhold = voice.env._params()
    coef, dcu, drs = D.from_numpy(mx.banks.filter_coeffs(0, cut, res)), D.from_numpy(cut), D.from_numpy(res)
    runs["voice3"] = lambda i: L.mxg_voice_render(0, V, N, freq.ptr, dcu.ptr, drs.ptr, coef.ptr, itrig.ptr, 1, dpar.ptr, dhold.ptr,
                                                  voice.osc_state.ptr, voice.flt_state.ptr, voice.env.dstate.ptr, voice.env.istate.ptr,
                                                  outs[i % a.rot].ptr, None)
    tot = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):  # alternating, one event pair per launch
        for k, f in runs.items():
            L.mxg_event_record(e0, None)
            mx._lib.check(f(i) or 0, k)
            L.mxg_event_record(e1, None)
            L.mxg_event_sync(e1)
            L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            if i >= a.warmup:
                tot[k].append(ms.value * 1e3)
    res_ = {"V": V, "N": N}
    for k, x in tot.items():
        us = float(np.median(x))
        res_[k] = {"us": round(us, 1), "min_us": round(float(np.min(x)), 1), "max_us": round(float(np.max(x)), 1),
                   "Gsamples_s": round(V * N / us / 1e3, 2)}
    for k in list(runs):
        if "/" in k:
            res_[k]["ratio_to_" + OSC_OF[k.split("/")[0]]] = round(res_[k]["us"] / res_[OSC_OF[k.split("/")[0]]]["us"], 3)
            res_[k]["ratio_to_voice3"] = round(res_[k]["us"] / res_["voice3"]["us"], 3)
    return res_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--voices", type=int, nargs="+", default=[65536, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drums_bench.json"))
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
