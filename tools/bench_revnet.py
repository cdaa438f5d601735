#!/usr/bin/env python3
"""tools/bench_revnet.py -- the reverb network bank (revnet.hip, K30) at 65 536 and 1024 voices x 512 samples, configured as
maxiSatReverb (4 plain combs, allpasses 125 / 42 / 12) and as maxiFreeVerb::play(x) (8 low-pass combs, 4 allpasses), each timed
alternately in the same process with the factory bank of the same numbers (reverb.hip, K13: maxiSatReverbBank,
maxiFreeVerbBank.play(x)).  Device events, one pair per launch, median of --reps blocks after a warm-up; the input / output blocks
rotate through --rot sets so that no launch finds its block in the caches from the launch before.  Writes one JSON object to
--out (default profiles/revnet_bench.json) and prints it: us per block, G samples/s, the algorithmic bytes per sample, the
fraction of 8 TB/s on them, and K30's time over K13's.

Algorithmic bytes per sample are the same for both kernels: 16 per ring step (read + write) + 8 in + 8 out:
Sat 7 steps -> 128; FreeVerb play(x) 12 -> 208.  K30 reads 8 more bytes per voice and stage per call for each parameter.

    python tools/bench_revnet.py [--reps 20] [--warmup 5] [--rot 3] [--out FILE]
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

BYTES = {"sat": 128, "freeverb4": 208}
SAT = ([778, 901, 1011, 1123], [125, 42, 12], None, 0.85)
FV = ([1557, 1617, 1491, 1422, 1277, 1356, 1188, 1116], [225, 556, 441, 341], [1] * 8, 0.84)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "revnet_bench.json"))
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
        xs = [mx.DeviceBuffer.from_numpy(rng.uniform(-1, 1, (N, V))) for _ in range(a.rot)]
        outs = [mx.DeviceBuffer((N, V), zero=False) for _ in range(a.rot)]
        for form, (combs, aps, lowp, fb) in (("sat", SAT), ("freeverb4", FV)):
            k13 = (mx.maxiSatReverbBank if form == "sat" else mx.maxiFreeVerbBank)(V)
            k30 = mx.maxiReverbNetBank(V, combs, aps, lowp, fb, 0.2, 0.85)
            assert k30.ring_doubles == sum(k13.lengths[:len(k30.lengths)])
            lp = k13.lp.ptr if k13.lp is not None else None
            wc = k13.wc.ptr if k13.wc is not None else None
            cs, asz, lpf = k30._cs.ctypes.data, k30._as.ctypes.data, k30._lowp.ctypes.data
            runs = {  # the C entry points directly: the host time between the two events is the same few microseconds for both
                "k13": lambda i: L.mxg_reverb_render(k13.KIND, 0, V, N, xs[i % a.rot].ptr, None, None, 0, k13.rings.ptr, k13.idx.ptr, lp, wc,
                                                     outs[i % a.rot].ptr, None),
                "k30": lambda i: L.mxg_revnet_render(k30.ncombs, k30.nallpasses, cs, asz, lpf, V, N, xs[i % a.rot].ptr, k30.comb_fb.ptr,
                                                     k30.comb_cut.ptr, k30.ap_fb.ptr, k30.rings.ptr, k30.idx.ptr, k30.lp.ptr,
                                                     outs[i % a.rot].ptr, None)}
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
            for k, t in tot.items():
                us = float(np.median(t))
                res["V%d_%s_%s" % (V, form, k)] = {
                    "us": round(us, 1), "min_us": round(float(np.min(t)), 1), "Gsamples_s": round(V * N / us / 1e3, 2),
                    "bytes_per_sample": BYTES[form], "frac_of_8TBs": round(BYTES[form] * V * N / us / 1e3 / 8000, 4)}
            res["V%d_%s_k30_over_k13" % (V, form)] = round(res["V%d_%s_k30" % (V, form)]["us"] / res["V%d_%s_k13" % (V, form)]["us"], 3)
            for buf in (k13.rings, k13.idx, k13.lp, k13.wc, k30.rings, k30.idx, k30.lp, k30.comb_fb, k30.comb_cut, k30.ap_fb):
                if buf is not None:
                    buf.free()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
