#!/usr/bin/env python3
"""tools/bench_convolve_bank.py -- maxiConvolveBank (kernel K24, csrc/convolve_bank.hip) at V = 64 and 1024 streams, fftsize 1024 /
hop 256, impulses of K = 8 and 43 frames (43 = a 1 s response at 44.1 kHz), nblocks = 1 and 8 per call, mode 1 -- beside its
yardstick, a loop over 64 maxiConvolve objects (mxg_convolve_play, the single-stream path) doing the same work as the V = 64 bank,
timed alternately with it in the same process.  Device events around each call on the default stream (for the loop: from before the
first object's call to after the last one's, so the launch gaps the loop cannot avoid are inside), median of --reps calls after a
warm-up; inputs, outputs AND banks rotate through --rot sets, so no call finds its input or its rings in the caches from the call
before.  A second pass with the library's per-kernel events (mxg_prof_enable) gives the multiply-accumulate kernel alone, with its
fraction of 8 TB/s on ALGORITHMIC bytes: per stream K - 1 + nblocks history rows read, nblocks rows written to the ring, nblocks + 1
rows of sums written and one pending row read, plus every impulse row once (a row = bins x (4 + 4) bytes).  Prints one JSON line
and writes it to --out; exit status 1 if a V = 64 bank call was not faster than the 64-object loop.

    python tools/bench_convolve_bank.py [--reps 20] [--warmup 5] [--rot 3] [--out profiles/convolve_bank_bench.json]
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

F, H, BINS = 1024, 256, 512
NIMP = 4  # impulses per bank, stream v on impulse v % 4


def impulses(K, rng):
    L = K * F - BINS  # + the reference's padding of one half frame = K whole frames
    return [rng.uniform(-1, 1, L) * np.exp(-np.arange(L) / (L / 5.0)) for _ in range(NIMP)]


def prof(L):
    got = {}
    label, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_size_t()
    for i in range(L.mxg_prof_count()):
        L.mxg_prof_read(i, ctypes.byref(label), ctypes.byref(ms), ctypes.byref(cnt))
        if cnt.value:
            got[label.value.decode()] = ms.value * 1e3 / cnt.value
    return got


def mac_bytes(V, K, nb):
    row = BINS * 8
    return V * ((K - 1 + nb) + nb + (nb + 1) + 1) * row + NIMP * K * row


def bench(L, V, K, nb, a, with_loop):
    D = mx.DeviceBuffer
    rng = np.random.default_rng(24 + K)
    imps = impulses(K, rng)
    banks = [mx.maxiConvolveBank(V, imps, [v % NIMP for v in range(V)], F, H) for _ in range(a.rot)]
    assert banks[0].frames == [K] * NIMP
    n = nb * F
    ins = [D.from_numpy(rng.uniform(-1, 1, (V, n)).astype(np.float32)) for _ in range(a.rot)]
    outs = [D((V, n), np.float32, zero=False) for _ in range(a.rot)]
    runs = {"bank": lambda i: mx._lib.check(L.mxg_convolve_bank_play(banks[i % a.rot].h, ins[i % a.rot].ptr, nb, outs[i % a.rot].ptr, 1, None), "bank")}
    if with_loop:
        objs = []
        for v in range(V):
            c = mx.maxiConvolve()
            c.setup(imps[v % NIMP], F, H)
            objs.append(c)
        step = n * 4

        def loop(i):
            src, dst = ins[i % a.rot].ptr, outs[i % a.rot].ptr
            for v, c in enumerate(objs):
                mx._lib.check(L.mxg_convolve_play(c.h, src + v * step, nb, dst + v * step, 1, None), "loop")
        runs["loop"] = loop
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    tot = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):  # alternating, one event pair per call
        for k, f in runs.items():
            L.mxg_event_record(e0, None)
            f(i)
            L.mxg_event_record(e1, None)
            L.mxg_event_sync(e1)
            L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            if i >= a.warmup:
                tot[k].append(ms.value * 1e3)
    res = {"V": V, "K": K, "nblocks": nb}
    for k, t in tot.items():
        res[k + "_us"] = round(float(np.median(t)), 1)
        res[k + "_min_us"] = round(float(np.min(t)), 1)
        res[k + "_max_us"] = round(float(np.max(t)), 1)
    res["bank_Msamples_s"] = round(V * n / res["bank_us"], 1)
    if with_loop:
        res["loop_over_bank"] = round(res["loop_us"] / res["bank_us"], 2)
        res["bank_faster_than_loop"] = bool(res["bank_us"] < res["loop_us"])
    # the kernels alone (the per-kernel events cost time of their own: a pass apart from the call timings)
    L.mxg_prof_enable(1)
    L.mxg_prof_reset()
    for i in range(a.reps):
        runs["bank"](i)
    mx._lib.check(L.mxg_sync(), "mxg_sync")
    p = prof(L)
    L.mxg_prof_enable(0)
    mac = p.get("conv_bank_mac_kernel")
    res["kernels_us"] = {k: round(v, 1) for k, v in p.items()}
    res["mac_us"] = round(mac, 1)
    res["mac_algorithmic_bytes"] = mac_bytes(V, K, nb)
    res["mac_frac_of_8TBs"] = round(mac_bytes(V, K, nb) / (mac * 1e-6) / 8e12, 4)
    for b in banks:
        b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convolve_bank_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    runs = [bench(L, V, K, nb, a, V == 64) for V in (64, 1024) for K in (8, 43) for nb in (1, 8)]
    res = {"fftsize": F, "hopsize": H, "impulses_per_bank": NIMP, "mode": 1, "reps": a.reps, "rot": a.rot, "yardstick": "64 x mxg_convolve_play",
           "runs": runs}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    sys.exit(0 if all(r.get("bank_faster_than_loop", True) for r in runs) else 1)


if __name__ == "__main__":
    main()
