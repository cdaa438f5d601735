#!/usr/bin/env python3
"""tools/bench_looper.py -- maxiLooperBank (kernel K25, csrc/looper.hip) at 1024 and 16 384 slots of 44 100 samples, 512 samples
per call: the overdub over the whole sample with and without the fused play head, a loop of 256 indices, a loop of one index, and
normalise -- beside yardsticks from the same run: the maxiDCBlocker bank at the same voice count and block (16 algorithmic bytes
per sample against the looper's 32 / 40), the library's host twin on the CPU (mxg_looprec_host, at 1024 slots), and, for scale,
what the drop-in maxiSample::loopRecord does per sample: one 8-byte host-to-device copy, timed over --dropin samples.

Device events around each call on the default stream, median of --reps calls after a warm-up; the input, enable and output blocks
AND the pools rotate through --rot sets, so no call finds its blocks or its slots in the caches from the call before.  The enable
is a block [N][R] (eps = 1), so its 8 bytes per sample are read.  Algorithmic bytes per slot-sample: 8 in + 8 enable + 8 read +
8 write, + 8 out with the play head; the fraction of 8 TB/s is taken on those.  A call of 512 samples is four launches (the
piece is mxg_looprec_piece() samples).  Prints one JSON line and writes it to --out.

    python tools/bench_looper.py [--reps 20] [--warmup 5] [--rot 2] [--out profiles/looper_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maximilian_amd as mx  # noqa: E402

LEN, N = 44100, 512
MODES = {  # name: (start, end, play)
    "overdub": (0.0, 1.0, "none"),
    "overdub_play": (0.0, 1.0, "playLoop"),
    "loop256": (0.25, 0.25 + 256.0 / LEN, "none"),
    "loop1": (0.5, 0.5, "none"),
}


def timed(L, f, a):
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    t = []
    for i in range(a.warmup + a.reps):
        L.mxg_event_record(e0, None)
        f(i)
        L.mxg_event_record(e1, None)
        L.mxg_event_sync(e1)
        L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
        if i >= a.warmup:
            t.append(ms.value * 1e3)
    L.mxg_event_destroy(e0)
    L.mxg_event_destroy(e1)
    return {"us": round(float(np.median(t)), 1), "min_us": round(float(np.min(t)), 1), "max_us": round(float(np.max(t)), 1)}


def bench(L, R, a):
    D = mx.DeviceBuffer
    rng = np.random.default_rng(25)
    banks = [mx.maxiLooperBank(R, LEN) for _ in range(a.rot)]
    for b in banks:
        b.trigger()
    xs = [D.from_numpy(rng.uniform(-1, 1, (N, R))) for _ in range(a.rot)]
    ens = [D.from_numpy(np.ones((N, R))) for _ in range(a.rot)]
    outs = [D((N, R), zero=False) for _ in range(a.rot)]
    res = {"slots": R}
    for name, (s, e, play) in MODES.items():
        for b in banks:
            b.setLoop(s, e)
            b.setPlayLoop(0.0, 1.0)

        def call(i, play=play):
            k = i % a.rot
            banks[k].loopRecord(xs[k], ens[k], N, play, outs[k] if play != "none" else None)
        r = timed(L, call, a)
        nbytes = R * N * (40 if play != "none" else 32)
        r["algorithmic_bytes"] = nbytes
        r["frac_of_8TBs"] = round(nbytes / (r["us"] * 1e-6) / 8e12, 4)
        res[name] = r
    lv = D.from_numpy(np.full(R, 0.99))

    def norm(i):
        b = banks[i % a.rot]
        mx._lib.check(L.mxg_sample_pool_normalise(R, b.pool, b.stride, b.cap, b.len.ptr, lv.ptr, None), "mxg_sample_pool_normalise")
    res["normalise"] = timed(L, norm, a)
    res["normalise"]["algorithmic_bytes"] = R * LEN * 24   # read, read, write
    res["normalise"]["frac_of_8TBs"] = round(R * LEN * 24 / (res["normalise"]["us"] * 1e-6) / 8e12, 4)
    coef, dcs = D.from_numpy(np.full(R, 0.995)), [D((3, R)) for _ in range(a.rot)]   # maxiDCBlockerBank.play without its per-call upload

    def dcb(i):
        k = i % a.rot
        mx._lib.check(L.mxg_filter2_render(0, R, N, xs[k].ptr, coef.ptr, dcs[k].ptr, outs[k].ptr, None), "mxg_filter2_render")
    res["dcblocker"] = timed(L, dcb, a)
    for k in MODES:
        res[k]["over_dcblocker"] = round(res[k]["us"] / res["dcblocker"]["us"], 2)
    assert not banks[0].dropped.numpy().any()
    for b in banks:
        b.free()
    return res


def host_twin(L, R, reps):
    """mxg_looprec_host on one CPU thread: the whole-sample overdub with the play head, the same block."""
    stride = L.mxg_sample_pool_stride(LEN)
    rng = np.random.default_rng(26)
    mem = np.zeros(R * stride)
    ln = np.full(R, LEN, np.uint64)
    x, en, out = rng.uniform(-1, 1, (N, R)), np.ones((N, R)), np.zeros((N, R))
    v = {k: np.zeros(R) for k in ("start", "recpos", "lag", "pstart", "pos")}
    one, mix = np.ones(R), np.full(R, 0.5)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        mx._lib.check(L.mxg_looprec_host(R, N, mem.ctypes.data + 32, stride, LEN, ln.ctypes.data, x.ctypes.data, en.ctypes.data, 1, mix.ctypes.data,
                                         v["start"].ctypes.data, one.ctypes.data, v["recpos"].ctypes.data, v["lag"].ctypes.data, 2,
                                         v["pstart"].ctypes.data, one.ctypes.data, v["pos"].ctypes.data, out.ctypes.data, None), "mxg_looprec_host")
        t.append((time.perf_counter() - t0) * 1e6)
    return {"slots": R, "us": round(float(np.median(t)), 1)}


def dropin_copies(L, count):
    """What the drop-in maxiSample::loopRecord moves per call: one element, host to device."""
    d = mx.DeviceBuffer(16)
    h = np.zeros(1)
    t0 = time.perf_counter()
    for _ in range(count):
        L.mxg_memcpy_h2d(d.ptr, h.ctypes.data, 8, None)
    return {"samples": count, "us_per_sample": round((time.perf_counter() - t0) * 1e6 / count, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=2)
    ap.add_argument("--dropin", type=int, default=4000)
    ap.add_argument("--slots", type=int, nargs="*", default=[1024, 16384])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "looper_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    res = {"len": LEN, "samples_per_call": N, "piece": L.mxg_looprec_piece(), "tile": L.mxg_looprec_tile(), "reps": a.reps, "rot": a.rot,
           "runs": [bench(L, R, a) for R in a.slots], "host_twin": host_twin(L, 1024, 5), "dropin_route": dropin_copies(L, a.dropin)}
    for r in res["runs"]:
        if r["slots"] == 1024:
            res["host_twin"]["over_gpu_overdub_play"] = round(res["host_twin"]["us"] / r["overdub_play"]["us"], 1)
    res["dropin_route"]["us_for_one_slot_512_samples"] = round(res["dropin_route"]["us_per_sample"] * N, 1)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
