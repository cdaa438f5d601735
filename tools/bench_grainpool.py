#!/usr/bin/env python3
"""tools/bench_grainpool.py -- K27 (mxg_granular_pool_render) at a bank-sized shape: S streams that each stretch their OWN slot of
a pool of R slots of one second, T samples a call, both forms of the kernel (knob grain_pool_tiles 1 = the walk, 2 = the tile form),
and beside them mxg_granular_render -- existing code: the yardstick -- with the same S, T and mode over ONE shared sample of the
same length.  Times are HIP events around one call on the library's stream (mxg_event_*), after warm-up calls of the same shape,
the three variants alternating inside every round; the median over the rounds is reported, with the spread.  The three outputs are
not comparable bit for bit (K27's streams read different slots); the K27 forms are compared with each other.

    python tools/bench_grainpool.py [--streams 4096] [--slots 4096] [--steps 512] [--runs 25] [--neg-fraction 0.5] [--json FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import maximilian_amd as mx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of a slot")
    ap.add_argument("--mode", type=int, default=1, help="1 = maxiStretch::play (default), 0 = maxiTimeStretch::play, 3 = maxiPitchShift::play")
    ap.add_argument("--grain", type=float, default=0.05)
    ap.add_argument("--overlaps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--neg-fraction", type=float, default=0.0, help="share of the streams whose pitch (the grains' step) is negative")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L, D = mx.lib(), mx.DeviceBuffer
    mx._lib.check(L.mxg_init(-1), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    S, R, T, n = a.streams, a.slots, a.steps, int(a.seconds * 44100)
    rng = np.random.default_rng(27)
    # the pool: every slot the same second of noise rotated by its index (the content does not matter to the time; the addresses do)
    base = rng.uniform(-1, 1, n)
    stride = ctypes.c_size_t(0)
    pool = L.mxg_sample_pool_alloc(R, n, ctypes.byref(stride))
    assert pool, L.mxg_last_error().decode()
    for r in range(R):
        row = np.roll(base, 17 * r)
        mx._lib.check(L.mxg_memcpy_h2d(pool + 8 * stride.value * r, row.ctypes.data, row.nbytes, None), "h2d")
    dlen = D.from_numpy(np.full(R, n, np.uint64))
    slot = D.from_numpy((np.arange(S) % R).astype(np.uint32))
    loop = D.from_numpy(np.stack([np.full(S, n // 4, np.uint64), np.full(S, n // 2, np.uint64)]))
    sb = mx.maxiSampleBank(1)
    sb.setSample(base)
    sign = np.where(np.arange(S) < a.neg_fraction * S, -1.0, 1.0)   # (whole wavefronts of one sign first)
    pitch, rate = D.from_numpy(rng.uniform(0.5, 1.5, S) * sign), D.from_numpy(rng.uniform(0.5, 1.5, S))
    plan = L.mxg_grain_plan_create(0, a.grain, 44100)
    state = {k: (D((4, S)), D((4, 8, S)), D((T, S))) for k in ("walk", "tiles", "shared")}
    b = rate.ptr if a.mode == 1 else None

    def call(kind):
        st, gst, out = state[kind]
        if kind == "shared":
            rc = L.mxg_granular_render(plan, a.mode, S, T, sb.d_samples, n, a.overlaps, pitch.ptr, b, None, None, 0, st.ptr, gst.ptr, out.ptr, None)
        else:
            L.mxg_tune(b"grain_pool_tiles", 1 if kind == "walk" else 2)
            rc = L.mxg_granular_pool_render(plan, a.mode, S, T, pool, stride.value, n, R, dlen.ptr, slot.ptr, loop.ptr if a.mode == 1 else None,
                                            a.overlaps, pitch.ptr, b, None, 0, None, 0, st.ptr, gst.ptr, out.ptr, None)
        mx._lib.check(rc, kind)

    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    times = {k: [] for k in state}
    for i in range(a.warmup + a.runs):
        for kind in ("walk", "tiles", "shared"):
            L.mxg_event_record(e0, None)
            call(kind)
            L.mxg_event_record(e1, None)
            L.mxg_event_sync(e1)
            ms = ctypes.c_float(0)
            mx._lib.check(L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed")
            if i >= a.warmup:
                times[kind].append(ms.value)
    L.mxg_tune(b"grain_pool_tiles", 0)
    assert L.mxg_last_async_error() == 0, L.mxg_last_error().decode()
    # the two forms of K27 ran the same calls from the same state: the same bits
    same = all((state["walk"][i].numpy().view(np.uint64) == state["tiles"][i].numpy().view(np.uint64)).all() for i in range(3))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"kernel": "K27 mxg_granular_pool_render", "streams": S, "slots": R, "slot_samples": n, "steps": T, "mode": a.mode, "grain": a.grain,
           "overlaps": a.overlaps, "neg_fraction": a.neg_fraction, "runs": a.runs, "ms_median": med, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
           "ms_max": {k: float(np.max(v)) for k, v in times.items()}, "tiles_over_walk": med["tiles"] / med["walk"],
           "pool_best_over_shared": min(med["walk"], med["tiles"]) / med["shared"], "forms_same_bits": bool(same),
           "stream_samples_per_s_best": S * T / (min(med["walk"], med["tiles"]) * 1e-3)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    L.mxg_grain_plan_destroy(plan)
    L.mxg_sample_pool_free(pool)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
