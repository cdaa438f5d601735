#!/usr/bin/env python3
"""tools/bench_spectral_bank.py -- maxiFFTBank / maxiIFFTBank (kernel K29, csrc/spectral_bank.hip) at V = 1024 and 65 536 streams,
N = 512 samples per call, fftSize 1024 / hop 256 (2 frames and 2 consumption points per stream and call): magnitudes only, all four
outputs, and the inverse bank on direct rows -- beside two yardsticks from the same run, timed alternately with the bank:
  (a) the floor: mxg_fft_batch / mxg_ifft_batch over the same number of frames of an already-float contiguous signal (for the
      inverse: ONE stream of V * 2 spectra, the overlap-add of a single object) -- what the bank does plus nothing;
  (b) the route a user has today: torch transpose + cast of the [N][V] block, concatenated behind each stream's carried history,
      then mxg_fft_batch once per frame index f: base = the lines + f * hop, frame_stride = the line length, nframes = V, outputs
      offset by f * V rows -- the bank's 2 V frame-major rows in F = 2 launches, no frame transformed that is not wanted.
Device events around each call on the default stream, median of --reps calls after a warm-up; inputs and outputs rotate through
--rot sets.  The fraction of 8 TB/s is on ALGORITHMIC bytes: 8 N V in, 4 bins per row and output, the carried history once each way
(forward: 4 (fftSize - hop) V read and written; inverse: 4 fftSize V read and written, rows of 2 x 4 bins in, 8 N V out).
Expectation (written before the first run): a bank call costs yardstick (a) plus one pass over the input bytes at the rate the
device streams them.  `expected_us` holds that sum with the pass at 4 TB/s (what a read+write copy reaches here); `within_expectation`
says whether the bank met it.  Prints one JSON line and writes it to --out.

    python tools/bench_spectral_bank.py [--reps 20] [--warmup 5] [--rot 3] [--out profiles/spectral_bank_bench.json]
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

FS, HOP, BINS, N = 1024, 256, 512, 512
HIST = FS - HOP
F = N // HOP


def timed(L, runs, a, st):
    e0, e1 = L.mxg_event_create(), L.mxg_event_create()
    ms = ctypes.c_float()
    tot = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):  # alternating, one event pair per call
        for k, f in runs.items():
            L.mxg_event_record(e0, st)
            f(i)
            L.mxg_event_record(e1, st)
            L.mxg_event_sync(e1)
            L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            if i >= a.warmup:
                tot[k].append(ms.value * 1e3)
    return {k: round(float(np.median(t)), 1) for k, t in tot.items()}


def bench(L, V, a):
    import torch
    chk = mx._lib.check
    dev = torch.device("cuda")
    ts = torch.cuda.Stream()  # torch ops and library calls on ONE stream: the events bracket both
    st = ctypes.c_void_p(ts.cuda_stream)
    with torch.cuda.stream(ts):
        return bench_on(L, V, a, torch, dev, st)


def bench_on(L, V, a, torch, dev, st):
    chk = mx._lib.check
    g = torch.Generator(device=dev).manual_seed(29)
    xs = [torch.rand((N, V), dtype=torch.float64, device=dev, generator=g) * 2 - 1 for _ in range(a.rot)]
    rows = V * F
    outs = [[torch.empty((rows, BINS), dtype=torch.float32, device=dev) for _ in range(4)] for _ in range(a.rot)]
    fbank, fbank4 = mx.maxiFFTBank(V, FS, HOP, stream=st), mx.maxiFFTBank(V, FS, HOP, stream=st)
    plan = mx.maxiFFT(stream=st)
    plan.setup(FS, HOP, 0)
    flat = [torch.rand(rows * HOP + HIST, dtype=torch.float32, device=dev, generator=g) for _ in range(a.rot)]
    hist = torch.zeros((V, HIST), dtype=torch.float32, device=dev)

    def today(i, four):
        line = torch.cat([hist, xs[i % a.rot].t().to(torch.float32)], dim=1).contiguous()
        o = outs[i % a.rot]
        for f in range(F):  # frame f of every stream: one launch, frames a line apart
            at = [p(t) + 4 * f * V * BINS for t in o]
            chk(L.mxg_fft_batch(plan.plan, line.data_ptr() + 4 * f * HOP, HIST + N, V, at[0] if four else None, at[1] if four else None,
                                at[2], at[3] if four else None, st), "today")
        hist.copy_(line[:, N:])

    p = lambda t: t.data_ptr()  # noqa: E731
    runs = {
        "bank_mags": lambda i: chk(L.mxg_fft_bank_process(fbank.h, p(xs[i % a.rot]), N, 0, None, None, p(outs[i % a.rot][2]), None, st), "bank"),
        "floor_mags": lambda i: chk(L.mxg_fft_batch(plan.plan, p(flat[i % a.rot]), HOP, rows, None, None, p(outs[i % a.rot][2]), None, st), "floor"),
        "today_mags": lambda i: today(i, False),
        "bank_all4": lambda i: chk(L.mxg_fft_bank_process(fbank4.h, p(xs[i % a.rot]), N, 0, *[p(t) for t in outs[i % a.rot]], st), "bank4"),
        "floor_all4": lambda i: chk(L.mxg_fft_batch(plan.plan, p(flat[i % a.rot]), HOP, rows, *[p(t) for t in outs[i % a.rot]], st), "floor4"),
        "today_all4": lambda i: today(i, True),
    }
    # the inverse bank on direct rows; floor: one stream of V * F spectra
    ibank = mx.maxiIFFTBank(V, FS, HOP, stream=st)
    iplan = mx.maxiIFFT(stream=st)
    iplan.setup(FS, HOP, 0)
    mags = [torch.rand((rows, BINS), dtype=torch.float32, device=dev, generator=g) for _ in range(a.rot)]
    phs = [(torch.rand((rows, BINS), dtype=torch.float32, device=dev, generator=g) * 6.28 - 3.14) for _ in range(a.rot)]
    ys = [torch.empty((N, V), dtype=torch.float64, device=dev) for _ in range(a.rot)]
    sig = torch.empty(rows * HOP, dtype=torch.float32, device=dev)
    runs["ibank"] = lambda i: chk(L.mxg_ifft_bank_process(ibank.h, 0, 0, 0, p(mags[i % a.rot]), p(phs[i % a.rot]), F, N, p(ys[i % a.rot]), st), "ibank")
    runs["ifloor"] = lambda i: chk(L.mxg_ifft_batch(iplan.plan, p(mags[i % a.rot]), p(phs[i % a.rot]), rows, iplan.buffer.ptr, p(sig), None, st), "ifloor")
    torch.cuda.synchronize()
    us = timed(L, runs, a, st)
    torch.cuda.synchronize()
    res = {"V": V, "N": N, "frames_per_call": rows, "us": us}
    in_bytes = 8 * N * V
    alg = {"bank_mags": in_bytes + 4 * BINS * rows + 2 * 4 * HIST * V, "bank_all4": in_bytes + 4 * 4 * BINS * rows + 2 * 4 * HIST * V,
           "ibank": 2 * 4 * BINS * rows + 8 * N * V + 2 * 4 * FS * V}
    res["algorithmic_bytes"] = alg
    res["frac_of_8TBs"] = {k: round(b / (us[k] * 1e-6) / 8e12, 4) for k, b in alg.items()}
    pass_us = in_bytes / 4e12 * 1e6
    res["expected_us"] = {"bank_mags": round(us["floor_mags"] + pass_us, 1), "bank_all4": round(us["floor_all4"] + pass_us, 1),
                          "ibank": round(us["ifloor"] + pass_us, 1)}
    res["within_expectation"] = {k: bool(us[k] <= v) for k, v in res["expected_us"].items()}
    res["today_over_bank"] = {"mags": round(us["today_mags"] / us["bank_mags"], 2), "all4": round(us["today_all4"] / us["bank_all4"], 2)}
    for b in (fbank, fbank4, ibank):
        b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_bank_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    res = {"fftSize": FS, "hopSize": HOP, "N": N, "reps": a.reps, "rot": a.rot,
           "yardsticks": {"floor": "mxg_fft_batch / mxg_ifft_batch, float contiguous signal, same number of frames",
                          "today": "torch transpose + cast + cat(history), then mxg_fft_batch once per frame index (stride = line length)"},
           "runs": [bench(L, V, a) for V in (1024, 65536)]}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
