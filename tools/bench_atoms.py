#!/usr/bin/env python3
"""tools/bench_atoms.py -- the K22 kernels (atoms.hip) at 1024 and 64 streams x 512 samples over a two-scale book (atoms of 256 and of
2048 samples) at three densities: about 8, 32 and 128 live atoms per output sample.  In front of every timed block each stream gets
nA atoms of 256 and nB of 2048 samples at random offsets inside the block (nA / 2 + 4 nB = the density; untimed: mxg_atoms_add), so
after the warm-up every block renders the same S * (256 nA + 2048 nB) atom-samples.  Timed, alternately in the same process:
  gabor / raw x block / sample   mxg_atoms_fill, K22a (atoms_due_kernel) and K22b (atoms_render_kernel) separately, from the library's
                                 per-kernel events (mxg_prof_*), one pair per launch;
  sinewave                       mxg_osc_render's sinewave at 65 536 voices x 512: one FP64 sine per sample, the yardstick;
  host16                         mxg_atoms_fill_host on 16 threads (a sixteenth of the streams each): OUR restatement of the
                                 arithmetic on the CPU, NOT the compiled reference.
Median of --reps blocks after --warmup; the output blocks rotate through --rot buffers so that no launch finds its block in the
caches from the launch before.  Prints one JSON line and writes it to --out: us per block, atom-samples per second, the ratio of
that rate to the sinewave's samples per second.

    python tools/bench_atoms.py [--reps 10] [--warmup 6] [--rot 3] [--out profiles/atoms_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maximilian_amd as mx  # noqa: E402

N = 512
DENSITIES = {8: (8, 1), 32: (32, 4), 128: (128, 16)}   # density -> (atoms of 256, atoms of 2048) per stream and block
POOL = 1 << 16


def block_adds(rng, S, nA, nB, kind):
    n = S * (nA + nB)
    stream = np.repeat(np.arange(S, dtype=np.int32), nA + nB)
    length = np.tile(np.array([256] * nA + [2048] * nB, np.uint32), S)
    offset = rng.integers(0, N, n).astype(np.uint32)
    par = np.stack([np.exp(rng.uniform(np.log(20.0), np.log(20000.0), n)), np.full(n, 44100.0), rng.uniform(0, 6.28, n), np.full(n, 0.01)], axis=1).astype(np.float32)
    raw_off = rng.integers(0, POOL - 2048, n).astype(np.uint32)
    return n, stream, np.full(n, kind, np.int32), length, offset, par, raw_off


def prof(L):
    got = {}
    label, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_size_t()
    for i in range(L.mxg_prof_count()):
        L.mxg_prof_read(i, ctypes.byref(label), ctypes.byref(ms), ctypes.byref(cnt))
        if cnt.value:
            got[label.value.decode()] = ms.value * 1e3 / cnt.value
    return got


def bench(L, S, density, a, sine_rate):
    nA, nB = DENSITIES[density]
    Q = 2 * nA + 6 * nB + 8
    rng = np.random.default_rng(22)
    pool = rng.uniform(-0.01, 0.01, POOL).astype(np.float32)
    outs = [mx.DeviceBuffer((S, N), np.float32) for _ in range(a.rot)]
    work = S * (256 * nA + 2048 * nB)
    res = {"S": S, "N": N, "density": density, "atom_samples_per_block": work, "Q": Q}
    for kname, kind in (("gabor", 0), ("raw", 1)):
        for oname, onset in (("block", 0), ("sample", 1)):
            bank = L.mxg_atoms_bank_create(S, Q, None, None, None, pool.ctypes.data, POOL)
            assert bank, L.mxg_last_error()
            due, render = [], []
            for i in range(a.warmup + a.reps):
                n, *arr = block_adds(rng, S, nA, nB, kind)
                mx._lib.check(L.mxg_atoms_add(bank, n, *[x.ctypes.data for x in arr]), "mxg_atoms_add")
                L.mxg_prof_reset()
                mx._lib.check(L.mxg_atoms_fill(bank, N, outs[i % a.rot].ptr, onset, 0, None), "mxg_atoms_fill")
                mx._lib.check(L.mxg_sync(), "mxg_sync")
                p = prof(L)
                if i >= a.warmup:
                    due.append(p["atoms_due_kernel"])
                    render.append(p["atoms_render_kernel"])
            L.mxg_atoms_bank_destroy(bank)
            r = float(np.median(render))
            res[kname + "/" + oname] = {"due_us": round(float(np.median(due)), 1), "render_us": round(r, 1), "render_min_us": round(float(np.min(render)), 1),
                                        "render_max_us": round(float(np.max(render)), 1), "G_atom_samples_s": round(work / r / 1e3, 2),
                                        "ratio_to_sinewave": round(work / r * 1e6 / sine_rate, 3)}
    # the CPU figure: our restatement (mxg_atoms_fill_host) on 16 threads, Gabor atoms, the reference's onsets
    T = 16
    per = S // T
    banks = [L.mxg_atoms_bank_create_host(per, Q, None, None, None, pool.ctypes.data, POOL) for _ in range(T)]
    bufs = [np.zeros((per, N), np.float32) for _ in range(T)]
    times = []
    import time
    with ThreadPoolExecutor(T) as ex:
        for i in range(a.warmup + 3):
            for b in banks:
                n, *arr = block_adds(rng, per, nA, nB, 0)
                mx._lib.check(L.mxg_atoms_add_host(b, n, *[x.ctypes.data for x in arr]), "mxg_atoms_add_host")
            t0 = time.perf_counter()
            list(ex.map(lambda k: L.mxg_atoms_fill_host(banks[k], N, bufs[k].ctypes.data, 0, 0), range(T)))
            if i >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e6)
    for b in banks:
        L.mxg_atoms_bank_destroy(b)
    us = float(np.median(times))
    res["host16"] = {"what": "mxg_atoms_fill_host, 16 threads: our restatement on the CPU, not the compiled reference", "us": round(us, 1),
                     "G_atom_samples_s": round(work / us / 1e3, 3)}
    return res


def sinewave(L, a):
    V = 65536
    e0, e1, ms = L.mxg_event_create(), L.mxg_event_create(), ctypes.c_float()
    rng = np.random.default_rng(21)
    outs = [mx.DeviceBuffer((N, V), zero=False) for _ in range(a.rot)]
    freq = mx.DeviceBuffer.from_numpy(np.exp(rng.uniform(np.log(20.0), np.log(8000.0), V)))
    osc = mx.maxiOscBank(V)
    t = []
    for i in range(a.warmup + a.reps):
        L.mxg_event_record(e0, None)
        mx._lib.check(L.mxg_osc_render(mx.OSC_WAVEFORMS["sinewave"], V, N, freq.ptr, 0, None, None, osc.phase.ptr, osc.output.ptr, outs[i % a.rot].ptr, None), "sinewave")
        L.mxg_event_record(e1, None)
        L.mxg_event_sync(e1)
        L.mxg_event_elapsed_ms(e0, e1, ctypes.byref(ms))
        if i >= a.warmup:
            t.append(ms.value * 1e3)
    for o in outs:
        o.free()
    us = float(np.median(t))
    return {"V": V, "N": N, "us": round(us, 1), "G_samples_s": round(V * N / us / 1e3, 2)}, V * N / us * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--streams", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--densities", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atoms_bench.json"))
    a = ap.parse_args()
    L = mx.lib()
    mx._lib.check(L.mxg_init(0), "mxg_init")
    mx.maxiSettings.setup(44100, 2, 1024)
    L.mxg_prof_enable(1)
    sw, rate = sinewave(L, a)
    res = {"sample_rate": 44100, "reps": a.reps, "rot": a.rot, "sinewave": sw, "runs": [bench(L, S, d, a, rate) for S in a.streams for d in a.densities]}
    sw2, _ = sinewave(L, a)
    res["sinewave_after"] = sw2
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
