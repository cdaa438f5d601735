#!/usr/bin/env python3
"""tools/gen/gen_golden_analysis.py -- TEST INFRASTRUCTURE.  Writes tests/golden/analysis.npz: outputs and states of the
UNMODIFIED reference's maxiZeroCrossingDetector / maxiZeroCrossingRate / maxiEnvelopeFollower / maxiSampleAndHold for the
cases below, the streams of tests/patches/analysis_patch.cpp and analysis_host_patch.cpp, and the stream and the stdout bytes
of the reference's example 22.Analysis, compiled verbatim from its own location.

It compiles tools/gen/analysis_ref_dump.cpp with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling
checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary directory outside the tree,
and records the compiler, flags, libc and the sha256 of the reference sources inside the file.  Nothing else in the tree changes.

Cases ("<case>/..."): V voices x 4000 samples at a sample rate of 1000 (a ring of 1000 slots: not a multiple of 64), played in
blocks cut at uneven positions (lengths 1 and 7 among them), every state array of include/maxigpu.h stored at every cut
("<case>/snap<i>/..."; the ring as packed bits, slot-major as numpy.packbits(axis=0, bitorder='little') leaves them).  Signals
are int16 q (the signal is q / 32768.0) with a list of patched samples (n, v, value): exact 0.0, -0.0, runs of zeros, one NaN,
and crossings placed on block edges and on the ring's wrap.  "a": hold times per voice; "b": a hold time per sample.

The generator ASSERTS on the reference's own output that every voice's rate takes at least 3 distinct values and both rises and
falls, that a crossing falls on the first sample of a block, on the last one and on the slot where the ring wraps, that every
follower voice takes both branches and that every sample-and-hold voice with a hold of at least one sample resamples at least
3 times: a test can then not pass on rows of zeros.

    python tools/gen/gen_golden_analysis.py [--ref DIR]
"""
import argparse
import ctypes
import hashlib
import os
import platform
import re
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(ROOT, "tests", "golden", "analysis.npz")
N = 4000
SR = 1000
PATCH_FRAMES = 6000
EX22_FRAMES = 7000
P = ctypes.c_void_p
CUTS = [0, 1, 8, 143, 999, 1000, 1429, 2500, 3999, N]
WINDOWS = [1000, 999, 64, 37, 500, 65]
HOLDS = [0.0, 1.0, 2.5, 37.0, 300.0, 2.5]
ATTACK_MS = [5.0, 10.0, 2.0, 50.0, 1.5, 100.0]
RELEASE_MS = [50.0, 20.0, 300.0, 50.0, 15.0, 100.0]


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def signals(V):
    """Chirps 40 -> 120 -> 15 Hz (the rate over a long window rises, then falls) under a slow tremolo, with a little noise."""
    rng = np.random.default_rng(1600)
    n = np.arange(N)[:, None]
    v = np.arange(V)[None, :]
    f = np.where(n < 1500, 40.0 + 80.0 * n / 1500.0, 120.0 - 105.0 * (n - 1500) / 2500.0) * (1.0 + 0.07 * v)
    ph = np.cumsum(f / SR, axis=0)
    amp = 0.55 + 0.4 * np.sin(2 * np.pi * n * (1.3 + 0.2 * v) / SR)
    x = np.sin(2 * np.pi * ph) * amp + 0.02 * rng.standard_normal((N, V))
    return np.round(np.clip(x, -0.999, 0.999) * 32767).astype(np.int16)


# (n, v, value): voice 0 carries the edges, voice 1 the special values.  Every value is exact in float32.
PATCHES = [(7, 0, -0.25), (8, 0, 0.25),            # a crossing on the first sample of block [8, 143)
           (141, 0, -0.25), (142, 0, 0.25),        # ... on the last sample of it
           (998, 0, -0.25), (999, 0, 0.25),        # ... on slot cap - 1: the push that wraps the ring (and a block of one sample)
           (1999, 0, -0.25), (2000, 0, 0.25)]      # ... on slot 0 after the wrap
PATCHES += [(n, 1, 0.0) for n in range(300, 320)] + [(320, 1, 0.5)]          # a run of exact zeros, then a crossing from 0.0
PATCHES += [(400, 1, -0.0), (401, 1, 0.375)]                                  # a crossing from -0.0
PATCHES += [(3500, 1, float("nan")), (3501, 1, 0.5), (3502, 1, -0.125), (3503, 1, 0.25)]  # NaN never crosses, nor lets 3501 cross


def patched(q):
    x = q / 32768.0
    for n, v, val in PATCHES:
        x[n, v] = val
    return np.ascontiguousarray(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "maximilian.h")]
    ex22 = os.path.join(args.ref, "cpp", "commandline", "maximilian_examples", "22.Analysis", "main.cpp")
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    out = {}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libanaref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "analysis_ref_dump.cpp"), ref_sources[0], "-lm"])
        R = ctypes.CDLL(so)
        R.ana_new.restype = P
        R.ana_new.argtypes = [ctypes.c_size_t]
        R.ana_free.argtypes = [P]
        R.ana_set_rate.argtypes = [ctypes.c_int]
        R.ana_set_follow.argtypes = [P] * 4
        R.ana_play.argtypes = [P, ctypes.c_size_t, P, P, P, ctypes.c_int] + [P] * 4
        R.ana_cap.restype = ctypes.c_size_t
        R.ana_cap.argtypes = [P]
        R.ana_state.argtypes = [P] * 6
        R.ana_set_rate(SR)
        V = len(WINDOWS)
        q = signals(V)
        x = patched(q)
        out["q"] = q
        out["patches"] = np.array(PATCHES, np.float64)
        rng = np.random.default_rng(1601)
        for name in ("a", "b"):
            window = np.array(WINDOWS, np.uint32)
            ams, rms = np.array(ATTACK_MS), np.array(RELEASE_MS)
            if name == "a":
                hold = np.array(HOLDS)
            else:  # a hold time per sample: each voice moves among the five times every 50 .. 400 samples
                hold = np.zeros((N, V))
                for v in range(V):
                    n = 0
                    while n < N:
                        m = int(rng.integers(50, 400))
                        hold[n:n + m, v] = [0.0, 1.0, 2.5, 37.0, 300.0][int(rng.integers(1, 5)) if v else 2]
                        n += m
                hold[2000:2200, 3] = 0.0
            h = R.ana_new(V)
            cap = R.ana_cap(h)
            assert cap == SR
            coef = np.zeros((2, V))
            R.ana_set_follow(h, ams.ctypes.data, rms.ctypes.data, coef.ctypes.data)
            rec = {"sr": np.int64(SR), "cap": np.int64(cap), "window": window, "hold": hold, "attack_ms": ams, "release_ms": rms,
                   "attack": coef[0].copy(), "release": coef[1].copy(), "cuts": np.array(CUTS, np.int64)}
            zx, zcr, env, sah = (np.zeros((N, V)) for _ in range(4))
            for i, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
                xb = np.ascontiguousarray(x[a:b])
                hb = hold if name == "a" else np.ascontiguousarray(hold[a:b])
                o = [np.zeros((b - a, V)) for _ in range(4)]
                R.ana_play(h, b - a, xb.ctypes.data, window.ctypes.data, hb.ctypes.data, 0 if name == "a" else 1, *[t.ctypes.data for t in o])
                zx[a:b], zcr[a:b], env[a:b], sah[a:b] = o
                prev, ring = np.zeros((2, V)), np.zeros((cap, V), np.uint8)
                pos, cnt, dst = np.zeros(V, np.int32), np.zeros(V, np.int64), np.zeros((3, V))
                R.ana_state(h, prev.ctypes.data, ring.ctypes.data, pos.ctypes.data, cnt.ctypes.data, dst.ctypes.data)
                assert np.array_equal(prev[0].view(np.uint64), prev[1].view(np.uint64))  # the rate's own detector saw the same samples
                assert (cnt >= 0).all()
                rec["snap%d/prev_x" % i] = prev[0].copy()
                rec["snap%d/ring" % i] = np.packbits(ring, axis=0, bitorder="little")
                rec["snap%d/pos" % i], rec["snap%d/count" % i], rec["snap%d/dst" % i] = pos, cnt, dst
            R.ana_free(h)
            # ---- what the file must hold for a test to mean something --------------------------------------------------------
            assert set(np.unique(zx)) <= {0.0, 1.0} and (zcr == np.round(zcr)).all() and zcr.min() >= 0 and zcr.max() < 65535
            d = np.diff(zcr, axis=0)
            assert all(len(np.unique(zcr[:, v])) >= 3 for v in range(V)) and ((d > 0).any(axis=0) & (d < 0).any(axis=0)).all(), name
            inner = CUTS[1:-1]
            assert zx[inner].any() and zx[[c - 1 for c in inner]].any(), "no crossing on the first / last sample of a block"
            assert zx[cap - 1::cap].any() and zx[cap::cap].any(), "no crossing where the ring wraps"
            assert zx[8, 0] == 1 and zx[142, 0] == 1 and zx[999, 0] == 1 and zx[2000, 0] == 1 and zx[320, 1] == 1 and zx[401, 1] == 1
            assert zx[3500, 1] == 0 and zx[3501, 1] == 0 and zx[3503, 1] == 1
            a = np.abs(x)
            envprev = np.vstack([np.zeros((1, V)), env[:-1]])
            att = a > envprev
            fin = np.isfinite(a) & np.isfinite(envprev)
            assert (att & fin).any(axis=0).all() and (~att & fin).any(axis=0).all(), "a follower voice misses a branch"
            hs = np.trunc(np.broadcast_to(hold, (N, V)) / 1000.0 * SR)
            changes = (np.diff(sah.view(np.uint64).astype(np.int64), axis=0) != 0).sum(axis=0)
            assert (changes[(hs >= 1).all(axis=0)] >= 3).all(), changes
            assert np.array_equal(sah.astype(np.float32).astype(np.float64).view(np.uint64), sah.view(np.uint64)) or \
                np.array_equal(np.isnan(sah.astype(np.float32)), np.isnan(sah))
            ok = ~np.isnan(sah)
            assert np.array_equal(sah.astype(np.float32).astype(np.float64)[ok], sah[ok])
            rec.update(zx=zx.astype(np.uint8), zcr=zcr.astype(np.uint16), sah=sah.astype(np.float32))
            if name == "a":
                rec["env"] = env
            else:  # the follower does not depend on the hold times: "b" stores a digest, "a" the stream
                assert np.array_equal(env.view(np.uint64), out["a/env"].view(np.uint64))
            print("%s: crossings per voice %s  rate max %s  resamples %s" % (name, zx.sum(axis=0).astype(int), zcr.max(axis=0).astype(int), changes))
            for k, arr in rec.items():
                out[name + "/" + k] = arr
        R.ana_set_rate(44100)

        # ---- the patches' streams: tests/patches/*.cpp + oracle/example_host.cpp (read only) + the reference; 22.Analysis verbatim ----
        for key, patch, frames in (("patch", os.path.join(ROOT, "tests", "patches", "analysis_patch.cpp"), PATCH_FRAMES),
                                   ("host_patch", os.path.join(ROOT, "tests", "patches", "analysis_host_patch.cpp"), PATCH_FRAMES),
                                   ("ex22", ex22, EX22_FRAMES)):
            exe = os.path.join(td, key)
            subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-o", exe,
                                   os.path.join(ROOT, "oracle", "example_host.cpp"), patch, ref_sources[0], "-lm", "-lpthread"])
            raw = os.path.join(td, key + ".f64")
            r = subprocess.run([exe, str(frames), raw], check=True, cwd=td, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
            s = np.fromfile(raw, np.float64).reshape(frames, 2)
            assert np.isfinite(s).all() and (s[:, 0] != 0).mean() > 0.5 and (s[:, 1] != 0).mean() > 0.3, key
            if key == "ex22":
                assert np.array_equal(s[:, 0], s[:, 1])
                out[key] = s[:, 0].copy()
            else:
                out[key] = s
            if key != "host_patch":
                assert r.stdout.count(b"zcr: ") >= 3, r.stdout
                out[key + "_stdout"] = np.frombuffer(r.stdout, np.uint8)
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    out["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; "
        "harness: tools/gen/analysis_ref_dump.cpp; patches: tests/patches/analysis_patch.cpp, analysis_host_patch.cpp and the reference's "
        "22.Analysis/main.cpp via oracle/example_host.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    out["cases"] = np.array(["a", "b"])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "seq.npz"))


if __name__ == "__main__":
    main()
