#!/usr/bin/env python3
"""tools/gen/gen_golden_dyn.py -- TEST INFRASTRUCTURE.  Writes tests/golden/dyn.npz: maxiDynamics / maxiRMS outputs and
states of the UNMODIFIED reference for the cases below, and the stream of tests/patches/dynamics_patch.cpp.

It compiles tools/gen/dyn_ref_dump.cpp with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling
checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary directory outside
the tree, and records the compiler, flags, libc and the sha256 of the reference sources inside the file.  Nothing else
in the tree changes.

Inputs are stored as int16 q (the signal is q / 32768.0, exact in double), so that the file stays small.  Every case is
played in blocks cut at CUTS plus the positions of its mid-stream setter calls; the small state arrays are stored at
every cut (key "<case>/snap<i>/..."), the rings after the last block (rows a run of N samples cannot have written are asserted zero and dropped).

For every stored case the generator ASSERTS that no sample's detector level lies within 1e-9 dB of a boundary it is
compared with (lowerKnee / higherKnee of a section with a knee, the bare threshold of one without): the device log10 is
good to about 1e-13 dB, so a sample that close could take the other branch on the GPU.  The smallest distance per
voice is stored as "<case>/margin_db"; the level itself as float32 "<case>/level_db" (a metering trace; the assertion
was made on the doubles).

    python tools/gen/gen_golden_dyn.py [--ref DIR]
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
OUT = os.path.join(ROOT, "tests", "golden", "dyn.npz")
N = 4000
CUTS = [0, 333, 397, N]
PATCH_FRAMES = 12000
NEAR_DB = 1e-9
SETTERS = {"attackHigh": 0, "releaseHigh": 1, "attackLow": 2, "releaseLow": 3, "lookAhead": 4, "rmsWindow": 5, "analyser": 6}
PEAK, RMS = 0, 1
ALL = -1  # a setter call made on every voice (the banks keep one envelope shape per bank, so attack / release calls are)


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


# ---- signals (int16) ----------------------------------------------------------------------------
def quant(x):
    return np.clip(np.round(np.asarray(x) * 32767.0), -32767, 32767).astype(np.int16)


def signals(rng, V, kinds):
    """One column per voice: 'noise' uniform in [-1, 1]; 'am_noise' / 'am_sine' sweep the level through the thresholds many
    times; 'gaps' has stretches of exact zeros and a burst after the silence."""
    n = np.arange(N)
    cols = []
    for v in range(V):
        k = kinds[v % len(kinds)]
        lfo = 0.5 - 0.5 * np.cos(2 * np.pi * n * rng.uniform(2.0, 5.0) / N + rng.uniform(0, 6.28))
        amp = 10.0 ** ((-55.0 + 55.0 * lfo) / 20.0)  # -55 dB .. 0 dB
        if k == "noise":
            x = rng.uniform(-1.0, 1.0, N)
        elif k == "am_noise":
            x = rng.uniform(-1.0, 1.0, N) * amp
        elif k == "am_sine":
            x = np.sin(2 * np.pi * n * rng.uniform(150.0, 900.0) / 44100.0) * amp
        else:  # gaps
            x = rng.uniform(-1.0, 1.0, N) * amp
            x[500:900] = 0.0
            x[900:930] = rng.uniform(-1.0, 1.0, 30)  # a burst after the silence
            x[2000:2600] = 0.0
        cols.append(quant(x))
    return np.ascontiguousarray(np.stack(cols, axis=1))


# name, sr_ctor (the rate in force when the objects are constructed: ring sizes), V, signal kinds, distinct side chain,
# analyser [V], parameters [6] (each [V] or a function (n, v) -> value), setter calls (n, what, voice, value)
CASES = [
    # compress(): RMS, knee > 0 and = 0, ratio > 1 and < 1; look-ahead 0 / 2 ms / above the ring; window 50 ms (ctor) / 10 ms /
    # 1 sample / 500 ms, and changed mid-stream; attack / release changed mid-stream
    ("compress", 44100, 4, ["am_noise", "am_sine", "gaps", "am_noise"], False, [RMS] * 4,
     [[-20, -25, -20, -30], [4, 4, 0.5, 0.25], [6, 0, 6, 0], [0] * 4, [0] * 4, [0] * 4],
     [(0, "rmsWindow", 1, 10.0), (0, "lookAhead", 1, 2.0), (0, "rmsWindow", 2, 0.03), (0, "rmsWindow", 3, 500.0),
      (0, "lookAhead", 3, 2000.0), (0, "attackHigh", ALL, 1.0), (0, "releaseHigh", ALL, 200.0),
      (1500, "rmsWindow", 1, 5.0), (2500, "attackHigh", ALL, 200.0), (2500, "releaseHigh", ALL, 1.0), (2500, "lookAhead", 0, 1.0)]),
    # play() with both sections, a distinct side chain, compandBelow, PEAK with |control| < 1; small rings (constructed at 3000 Hz:
    # 1500 / 3000 slots) so that both wrap; a look-ahead above the ring; a window request above the ring (ignored, sum zeroed)
    ("play", 3000, 4, ["am_noise", "gaps", "am_sine", "noise"], True, [RMS, RMS, PEAK, PEAK],
     [[-15, -12, 0, -20], [3, 0.5, 0, 4], [4, 0, 0, 0], [-40, -35, -30, -45], [2, 0.5, 3, 0], [6, 0, 5, 0]],
     [(0, "rmsWindow", 0, 10.0), (0, "lookAhead", 0, 2.0), (0, "rmsWindow", 1, 30.0), (0, "attackLow", ALL, 1.0),
      (0, "releaseLow", ALL, 200.0), (0, "lookAhead", 3, 100.0), (0, "lookAhead", 2, 2.0),
      (1200, "lookAhead", 0, 5.0), (2000, "rmsWindow", 1, 400.0), (3000, "attackLow", ALL, 50.0), (3000, "releaseLow", ALL, 3.0),
      (3000, "attackHigh", ALL, 33.3)]),
    # per-sample threshold and ratio
    ("persample", 44100, 4, ["am_sine", "am_noise", "noise", "gaps"], False, [RMS, PEAK, RMS, RMS],
     [lambda n, v: -30.0 + 20.0 * n / N - 1.5 * v, lambda n, v: 0.3 + 5.0 * ((n * (3 + v)) % 1000) / 1000.0, [5, 0, 2, 0],
      lambda n, v: -50.0 + 0.002 * n + v, [0, 2, 0.5, 0], [0, 3, 0, 0]],
     [(0, "rmsWindow", 0, 10.0), (0, "rmsWindow", 2, 2.0), (0, "lookAhead", 2, 2.0), (0, "attackHigh", ALL, 200.0),
      (0, "releaseHigh", ALL, 1.0), (2000, "attackHigh", ALL, 2.5)]),
]


def expand(p, V):
    if callable(p):
        return np.array([[p(n, v) for v in range(V)] for n in range(N)], np.float64), True
    return np.ascontiguousarray(np.broadcast_to(np.asarray(p, np.float64), (N, V))), False


def margin(level, par):
    """Smallest distance in dB, per voice, between the detector level and a boundary the sample is compared with."""
    th, rh, kh, tl, rl, kl = par
    m = np.full(level.shape, np.inf)
    for t, r, k in ((th, rh, kh), (tl, rl, kl)):
        on, knee = r > 0, k > 0
        with np.errstate(invalid="ignore"):
            for b, use in ((t - k / 2.0, on & knee), (t + k / 2.0, on & knee), (t, on & ~knee)):
                d = np.abs(level - b)
                m = np.where(use & ~np.isnan(d), np.minimum(m, d), m)
    return m.min(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "maximilian.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    out = {}
    P = ctypes.c_void_p
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libdynref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "dyn_ref_dump.cpp"), ref_sources[0], "-lm"])
        L = ctypes.CDLL(so)
        L.dyn_new.restype = P
        L.dyn_new.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
        L.dyn_free.argtypes = [P]
        L.dyn_set.argtypes = [P, ctypes.c_int, ctypes.c_size_t, ctypes.c_double]
        L.dyn_play.argtypes = [P, ctypes.c_size_t, P, P, P, P, P]
        L.dyn_sizes.argtypes = [P, P, P]
        L.dyn_state.argtypes = [P] * 14
        L.rms_new.restype = P
        L.rms_new.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_double]
        L.rms_free.argtypes = [P]
        L.rms_set_window.argtypes = [P, ctypes.c_size_t, ctypes.c_double]
        L.rms_play.argtypes = [P, ctypes.c_size_t, P, P]
        L.rms_cap.restype = ctypes.c_int64
        L.rms_cap.argtypes = [P]
        L.rms_state.argtypes = [P] * 5
        L.envgen_set_time.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_size_t, ctypes.c_double, P]

        for ci, (name, sr_ctor, V, kinds, side, analyser, params, ops) in enumerate(CASES):
            rng = np.random.default_rng(7000 + ci)
            q = signals(rng, V, kinds)
            sig = q / 32768.0
            rec = {"sig_q": q, "sr_ctor": np.int64(sr_ctor), "analyser": np.array(analyser, np.int32)}
            control = sig
            if side:
                cq = signals(rng, V, kinds[::-1])
                rec["control_q"] = cq
                control = cq / 32768.0
            full, ps = [], 0
            for k, p in enumerate(params):
                a, per = expand(p, V)
                full.append(a)
                ps |= int(per) << k
                rec["par%d" % k] = a if per else a[0].copy()
            rec["ps"] = np.int32(ps)
            rec["ops"] = np.array([[n, SETTERS[w], v, val] for n, w, v, val in ops], np.float64).reshape(-1, 4)
            cuts = sorted(set(CUTS) | {int(o[0]) for o in ops})
            rec["cuts"] = np.array(cuts, np.int64)
            h = L.dyn_new(V, sr_ctor, 44100)
            for v in range(V):
                L.dyn_set(h, SETTERS["analyser"], v, float(analyser[v]))
            cr, cl = ctypes.c_int64(0), ctypes.c_int64(0)
            L.dyn_sizes(h, ctypes.byref(cr), ctypes.byref(cl))
            cr, cl = cr.value, cl.value
            rec["cap_rms"], rec["cap_la"] = np.int64(cr), np.int64(cl)
            y, lvl = np.zeros((N, V)), np.zeros((N, V))

            def snapshot():
                st = dict(rring=np.zeros((cr, V)), lring=np.zeros((cl, V)), rpos=np.zeros(V, np.int32), lpos=np.zeros(V, np.int32),
                          window=np.zeros(V, np.uint32), look=np.zeros(V, np.uint32), running=np.zeros(V),
                          dst_h=np.zeros((5, V)), ist_h=np.zeros((7, V), np.int64), dst_l=np.zeros((5, V)),
                          ist_l=np.zeros((7, V), np.int64), stages_h=np.zeros((V, 3, 6)), stages_l=np.zeros((V, 3, 6)))
                L.dyn_state(h, *[st[k].ctypes.data for k in ("rring", "lring", "rpos", "lpos", "window", "look", "running", "dst_h",
                                                                 "ist_h", "dst_l", "ist_l", "stages_h", "stages_l")])
                return st

            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                for n, w, v, val in ops:
                    if n == a:
                        for vv in (range(V) if v == ALL else [v]):
                            L.dyn_set(h, SETTERS[w], vv, float(val))
                blk = [np.ascontiguousarray(x[a:b]) for x in [sig, control] + full]
                pp = (P * 6)(*[x.ctypes.data for x in blk[2:]])
                yb, lb = np.zeros((b - a, V)), np.zeros((b - a, V))
                L.dyn_play(h, b - a, blk[0].ctypes.data, blk[1].ctypes.data, pp, yb.ctypes.data, lb.ctypes.data)
                y[a:b], lvl[a:b] = yb, lb
                st = snapshot()
                last = i == len(cuts) - 2
                for k, arr in st.items():
                    if k in ("rring", "lring"):
                        if not last:
                            continue
                        rows = min(arr.shape[0], N)
                        assert not arr[rows:].any(), (name, k)  # a ring longer than the run: the rest was never written
                        arr = arr[:rows].copy()
                    rec["snap%d/%s" % (i, k)] = arr
            L.dyn_free(h)
            assert not np.isnan(y).any(), name  # the reference's output has exact zeros where outDB is NaN, never NaN
            mg = margin(lvl, full)
            assert (mg > NEAR_DB).all(), "%s: a level within %g dB of a compared boundary (margins %s)" % (name, NEAR_DB, mg)
            assert np.abs(lvl[np.isfinite(lvl)]).max() < 1000.0, name  # far below the 6000 dB where pow would underflow
            rec.update(out=y, level_db=lvl.astype(np.float32), margin_db=mg)
            print("%-10s zeros %5.1f %%  margin %.2e dB" % (name, 100.0 * (y == 0).mean(), mg.min()))
            for k, a in rec.items():
                out[name + "/" + k] = a

        # maxiRMS alone: window 10 ms of a 100 ms ring (wraps), changed to 1 sample, then to a request above the ring
        V = 4
        rng = np.random.default_rng(7100)
        q = signals(rng, V, ["am_noise", "gaps", "noise", "am_sine"])
        h = L.rms_new(V, 10000, 100.0, 10.0)
        cap = L.rms_cap(h)
        y = np.zeros((N, V))
        rops = [(1000, 1, 0.1), (2000, 2, 250.0), (3000, 3, 50.0)]
        cuts = [0, 333, 1000, 2000, 3000, N]
        wins = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            for n, v, ms in rops:
                if n == a:
                    L.rms_set_window(h, v, ms)
            x = np.ascontiguousarray(q[a:b] / 32768.0)
            yb = np.zeros((b - a, V))
            L.rms_play(h, b - a, x.ctypes.data, yb.ctypes.data)
            y[a:b] = yb
            ring, pos, win, run = np.zeros((cap, V)), np.zeros(V, np.int32), np.zeros(V, np.uint32), np.zeros(V)
            L.rms_state(h, ring.ctypes.data, pos.ctypes.data, win.ctypes.data, run.ctypes.data)
            wins.append(win)
        L.rms_free(h)
        out.update({"rms/in_q": q, "rms/out": y, "rms/cap": np.int64(cap), "rms/cuts": np.array(cuts, np.int64),
                    "rms/window": np.stack(wins), "rms/ring": ring, "rms/pos": pos, "rms/running": run,
                    "rms/ops": np.array(rops, np.float64), "rms/sr": np.int64(10000)})

        # maxiEnvGen::setTime on setupASR(10, 10) tables
        rows = []
        for sr, idx, ms in [(44100, 0, 1.0), (44100, 2, 200.0), (44100, 0, 0.01), (48000, 2, 33.3), (44100, 1, 5.0), (44100, 0, -46692.0),
                            (22050, 2, 0.5)]:
            tab = np.zeros((3, 6))
            err = L.envgen_set_time(sr, 10.0, 10.0, idx, ms, tab.ctypes.data)
            rows.append(np.concatenate([[sr, idx, ms, err], tab.reshape(-1)]))
        out["set_time"] = np.array(rows)

        # the drop-in patch's stream: tests/patches/dynamics_patch.cpp + oracle/example_host.cpp (read only) + the reference
        exe = os.path.join(td, "dyn_patch")
        subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-o", exe,
                               os.path.join(ROOT, "oracle", "example_host.cpp"),
                               os.path.join(ROOT, "tests", "patches", "dynamics_patch.cpp"), ref_sources[0], "-lm", "-lpthread"])
        raw = os.path.join(td, "patch.f64")
        subprocess.run([exe, str(PATCH_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out["patch"] = np.fromfile(raw, np.float64).reshape(PATCH_FRAMES, 2)
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    out["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; "
        "harness: tools/gen/dyn_ref_dump.cpp; patch: tests/patches/dynamics_patch.cpp via oracle/example_host.cpp"
        % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    out["cases"] = np.array([c[0] for c in CASES])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
