#!/usr/bin/env python3
"""tools/gen/gen_golden_fx.py -- TEST INFRASTRUCTURE.  Writes tests/golden/fx.npz: maxiFlanger / maxiChorus outputs,
draws and final states of the UNMODIFIED reference for the cases below.

It compiles tools/gen/fx_ref_dump.cpp with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling
checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary directory outside
the tree, and records the compiler, flags, libc and the sha256 of the reference sources inside the file.  Nothing else
in the tree changes (tests/golden/MANIFEST.json included).

    python tools/gen/gen_golden_fx.py [--ref DIR]
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
OUT = os.path.join(ROOT, "tests", "golden", "fx.npz")


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


# name, kind, V, N, params: delay, feedback, speed, depth -- each a [V] list (block rate) or a function (n, v) -> value
N0 = 1000
PATCH_FRAMES = 12000


def _ramp(a, b):
    return lambda n, v, N: a + (b - a) * n / N + 0.37 * v


CASES = [
    # flanger
    ("fl_large", "flanger", 4, N0, [800, 800, 700, 1000], [0.0, 0.5, 0.99, 0.3], [0.5, 1.0, 3.0, 0.2], [0.5, 0.5, 1.0, 0.8]),
    ("fl_short", "flanger", 4, N0, [20, 40, 10, 63], [0.99, 0.7, 0.5, 0.2], [2.0, 5.0, 11.0, 0.7], [0.5, 1.0, 0.3, 0.9]),
    ("fl_edges", "flanger", 5, N0, [0, 1, 30, 800, 200], [1.2, 0.99, 1.2, 0.0, 0.5], [1.0, 7.0, 20.0, 0.05, 9.0],
     [0.0, 1.5, 1.5, 1.0, float("nan")]),
    ("fl_ps", "flanger", 3, N0, lambda n, v, N: 50 + (n * (7 + 3 * v)) % 900, _ramp(0.2, 0.95),
     lambda n, v, N: 0.5 + 15.0 * n / N + v, _ramp(0.1, 1.4)),
    # chorus
    ("ch_large", "chorus", 4, N0, [800, 800, 700, 1000], [0.0, 0.5, 0.99, 0.3], [5.0, 10.0, 11.0, 200.0], [0.5, 0.5, 1.0, 0.8]),
    ("ch_short", "chorus", 4, N0, [20, 40, 10, 63], [0.99, 0.7, 0.5, 0.2], [0.0001, 10.0, 3000.0, 9.99], [0.5, 1.0, 0.3, 0.9]),
    ("ch_edges", "chorus", 5, N0, [0, 1, 30, 800, 200], [1.2, 0.99, 1.2, 0.0, 0.5], [1.0, 7.0, 20.0, 0.05, 9.0],
     [0.0, 1.5, 1.5, 1.0, float("nan")]),
    ("ch_ps", "chorus", 3, N0, lambda n, v, N: 50 + (n * (7 + 3 * v)) % 900, _ramp(0.2, 0.95),
     lambda n, v, N: 2.0 + 40.0 * n / N + 30 * v, _ramp(0.1, 1.4)),
]


def expand(p, V, N, dtype):
    if callable(p):
        return np.array([[p(n, v, N) for v in range(V)] for n in range(N)], dtype=dtype), True
    return np.broadcast_to(np.asarray(p, dtype), (N, V)).copy(), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "maximilian.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    out = {}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libfxref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "fx_ref_dump.cpp"),
                                               ref_sources[0], "-lm"])
        L = ctypes.CDLL(so)
        P = ctypes.c_void_p
        L.fx_flange.argtypes = [ctypes.c_size_t, ctypes.c_size_t] + [P] * 8
        L.fx_chorus.argtypes = [ctypes.c_size_t, ctypes.c_size_t] + [P] * 5 + [ctypes.c_uint] + [P] * 4
        for ci, (name, kind, V, N, delay, fb, speed, depth) in enumerate(CASES):
            rng = np.random.default_rng(1000 + ci)
            x = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (N, V)))
            d, dps = expand(delay, V, N, np.uint32)
            f, fps = expand(fb, V, N, np.float64)
            s, sps = expand(speed, V, N, np.float64)
            p, pps = expand(depth, V, N, np.float64)
            y = np.zeros((N, V))
            rec = {"in": x, "out": y, "ps": np.array([dps, fps, sps, pps], np.int32)}
            if kind == "flanger":
                ph, lph = np.zeros(V, np.int32), np.zeros(V)
                L.fx_flange(V, N, x.ctypes.data, d.ctypes.data, f.ctypes.data, s.ctypes.data, p.ctypes.data,
                            y.ctypes.data, ph.ctypes.data, lph.ctypes.data)
                rec.update(phase=ph, lfo_phase=lph)
            else:
                ph, lp, rd = np.zeros((2, V), np.int32), np.zeros((2, V)), np.zeros((N, V), np.int32)
                L.fx_chorus(V, N, x.ctypes.data, d.ctypes.data, f.ctypes.data, s.ctypes.data, p.ctypes.data,
                            4242 + ci, rd.ctypes.data, y.ctypes.data, ph.ctypes.data, lp.ctypes.data)
                rec.update(phase=ph, lp=lp, rand=rd)
            # block-rate parameters are stored as [V], per-sample ones as [N][V]
            for k, a, ps in (("delay", d, dps), ("feedback", f, fps), ("speed", s, sps), ("depth", p, pps)):
                rec[k] = a if ps else a[0].copy()
            for k, a in rec.items():
                out[name + "/" + k] = a
        # the drop-in patch's stream: tests/patches/fx_patch.cpp + oracle/example_host.cpp (read only) + the reference
        exe = os.path.join(td, "fx_patch")
        subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-o", exe,
                               os.path.join(ROOT, "oracle", "example_host.cpp"),
                               os.path.join(ROOT, "tests", "patches", "fx_patch.cpp"), ref_sources[0], "-lm", "-lpthread"])
        raw = os.path.join(td, "patch.f64")
        subprocess.run([exe, str(PATCH_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out["patch"] = np.fromfile(raw, np.float64).reshape(PATCH_FRAMES, 2)
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    out["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; "
        "harness: tools/gen/fx_ref_dump.cpp; patch: tests/patches/fx_patch.cpp via oracle/example_host.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    out["cases"] = np.array([c[0] for c in CASES])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
