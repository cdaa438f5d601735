#!/usr/bin/env python3
"""tools/gen/gen_golden_dattaro.py -- TEST INFRASTRUCTURE.  Writes tests/golden/dattaro.npz: outputs and final states of the
UNMODIFIED reference's maxiDattaroReverb for the cases of tests/dattaro_cases.py, and the lengths and tap positions its
constructor computes at the five rates and at both ends of the accepted range.

It compiles tools/gen/dattaro_ref_dump.cpp with the reference's src/maximilian.cpp and src/libs/maxiReverb.cpp (path:
$MAXI_REF, default the sibling checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a
temporary directory outside the tree, and records the compiler, flags, libc and the sha256 of the reference sources inside
the file.  Nothing else in the tree changes.

The file keeps every output sample.  Inputs are not stored: tests/dattaro_host.py regenerates them from the case table
(numpy's PCG64 streams are stable) and checks their sha256 against the one recorded here.  Final state: indices and the
five state doubles whole; the rings as a sha256 per case, and whole for the 8 000 Hz case.  The generator asserts that no
ring slot beyond a ring's length (and none of the two rings the class never touches) is non-zero, and that no output is a
NaN.

    python tools/gen/gen_golden_dattaro.py [--ref DIR]
"""
import argparse
import ctypes
import hashlib
import os
import platform
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(ROOT, "tests", "golden", "dattaro.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dattaro_cases as dc  # noqa: E402  (the case table, shared with the tests)


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def run_ref(L, rate, x):
    N, V = x.shape
    _, offs, S = dc.layout(rate)
    out = np.zeros((2, N, V))
    rings, idx, state = np.zeros((V, S)), np.zeros((V, dc.RINGS), np.int32), np.zeros((V, dc.STATE))
    lens, taps, fbap = np.zeros(dc.RINGS, np.int32), np.zeros(dc.TAPS, np.int32), np.zeros(8, np.int32)
    oa = np.asarray(offs, np.int32)
    stray = L.dt_run(rate, V, N, x.ctypes.data, out.ctypes.data, oa.ctypes.data, S, rings.ctypes.data, idx.ctypes.data,
                     state.ctypes.data, lens.ctypes.data, taps.ctypes.data, fbap.ctypes.data)
    assert stray == 0, "rate %d: the reference's lengths differ from the layout, or it touched a slot beyond a ring's length (%d)" % (rate, stray)
    assert not np.isnan(out).any(), "a NaN in the reference's output for finite input"
    return out, rings, idx, state, lens, taps, fbap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "libs", "maxiReverb.cpp"),
                   os.path.join(src, "maximilian.h"), os.path.join(src, "libs", "maxiReverb.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    inc = ["-I" + src, "-I" + os.path.join(src, "libs")]
    out = {}
    lo, hi = dc.accepted_ends()
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libdtref.so")
        subprocess.check_call([cxx] + flags + inc + ["-o", so, os.path.join(HERE, "dattaro_ref_dump.cpp")] + ref_sources[:2] + ["-lm"])
        L = ctypes.CDLL(so)
        P = ctypes.c_void_p
        L.dt_run.restype = ctypes.c_long
        L.dt_run.argtypes = [ctypes.c_size_t] * 3 + [P] * 3 + [ctypes.c_size_t] + [P] * 6
        # the constructor's lengths: the five rates, both ends of the accepted range and the rates just outside it
        table = dc.RATES + [lo, hi]
        z = np.zeros((1, 1))
        out["rates"] = np.array(table)
        out["lengths"] = np.stack([run_ref(L, r, z)[4] for r in table])
        out["taps"] = np.stack([run_ref(L, r, z)[5] for r in table])
        out["fbap"] = np.stack([run_ref(L, r, z)[6] for r in table])
        out["accepted_ends"] = np.array([lo, hi])
        for case in dc.CASES:
            name, rate = case["name"], dc.case_rate(case)
            x = dc.inputs(case)
            y, rings, idx, state, lens, taps, _ = run_ref(L, rate, x)
            if case["signal"] == "tail":
                assert case["N"] - case["noise"] > 2 * max(lens), name  # the silence wraps every ring twice
                assert (y[:, -100:] != 0).any(), name
            assert (y != 0).any(axis=1).all(), name
            out[name + "/rate"] = np.array(rate)
            out[name + "/out"] = y
            out[name + "/idx"] = idx
            out[name + "/state"] = state
            out[name + "/ring_sha256"] = np.array(hashlib.sha256(rings.tobytes()).hexdigest())
            out[name + "/in_sha256"] = np.array(dc.inputs_digest(x))
            if case.get("keep_rings"):
                out[name + "/rings"] = rings
        # the drop-in patch's stream: tests/patches/dattaro_patch.cpp + oracle/example_host.cpp (read only) + the reference
        exe = os.path.join(td, "dattaro_patch")
        subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w"] + inc + ["-o", exe,
                               os.path.join(ROOT, "oracle", "example_host.cpp"),
                               os.path.join(ROOT, "tests", "patches", "dattaro_patch.cpp")] + ref_sources[:2] + ["-lm", "-lpthread"])
        raw = os.path.join(td, "patch.f64")
        subprocess.run([exe, str(dc.PATCH_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        patch = np.fromfile(raw, np.float64).reshape(dc.PATCH_FRAMES, 2)
        assert not np.isnan(patch).any() and (patch[1000:] != 0).mean() > 0.9
        out["patch"] = patch
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    out["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp, src/libs/maxiReverb.cpp, their .h) sha256: %s; "
        "harness: tools/gen/dattaro_ref_dump.cpp; cases: tests/dattaro_cases.py; patch: tests/patches/dattaro_patch.cpp via "
        "oracle/example_host.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    out["cases"] = np.array([c["name"] for c in dc.CASES])
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print("wrote %s (%d bytes)" % (OUT, size))


if __name__ == "__main__":
    main()
