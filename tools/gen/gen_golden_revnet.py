#!/usr/bin/env python3
"""tools/gen/gen_golden_revnet.py -- TEST INFRASTRUCTURE.  Writes tests/golden/revnet.npz: outputs and final states of networks
built from arrays of the UNMODIFIED reference's maxiReverbFilters objects (tests/revnet_cases.py), and the stream of
tests/patches/revfilt_patch.cpp, which drives every public method of single objects.

It compiles tools/gen/revnet_ref_dump.cpp with the reference's src/maximilian.cpp and src/libs/maxiReverb.cpp (path: $MAXI_REF,
default the sibling checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary
directory outside the tree, and records the compiler, flags, libc and the sha256 of the reference sources inside the file.
Nothing else in the tree changes.

The file keeps every output sample.  Inputs and parameters are not stored: tests/revnet_host.py regenerates them from the
case table (numpy's PCG64 streams are stable) and checks their sha256 against the one recorded here.  Final state: indices and
low-pass states whole; the rings as a sha256 per case, and whole for the small cases.

    python tools/gen/gen_golden_revnet.py [--ref DIR]
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
OUT = os.path.join(ROOT, "tests", "golden", "revnet.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import revnet_cases as rc  # noqa: E402  (the case table, shared with the tests)


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def run_ref(L, case):
    x, comb_fb, comb_cut, ap_fb = rc.inputs(case)
    combs, aps, lowp = rc.topology(case)
    N, V = x.shape
    P, A = len(combs), len(aps)
    offs, S = rc.layout(combs, aps)
    sizes = np.asarray(combs + aps, np.float64)
    lp_flags, oa = np.asarray(lowp + [0], np.int32), np.asarray(offs + [0], np.int32)
    out = np.zeros((N, V))
    rings, idx, lp = np.zeros((V, S)), np.zeros((V, P + A), np.int32), np.zeros((V, P))
    stray = L.rn_run(V, N, x.ctypes.data, P, A, sizes.ctypes.data, lp_flags.ctypes.data, comb_fb.ctypes.data, comb_cut.ctypes.data,
                     ap_fb.ctypes.data, out.ctypes.data, oa.ctypes.data, S, rings.ctypes.data, idx.ctypes.data, lp.ctypes.data)
    assert stray == 0, "the reference touched a ring slot beyond the stage's length"
    return (x, comb_fb, comb_cut, ap_fb), out, rings, idx, lp


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
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "librnref.so")
        subprocess.check_call([cxx] + flags + inc + ["-o", so, os.path.join(HERE, "revnet_ref_dump.cpp")] + ref_sources[:2] + ["-lm"])
        L = ctypes.CDLL(so)
        P = ctypes.c_void_p
        L.rn_run.restype = ctypes.c_long
        L.rn_run.argtypes = [ctypes.c_size_t, ctypes.c_size_t, P, ctypes.c_int, ctypes.c_int] + [P] * 7 + [ctypes.c_size_t] + [P] * 3
        for case in rc.CASES:
            name = case["name"]
            ins, y, rings, idx, lp = run_ref(L, case)
            assert np.isfinite(y).all() and (y != 0).mean() > 0.5, name
            if case.get("subnormal"):
                a = np.abs(y)
                n_sub = int(((a > 0) & (a < np.finfo(np.float64).tiny)).sum())
                assert n_sub >= 100, "%s: only %d subnormal outputs" % (name, n_sub)
                out[name + "/n_subnormal"] = np.array(n_sub)
            out[name + "/out"] = y
            out[name + "/idx"] = idx
            out[name + "/lp"] = lp
            out[name + "/ring_sha256"] = np.array(hashlib.sha256(rings.tobytes()).hexdigest())
            out[name + "/in_sha256"] = np.array(rc.inputs_digest(case, *ins))
            if case.get("keep_rings"):
                out[name + "/rings"] = rings
        # the drop-in patch's stream: tests/patches/revfilt_patch.cpp + oracle/example_host.cpp (read only) + the reference
        exe = os.path.join(td, "revfilt_patch")
        subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w"] + inc + ["-o", exe,
                               os.path.join(ROOT, "oracle", "example_host.cpp"),
                               os.path.join(ROOT, "tests", "patches", "revfilt_patch.cpp")] + ref_sources[:2] + ["-lm", "-lpthread"])
        raw = os.path.join(td, "patch.f64")
        subprocess.run([exe, str(rc.PATCH_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        patch = np.fromfile(raw, np.float64).reshape(rc.PATCH_FRAMES, rc.PATCH_CHANNELS)
        assert np.isfinite(patch).all()
        for ch in range(rc.PATCH_CHANNELS):
            assert len(np.unique(patch[:, ch])) > 500, "channel %d of the patch is not alive" % ch
        out["patch"] = patch
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    out["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp, src/libs/maxiReverb.cpp, their .h) sha256: %s; "
        "harness: tools/gen/revnet_ref_dump.cpp; cases: tests/revnet_cases.py; patch: tests/patches/revfilt_patch.cpp via "
        "oracle/example_host.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    out["cases"] = np.array([c["name"] for c in rc.CASES])
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print("wrote %s (%d bytes)" % (OUT, size))


if __name__ == "__main__":
    main()
