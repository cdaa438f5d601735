#!/usr/bin/env python3
"""tools/gen/gen_golden_reverb.py -- TEST INFRASTRUCTURE.  Writes tests/golden/reverb.npz: outputs and final states of the
UNMODIFIED reference's maxiSatReverb / maxiFreeVerb / maxiFreeVerbStereo for the cases below.

It compiles tools/gen/reverb_ref_dump.cpp with the reference's src/maximilian.cpp and src/libs/maxiReverb.cpp (path:
$MAXI_REF, default the sibling checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a
temporary directory outside the tree, and records the compiler, flags, libc and the sha256 of the reference sources inside
the file.  Nothing else in the tree changes.

The file keeps every output sample.  Inputs and parameters are not stored: tests/reverb_host.py regenerates them from the
case table below (numpy's PCG64 streams are stable) and checks their sha256 against the one recorded here.  Final state:
indices, low-pass states and (w, cut) whole; the rings as a sha256 per case, and whole for the maxiSatReverb case.

    python tools/gen/gen_golden_reverb.py [--ref DIR]
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
OUT = os.path.join(ROOT, "tests", "golden", "reverb.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reverb_cases as rc  # noqa: E402  (the case table, shared with the tests)


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def run_ref(L, kind, x, mode, room, absorb):
    N, V = x.shape
    lens, offs, S = rc.layout(kind)
    F = len(lens)
    out = np.zeros((rc.CHANNELS[kind], N, V))
    rings, idx, lp, wc = np.zeros((V, S)), np.zeros((V, F), np.int32), np.zeros((V, 8)), np.zeros((V, 2))
    la, oa = np.asarray(lens, np.int32), np.asarray(offs, np.int32)
    stray = L.rv_run(kind, V, N, x.ctypes.data, mode.ctypes.data, room.ctypes.data, absorb.ctypes.data, out.ctypes.data,
                     rc.NCOMB[kind], F - rc.NCOMB[kind], la.ctypes.data, oa.ctypes.data, S, rings.ctypes.data, idx.ctypes.data,
                     lp.ctypes.data, wc.ctypes.data)
    assert stray == 0, "the reference touched a ring slot beyond the filter's length"
    return out, rings, idx, lp, wc


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
        so = os.path.join(td, "librvref.so")
        subprocess.check_call([cxx] + flags + inc + ["-o", so, os.path.join(HERE, "reverb_ref_dump.cpp")] + ref_sources[:2] + ["-lm"])
        L = ctypes.CDLL(so)
        P = ctypes.c_void_p
        L.rv_run.restype = ctypes.c_long
        L.rv_run.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t] + [P] * 5 + [ctypes.c_int, ctypes.c_int, P, P,
                                                                                           ctypes.c_size_t] + [P] * 4
        for case in rc.CASES:
            name, kind = case["name"], case["kind"]
            x, mode, room, absorb = rc.inputs(case)
            y, rings, idx, lp, wc = run_ref(L, kind, x, mode, room, absorb)
            if case.get("subnormal"):
                a = np.abs(y)
                n_sub = int(((a > 0) & (a < np.finfo(np.float64).tiny)).sum())
                assert n_sub >= 100, "%s: only %d subnormal outputs" % (name, n_sub)
                out[name + "/n_subnormal"] = np.array(n_sub)
            if case.get("clamps"):
                assert (room < -8.4).any() and (room > 1.6).any() and (absorb < 0).any() and (absorb > 1).any(), name
            if kind == rc.STEREO:
                # the quirk that guards the restatement: the parameters change nothing, and the right channel is not silent
                y2 = run_ref(L, kind, x, mode, room * -3.0 + 1.0, absorb * 0.5 + 0.3)[0]
                assert np.array_equal(y.view(np.uint64), y2.view(np.uint64)), name
                assert (y[1] != 0).any(), name
            out[name + "/out"] = y
            out[name + "/idx"] = idx
            out[name + "/ring_sha256"] = np.array(hashlib.sha256(rings.tobytes()).hexdigest())
            out[name + "/in_sha256"] = np.array(rc.inputs_digest(x, mode, room, absorb))
            if kind == rc.FREEVERB:
                out[name + "/lp"] = lp
                out[name + "/wc"] = wc
            if case.get("keep_rings"):
                out[name + "/rings"] = rings
        # the drop-in patch's stream: tests/patches/reverb_patch.cpp + oracle/example_host.cpp (read only) + the reference
        exe = os.path.join(td, "reverb_patch")
        subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w"] + inc + ["-o", exe,
                               os.path.join(ROOT, "oracle", "example_host.cpp"),
                               os.path.join(ROOT, "tests", "patches", "reverb_patch.cpp")] + ref_sources[:2] + ["-lm", "-lpthread"])
        raw = os.path.join(td, "patch.f64")
        subprocess.run([exe, str(rc.PATCH_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        patch = np.fromfile(raw, np.float64).reshape(rc.PATCH_FRAMES, 2)
        assert (patch[:, 0] != 0).mean() > 0.9 and (patch[3000:, 1] != 0).mean() > 0.9
        out["patch"] = patch
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    out["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp, src/libs/maxiReverb.cpp, their .h) sha256: %s; "
        "harness: tools/gen/reverb_ref_dump.cpp; cases: tests/reverb_cases.py; patch: tests/patches/reverb_patch.cpp via "
        "oracle/example_host.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    out["cases"] = np.array([c["name"] for c in rc.CASES])
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print("wrote %s (%d bytes)" % (OUT, size))


if __name__ == "__main__":
    main()
