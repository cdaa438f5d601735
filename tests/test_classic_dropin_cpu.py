"""CPU (-m "not gpu"): the drop-in maxiDyn and maxiEnvelope (with maxiLagExp, maxiMap) are host value types.
tests/patches/classic_patch.cpp and tests/patches/classic_members_patch.cpp -- which touches every public member of the two new
classes -- compile against include/maximilian.h and, where the reference is present, against the reference.  Built with
-DCLASSIC_PATCH_ARITH (plain arithmetic sources instead of oscillators, so that no device is needed) classic_patch.cpp runs here
and its stream is the one recorded from the reference build (tests/golden/classic.npz["patch_arith"]), bit for bit in both
channels: output[0] -- the gate, the envelope, the lag, the maps -- and output[1] -- the compressors, whose make-up factor (log) and
setter coefficients (pow) come from the host libm, the same values tests/test_classic_host.py pins to the same file."""
import os
import re
import subprocess

import numpy as np

import classic_host as ch
from conftest import GOLDEN, ROOT, assert_bits_equal

PATCH = os.path.join(ROOT, "tests", "patches", "classic_patch.cpp")
MEMBERS = os.path.join(ROOT, "tests", "patches", "classic_members_patch.cpp")
INC = "-I" + os.path.join(ROOT, "include")
FRAMES = 4000


def ref_src():
    ref = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    src = os.path.join(os.environ.get("MAXI_REF") or ref, "src")
    return src if os.path.exists(os.path.join(src, "maximilian.cpp")) else None


def test_patches_compile_both_ways():
    for patch in (PATCH, MEMBERS):
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", INC, patch])
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-DCLASSIC_PATCH_ARITH", INC, PATCH])
    src = ref_src()
    if src:   # the reference is not in this tree
        for patch in (PATCH, MEMBERS):
            subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I" + src, patch])


def build_and_run(tmp_path, name, patch, defs, frames):
    import maximilian_amd as mx
    libdir = os.path.dirname(mx.LIB_PATH)
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17"] + ch.fpflags() + ["-w"] + defs + [INC, "-o", exe, os.path.join(ROOT, "oracle", "example_host.cpp"), patch,
                           "-L" + libdir, "-lmaxigpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    raw = str(tmp_path / (name + ".f64"))
    r = subprocess.run([exe, str(frames), raw], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(raw, np.float64).reshape(frames, 2)


def test_arithmetic_patch_runs_without_a_device_and_matches_the_recorded_reference(tmp_path):
    exp = np.load(os.path.join(GOLDEN, "classic.npz"))["patch_arith"]
    assert exp.shape == (FRAMES, 2) and len(np.unique(exp[:, 0])) > 1000 and len(np.unique(exp[:, 1])) > 1000
    got = build_and_run(tmp_path, "dropin", PATCH, ["-DCLASSIC_PATCH_ARITH"], FRAMES)
    assert_bits_equal(got[:, 0], exp[:, 0], "gate, envelope, lag, linlin, clamp")
    assert_bits_equal(got[:, 1], exp[:, 1], "compressor, compress() after the setters")


def test_members_patch_runs_and_copies_carry_their_state(tmp_path):
    got = build_and_run(tmp_path, "members", MEMBERS, [], 64)
    assert np.isfinite(got).all() and len(np.unique(got[:, 0])) > 8 and len(np.unique(got[:, 1])) > 8
    src = ref_src()
    if not src:
        return   # the reference is not in this tree: the compile and the run above are the test
    exe = str(tmp_path / "ref")
    subprocess.check_call(["g++", "-std=c++17"] + ch.fpflags() + ["-w", "-I" + src, "-o", exe, os.path.join(ROOT, "oracle", "example_host.cpp"), MEMBERS,
                           os.path.join(src, "maximilian.cpp"), "-lm", "-lpthread"])
    raw = str(tmp_path / "ref.f64")
    subprocess.run([exe, "64", raw], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
    exp = np.fromfile(raw, np.float64).reshape(64, 2)
    assert_bits_equal(got, exp, "every public member, copies and arrays (the same libm on both sides)")
