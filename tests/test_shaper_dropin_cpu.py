"""CPU (-m "not gpu"): the K18 drop-in classes (maxiNonlinearity / maxiDistortion, maxiXFade, maxiSelect, maxiSelectX, maxiLine,
maxiBits) are host value types.  tests/patches/shaper_patch.cpp compiles against include/maximilian.h and, where the reference is
present, against the reference; built with -DSHAPER_PATCH_ARITH (plain arithmetic sources instead of oscillators, so that no
device is needed) the two builds run here and their streams agree bit for bit -- both call the same libm."""
import os
import re
import subprocess

import numpy as np

import shaper_host as sh
from conftest import ROOT, assert_bits_equal

PATCH = os.path.join(ROOT, "tests", "patches", "shaper_patch.cpp")
FRAMES = 6000


def ref_src():
    ref = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    src = os.path.join(os.environ.get("MAXI_REF") or ref, "src")
    return src if os.path.exists(os.path.join(src, "maximilian.cpp")) else None


def test_patch_compiles_both_ways():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), PATCH])
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-DSHAPER_PATCH_ARITH", "-I" + os.path.join(ROOT, "include"), PATCH])
    src = ref_src()
    if src:   # the reference is not in this tree
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I" + src, PATCH])


def run(exe, tmp_path, name):
    raw = str(tmp_path / (name + ".f64"))
    r = subprocess.run([exe, str(FRAMES), raw], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(raw, np.float64).reshape(FRAMES, 2)


def test_arithmetic_patch_runs_without_a_device_and_matches_the_reference(tmp_path):
    import maximilian_amd as mx
    libdir = os.path.dirname(mx.LIB_PATH)
    host = os.path.join(ROOT, "oracle", "example_host.cpp")
    exe = str(tmp_path / "dropin")
    subprocess.check_call(["g++", "-std=c++17"] + sh.fpflags() + ["-w", "-DSHAPER_PATCH_ARITH", "-I" + os.path.join(ROOT, "include"), "-o", exe, host,
                           PATCH, "-L" + libdir, "-lmaxigpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    got = run(exe, tmp_path, "dropin")
    assert np.isfinite(got).all() and len(np.unique(got[:, 0])) > 1000 and len(np.unique(got[:, 1])) > 1000
    assert (np.abs(got[:, 1]) > 1.5).any()   # the clipped branches of softclip and atanDist at once
    src = ref_src()
    if not src:
        return   # the reference is not in this tree: the compile and the run above are the test
    ref = str(tmp_path / "ref")
    subprocess.check_call(["g++", "-std=c++17"] + sh.fpflags() + ["-w", "-DSHAPER_PATCH_ARITH", "-I" + src, "-o", ref, host, PATCH,
                           os.path.join(src, "maximilian.cpp"), "-lm", "-lpthread"])
    exp = run(ref, tmp_path, "ref")
    assert_bits_equal(got[:, 0], exp[:, 0], "hardclip, fastatan, fastAtanDist, cross-fades, selects, lines, bit signals")
    assert_bits_equal(got[:, 1], exp[:, 1], "softclip, atanDist, asymclip (the same libm)")
