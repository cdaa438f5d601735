"""CPU (-m "not gpu"): the analysis classes of the drop-in header are host value types.  tests/patches/analysis_host_patch.cpp --
maxiZeroCrossingDetector, maxiZeroCrossingRate (a ring that wraps, a window that changes over a filled ring), maxiEnvelopeFollower,
maxiEnvelopeFollowerF and maxiSampleAndHold on arithmetic signals -- compiled against include/maximilian.h runs without a device
and gives the stream the same patch gives with the reference (tests/golden/analysis.npz["host_patch"]) bit for bit.  The patches,
and the reference's example 22.Analysis from its own location where the reference is present, compile against the header."""
import os
import re
import subprocess

import numpy as np

import analysis_host as ah
from conftest import ROOT, assert_bits_equal


def test_host_patch_against_dropin_header(golden, tmp_path):
    import maximilian_amd as mx
    exp = golden("analysis.npz")["host_patch"]
    exe = str(tmp_path / "patch")
    libdir = os.path.dirname(mx.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17"] + ah.fpflags() + ["-w", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "oracle", "example_host.cpp"), os.path.join(ROOT, "tests", "patches", "analysis_host_patch.cpp"),
                           "-L" + libdir, "-lmaxigpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    raw = str(tmp_path / "o.f64")
    r = subprocess.run([exe, str(exp.shape[0]), raw], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(raw, np.float64).reshape(exp.shape)
    assert len(np.unique(exp[:, 0])) > 1000 and len(np.unique(exp[:, 1])) > 1000 and exp[:, 1].max() > 50   # levels and rates, not zeros
    assert_bits_equal(got[:, 1], exp[:, 1], "rates, crossings and held samples")
    assert_bits_equal(got[:, 0], exp[:, 0], "followers")


def test_patches_compile_against_dropin_header():
    srcs = [os.path.join(ROOT, "tests", "patches", p) for p in ("analysis_patch.cpp", "analysis_host_patch.cpp")]
    ref = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    ex22 = os.path.join(os.environ.get("MAXI_REF") or ref, "cpp", "commandline", "maximilian_examples", "22.Analysis", "main.cpp")
    if os.path.exists(ex22):   # the example is compiled from its own location; it is not in this tree
        srcs.append(ex22)
    for src in srcs:
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), src])
