"""GPU: tests/patches/bands_patch.cpp (maxiFFT -> maxiBark::specificLoudness and maxiFFTOctaveAnalyzer::calculate on every new
frame) linked against the library and compared with the stream recorded from the reference (tests/golden/bands.npz): the octave
channel (averages, peaks, hold counters) bit for bit, the Bark channel within ULP_SPECIFIC of bands_host.py."""
import os
import subprocess

import numpy as np
import pytest

import bands_host as bh
from conftest import ROOT, assert_bits_equal, ulp_diff

pytestmark = pytest.mark.gpu


def test_patch_stream_against_the_reference(mx, golden, tmp_path):
    ref = golden("bands.npz")["patch"]
    libdir = os.path.dirname(mx.LIB_PATH)
    exe, raw = str(tmp_path / "dropin"), str(tmp_path / "out.f64")
    subprocess.check_call(["g++", "-std=c++17"] + bh.fpflags() + ["-w", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "oracle", "example_host.cpp"), os.path.join(ROOT, "tests", "patches", "bands_patch.cpp"),
                           "-L" + libdir, "-lmaxigpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(bh.PATCH_FRAMES), raw], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(raw, np.float64).reshape(bh.PATCH_FRAMES, 2)
    assert_bits_equal(got[:, 0], ref[:, 0], "the octave channel: averages, peaks and hold counters")
    assert np.isfinite(got[:, 1]).all()
    worst = int(ulp_diff(got[:, 1], ref[:, 1]).max())
    print("the Bark channel: %d ULP from the reference (bound %d)" % (worst, bh.ULP_SPECIFIC))
    assert worst <= bh.ULP_SPECIFIC


def test_copies_continue_identically(mx, tmp_path):
    """tests/patches/bands_copy_main.cpp: maxiBark and maxiFFTOctaveAnalyzer copied mid-stream (copy construction and assignment over
    an object set up differently) continue bit for bit like the original; the public arrays are the state."""
    libdir = os.path.dirname(mx.LIB_PATH)
    exe = str(tmp_path / "copy")
    subprocess.check_call(["g++", "-std=c++17"] + bh.fpflags() + ["-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "patches", "bands_copy_main.cpp"), "-L" + libdir, "-lmaxigpu", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "bands_copy_main: ok" in r.stdout and "ERROR" not in r.stderr, r.stderr


def test_facade_bands_smoke():
    exe = os.path.join(ROOT, "host", "facade_bands_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_bands_smoke"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    print(r.stdout)
