"""CPU (-m "not gpu"): the Kuramoto classes of the drop-in header are host value types.  tests/patches/kuramoto_patch.cpp -- a
sync set of 2 and of 7, two async sets exchanging phases every 2000 samples through setPhase / setPhases, getPhase, size, the
pair's mix through maxiMap::linexp -- compiled against include/maximilian.h with -DKURAMOTO_PATCH_NO_OSC (which leaves out the
one maxiOsc, a device object) runs without a device.  Channel 0 is compared with the stream the same patch gives with the
UNMODIFIED reference (tests/golden/kuramoto.npz["patch"]): bit for bit where the running libc is the recorded one -- the classes
restate the reference's arithmetic and call the same sin() and pow() -- and otherwise within the largest `tol` of the file's
cases scaled to the patch (see PATCH_TOL)."""
import os
import platform
import subprocess

import numpy as np

import kuramoto_host as kh
from conftest import ROOT, assert_bits_equal

# Another libm may round a sine or the pitch's pow() differently in the last place.  The sets of the patch are the file's cases in
# kind (kt is the pair: 44 100 Hz, K = 1900, N = 2); channel 0 is 0.001 * pitch (<= 0.88, relative error of pow a few ULP: 1e-18)
# + the seven's mix + 0.25 * (two mixes) + 0.25 * a phase: four phase-like terms with weights summing to 2, each within the
# largest tol of the file (6.9e-13).
PATCH_TOL = 2 * 6.9e-13


def test_patch_against_dropin_header(golden, tmp_path):
    import maximilian_amd as mx
    g = golden("kuramoto.npz")
    exp = g["patch"]
    exe = str(tmp_path / "patch")
    libdir = os.path.dirname(mx.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17"] + kh.fpflags() + ["-w", "-DKURAMOTO_PATCH_NO_OSC", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "oracle", "example_host.cpp"), os.path.join(ROOT, "tests", "patches", "kuramoto_patch.cpp"),
                           "-L" + libdir, "-lmaxigpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    raw = str(tmp_path / "o.f64")
    r = subprocess.run([exe, str(exp.shape[0]), raw], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(raw, np.float64).reshape(exp.shape)
    assert exp.shape[0] > 4000 and len(np.unique(exp[:, 0])) > 0.9 * exp.shape[0]   # both kinds of exchange happen; nothing constant
    assert max(float(g[n + "/tol"]) for n in g["cases"]) <= 6.9e-13
    assert (got[:, 1] == 0).all()
    same_libc = " ".join(platform.libc_ver()) == str(g["libc"])
    dev = float(np.abs(got[:, 0] - exp[:, 0]).max())
    print("kuramoto_patch channel 0: max |difference| %.3e (libc %s the recorded one)" % (dev, "is" if same_libc else "is NOT"))
    if same_libc:
        assert_bits_equal(got[:, 0], exp[:, 0], "kuramoto_patch, channel 0")
    else:
        assert dev <= PATCH_TOL


def test_patch_compiles_against_dropin_header_with_the_oscillator():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "patches", "kuramoto_patch.cpp")])
