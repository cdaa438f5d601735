"""GPU: the drop-in maxiDynamics / maxiRMS / maxiRingBuf (include/maximilian.h), one bank-of-one launch per call.
tests/patches/dynamics_patch.cpp built as host/dropin_p8 against the same patch compiled with the reference
(tests/golden/dyn.npz["patch"]), 12 000 frames: positions of NaN and of exact 0.0 identical, the rest within the tolerance of
tests/test_gpu_dyn.py.  tests/patches/dynamics_copy_patch.cpp (host/dropin_p9): a copy made mid-stream continues with the same
samples as its source; maxiRMS against the host checker and maxiRingBuf::tail bit for bit.  host/facade_dyn_smoke exits 0."""
import os
import subprocess

import numpy as np
import pytest

import dyn_host
from conftest import GOLDEN, ROOT, assert_bits_equal
from test_gpu_dyn import TOL

pytestmark = pytest.mark.gpu


def run_host(name, frames, tmp_path):
    exe = os.path.join(ROOT, "host", name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), name])
    out = str(tmp_path / (name + ".f64"))
    r = subprocess.run([exe, str(frames), out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    assert "ERROR" not in r.stderr, r.stderr
    return np.fromfile(out, np.float64).reshape(frames, 2)


def test_dynamics_patch_against_reference(tmp_path):
    exp = np.load(os.path.join(GOLDEN, "dyn.npz"))["patch"]
    assert exp.shape[0] == 12000
    got = run_host("dropin_p8", exp.shape[0], tmp_path)
    assert (exp[:, 0] != 0).mean() > 0.2 and (exp[:, 1] != 0).mean() > 0.2  # both compressors are audible in the stream
    for ch, what in ((0, "compress (RMS, look-ahead, moving threshold and ratio, setter mid-stream)"),
                     (1, "compandBelow (PEAK, side chain, copied mid-stream)")):
        rel = dyn_host.compare_output(got[:, ch], exp[:, ch], np.ones(exp.shape[0], bool), what)
        print("%s: rel %.3e" % (what, rel))
        assert rel <= TOL, "%s: relative error %.3e > %.1e" % (what, rel, TOL)


def test_copy_rms_and_ringbuf(tmp_path, tmp_path_factory, mx):
    frames = 6000
    got = run_host("dropin_p9", frames, tmp_path)
    n = np.arange(frames)
    x = ((n * 37) % 1000 / 1000.0 - 0.5) * np.where((n // 700) % 2 == 1, 1.6, 0.05)
    # maxiRingBuf: tail(7) after the push = the value pushed 7 pushes ago, counting this one (zeros before the ring has them)
    exp = np.concatenate([np.zeros(6), x])[:1000]
    assert_bits_equal(got[:1000, 1], exp, "maxiRingBuf::tail")
    # maxiRMS: setup(100, 10) at 44100, against the host build of the same arithmetic
    L = dyn_host.build(tmp_path_factory.mktemp("dyn"))
    N, cap = 2000, 4410
    xb, ob = np.ascontiguousarray(x[1000:3000]).reshape(N, 1), np.zeros((N, 1))
    ring, pos, run, ovf, win = np.zeros((cap, 1)), np.zeros(1, np.int32), np.zeros(1), np.zeros(1, np.uint32), np.full(1, 441, np.uint32)
    L.rms_host_render(1, N, xb.ctypes.data, win.ctypes.data, ring.ctypes.data, cap, pos.ctypes.data, run.ctypes.data, ovf.ctypes.data,
                      ob.ctypes.data)
    assert_bits_equal(got[1000:3000, 1], ob[:, 0], "maxiRMS::play")
    # the copy made at frame 2999 plays the same samples as its source from frame 3000 on
    assert (got[3000:, 0] != 0).any()
    assert_bits_equal(got[3000:, 1], got[3000:, 0], "copy of a maxiDynamics")


def test_facade_dyn_smoke():
    exe = os.path.join(ROOT, "host", "facade_dyn_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_dyn_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
