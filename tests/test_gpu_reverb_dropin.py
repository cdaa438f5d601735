"""GPU: the drop-in maxiSatReverb / maxiFreeVerb / maxiFreeVerbStereo (include/maxiReverb.h), one bank-of-one launch per call.
tests/patches/reverb_patch.cpp built as host/dropin_rv against include/ equals the same patch compiled with the reference
(tests/golden/reverb.npz["patch"]) bit for bit: all three classes, both maxiFreeVerb overloads on one object, playStereo into both
channels, copies made mid-stream, a std::vector of reverbs that grows.  A dead engine plays silence.  host/facade_reverb_smoke
exits 0."""
import os
import subprocess

import numpy as np
import pytest

import reverb_cases as rc
import reverb_host as rh
from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu


def run_host(name, frames, tmp_path, env=None):
    exe = os.path.join(ROOT, "host", name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), name])
    out = str(tmp_path / (name + ".f64"))
    r = subprocess.run([exe, str(frames), out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    return np.fromfile(out, np.float64).reshape(frames, 2), r.stderr


def test_reverb_patch_against_reference(tmp_path):
    exp = rh.load_golden()["patch"]
    assert exp.shape == (rc.PATCH_FRAMES, 2)
    got, log = run_host("dropin_rv", exp.shape[0], tmp_path)
    assert "ERROR" not in log, log
    assert (exp[:, 0] != 0).mean() > 0.9 and (exp[3000:, 1] != 0).mean() > 0.9  # the reverbs are audible on both channels
    assert_bits_equal(got[:, 0], exp[:, 0], "left: sat + freeverb (both overloads) + stereo left + vector")
    assert_bits_equal(got[:, 1], exp[:, 1], "right: stereo right + the copies made at frame 2500")


def test_dead_engine_returns_silence(tmp_path):
    got, log = run_host("dropin_rv", 300, tmp_path, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert log.count("ERROR: maxigpu") == 1 and "no CPU fallback" in log, log
    assert not got.any(), "silence, not a CPU rendering"


def test_facade_reverb_smoke():
    exe = os.path.join(ROOT, "host", "facade_reverb_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_reverb_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
