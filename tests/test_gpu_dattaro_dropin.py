"""GPU: the drop-in maxiDattaroReverb (include/maxiReverb.h), one bank-of-one launch per call.
tests/patches/dattaro_patch.cpp built as host/dropin_dt against include/ equals the same patch compiled with the reference
(tests/golden/dattaro.npz["patch"]) bit for bit: an object at 44 100 Hz and one constructed at 22 050 Hz, a copy made mid-stream
and played beside its source, an object destroyed and constructed again.  A dead engine plays silence.
host/facade_dattaro_smoke exits 0.  Every GPU program runs under its own time limit."""
import os
import subprocess

import numpy as np
import pytest

import dattaro_cases as dc
import dattaro_host as dh
from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu


def run_host(name, frames, tmp_path, env=None):
    exe = os.path.join(ROOT, "host", name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), name])
    out = str(tmp_path / (name + ".f64"))
    r = subprocess.run(["timeout", "-k", "10", "600", exe, str(frames), out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       env=env)
    assert r.returncode == 0, r.stderr
    return np.fromfile(out, np.float64).reshape(frames, 2), r.stderr


def test_dattaro_patch_against_reference(tmp_path):
    exp = dh.load_golden()["patch"]
    assert exp.shape == (dc.PATCH_FRAMES, 2)
    got, log = run_host("dropin_dt", exp.shape[0], tmp_path)
    assert "ERROR" not in log, log
    assert (exp[1000:] != 0).mean() > 0.9  # the reverbs are audible on both channels
    assert_bits_equal(got[:, 0], exp[:, 0], "left")
    assert_bits_equal(got[:, 1], exp[:, 1], "right")


def test_dead_engine_returns_silence(tmp_path):
    got, log = run_host("dropin_dt", 300, tmp_path, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert log.count("ERROR: maxigpu") == 1 and "no CPU fallback" in log, log
    assert not got.any(), "silence, not a CPU rendering"


def test_facade_dattaro_smoke():
    exe = os.path.join(ROOT, "host", "facade_dattaro_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_dattaro_smoke"])
    r = subprocess.run(["timeout", "-k", "10", "300", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
