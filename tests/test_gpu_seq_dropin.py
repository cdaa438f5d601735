"""GPU: tests/patches/seq_patch.cpp -- the graph of the reference's example 9.Envelopes3 with maxiOsc::saw and fixed envelopes of
curve 1, plus a maxiCounter, a maxiIndex and a maxiZXToPulse -- built against the drop-in header as host/dropin_sq, against the
same patch compiled with the reference (tests/golden/seq.npz["patch"]): bit for bit.  The sequencing classes are host value
types; the oscillators, envelopes and the filter they drive run on the device.  host/facade_seq_smoke exits 0."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu


def run_host(name, frames, tmp_path):
    exe = os.path.join(ROOT, "host", name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), name])
    out = str(tmp_path / (name + ".f64"))
    r = subprocess.run([exe, str(frames), out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "ERROR" not in r.stderr, r.stderr
    return np.fromfile(out, np.float64).reshape(frames, 2)


def test_seq_patch_against_reference(tmp_path):
    exp = np.load(os.path.join(GOLDEN, "seq.npz"))["patch"]
    assert exp.shape[0] == 8000
    got = run_host("dropin_sq", exp.shape[0], tmp_path)
    assert (exp[:, 0] != 0).mean() > 0.5 and (exp[:, 1] != 0).mean() > 0.3  # both voices are audible in the stream
    assert_bits_equal(got[:, 1], exp[:, 1], "fixed clock: playTrig -> maxiEnvGen * saw(maxiStep)")
    assert_bits_equal(got[:, 0], exp[:, 0], "modulated clock, counter, index, pulse, SVF")


def test_facade_seq_smoke():
    exe = os.path.join(ROOT, "host", "facade_seq_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_seq_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
