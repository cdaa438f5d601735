"""GPU: the drop-in maxiDyn, maxiEnvelope, maxiLagExp and maxiMap inside a patch whose oscillators run on the device.
tests/patches/classic_patch.cpp (saw and phasor only: exact sources) built as host/dropin_cl gives the stream the same patch gives
with the reference (tests/golden/classic.npz["patch"]), bit for bit in both channels: output[0] -- the gate, the envelope, the lag,
the maps -- and output[1] -- the compressors with their host-libm make-up factor and setter coefficients.  host/facade_classic_smoke
exits 0."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu


def test_classic_patch_against_reference(tmp_path):
    exp = np.load(os.path.join(GOLDEN, "classic.npz"))["patch"]
    exe = os.path.join(ROOT, "host", "dropin_cl")
    if not os.path.exists(exe):
        pytest.fail("host/dropin_cl is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)")
    out = str(tmp_path / "o.f64")
    r = subprocess.run([exe, str(exp.shape[0]), out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert b"ERROR" not in r.stderr, r.stderr.decode()
    got = np.fromfile(out, np.float64).reshape(exp.shape)
    assert len(np.unique(exp[:, 0])) > 1000 and len(np.unique(exp[:, 1])) > 1000
    assert_bits_equal(got[:, 0], exp[:, 0], "gate, envelope, lag, linlin, clamp")
    assert_bits_equal(got[:, 1], exp[:, 1], "compressor, compress() after the setters")


def test_facade_classic_smoke():
    exe = os.path.join(ROOT, "host", "facade_classic_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_classic_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
