"""GPU: the K18 drop-in classes inside a patch whose oscillators run on the device.  tests/patches/shaper_patch.cpp (saw, phasor
and triangle only: exact sources) built as host/dropin_sh gives the stream the same patch gives with the reference
(tests/golden/shaper.npz["patch"]): output[0] -- every bit-exact member -- bit for bit; output[1] -- softclip's pow, atanDist and
asymclip, which go through the libm of the machine that runs the test -- within 2 ULP of the reference's samples.
host/facade_shaper_smoke exits 0."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, assert_bits_equal, ulp_diff

pytestmark = pytest.mark.gpu


def test_shaper_patch_against_reference(tmp_path):
    exp = np.load(os.path.join(GOLDEN, "shaper.npz"))["patch"]
    exe = os.path.join(ROOT, "host", "dropin_sh")
    if not os.path.exists(exe):
        pytest.fail("host/dropin_sh is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)")
    out = str(tmp_path / "o.f64")
    r = subprocess.run([exe, str(exp.shape[0]), out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert b"ERROR" not in r.stderr, r.stderr.decode()
    got = np.fromfile(out, np.float64).reshape(exp.shape)
    assert len(np.unique(exp[:, 0])) > 1000 and len(np.unique(exp[:, 1])) > 1000
    assert_bits_equal(got[:, 0], exp[:, 0], "hardclip, fastatan, fastAtanDist, cross-fades, selects, lines, bit signals")
    # the sum of three libm-made terms: each within 1 ULP of its own (smaller) value, so 2 ULP of the sum wherever the sum is not
    # a cancellation; the bound is applied in ULPs of max(|sum|, 1), the size of the largest term
    d = np.abs(got[:, 1] - exp[:, 1]) / np.spacing(np.maximum(np.abs(exp[:, 1]), 1.0))
    print("shaper patch: softclip + atanDist + asymclip within %.2f ULP" % d.max())
    assert d.max() <= 2.0


def test_facade_shaper_smoke():
    exe = os.path.join(ROOT, "host", "facade_shaper_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_shaper_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
