"""GPU: the drop-in maxiFlanger / maxiChorus (include/maximilian.h) in a patch -- tests/patches/fx_patch.cpp built as
host/dropin_p7 -- bit-identical to the same patch compiled against the reference (tests/golden/fx.npz["patch"])."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_fx_cpu import bits_equal

pytestmark = pytest.mark.gpu


def test_fx_patch_bit_exact(tmp_path):
    exp = np.load(os.path.join(GOLDEN, "fx.npz"))["patch"]
    exe = os.path.join(ROOT, "host", "dropin_p7")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "dropin_p7"])
    out = str(tmp_path / "p7.f64")
    r = subprocess.run([exe, str(exp.shape[0]), out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr
    assert "ERROR" not in r.stderr, r.stderr
    got = np.fromfile(out, np.float64).reshape(exp.shape)
    assert bits_equal(got[:, 0], exp[:, 0]), "flanger channel"
    assert bits_equal(got[:, 1], exp[:, 1]), "chorus channel"
