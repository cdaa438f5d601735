"""GPU (-m gpu): the drop-in maxiStretch<F> with loop points and playAtPosition.  tests/patches/stretch_loop_patch.cpp --
setLoopStart(0.25), setLoopEnd(0.5), play() with stepping pitch and timestretch (a negative one among them), then playAtPosition --
is compiled against include/maximilian.h + include/maxiGrains.h (host/Makefile dropin_sl), where a maxiStretch whose loop is not the
whole sample and every playAtPosition call go through mxg_granular_pool_render (K27) on the object's own sample as a pool of one
slot.  Expected: the stream patch_sl of tests/golden/grainpool.npz, the SAME source file linked with the unmodified reference
(tools/gen/gen_golden_grainpool.py).  Every sample of both channels bit for bit: the grain arithmetic, the loop wraps, the rewinds
at argument changes and the order of the rand() draws."""
import os
import subprocess

import numpy as np
import pytest

import grainpool_host as gh
from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu


def _run(frames, tmp_path):
    exe = os.path.join(ROOT, "host", "dropin_sl")
    if not os.path.exists(exe):
        pytest.fail("host/dropin_sl is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)")
    out = str(tmp_path / "dropin_sl.f64")
    r = subprocess.run([exe, str(frames), out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return np.fromfile(out, np.float64).reshape(frames, 2), r.stderr


def test_stretch_loop_patch_bit_exact(golden, tmp_path):
    exp = golden("grainpool.npz")["patch_sl"]
    assert exp.shape == (gh.PATCH_SL_FRAMES, 2)
    got, log = _run(exp.shape[0], tmp_path)
    assert "ERROR" not in log, log
    assert_bits_equal(got[:, 0], exp[:, 0], "stretch loop patch, left")
    assert_bits_equal(got[:, 1], exp[:, 1], "stretch loop patch, right (the public loop members)")
    assert np.abs(exp[:9000, 0]).max() > 0.2 and np.abs(exp[9000:, 0]).max() > 0.2
