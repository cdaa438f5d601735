"""GPU: the drop-in maxiKick / maxiSnare / maxiHats / maxiClock in running programs.  tests/patches/drums_patch.cpp (host/dropin_dr)
and the reference's example 7.Counting1 compiled VERBATIM against include/ (oracle/_ref/dropin_07) are run, and their streams are
checked against tests/golden/drums_streams.npz, which tools/gen/gen_golden_drums.py recorded from the same two sources compiled
against the reference: the patch's snare + hats channel -- no sinewave -- BIT FOR BIT (the clock, the rand() draws in call order, a
copy in mid-stream, the setters on the public envelope and filter); its kick channel and the example, which are sinewaves, within
the bound of the existing drop-in sinewave streams (tests/test_gpu_dropin.py, 08c: 1.2e-16 per unit amplitude).

Measured on an MI355X: the printout of the two tests; DESIGN.md section 4 has the figures."""
import os
import subprocess

import numpy as np
import pytest

import drums_host as dh
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SINE_BOUND = 1.2e-16   # per unit amplitude


@pytest.fixture(scope="module")
def streams():
    return np.load(os.path.join(GOLDEN, "drums_streams.npz"))


def run(exe, frames, tmp_path):
    path = os.path.join(ROOT, exe)
    if not os.path.exists(path):
        pytest.fail("%s is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)" % exe)
    out = str(tmp_path / "o.f64")
    r = subprocess.run([path, str(frames), out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert b"ERROR" not in r.stderr, r.stderr.decode()
    return np.fromfile(out, np.float64).reshape(frames, 2)


def expected(streams, key):
    ch, frames = int(streams[key + "/channels"]), dh.STREAM_FRAMES[key]
    e = dh.unshuffle(streams[key], (frames, ch))
    return e if ch == 2 else np.repeat(e, 2, axis=1)


def test_drums_patch_against_reference(streams, tmp_path):
    exp = expected(streams, "patch")
    got = run("host/dropin_dr", dh.STREAM_FRAMES["patch"], tmp_path)
    assert len(np.unique(exp[:, 0])) > 1000 and len(np.unique(exp[:, 1])) > 1000
    dh.bits_equal(got[:, 0], exp[:, 0], "snare + hats + the copied hats, triggered by the clock")
    d = float(np.abs(got[:, 1] - exp[:, 1]).max())
    print("drums patch: the kick within %.3e (bound %.3e)" % (d, SINE_BOUND))
    assert d <= SINE_BOUND   # (the kick's output stays at or below 1, after fastAtanDist's normalisation too)


def test_counting1_verbatim(streams, tmp_path):
    exp = expected(streams, "07")
    got = run("oracle/_ref/dropin_07", dh.STREAM_FRAMES["07"], tmp_path)
    assert len(np.unique(exp[:, 0])) > 1000 and np.abs(np.diff(np.sign(exp[22100:, 0]))).sum() > 1.5 * np.abs(np.diff(np.sign(exp[:22000, 0]))).sum()   # (the tick at frame 22 050 raises 20 Hz to 120 Hz)
    d = np.abs(got - exp)
    print("7.Counting1: max |difference| %.3e at frame %d (bound %.3e)" % (d.max(), int(d.max(axis=1).argmax()), SINE_BOUND))
    assert d.max() <= SINE_BOUND
