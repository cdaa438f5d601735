"""GPU: the drop-in maxiPolyBLEP inside patches whose other classes run on the device too, against the streams the same sources
give with the reference (tests/golden/polyblep_streams.npz, tools/gen/gen_golden_polyblep.py).

tests/patches/polyblep_patch.cpp built as host/dropin_pb: output[0] -- the ten arithmetic waveforms, sync, setPulseWidth,
setSampleRate, a copied object, a negative frequency, maxiEnvGen::setLevel -- BIT FOR BIT; output[1] -- SINE, COSINE, the two
rectified sines and a sawtooth swept through sampleRate / 4 -- within the sum of its terms' bounds (PATCH_CH1_BOUND below).

The reference's examples 9.Envelopes1 / 2 / 3 VERBATIM (oracle/_ref/dropin_09a / b / c, built by host/Makefile where the
reference is present): curved envelopes (the device's pow), maxiSVF / maxiBiquad recursions and atanDist, so no bound is
derivable in advance; the bound is 20 x the maximum |difference| measured on an MI355X against the recorded reference stream,
the project's convention (5.FM1, 22.Analysis).  Measured over 6000 frames: 9.Envelopes1 4.441e-16 (peak 1.400), 9.Envelopes2
4.441e-15 (peak 2.479), 9.Envelopes3 1.388e-16 (peak 0.565) -- a few ULP of the peak; bounds 8.9e-15, 8.9e-14, 2.8e-15.
9.Envelopes3's maxiPoll text is the reference's to the printed digits.  The patch's output[1] measured 1.665e-16.

host/facade_polyblep_smoke -- maxiPolyBLEPBank of include/maximilian_bank.hpp against the C-ABI calls and the host arithmetic --
exits 0."""
import os
import subprocess

import numpy as np
import pytest

import polyblep_host as ph
from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

# output[1] = (SINE + COSINE + HALF + FULL + sweep) / 5.0: the terms differ by at most 2^-53 (1 ULP of a value below 1: SINE, COSINE,
# the swept sawtooth where it is a sine) and 2^-50 (each rectified sine) = 19 * 2^-53 in all; each of the five additions rounds a
# partial sum below 4 (two roundings at most 2^-51 apart); the division by 5 rounds a value below 2 (2^-52 apart).
PATCH_CH1_BOUND = (19 + 5 * 4) * 2.0 ** -53 / 5 + 2.0 ** -52
EXAMPLE_BOUND = {"09a": 20 * 4.441e-16, "09b": 20 * 4.441e-15, "09c": 20 * 1.388e-16}


@pytest.fixture(scope="module")
def streams():
    return np.load(os.path.join(GOLDEN, "polyblep_streams.npz"))


def run(exe, tmp_path, what):
    path = os.path.join(ROOT, exe)
    if not os.path.exists(path):
        pytest.fail("%s is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)" % exe)
    out = str(tmp_path / "o.f64")
    r = subprocess.run([path, str(ph.STREAM_FRAMES), out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert b"ERROR" not in r.stderr, r.stderr.decode()
    return np.fromfile(out, np.float64).reshape(ph.STREAM_FRAMES, 2), r.stdout.decode()


def expected(streams, key):
    ch = int(streams[key + "/channels"])
    e = ph.unshuffle(streams[key], (ph.STREAM_FRAMES, ch))
    return e if ch == 2 else np.repeat(e, 2, axis=1)


def test_polyblep_patch_against_reference(streams, tmp_path):
    exp = expected(streams, "patch")
    got, _ = run("host/dropin_pb", tmp_path, "patch")
    assert len(np.unique(exp[:, 0])) > 1000 and len(np.unique(exp[:, 1])) > 1000
    assert_bits_equal(got[:, 0], exp[:, 0], "the ten arithmetic waveforms, sync, setPulseWidth, setSampleRate, a copy, setLevel")
    d = float(np.abs(got[:, 1] - exp[:, 1]).max())
    print("polyblep patch: the sine waveforms within %.3e (bound %.3e)" % (d, PATCH_CH1_BOUND))
    assert d <= PATCH_CH1_BOUND


@pytest.mark.parametrize("key", sorted(ph.EXAMPLES))
def test_reference_example_verbatim(streams, tmp_path, key):
    exp = expected(streams, key)
    got, text = run("oracle/_ref/dropin_" + key, tmp_path, ph.EXAMPLES[key])
    assert len(np.unique(exp[:, 0])) > 1000
    d = np.abs(got - exp)
    print("%s: max |difference| %.3e at frame %d, peak %.3f (bound %.3e)" % (ph.EXAMPLES[key], d.max(), int(d.max(axis=1).argmax()),
                                                                             np.abs(exp).max(), EXAMPLE_BOUND[key]))
    assert d.max() <= EXAMPLE_BOUND[key]
    if key == "09c":   # what maxiPoll printed (the reference's setup() also prints its stage table: those lines are its own)
        want = [ln for ln in str(streams["09c/poll"]).splitlines() if not ln.startswith("Stage")]
        assert want and [ln for ln in text.splitlines() if not ln.startswith("Stage")] == want


def test_facade_polyblep_smoke():
    exe = os.path.join(ROOT, "host", "facade_polyblep_smoke")
    if not os.path.exists(exe):
        pytest.fail("host/facade_polyblep_smoke is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
