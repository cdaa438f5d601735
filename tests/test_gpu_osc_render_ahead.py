"""GPU parity (-m gpu): K1's paced branches render each chunk of eight samples AHEAD of its slot and store it on the slot
(csrc/osc.hip, osc_kernel).  Timing only: every case is three carried blocks under a forced or controlled schedule against the
free-running kernel (knob osc_pace 1) bit for bit -- blocks, `phase` and the `output` member -- and a subsample of voices against
the oracle."""
import numpy as np
import pytest

from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SINEBUF, SAW = 8, 3


def _run(mx, wf, freq, N, pace):
    L = mx.lib()
    prev = L.mxg_tune(b"osc_pace", pace)
    try:
        bank = mx.maxiOscBank(freq.shape[0])
        outs = [bank.render(wf, freq, N).numpy() for _ in range(3)]
        return np.concatenate(outs), bank.phase.numpy().copy(), bank.output.numpy().copy()
    finally:
        L.mxg_tune(b"osc_pace", prev)


def _check(mx, port, wf, V, N, paces):
    rng = np.random.default_rng(V + 31 * N + wf)
    freq = rng.uniform(20, 20000, V)
    ref = _run(mx, wf, freq, N, 1)
    assert ref[0].shape == (3 * N, V)
    for pace in paces:
        got = _run(mx, wf, freq, N, pace)
        for a, b, what in zip(ref, got, ("blocks", "phase", "output member")):
            assert_bits_equal(b, a, "V=%d N=%d osc_pace=%d, %s" % (V, N, pace, what))
    sel = np.unique(np.concatenate([np.arange(0, V, 997), [V - 2, V - 1]]).astype(np.int64))
    eo, eph, _ = port.osc(wf, freq[sel], 3 * N)
    assert_bits_equal(ref[0][:, sel], eo, "oracle, blocks")
    assert_bits_equal(ref[1][sel], eph, "oracle, phase")


@pytest.mark.parametrize("N", [512, 515, 8, 7, 9, 1])
def test_headline_shape_forced_period(mx, port, N):
    """sinebuf at 65 536 voices with the paced branch forced by a fixed period: blocks of 512 / 515 samples take the pair-row kernel
    (its paced branch, then the pair loop and the ragged tail), the short ones the plain-store kernel -- whole chunks, no whole
    chunk, one sample on either side of a chunk."""
    _check(mx, port, SINEBUF, 65536, N, (54, 60))


@pytest.mark.parametrize("N", [512, 9])
def test_odd_bank_forced_period(mx, port, N):
    """An odd bank just above the headline's: no voice pairs, a partial last wavefront, one part and one pass -- the plain-store
    kernel's paced branch.  The block is exactly [3 N][V]: a row or a voice out of range would show as a difference, or fault."""
    _check(mx, port, SINEBUF, 65536 + 127, N, (54, 60))


def test_table_free_waveform_forced_period(mx, port):
    """saw has no staged chunk form: its chunk is eight ticks into registers, stored on the slot.  (An even saw bank of the
    headline's size renders two voices per lane and is never paced: the odd one, and the 131 072-voice one under the controller.)"""
    _check(mx, port, SAW, 65536 + 127, 515, (54, 60))
    _check(mx, port, SAW, 131072, 203, (0, 108))


def test_sinebuf_131072_under_the_controller(mx, port):
    """The 131 072-voice sinebuf bank is paced by the controller (osc_pace 0) and shares the plain-store kernel's paced branch."""
    _check(mx, port, SINEBUF, 131072, 203, (0, 108))
    _check(mx, port, SINEBUF, 131072, 512, (0,))
