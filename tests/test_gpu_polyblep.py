"""GPU: mxg_polyblep_render (kernel K20) and maxiPolyBLEPBank against tests/golden/polyblep.npz under the contract of DESIGN.md
section 4 (tests/polyblep_host.py check_contract): the phase and the ten exact waveforms BIT FOR BIT, SINE / COSINE and every
fallback sample within 1 ULP, the two rectified sines within 2^-50 absolute.  Every waveform through the C-ABI and through the
Python bank; the shapes where the kernel can go wrong -- V in {1, 2, 63, 64, 65, 129, 257}: surplus lanes, odd V, more than one
workgroup; N in {1, 7, 8, 9, 17, 513}: shorter than a chunk, a ragged last chunk, many chunks -- with the voices repeated from
the six stored ones, per-voice and per-sample frequencies; the 16-byte pair-row stores (knob rw_store) against the 8-byte ones;
d_pw NULL against an explicit 0.5; a block rendered in one call against the same block in uneven cuts with the phase carried,
bit-identical, the sine waveforms included; a guard band around d_out and d_t untouched (GpuBackend checks it on every call).

Measured on an MI355X (the printout of test_every_waveform_through_the_cabi): see DESIGN.md section 4."""
import numpy as np
import pytest

import polyblep_host as ph
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

VS = (1, 2, 63, 64, 65, 129, 257)
NS = (1, 7, 8, 9, 17, 513)


@pytest.fixture(scope="module")
def g(golden):
    return golden("polyblep.npz")


@pytest.fixture(scope="module")
def be(mx):
    return ph.GpuBackend(mx)


@pytest.mark.parametrize("fps", [False, True])
def test_every_waveform_through_the_cabi(be, g, fps):
    worst = {}
    for wf in ph.WAVEFORMS:
        out, phases = ph.play_case(be, g, wf, fps=fps)
        worst[wf] = ph.check_contract(g, wf, out, phases, "C-ABI")
    print("measured:", {wf: r for wf, r in worst.items()})


@pytest.mark.parametrize("V", VS)
def test_shapes(be, g, V):
    tile = (V + ph.V - 1) // ph.V
    for N in NS:
        for wf in ph.WAVEFORMS:
            for fps in (False, True):
                out, phases = ph.play_case(be, g, wf, fps=fps, tile=tile, voices=V, upto=N)
                ph.check_contract(g, wf, out, phases, "V=%d N=%d fps=%d" % (V, N, fps), tile=tile, voices=V)


@pytest.mark.parametrize("rw", [2, 3, 4])
def test_pair_row_stores_give_the_same_bits(mx, be, g, rw):
    """Knob rw_store: the 16-byte pair rows (plain / write-through / non-temporal) on an even bank, against the stored reference."""
    L = mx.lib()
    prev = L.mxg_tune(b"rw_store", rw)
    try:
        for V in (2, 64, 130):
            tile = (V + ph.V - 1) // ph.V
            for wf in ph.WAVEFORMS:
                for fps in (False, True):
                    out, phases = ph.play_case(be, g, wf, fps=fps, tile=tile, voices=V, upto=601)
                    ph.check_contract(g, wf, out, phases, "rw_store=%d V=%d" % (rw, V), tile=tile, voices=V)
    finally:
        L.mxg_tune(b"rw_store", prev)


@pytest.mark.parametrize("V", [6, 65])
def test_one_call_equals_uneven_cuts(be, g, V):
    """The split cannot change a lane's arithmetic: one launch over 1200 samples against the launches of the stored cuts and
    a few more, the phase carried -- bit-identical, the sine waveforms included.  (One pulse width per voice throughout.)"""
    tile = (V + ph.V - 1) // ph.V
    f = np.tile(ph.freqs(g), (1, tile))[:, :V]
    pw = np.tile(np.array(ph.PW), tile)[:V]
    cuts = sorted(set(ph.CUTS) | {2, 64, 65, 513, 777})
    for wf in ph.WAVEFORMS:
        whole, tw = be.render(wf, f, pw, ph.SR, np.zeros(V))
        parts, t = np.zeros_like(whole), np.zeros(V)
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts[a:b], t = be.render(wf, f[a:b], pw, ph.SR, t)
        assert_bits_equal(whole, parts, wf)
        assert_bits_equal(tw, t, wf + " phase")
        assert len(np.unique(whole)) > 100


def test_null_pulse_width_is_one_half(be, g):
    f = ph.freqs(g)[:513]
    for wf in ph.WAVEFORMS:
        a, ta = be.render(wf, f, None, ph.SR, np.zeros(ph.V))
        b, tb = be.render(wf, f, np.full(ph.V, 0.5), ph.SR, np.zeros(ph.V))
        assert_bits_equal(a, b, wf)
        assert_bits_equal(ta, tb, wf + " phase")


def test_python_bank(mx, g):
    """maxiPolyBLEPBank: set_waveform, set_pulse_width at every stored cut, sync at sample 601, per-voice and per-sample
    frequencies, the phase carried from call to call."""
    f = ph.freqs(g)
    for wf in ph.WAVEFORMS:
        bank = mx.maxiPolyBLEPBank(ph.V, sampleRate=ph.SR)
        bank.set_waveform(wf)
        out, phases = np.zeros((ph.N, ph.V)), [np.zeros(ph.V)]
        for blk, (a, b) in enumerate(zip(ph.CUTS[:-1], ph.CUTS[1:])):
            bank.set_pulse_width(ph.pulse_widths(g, blk))
            if a == ph.SYNC_AT:
                bank.sync([p for _, p in ph.SYNC], voices=[v for v, _ in ph.SYNC])
            if b <= ph.PS_FROM:
                out[a:b] = bank.render(f[a], b - a).numpy()
            else:
                out[a:b] = bank.render(f[a:b], per_sample=True).numpy()
            phases.append(bank.t.numpy().copy())
        ph.check_contract(g, wf, out, np.array(phases), "bank")
    with pytest.raises(ValueError):
        mx.maxiPolyBLEPBank(4).set_waveform(14)
