"""GPU parity (-m gpu): the core families at maxiSettings::sampleRate other than 44100 -- the banks and the C-ABI against the
plain-C oracle under the same setting (tests/rates_cases.at_rate), each family compared exactly as its 44.1 kHz test compares it.
The rate reaches the device as a kernel argument or a host-computed coefficient at some twenty call sites; a stale value, a
reciprocal where the reference divides or an integer / float mix-up can be invisible at 44100.  One function per family."""
import numpy as np
import pytest

import rates_cases as rc
from conftest import assert_bits_equal, assert_close_scaled, mix_tol, ulp_diff
from rates_cases import RATES, at_rate

pytestmark = pytest.mark.gpu

MOD_FILTER_RTOL = 1e-11   # test_gpu_voice.py: device cos / sqrt coefficients through a recursive filter
MFCC_RTOL = 1e-12         # test_gpu_spectral.py: device log() vs glibc log() through the DCT
SHAPES = [(65, 200), (130, 200), (65, 71)]   # a wavefront + one ragged lane; an even bank (pair rows); a ragged last chunk of 8


def D(mx, a, dtype=None):
    return mx.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype))


def halves(N):
    return [(0, N // 2), (N // 2, N)]


@pytest.mark.parametrize("V,N", SHAPES)
@pytest.mark.parametrize("sr", RATES)
def test_osc_bank(mx, port, sr, V, N):
    """maxiOscBank, every waveform from phase 0 and from a random phase, and the per-sample FM form: output, phase and hold bit for
    bit (test_gpu_osc.py::test_osc_golden); sinewave / coswave <= 1 ULP with the phase bit-exact (test_gpu_edges.py:37,
    test_gpu_osc.py::test_trig_osc_ulp).  freq holds 0, sr/4 and sr/2."""
    c = rc.cases(sr, V, N, 21)
    with at_rate(sr, port, mx=mx):
        for wf, name in enumerate(rc.OSC):
            p1, p2 = (c["duty"], None) if name == "pulse" else (c["p1"], c["p2"])
            for ph0 in (None, c["phase0_tab"] if wf in (8, 9) else c["phase0"]):
                bank = mx.maxiOscBank(V)
                if ph0 is not None:
                    bank.phaseReset(ph0)
                o = bank.render(wf, c["freq"], N, p1=p1, p2=p2).numpy()
                e, eph, ehd = port.osc(wf, c["freq"], N, phase=ph0, p1=p1, p2=p2)
                what = "%s at %d" % (name, sr)
                if wf in (0, 1):
                    d = ulp_diff(o, e)
                    print("%s: max %d ULP" % (what, int(d.max())))
                    assert int(d.max()) <= 1, what
                else:
                    assert_bits_equal(o, e, what)
                    assert_bits_equal(bank.output.numpy(), ehd, what + " hold")
                assert_bits_equal(bank.phase.numpy(), eph, what + " phase")
        for name in rc.FM_OSC:
            wf = rc.OSC.index(name)
            bank = mx.maxiOscBank(V)
            o = bank.render(wf, c["fm"], N, per_sample=True).numpy()
            e, eph, _ = port.osc(wf, c["fm"], N, per_sample=True)
            assert_bits_equal(o, e, "%s fm at %d" % (name, sr))
            assert_bits_equal(bank.phase.numpy(), eph, "%s fm phase at %d" % (name, sr))


@pytest.mark.parametrize("V,N", SHAPES)
@pytest.mark.parametrize("sr", RATES)
def test_filter_bank(mx, port, sr, V, N):
    """maxiFilterBank: the five kinds with per-voice parameters bit for bit, output and state, over two carried blocks
    (test_gpu_voice.py:17,31), kinds 0-2 again with the pair-row streams (rw_store 2, test_gpu_voice.py:44); the device-modulated
    lores within the scaled 1e-11 (test_gpu_voice.py:69).  lores / hires cutoffs reach sr (the clamp), bandpass 0.45 sr."""
    c = rc.cases(sr, V, N, 22)
    L = mx.lib()
    with at_rate(sr, port, mx=mx):
        for rw in (None, 2):
            for kind in range(5 if rw is None else 3):
                cu = c["lp"] if kind >= 3 else (c["bp_cutoff"] if kind == 2 else c["cutoff"])
                rs = None if kind >= 3 else (c["bres"] if kind == 2 else c["res"])
                prev = L.mxg_tune(b"rw_store", rw) if rw is not None else None
                try:
                    bank = mx.maxiFilterBank(V)
                    o = np.concatenate([bank.render(kind, D(mx, c["x"][a:b]), cu, rs).numpy() for a, b in halves(N)])
                finally:
                    if rw is not None:
                        L.mxg_tune(b"rw_store", prev)
                e, est = port.filter(kind, c["x"], cu, rs)
                what = "%s at %d, rw_store %s" % (rc.FLT[kind], sr, rw)
                assert_bits_equal(o, e, what)
                assert_bits_equal(bank.state.numpy(), est, what + " state")
                if kind <= 2:
                    assert_bits_equal(mx.banks.filter_coeffs(kind, cu, rs), port.filter_coeffs(kind, cu, rs), what + " coefficients")
        bank = mx.maxiFilterBank(V)
        o = bank.render("lores", D(mx, c["x"]), c["cutoff_mod"], c["res_mod"], cutoff_per_sample=True).numpy()
        e, _ = port.filter(0, c["x"], c["cutoff_mod"], c["res_mod"], cps=True)
        worst = assert_close_scaled(o, e, MOD_FILTER_RTOL, "lores modulated at %d" % sr)
        print("lores modulated at %d: %.3e of the peak" % (sr, worst))


def _set_env(bank, ms):
    bank.setAttack(ms["attack"]); bank.setDecay(ms["decay"]); bank.setSustain(ms["sustain"]); bank.setRelease(ms["release"])


def _env_par(port, ms, V):
    return np.array([[port.env_coeff(0, ms["attack"])], [port.env_coeff(1, ms["decay"])], [ms["sustain"]],
                     [port.env_coeff(2, ms["release"])]]) * np.ones((4, V))


@pytest.mark.parametrize("sr", RATES)
def test_env_bank(mx, port, sr):
    """maxiEnvBank adsr / ar with the setters called after the rate change: the setters' coefficients, the output, the amplitude
    and every flag bit for bit over two carried blocks (test_gpu_voice.py:86)."""
    N = 200
    for V in (65, 130):
        c = rc.cases(sr, V, N, 23)
        with at_rate(sr, port, mx=mx):
            b = mx.maxiEnvBank(len(c["setter_ms"]))
            exp = np.array([[port.env_coeff(w, ms) for ms in c["setter_ms"]] for w in range(4)])
            b.setAttack(c["setter_ms"]); assert_bits_equal(b.par[0], exp[0], "setAttack at %d" % sr)
            b.setDecay(c["setter_ms"]); assert_bits_equal(b.par[1], exp[1], "setDecay at %d" % sr)
            b.setRelease(c["setter_ms"]); assert_bits_equal(b.par[3], exp[2], "setRelease at %d" % sr)
            b.setAttackMS(c["setter_ms"]); assert_bits_equal(b.par[0], exp[3], "setAttackMS at %d" % sr)
            par = _env_par(port, c["env_ms"], V)
            for mode in (0, 1):
                for x, trig in ((c["x"], c["gate"]), (None, c["gate_v"])):
                    bank = mx.maxiEnvBank(V)
                    _set_env(bank, c["env_ms"])
                    bank.holdtime[:] = c["hold"]; bank._dirty = True
                    assert_bits_equal(bank.par, par, "setters")
                    o = np.concatenate([bank.render(mode, None if x is None else D(mx, x[a:b]), trig[a:b], b - a).numpy()
                                        for a, b in halves(N)])
                    e, edst, eist = port.env(mode, x, trig, par, c["hold"])
                    what = "env mode %d at %d, V %d" % (mode, sr, V)
                    assert_bits_equal(o, e, what)
                    assert_bits_equal(bank.dstate.numpy(), edst, what + " amplitude / output")
                    assert np.array_equal(bank.istate.numpy(), eist), what + " flags"
                    assert e.max() > 0.4


def _voice_bank(mx, c, V):
    vb = mx.maxiVoiceBank(V)
    _set_env(vb.env, c["env_ms"])
    vb.env.holdtime[:] = c["hold"]; vb.env._dirty = True
    return vb


@pytest.mark.parametrize("V", [65, 130])
@pytest.mark.parametrize("sr", RATES)
def test_fused_voice(mx, port, sr, V):
    """mxg_voice_render: mode A bit for bit with every state array (test_gpu_voice.py::test_voice_golden_mode_a_bit_exact), mode B
    within the scaled 1e-11 with envelope and oscillator state bit-exact (::test_voice_golden_mode_b_tolerance);
    mxg_voice_render_mix: the per-voice block as mxg_voice_render's, the mix within conftest.mix_tol
    (::test_voice_render_mix...).  Two carried blocks; frequencies and cutoffs scale with the rate."""
    N = 200
    c = rc.cases(sr, V, N, 24)
    with at_rate(sr, port, mx=mx):
        par = _env_par(port, c["env_ms"], V)
        for mode, cu in ((0, c["vcutoff"]), (1, c["cutoff_b"])):
            vb = _voice_bank(mx, c, V)
            o = np.concatenate([vb.render(mode, c["vfreq"], cu, c["vres"], c["gate"][a:b], b - a).numpy() for a, b in halves(N)])
            e, eost, efst, edst, eist = port.voice(mode, c["vfreq"], cu, c["vres"], c["gate"], par, c["hold"])
            what = "voice mode %d at %d" % (mode, sr)
            assert np.isfinite(e).all() and np.abs(e).max() > 0.05
            assert_bits_equal(vb.env.dstate.numpy(), edst, what + " envelope")
            assert np.array_equal(vb.env.istate.numpy(), eist), what + " flags"
            assert_bits_equal(vb.osc_state.numpy(), eost, what + " osc state")
            if mode == 0:
                assert_bits_equal(o, e, what)
                assert_bits_equal(vb.flt_state.numpy(), efst, what + " filter state")
            else:
                worst = assert_close_scaled(o, e, MOD_FILTER_RTOL, what)
                print("%s: %.3e of the peak" % (what, worst))
        vb = _voice_bank(mx, c, V)
        outs, mixes = [], []
        for a, b in halves(N):
            o, m = vb.render_mix(0, c["vfreq"], c["vcutoff"], c["vres"], c["gate"][a:b], c["pan"], b - a)
            outs.append(o.numpy()); mixes.append(m.numpy())
        e = port.voice(0, c["vfreq"], c["vcutoff"], c["vres"], c["gate"], par, c["hold"])
        assert_bits_equal(np.concatenate(outs), e[0], "mixdown form, mode A, at %d" % sr)
        assert_bits_equal(vb.flt_state.numpy(), e[2], "mixdown form filter state")
        em = port.mix_stereo(e[0], c["pan"])
        assert np.abs(np.concatenate(mixes) - em).max() <= mix_tol(V, np.abs(e[0]).max(), sums=em)


@pytest.mark.parametrize("sr", RATES)
def test_filter2_banks(mx, port, sr):
    """maxiSVFBank / maxiBiquadBank: host-libm coefficients, outputs and state bit for bit over two carried blocks
    (test_gpu_filter2.py::test_svf, ::test_biquad, all seven biquad types in one bank as ::test_biquad_mixed_types_and_errors)."""
    N = 200
    for V in (65, 130):
        c = rc.cases(sr, V, N, 25)
        with at_rate(sr, port, mx=mx):
            cutoff, res, mix = c["svf"][0], c["svf"][1], c["svf"][2:]
            bank = mx.maxiSVFBank(V)
            _, _, c0 = port.filter2(1, c["x"][:1], np.stack([np.full(V, 1000.0), np.ones(V), *mix]))
            assert_bits_equal(bank.coefficients(), c0, "ctor setParams(1000, 1) at %d" % sr)
            bank.setCutoff(cutoff); bank.setResonance(res)
            o = np.concatenate([bank.play(D(mx, c["x"][a:b]), *mix).numpy() for a, b in halves(N)])
            e, st, coef = port.filter2(1, c["x"], c["svf"])
            assert_bits_equal(bank.coefficients(), coef, "svf g1..g4, k at %d" % sr)
            assert_bits_equal(o, e, "svf at %d" % sr)
            assert_bits_equal(bank.state.numpy(), st, "svf v0z, v1, v2 at %d" % sr)
            t, cu, q, gain = c["biquad"]
            bank = mx.maxiBiquadBank(V)
            bank.set(t.astype(np.int32), cu, q, gain)
            o = np.concatenate([bank.play(D(mx, c["x"][a:b])).numpy() for a, b in halves(N)])
            e, st, coef = port.filter2(2, c["x"], c["biquad"])
            assert_bits_equal(bank.host_coef, coef, "biquad a0, a1, a2, b1, b2 at %d" % sr)
            assert_bits_equal(o, e, "biquad at %d" % sr)
            assert_bits_equal(bank.state.numpy(), st, "biquad v[0..2] at %d" % sr)


@pytest.mark.parametrize("sr", RATES)
def test_envgen_bank(mx, port, sr):
    """maxiEnvGenBank with loop and retrigger on and off: the stage table (ms -> samples at the rate), the output and both state
    arrays bit for bit over two carried blocks (test_gpu_envgen.py::test_envgen_per_voice_triggers, curve == 1)."""
    N = 200
    lv, tm, cv = rc.ENVGEN
    for V in (65, 130):
        c = rc.cases(sr, V, N, 26)
        trig = c["envgen_trig"]
        with at_rate(sr, port, mx=mx):
            for loop in (0, 1):
                for retrig in (0, 1):
                    bank = mx.maxiEnvGenBank(V)
                    assert bank.setup(lv, tm, cv, bool(loop), bool(retrig))
                    o = np.concatenate([bank.play(trig[a:b]).numpy() for a, b in halves(N)])
                    e, d, i, stages = port.envgen(trig, lv, tm, cv, loop, retrig)
                    what = "envgen loop %d retrigger %d at %d" % (loop, retrig, sr)
                    assert_bits_equal(bank.host_stages, stages, what + " stage table")
                    assert_bits_equal(o, e, what)
                    assert np.array_equal(bank.istate.numpy(), i), what + " phase / state / counters"
                    assert_bits_equal(bank.dstate.numpy(), d, what + " envval, currentlevel, detectors")
                    assert e.max() == 1.0


def _sample_family(port, bank, c, N, my, what):
    runs = [("playAtSpeed", 4, dict(a=c["speed"])), ("playOnceAtSpeed", 5, dict(a=c["speed"])),
            ("playUntilAtSpeed", 6, dict(a=c["speed"], end=c["end"]))]
    for name, mode, kw in runs:
        bank.position.upload(c["pos0"])
        o = np.concatenate([bank.render(name, b - a, **kw).numpy() for a, b in halves(N)])
        e, ep = port.sample(mode, c["samples"], N, c["pos0"], mySampleRate=my, **kw)
        assert_bits_equal(o, e, "%s %s" % (name, what))
        assert_bits_equal(bank.position.numpy(), ep, "%s position %s" % (name, what))
    bank.position.upload(c["pos0"])
    o = bank.playAtSpeed(c["speed_mod"], N, per_sample=True).numpy()
    e, ep = port.sample(4, c["samples"], N, c["pos0"], a=c["speed_mod"], aps=True, mySampleRate=my)
    assert_bits_equal(o, e, "playAtSpeed, per-sample speed, " + what)
    assert_bits_equal(bank.position.numpy(), ep, "per-sample speed position " + what)


@pytest.mark.parametrize("sr,my", rc.QUOTIENT_PAIRS)
def test_sample_bank_at_speed(mx, port, sr, my):
    """maxiSampleBank playAtSpeed / playOnceAtSpeed / playUntilAtSpeed through setSampleAndRate, block-constant and per-sample speed:
    output and position bit for bit (test_gpu_sample.py:63, ::test_sample_vs_oracle_large).  The step is speed / (sr / mySampleRate)
    with the integer quotient: 2, 1, 1, 2, 1, 1 for these pairs."""
    N = 200
    for V in (65, 130):
        c = rc.cases(sr, V, N, 27)
        with at_rate(sr, port, mx=mx):
            bank = mx.maxiSampleBank(V)
            assert bank.mySampleRate == sr                   # the constructor takes maxiSettings::sampleRate
            bank.setSampleAndRate(c["samples"], my)
            _sample_family(port, bank, c, N, my, "at %d / %d, V %d" % (sr, my, V))


@pytest.mark.parametrize("sr", [96000, 48000])
def test_sample_bank_set_sample_resets_rate(mx, port, sr):
    """A plain setSample() leaves mySampleRate at 44100 whatever the setting (H:670-678): quotient 2 at 96 kHz, 1 at 48 kHz."""
    V, N = 65, 200
    c = rc.cases(sr, V, N, 28)
    with at_rate(sr, port, mx=mx):
        bank = mx.maxiSampleBank(V)
        bank.setSample(c["samples"])
        assert bank.mySampleRate == 44100
        _sample_family(port, bank, c, N, 44100, "after setSample at %d" % sr)


@pytest.mark.parametrize("voices,NS", [(32, 3), (3, 22)])
@pytest.mark.parametrize("sr", RATES)
def test_sampler(mx, port, sr, voices, NS):
    """mxg_sampler_render (+ mxg_sampler_freq_host: pitch ratio x sampleRate / length): per-slot outputs, the mix and the slot
    state bit for bit over two carried blocks (test_gpu_sampler.py::test_sampler_render_vs_oracle)."""
    import ctypes
    N = 100
    s = rc.sampler_case(sr, voices, NS, 29)
    V = NS * voices
    L = mx.lib()
    port.L.mxo_sampler_frequency.restype = ctypes.c_double
    port.L.mxo_sampler_frequency.argtypes = [ctypes.c_double, ctypes.c_size_t]
    with at_rate(sr, port, mx=mx):
        sb = mx.maxiSampleBank(1)
        sb.setSample(s["smp"])
        freq = np.zeros(V)
        assert L.mxg_sampler_freq_host(V, s["pitch"].ctypes.data, s["smp"].size, freq.ctypes.data) == 0
        assert_bits_equal(freq, np.array([port.L.mxo_sampler_frequency(p, s["smp"].size) for p in s["pitch"]]), "freq at %d" % sr)
        dpos, dtrig, dout = D(mx, np.zeros(V)), D(mx, s["trig"]), D(mx, np.zeros(V))
        ddst, dist = D(mx, np.zeros((2, V))), D(mx, np.zeros((6, V), np.int64))
        dfreq, dgain, dpar, dhold = D(mx, freq), D(mx, s["gain"]), D(mx, s["par"]), D(mx, s["hold"])
        e = None
        for blk in range(2):
            mix, outputs = mx.DeviceBuffer((N, NS)), mx.DeviceBuffer((N, V))
            assert L.mxg_sampler_render(V, N, voices, 1, sb.d_samples, s["smp"].size, dfreq.ptr, dgain.ptr, dpar.ptr, dhold.ptr,
                                        dpos.ptr, dtrig.ptr, dout.ptr, ddst.ptr, dist.ptr, mix.ptr, outputs.ptr, None) == 0
            args = (voices, s["smp"], N, s["pitch"], s["gain"], s["par"], s["hold"])
            e = port.sampler(*args, np.zeros(V), s["trig"], True) if e is None else \
                port.sampler(*args, e[2], e[3], True, e[4], e[5], e[6])
            what = "sampler at %d, block %d" % (sr, blk)
            assert_bits_equal(outputs.numpy(), e[1], what + " outputs")
            assert_bits_equal(mix.numpy(), e[0], what + " mix")
            assert_bits_equal(dpos.numpy(), e[2], what + " position")
            assert np.array_equal(dtrig.numpy(), e[3]), what + " trigger"
            assert_bits_equal(dout.numpy(), e[4], what + " outputs hold")
            assert_bits_equal(ddst.numpy(), e[5], what + " envelope")
            assert np.array_equal(dist.numpy(), e[6]), what + " flags"
        assert np.abs(e[0]).max() > 0.01


@pytest.mark.parametrize("V,N", SHAPES[:2])
@pytest.mark.parametrize("sr", RATES)
def test_per_voice_tables(mx, port, sr, V, N):
    """mxg_osc_render_tables against port.osc_tables: output, phase and the output member bit for bit over two carried blocks
    (test_gpu_osctab.py::test_tables_bank_against_the_oracle)."""
    c = rc.cases(sr, V, N, 30)
    with at_rate(sr, port, mx=mx):
        bank = mx.maxiOscBank(V)
        d_tabs = D(mx, c["tables"])
        o = np.concatenate([bank.sinebuf_tables(c["freq"], d_tabs, b - a)[0].numpy() for a, b in halves(N)])
        e, eph, ehd = port.osc_tables(c["freq"], c["tables"], N)
        assert_bits_equal(o, e, "per-voice tables at %d" % sr)
        assert_bits_equal(bank.phase.numpy(), eph, "phase")
        assert_bits_equal(bank.output.numpy(), ehd, "output member")


@pytest.mark.parametrize("sr", RATES)
def test_mfcc_and_centroid(mx, port, sr):
    """maxiMFCC set up under the rate: the plan's mel / DCT tables bit for bit the oracle's (host libm,
    test_spectral_cpu.py::test_product_mfcc_host_tables); mfcc() of 8 frames on the exact route with its bands
    (test_gpu_spectral.py:119) and on the default fused route, which takes the matrix pipe when only coefficients are asked for
    (::test_fused_automatic_form), both at the existing 1e-12; the spectral centroid bit for bit (test_gpu_spectral.py:499)."""
    nfr = 8
    sig, mags = rc.spectral_case(sr, nfr, 31)
    cfg = rc.mfcc_args(sr)
    with at_rate(sr, port, mx=mx):
        m = mx.maxiMFCC()
        m.setup(*cfg)
        W, Dt, used = m.tables()
        We, De = port.mfcc_tables(*cfg)
        assert_bits_equal(W, We, "mel filter bank at %d" % sr)
        assert_bits_equal(Dt, De, "DCT matrix at %d" % sr)
        assert used == np.nonzero(We.reshape(cfg[0], cfg[1]).any(axis=1))[0].max() + 1
        emel, emf = port.mfcc(mags, *cfg[1:])
        out = m.mfcc(D(mx, mags), want_bands=True).numpy()
        bands = m.melBands.numpy()
        scale = np.abs(emel).max()
        print("mfcc at %d: bands %.3e, coefficients %.3e of the scale" % (sr, np.abs(bands - emel).max() / scale,
                                                                          np.abs(out - emf).max() / scale))
        assert np.abs(bands - emel).max() <= MFCC_RTOL * scale
        assert np.abs(out - emf).max() <= MFCC_RTOL * scale
        assert np.array_equal(bands == 0.0, emel == 0.0)
        f = mx.maxiFFT()
        f.setup(1024, 1024, 1024)
        d = D(mx, sig.reshape(-1))
        fused = m.mfcc_of_frames(f, d.ptr, nfr).numpy()
        e = port.fft_stream(sig.reshape(-1), 1024, 1024, 1024, want=("mags",))["mags"]
        emel, emf = port.mfcc(e, *cfg[1:])
        assert np.abs(fused - emf).max() <= MFCC_RTOL * max(np.abs(emel).max(), 1.0)
        for fftSize in (1024, 64):
            f = mx.maxiFFT()
            f.setup(fftSize, fftSize // 2, fftSize)
            mm = np.ascontiguousarray(mags[:, :fftSize // 2])
            _, ecen = port.fft_features(mm, fftSize)
            assert_bits_equal(f.spectralCentroid(D(mx, mm)).numpy(), ecen, "centroid, fftSize %d at %d" % (fftSize, sr))
            assert ecen[2] == 0 and ecen.max() > 0


@pytest.fixture(params=[(1, 1), (1, 0), (0, 1)], ids=["tiles", "walk", "serial"])
def chunked(mx, request):
    """As test_gpu_grains.py:26: the scheduler pre-pass + tile renders (K8a + K8c / K8d, the default), the (stream, chunk) walk K8b
    in place of K8d, and the serial K8."""
    prev = mx.lib().mxg_tune(b"grain_chunked", request.param[0])
    prev2 = mx.lib().mxg_tune(b"grain_line", request.param[1])
    yield request.param[0]
    mx.lib().mxg_tune(b"grain_chunked", prev)
    mx.lib().mxg_tune(b"grain_line", prev2)


# (sr, mySampleRate, grainLength, overlaps, S, T per call, calls)
GRAIN_CASES = {
    "unit_96k": (96000, 96000, 0.05, 4, 65, 6000, 1),       # inc == 1: the K8c route
    "inc_96k_44k": (96000, 44100, 0.05, 3, 65, 6000, 1),    # inc != 1: the K8d route
    "trunc_7919": (7919, 7919, 0.05, 4, 65, 3000, 1),       # sampleDur = 395.95 truncates
    "long_96k": (96000, 96000, 0.4, 4, 5, 22500, 2),        # sampleDur 38400 >= 2^15: no tile route, grains carried in are > 32000
}


@pytest.mark.parametrize("name", list(GRAIN_CASES))
def test_granular_banks(mx, port, chunked, name):
    """maxiTimeStretchBank, maxiStretchBank and maxiPitchShiftBank under the rate: output, stream state and grain state bit for bit
    and no error where the port reports none (test_gpu_grains.py::test_fast_scheduler_random_rates, ::test_pitch_shift).  The long
    grain is 38 400 samples: K8c packs durations into 15 bits and K8d carries 16-bit ages, so both must be refused and the walk must
    give the reference's bits, over two carried calls whose second starts with grains older than 32 000 samples."""
    sr, my, gl, ov, S, T, calls = GRAIN_CASES[name]
    g = rc.grain_case(sr, my, gl, ov, S, T * calls, 32)
    L = mx.lib()
    with at_rate(sr, port, mx=mx):
        sb = mx.maxiSampleBank(1)
        sb.setSampleAndRate(g["smp"], my)
        for mode in (0, 1, 3):
            bank = (mx.maxiTimeStretchBank, mx.maxiStretchBank, None, mx.maxiPitchShiftBank)[mode](S, sb, "hann")
            bank.setPosition(g["pos0"])
            st, gst = bank.state.numpy(), None
            assert_bits_equal(st[0], np.clip(g["pos0"] * g["smp"].size, 0, g["smp"].size - 1), "setPosition")
            outs, exps = [], []
            for _ in range(calls):
                if mode == 0:
                    o = bank.play(g["speed"], gl, ov, T, posMod=g["pm"], rnd=g["rnd"])
                elif mode == 1:
                    o = bank.play(g["speed"], g["ts"], gl, ov, T, posMod=g["pm"], rnd=g["rnd"])
                else:
                    o = bank.play(g["speed"], gl, ov, T, posMod=g["pm"])
                outs.append(o.numpy())                       # (a deferred kernel error would be raised by this download)
                e, st, gst, rc_port = rc.granular(port, mode, g, T, my, gl, ov, st=st, gst=gst)
                exps.append(e)
                assert rc_port == 0 and L.mxg_last_async_error() == 0
            what = "%s mode %d" % (name, mode)
            assert_bits_equal(np.concatenate(outs), np.concatenate(exps), what)
            assert_bits_equal(bank.state.numpy(), st, what + " stream state")
            assert_bits_equal(bank.grains.numpy(), gst, what + " grains")
            assert np.abs(exps[-1]).max() > 0.05
            if name == "long_96k":
                assert (gst[3] == 38400).any() and gst[2].max() > 32000   # grains older than 32 000 samples are alive at the end
            bank.close()


@pytest.mark.parametrize("V", [65, 130])
def test_rate_change_mid_stream(mx, port, V):
    """71 samples at 44100, then maxiSettings::setup(48000) and 71 more on the SAME banks with their carried state: sinebuf, saw,
    lores, maxiSVF and the mode A fused voice, bit for bit against the port called the same way (its calls are stateless: the
    carried state goes in, the current setting applies).  A rate cached at construction or in a launch plan would show here.  The
    coefficients of lores and maxiSVF are functions of the rate: the setters run again after the change, as a reference program that
    calls lores(x, cutoff, res) / setCutoff() per block does."""
    N = 71
    c = rc.cases(44100, V, 2 * N, 33)
    osc = {wf: mx.maxiOscBank(V) for wf in (8, 3)}
    flt, svf, vb = mx.maxiFilterBank(V), mx.maxiSVFBank(V), None
    cu, rs = np.minimum(c["cutoff"], 20000.0), c["res"]
    exp = {}
    got = {k: [] for k in ("sinebuf", "saw", "lores", "svf", "voice")}
    for blk, sr in enumerate((44100, 48000)):
        x = c["x"][blk * N:(blk + 1) * N]
        gate = c["gate"][blk * N:(blk + 1) * N]
        with at_rate(sr, port, mx=mx):
            for wf, name in ((8, "sinebuf"), (3, "saw")):
                got[name].append(osc[wf].render(wf, c["freq"], N).numpy())
                p = exp.get(name)
                exp[name] = port.osc(wf, c["freq"], N, phase=None if p is None else p[1], hold=None if p is None else p[2])
                assert_bits_equal(got[name][-1], exp[name][0], "%s block %d at %d" % (name, blk, sr))
                assert_bits_equal(osc[wf].phase.numpy(), exp[name][1], name + " phase")
            got["lores"].append(flt.render("lores", D(mx, x), cu, rs).numpy())
            p = exp.get("lores")
            exp["lores"] = port.filter(0, x, cu, rs, state=None if p is None else p[1])
            assert_bits_equal(got["lores"][-1], exp["lores"][0], "lores block %d at %d" % (blk, sr))
            assert_bits_equal(flt.state.numpy(), exp["lores"][1], "lores state")
            svf.setCutoff(c["svf"][0]); svf.setResonance(c["svf"][1])
            got["svf"].append(svf.play(D(mx, x), *c["svf"][2:]).numpy())
            p = exp.get("svf")
            exp["svf"] = port.filter2(1, x, c["svf"], st=None if p is None else p[1])
            assert_bits_equal(svf.coefficients(), exp["svf"][2], "svf coefficients at %d" % sr)
            assert_bits_equal(got["svf"][-1], exp["svf"][0], "svf block %d at %d" % (blk, sr))
            assert_bits_equal(svf.state.numpy(), exp["svf"][1], "svf state")
            if vb is None:
                vb = _voice_bank(mx, c, V)      # (the envelope's coefficients are set once, at 44100, on both sides)
                par = vb.env.par.copy()
            got["voice"].append(vb.render(0, c["vfreq"], c["vcutoff"], c["vres"], gate, N).numpy())
            p = exp.get("voice")
            exp["voice"] = port.voice(0, c["vfreq"], c["vcutoff"], c["vres"], gate, par, c["hold"],
                                      *(() if p is None else (p[1], p[2], p[3], p[4])))
            assert_bits_equal(got["voice"][-1], exp["voice"][0], "voice block %d at %d" % (blk, sr))
            assert_bits_equal(vb.flt_state.numpy(), exp["voice"][2], "voice filter state")
            assert_bits_equal(vb.osc_state.numpy(), exp["voice"][1], "voice osc state")
            assert np.array_equal(vb.env.istate.numpy(), exp["voice"][4])


def test_zz_default_rate_restored(mx, port):
    """Run last in this file: mxg_sample_rate() is 44100 again, and the bank and the port render at it."""
    L = mx.lib()
    assert L.mxg_sample_rate() == 44100 and mx.maxiSettings.sampleRate == 44100
    out, _, _ = port.osc(3, np.array([440.0]), 4)
    assert_bits_equal(mx.maxiOscBank(1).saw(np.array([440.0]), 4).numpy(), out, "saw(440) at the default rate")
