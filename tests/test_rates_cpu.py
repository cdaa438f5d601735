"""CPU tests (-m "not gpu"): the plain-C oracle at sample rates other than 44.1 kHz -- (a) against the compiled reference where
oracle/_ref is present, on the inputs of tests/rates_cases.py, bit for bit; (b) against tests/golden/rates.npz, the reference's
outputs for one small case per family and rate (oracle/gen_golden_rates.py), which pins the port where _ref is absent.
The core families only: the later families' host models take an explicit rate."""
import numpy as np
import pytest

import rates_cases as rc
from conftest import assert_bits_equal

CPU_RATES = rc.RATES + (192000,)
V, N = 13, 400


def _same(a, b, what):
    """Two result tuples of one Oracle method: float arrays bit for bit, integer arrays and return codes equal."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray) and x.dtype.kind == "f":
            assert_bits_equal(x, y, "%s item %d" % (what, i))
        else:
            assert np.array_equal(x, y), "%s item %d" % (what, i)


# ---- (a) port against the compiled reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", CPU_RATES)
def test_osc_port_vs_reference(port, ref, sr):
    c = rc.cases(sr, V, N, 1)
    with rc.at_rate(sr, port, ref):
        for wf, name in enumerate(rc.OSC):
            p1, p2 = (c["duty"], None) if name == "pulse" else (c["p1"], c["p2"])
            ph0 = c["phase0_tab"] if wf in (8, 9) else c["phase0"]
            for ph in (None, ph0):
                _same(port.osc(wf, c["freq"], N, phase=ph, p1=p1, p2=p2), ref.osc(wf, c["freq"], N, phase=ph, p1=p1, p2=p2),
                      "%s at %d" % (name, sr))
        for name in rc.FM_OSC:
            wf = rc.OSC.index(name)
            _same(port.osc(wf, c["fm"], N, per_sample=True), ref.osc(wf, c["fm"], N, per_sample=True), "%s fm at %d" % (name, sr))


@pytest.mark.parametrize("sr", CPU_RATES)
def test_filter_port_vs_reference(port, ref, sr):
    c = rc.cases(sr, V, N, 2)
    with rc.at_rate(sr, port, ref):
        for kind in range(3):
            cu, rs = (c["bp_cutoff"], c["bres"]) if kind == 2 else (c["cutoff"], c["res"])
            _same(port.filter(kind, c["x"], cu, rs), ref.filter(kind, c["x"], cu, rs), "%s at %d" % (rc.FLT[kind], sr))
            assert_bits_equal(port.filter_coeffs(kind, cu, rs), ref.filter_coeffs(kind, cu, rs), "%s coeffs at %d" % (rc.FLT[kind], sr))
        _same(port.filter(0, c["x"], c["cutoff_mod"], c["res_mod"], cps=True),
              ref.filter(0, c["x"], c["cutoff_mod"], c["res_mod"], cps=True), "lores per-sample cutoff at %d" % sr)


def _env_par(o, c):
    m = c["env_ms"]
    return np.array([[o.env_coeff(0, m["attack"])], [o.env_coeff(1, m["decay"])], [m["sustain"]], [o.env_coeff(2, m["release"])]]) \
        * np.ones((4, V))


@pytest.mark.parametrize("sr", CPU_RATES)
def test_env_voice_port_vs_reference(port, ref, sr):
    c = rc.cases(sr, V, N, 3)
    with rc.at_rate(sr, port, ref):
        a = np.array([[port.env_coeff(w, ms) for ms in c["setter_ms"]] for w in range(4)])
        b = np.array([[ref.env_coeff(w, ms) for ms in c["setter_ms"]] for w in range(4)])
        assert_bits_equal(a, b, "setters at %d" % sr)
        par = _env_par(port, c)
        assert_bits_equal(par, _env_par(ref, c), "adsr parameters")
        for mode in (0, 1):
            _same(port.env(mode, c["x"], c["gate"], par, c["hold"]), ref.env(mode, c["x"], c["gate"], par, c["hold"]),
                  "env mode %d at %d" % (mode, sr))
            _same(port.env(mode, None, c["gate_v"], par, c["hold"]), ref.env(mode, None, c["gate_v"], par, c["hold"]),
                  "env mode %d, per-voice gates, at %d" % (mode, sr))
        for mode, cu in ((0, c["vcutoff"]), (1, c["cutoff_b"])):
            _same(port.voice(mode, c["vfreq"], cu, c["vres"], c["gate"], par, c["hold"]),
                  ref.voice(mode, c["vfreq"], cu, c["vres"], c["gate"], par, c["hold"]), "voice mode %d at %d" % (mode, sr))


@pytest.mark.parametrize("sr", CPU_RATES)
def test_filter2_envgen_port_vs_reference(port, ref, sr):
    c = rc.cases(sr, V, N, 4)
    lv, tm, cv = rc.ENVGEN
    with rc.at_rate(sr, port, ref):
        for kind, par in ((1, c["svf"]), (2, c["biquad"])):
            _same(port.filter2(kind, c["x"], par), ref.filter2(kind, c["x"], par), "filter2 kind %d at %d" % (kind, sr))
        for loop in (0, 1):
            for retrig in (0, 1):
                _same(port.envgen(c["envgen_trig"], lv, tm, cv, loop, retrig), ref.envgen(c["envgen_trig"], lv, tm, cv, loop, retrig),
                      "envgen loop %d retrigger %d at %d" % (loop, retrig, sr))


@pytest.mark.parametrize("sr,my", rc.QUOTIENT_PAIRS)
def test_sample_port_vs_reference(port, ref, sr, my):
    c = rc.cases(sr, V, N, 5)
    with rc.at_rate(sr, port, ref):
        for mode in (4, 5, 6):
            kw = dict(a=c["speed"], end=c["end"], mySampleRate=my)
            _same(port.sample(mode, c["samples"], N, c["pos0"], **kw), ref.sample(mode, c["samples"], N, c["pos0"], **kw),
                  "sample mode %d at %d / %d" % (mode, sr, my))
        kw = dict(a=c["speed_mod"], aps=True, mySampleRate=my)
        _same(port.sample(4, c["samples"], N, c["pos0"], **kw), ref.sample(4, c["samples"], N, c["pos0"], **kw),
              "playAtSpeed, per-sample speed, at %d / %d" % (sr, my))


@pytest.mark.parametrize("sr", CPU_RATES)
def test_sampler_spectral_port_vs_reference(port, ref, sr):
    voices, NS = 4, 3
    s = rc.sampler_case(sr, voices, NS, 6)
    _, mags = rc.spectral_case(sr, 8, 7)
    nb, nf, nc, lo, hi = rc.mfcc_args(sr)
    with rc.at_rate(sr, port, ref):
        args = (voices, s["smp"], N, s["pitch"], s["gain"], s["par"], s["hold"], np.zeros(NS * voices), s["trig"], True)
        _same(port.sampler(*args), ref.sampler(*args), "sampler at %d" % sr)
        _same(port.mfcc_tables(nb, nf, nc, lo, hi), ref.mfcc_tables(nb, nf, nc, lo, hi), "mfcc tables at %d" % sr)
        _same(port.mfcc(mags, nf, nc, lo, hi), ref.mfcc(mags, nf, nc, lo, hi), "mfcc at %d" % sr)
        for fftSize in (1024, 64):
            m = mags[:, :fftSize // 2]
            _same(port.fft_features(m, fftSize), ref.fft_features(m, fftSize), "fft features at %d" % sr)


@pytest.mark.parametrize("sr,my,gl,ov", rc.GRAIN_SETTINGS)
@pytest.mark.parametrize("mode", range(4))
def test_granular_port_vs_reference(port, ref, mode, sr, my, gl, ov):
    S = 3
    T = int(2.6 * gl * my)          # the first grains finish, several are alive at the end
    g = rc.grain_case(sr, my, gl, ov, S, 2 * T, 8)
    with rc.at_rate(sr, port, ref):
        a1, b1 = rc.granular(port, mode, g, T, my, gl, ov), rc.granular(ref, mode, g, T, my, gl, ov)
        _same(a1, b1, "granular mode %d at %d" % (mode, sr))
        if mode != 2:   # a second block with carried grains
            _same(rc.granular(port, mode, g, T, my, gl, ov, st=a1[1], gst=a1[2]), rc.granular(ref, mode, g, T, my, gl, ov, st=b1[1], gst=b1[2]),
                  "granular mode %d at %d, carried" % (mode, sr))
    assert a1[3] == 0 and np.abs(a1[0]).max() > 0.05


# ---- (b) port against the committed reference outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("sr", CPU_RATES)
def test_port_vs_golden_rates(port, golden, sr):
    g = golden("rates.npz")
    got = rc.golden_run(port, sr)
    keys = [k for k in g.files if k.startswith("sr%d/" % sr)]
    assert sorted(keys) == sorted("sr%d/%s" % (sr, k) for k in got), "the fixture holds exactly the cases of golden_run()"
    for k, v in got.items():
        e = g["sr%d/%s" % (sr, k)]
        if v.dtype.kind == "f":
            assert_bits_equal(v, e, "%s at %d" % (k, sr))
        else:
            assert np.array_equal(v, e), "%s at %d" % (k, sr)


def test_zz_default_rate_restored(port):
    """Run last in this file: no test above may leak its rate (the fixtures are session-wide).  The 440 Hz sinewave's first four
    samples at 44.1 kHz, as test_oracle_golden.py::test_kat_sinewave_440 has them."""
    out, _, _ = port.osc(0, np.array([440.0]), 4)
    assert [repr(float(x)) for x in out[:, 0]] == ["0.0", "0.06264832417874368", "0.1250505236945281", "0.18696144082725336"]
