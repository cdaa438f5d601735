"""Inputs of the sample-rate tests (tests/test_rates_cpu.py, tests/test_gpu_rates.py) and of oracle/gen_golden_rates.py, which runs the
reference over them for tests/golden/rates.npz.  Everything here is a function of maxiSettings::sampleRate: frequencies and cutoffs
scale with the rate, envelope and stage times are milliseconds short enough for every stage to complete within a block at 96 kHz,
and every input stays where the reference is defined (wavetable oscillators within [0, sr/2], *AtSpeed players with
mySampleRate <= sampleRate, grains shorter than sr/2 samples)."""
import contextlib

import numpy as np

# 48000: the common rate.  96000: the integer quotient sr / 44100 is 2, and grains longer than 2^15 samples exist.  22050: below the
# default.  7919: prime -- sr / 2.0, ms -> samples and sr / fftSize all truncate.
RATES = (48000, 96000, 22050, 7919)
DEFAULT = (44100, 2, 1024)

OSC = ["sinewave", "coswave", "phasor", "saw", "triangle", "square", "pulse", "impulse", "sinebuf", "sinebuf4", "sawn",
       "phasorBetween"]
FM_OSC = ("sinebuf", "saw", "sawn")
FLT = ["lores", "hires", "bandpass", "lopass", "hipass"]

# (sampleRate, mySampleRate) of the *AtSpeed players: the step is speed / (sampleRate / mySampleRate) with the INTEGER quotient
# (src/maximilian.cpp:1070) -- 2, 1, 1, 2, 1, 1 here; mySampleRate > sampleRate would divide by zero in the reference
QUOTIENT_PAIRS = ((96000, 44100), (48000, 44100), (22050, 22050), (22050, 11025), (7919, 7919), (96000, 96000))

# (sampleRate, mySampleRate, grainLength, overlaps): sampleDur = 38400, 57600 (>= 2^15), 4800, 2205, 395 (truncated), 1008
GRAIN_SETTINGS = ((96000, 96000, 0.4, 4), (192000, 192000, 0.3, 4), (96000, 96000, 0.05, 4), (96000, 44100, 0.05, 3),
                  (7919, 7919, 0.05, 4), (48000, 48000, 0.021, 5))

HOLD = -46692.0   # maxiEnvGen's HOLD marker
ENVGEN = ([0, 1, 0.4, 0.4, 0], [0.5, 0.3, HOLD, 0.5], [1, 1, 1, 1])   # levels, times (ms), curves of an ADSR


@contextlib.contextmanager
def at_rate(sr, *oracles, mx=None):
    """maxiSettings::setup(sr, 2, 1024) on every oracle (and on the product when `mx` is given) for the body, the default
    44100 / 2 / 1024 again afterwards whatever happens: the port / ref / mx fixtures are shared by the whole session."""
    try:
        for o in oracles:
            o.settings(int(sr), 2, 1024)
        if mx is not None:
            mx.maxiSettings.setup(int(sr), 2, 1024)
        yield
    finally:
        for o in oracles:
            o.settings(*DEFAULT)
        if mx is not None:
            mx.maxiSettings.setup(*DEFAULT)


def cases(sr, V, N, seed):
    """The inputs of every per-voice family for a bank of V voices and a block of N samples at rate sr (V >= 5)."""
    rng = np.random.default_rng([int(seed), int(sr), V, N])
    sr = float(sr)
    c = {}
    # oscillators: every waveform sees 0, sr/4, sr/2 and sr/2 less one ULP-ish step
    c["freq"] = np.concatenate([[0.0, sr / 4, sr / 2, sr / 2 - 1e-9], rng.uniform(0.05, sr / 2, V - 4)])
    c["fm"] = np.clip(c["freq"][None, :] * (1.0 + 0.25 * rng.uniform(-1, 1, (N, V))), 0.0, sr / 2)
    c["p2"] = rng.uniform(0.3, 1.0, V)
    c["p1"] = c["p2"] * rng.uniform(0.0, 0.9, V)
    c["duty"] = rng.uniform(-0.1, 1.1, V)
    c["phase0"] = rng.uniform(0, 1, V)          # phasor-family oscillators
    c["phase0_tab"] = rng.uniform(0, 500, V)    # sinebuf / sinebuf4: the phase is a table index
    c["tables"] = rng.uniform(-1, 1, (V, 514))  # per-voice wavetables of the extension
    # maxiFilter: lores / hires up to sr INCLUSIVE (the clamp, where the reference's r is 0 / 0), bandpass up to 0.45 sr
    c["x"] = rng.uniform(-1, 1, (N, V))
    c["cutoff"] = np.concatenate([[5.0, sr, 0.5 * sr, 0.999 * sr], rng.uniform(1.0, sr, V - 4)])
    c["res"] = np.concatenate([[0.5, 1.0, 30.0, 2.0], rng.uniform(0.2, 25, V - 4)])
    c["bp_cutoff"] = np.concatenate([[0.45 * sr], rng.uniform(1.0, 0.45 * sr, V - 1)])
    c["bres"] = rng.uniform(0.01, 1.3, V)
    c["lp"] = rng.uniform(0.0, 1.0, V)
    base = rng.uniform(0.0005 * sr, 0.15 * sr, V)
    c["cutoff_mod"] = base[None, :] * (1.0 + 0.5 * rng.uniform(-1, 1, (N, V)))   # per-sample cutoff, <= 0.225 sr
    c["res_mod"] = rng.uniform(1, 8, V)
    # maxiEnv: setter arguments in ms (the setters run AFTER the rate change) and a gate that is high for 120 of every 200 samples
    c["env_ms"] = dict(attack=0.5, decay=0.3, sustain=0.5, release=0.5)
    c["setter_ms"] = np.array([0.25, 0.5, 1.0, 3.0, 10.0, 100.0])
    c["gate"] = ((np.arange(N) % 200) < 120).astype(np.int32)
    c["gate_v"] = (((np.arange(N)[:, None] + 37 * np.arange(V)[None, :]) % 200) < 120).astype(np.int32)
    c["hold"] = rng.integers(1, 40, V).astype(np.int64)
    # fused voice: mode A with block-constant cutoffs, mode B with amplitude * cutoff_b (10 kHz at 44.1 kHz, scaled with the rate)
    c["vfreq"] = rng.uniform(20.0 / 44100 * sr, 5000.0 / 44100 * sr, V)
    c["vcutoff"] = 200.0 / 44100 * sr + c["vfreq"]                         # up to 0.12 sr: the resonant filter stays bounded
    c["vres"] = 1.0 + (np.arange(V) % 16)
    c["cutoff_b"] = np.full(V, 10000.0 / 44100 * sr)
    c["pan"] = rng.uniform(-0.1, 1.1, V)
    # maxiSVF / maxiBiquad
    c["svf"] = np.stack([rng.uniform(20.0, 0.45 * sr, V), rng.uniform(0, 12, V), *rng.uniform(0, 1, (4, V))])
    c["svf"][1, :2] = 0.0                                              # damping = 0 branch
    c["biquad"] = np.stack([(np.arange(V) % 7).astype(np.float64), rng.uniform(30.0 / 44100 * sr, 0.4 * sr, V),
                            rng.uniform(0.3, 8, V), rng.uniform(-18, 18, V)])
    # maxiEnvGen: per-voice square-ish trigger signals (+1 / -1 / exact zeros), stages that complete within N at 96 kHz
    n = np.arange(N)[:, None]
    t = np.sign(np.sin(n * rng.uniform(0.02, 0.08, V)[None, :] + rng.uniform(0, 6, V)))
    t[:, 3] = 1.0
    t[:, 4] = (np.arange(N) % 90 < 5) * 1.0
    if V > 5:
        t[:, 5] = 0.0
    c["envgen_trig"] = t
    # maxiSample / maxiSampler
    Ls = 777
    c["samples"] = np.round((0.6 * np.sin(2 * np.pi * 5 * np.arange(Ls) / Ls) + 0.3 * rng.uniform(-1, 1, Ls)) * 32767) / 32767.0
    c["pos0"] = rng.uniform(1, Ls - 5, V)
    c["speed"] = np.concatenate([[1.0, 2.0, 0.5], rng.uniform(0.2, 3.0, V - 3)])
    c["speed_mod"] = rng.uniform(0.1, 2.5, (N, V))
    c["end"] = rng.uniform(0.5, 1.1, V)
    return c


def sampler_case(sr, voices, NS, seed):
    rng = np.random.default_rng([int(seed), int(sr), voices, NS])
    V = NS * voices
    return dict(smp=rng.uniform(-1, 1, 1500), pitch=rng.integers(-24, 25, V).astype(np.float64), gain=rng.uniform(0.2, 1.0, V),
                par=np.stack([rng.uniform(0.001, 0.2, V), rng.uniform(0.9, 0.999, V), rng.uniform(0.3, 1.0, V),
                              rng.uniform(0.9, 0.999, V)]),
                hold=rng.integers(1, 50, V).astype(np.int64), trig=(rng.uniform(size=V) < 0.6).astype(np.int32))


def mfcc_args(sr):
    """numBins, numFilters, numCoeffs, minFreq, maxFreq: the band edges stay below the Nyquist frequency of the rate."""
    return 512, 42, 13, 20.0, min(20000.0, 0.45 * float(sr))


def spectral_case(sr, nframes, seed):
    """[nframes][1024] fp32 signal frames and [nframes][512] fp32 magnitudes with rows spread over five decades."""
    rng = np.random.default_rng([int(seed), int(sr), nframes])
    sig = (rng.uniform(-1, 1, (nframes, 1024)) * 10.0 ** rng.uniform(-4, 0, (nframes, 1))).astype(np.float32)
    mags = (np.abs(rng.standard_normal((nframes, 512))) * 10.0 ** rng.uniform(-3, 1.5, (nframes, 1))).astype(np.float32)
    mags[min(2, nframes - 1)] = 0          # all-zero frame: the centroid's 0 branch
    return sig, mags


def grain_case(sr, my, gl, ov, S, T, seed):
    """Sample, rates and random draws of a granular bank of S streams over T samples.  rnd in [0, 10) as rand() % 10 gives them;
    enough draws for a spawn every cycle."""
    rng = np.random.default_rng([int(seed), int(sr), int(my), S, T])
    Ls = 20011
    n = np.arange(Ls)
    smp = 0.5 * np.sin(2 * np.pi * 110 * n / 44100.0) + 0.25 * np.sin(2 * np.pi * 331 * n / 44100.0) + 0.05 * rng.uniform(-1, 1, Ls)
    cycle = gl * sr / ov
    R = int(T / max(cycle, 1.0)) + 4
    speed = rng.uniform(0.25, 1.75, S)
    speed[:3] = [1.0, 0.5, -0.75]
    return dict(smp=smp, speed=speed, ts=rng.uniform(0.3, 1.7, S), pm=rng.uniform(-0.2, 0.2, S),
                rnd=rng.integers(0, 10, (S, R)).astype(np.int32), pos0=rng.uniform(0, 1, S),
                pos=((np.arange(T)[:, None] * rng.uniform(0.2, 2.0, S)[None, :] / Ls) + rng.uniform(0, 1, S)) % 1.0)


def granular(o, mode, g, T, my, gl, ov, st=None, gst=None):
    if mode == 2:
        return o.granular(2, 0, g["smp"], T, g["pos"], grainLength=gl, overlaps=ov, mySampleRate=my, st=st, gst=gst)
    st = st if st is not None else np.concatenate([[g["pos0"] * g["smp"].size], np.zeros((3, g["pos0"].size))])
    rnd = None if mode == 3 else g["rnd"]
    return o.granular(mode, 0, g["smp"], T, g["speed"], b=g["ts"], posMod=g["pm"], rnd=rnd, grainLength=gl, overlaps=ov,
                      mySampleRate=my, st=st, gst=gst)


GV, GN, GS = 5, 200, 3
TAIL = 64   # rows kept of the recurrences' per-sample outputs (every later row depends on all earlier ones); the final state is kept whole


def golden_run(o, sr):
    """One small case per family at rate sr -> {name: array}: what oracle/gen_golden_rates.py stores (run on the reference)
    and what the test below recomputes (on the port).  Inputs are regenerated from seeds; only outputs are stored."""
    c = cases(sr, GV, GN, 11)
    out = {}
    with at_rate(sr, o):
        for wf, name in enumerate(OSC):
            p1, p2 = (c["duty"], None) if name == "pulse" else (c["p1"], c["p2"])
            r = o.osc(wf, c["freq"], GN, p1=p1, p2=p2)
            out["osc_" + name] = np.concatenate([r[0], r[1][None], r[2][None]])
        for kind in range(3):
            cu, rs = (c["bp_cutoff"], c["bres"]) if kind == 2 else (c["cutoff"], c["res"])
            r = o.filter(kind, c["x"], cu, rs)
            out["flt_" + FLT[kind]] = np.concatenate([r[0][-TAIL:], r[1], o.filter_coeffs(kind, cu, rs)])
        out["flt_mod"] = o.filter(0, c["x"], c["cutoff_mod"], c["res_mod"], cps=True)[0][-TAIL:]
        out["setters"] = np.array([[o.env_coeff(w, ms) for ms in c["setter_ms"]] for w in range(4)])
        m = c["env_ms"]
        par = np.array([[o.env_coeff(0, m["attack"])], [o.env_coeff(1, m["decay"])], [m["sustain"]],
                        [o.env_coeff(2, m["release"])]]) * np.ones((4, GV))
        for mode in (0, 1):
            r = o.env(mode, c["x"], c["gate"], par, c["hold"])
            out["env%d" % mode] = np.concatenate([r[0][-TAIL:], r[1], r[2].astype(np.float64)])
            r = o.voice(mode, c["vfreq"], c["vcutoff"] if mode == 0 else c["cutoff_b"], c["vres"], c["gate"], par, c["hold"])
            out["voice%d" % mode] = np.concatenate([r[0][-TAIL:], r[1], r[2], r[3], r[4].astype(np.float64)])
        for kind, p in ((1, c["svf"]), (2, c["biquad"])):
            r = o.filter2(kind, c["x"], p)
            out["filter2_%d" % kind] = np.concatenate([r[0][-TAIL:], r[1], r[2]])
        lv, tm, cv = ENVGEN
        r = o.envgen(c["envgen_trig"], lv, tm, cv, 1, 1)
        out["envgen"] = np.concatenate([r[0], r[1], r[2].astype(np.float64)])
        out["envgen_stages"] = r[3]
        for my in sorted({p[1] for p in QUOTIENT_PAIRS if p[0] == sr} or {min(sr, 44100)}):
            r = o.sample(4, c["samples"], GN, c["pos0"], a=c["speed_mod"], aps=True, mySampleRate=my)
            out["sample_%d" % my] = np.concatenate([r[0][-TAIL:], r[1][None]])
        s = sampler_case(sr, 2, 2, 12)
        r = o.sampler(2, s["smp"], GN, s["pitch"], s["gain"], s["par"], s["hold"], np.zeros(4), s["trig"], True)
        out["sampler_mix"], out["sampler_pos"] = r[0], r[2]
        nb, nf, nc, lo, hi = mfcc_args(sr)
        sig, mags = spectral_case(sr, 4, 13)
        W, D = o.mfcc_tables(nb, nf, nc, lo, hi)
        nz = np.flatnonzero(W)
        out["mfcc_W_idx"], out["mfcc_W_val"] = nz.astype(np.int32), W[nz]      # (the mel matrix is sparse: stored as such)
        out["mfcc"] = o.mfcc(mags, nf, nc, lo, hi)[1]
        out["centroid"] = o.fft_features(mags, 1024)[1]
        for gsr, my, gl, ov in GRAIN_SETTINGS:
            if gsr != sr:
                continue
            T = max(int(2.6 * gl * my), 512)
            g = grain_case(sr, my, gl, ov, GS, T, 14)
            for mode in (0, 1, 3):
                r = granular(o, mode, g, T, my, gl, ov)
                assert r[3] == 0
                tag = "grain%d_%d_%g" % (mode, my, gl)
                out[tag + "_tail"], out[tag + "_st"] = r[0][-(512 if gl * my >= 32768 else 128):], r[1]
                out[tag + "_gst"] = r[2].reshape(-1, GS)
    return out
