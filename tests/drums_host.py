"""Shared by the drum tests and tools/gen/gen_golden_drums.py: the recorded case of tests/golden/drums.npz, the backends that play
it (the library's host pass, a g++ build of mxg_drums.h, the device), a numpy model of each drum's step, and the derived error
bound of the kick.

THE CASE, at 44 100 Hz and again at 48 000 Hz: N = 1200 samples, srand(1) before the run, trigger() before samples TRIG_AT -- silence
first, a retrigger in decay or hold (which the state machine refuses), retriggers in release, a long tail.  Releases of 4 / 6 / 3
ms (kick / snare / hats), snare decay 3 ms, hats decay 2 ms.  Two variants per drum: `plain` (all switches at the class defaults,
cutoff / resonance set) and `full` (distortion, filter and limiter on, the snare inverse, the kick at pitch 1000).  The state rows
(ROWS) are stored in front of every CUTS position.

THE KICK'S BOUND: the only inexact operation is the sine, <= 1 ULP, i.e. <= 2^-53 absolute since |sin| <= 1.
Per sample the output may differ by 2^-53 * envOut * D * H * gain plus one rounding (2^-53 relative) per later operation, where D
is the largest slope of fastAtanDist in its input for the case's distortion (1 if off) and H = sum |h_k| of the lores impulse
response over the block (1 if off).  kick_bound computes both from the recorded parameters."""
import ctypes
import os

import numpy as np

N = 1200
RATES = (44100, 48000)
TRIG_AT = (3, 40, 41, 300, 301, 302, 900)
CUTS = (0, 3, 41, 302, 555, 901, 1200)
KINDS = ("kick", "snare", "hats")
KIND = {"kick": 0, "snare": 1, "hats": 2}
VARIANTS = ("plain", "full")
INVERSE, DISTORTION, FILTER, LIMITER = 1, 2, 4, 8
ROWS = ("phase", "amplitude", "output", "holdcount", "attackphase", "decayphase", "sustainphase", "holdphase", "releasephase",
        "f0", "f1", "f2")
# the constructors (maxiSynths.cpp:11-21, 93-103, 176-188): attack ms, decay ms, sustain, release ms, pitch; holdtime 1
CTOR = {"kick": (0, 1, 1.0, 500, 200.0), "snare": (0, 20, 0.05, 300, 800.0), "hats": (0, 20, 0.1, 300, 12000.0)}
NAN = float("nan")
# pitch (None: the constructor's), release ms, decay ms (None: the constructor's), distortion, cutoff, resonance, gain, and for the
# hats the SVF's setCutoff / setResonance (None: the constructor's 8000, 1); the switches of `full` are in FULL_FLAGS
CASES = {
    ("kick", "plain"): dict(pitch=None, release=4, decay=None, distortion=0.0, cutoff=900.0, resonance=2.0, gain=1.0, svf=None),
    ("kick", "full"): dict(pitch=1000.0, release=4, decay=None, distortion=2.5, cutoff=1200.0, resonance=4.0, gain=1.0, svf=None),
    ("snare", "plain"): dict(pitch=None, release=6, decay=3, distortion=0.0, cutoff=3000.0, resonance=3.0, gain=1.0, svf=None),
    ("snare", "full"): dict(pitch=None, release=6, decay=3, distortion=3.0, cutoff=3000.0, resonance=3.0, gain=1.7, svf=None),
    ("hats", "plain"): dict(pitch=None, release=3, decay=2, distortion=0.0, cutoff=5000.0, resonance=2.0, gain=1.0, svf=None),
    ("hats", "full"): dict(pitch=None, release=3, decay=2, distortion=1.5, cutoff=5000.0, resonance=2.0, gain=2.0, svf=(7000.0, 2.0)),
}
PLAIN_FLAGS = {"kick": 0, "snare": FILTER, "hats": 0}   # maxiSnare::useFilter is true by default
FULL_FLAGS = {"kick": DISTORTION | FILTER | LIMITER, "snare": INVERSE | DISTORTION | FILTER | LIMITER, "hats": DISTORTION | FILTER | LIMITER}
# tests/golden/drums_streams.npz: the patch tests/patches/drums_patch.cpp and the reference's example 7.Counting1 (a maxiClock that raises
# a sinewave's frequency on every tick: 120 bpm, so the first tick falls at frame 22 050)
EXAMPLES = {"07": "7.Counting1"}
STREAM_FRAMES = {"patch": 8820, "07": 30000}
# the clock: setTicksPerBeat(4), setTempo(9000) -> bps 600; one run more with setLastCount(1)
CLOCK_TICKS, CLOCK_TEMPO = 4, 9000.0


def flags_of(kind, variant):
    return (PLAIN_FLAGS if variant == "plain" else FULL_FLAGS)[kind]


def cfg_array(kind, variant):
    """The case as tools/gen/drums_ref_dump.cpp's dr_run takes it."""
    c, fl = CASES[(kind, variant)], flags_of(kind, variant)
    svf = c["svf"] or (NAN, NAN)
    return np.array([NAN if c["pitch"] is None else c["pitch"], c["release"], NAN if c["decay"] is None else c["decay"],
                     bool(fl & DISTORTION), c["distortion"], -1.0 if variant == "plain" else float(bool(fl & FILTER)), c["cutoff"],
                     c["resonance"], bool(fl & LIMITER), c["gain"], bool(fl & INVERSE), svf[0], svf[1]], np.float64)


def triggers(n=N):
    t = np.zeros(n)
    t[[i for i in TRIG_AT if i < n]] = 1.0
    return t


def shuffle(a):
    """float64 -> uint8 [8][n]: the bytes of equal weight side by side (the archive compresses them better)."""
    return np.ascontiguousarray(np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint8).reshape(-1, 8).T)


def unshuffle(b, shape):
    return np.ascontiguousarray(b.T).view(np.float64).reshape(shape)


def key(kind, variant, sr):
    return "%s/%s/%d" % (kind, variant, sr)


def ref_out(g, kind, variant, sr):
    return unshuffle(g["out/" + key(kind, variant, sr)], (N,))


def ref_rows(g, kind, variant, sr):
    """[len(CUTS)][12]: the state in front of every CUTS position."""
    return g["rows/" + key(kind, variant, sr)]


class Params:
    """One voice's (or V voices') arguments of mxg_drum_render, host side.  The envelope coefficients and the filter coefficients
    come from the library's host functions at the CURRENT mxg_settings sample rate."""

    def __init__(self, L, kind, pitch, attack_ms, decay_ms, sustain, release_ms, distortion, cutoff, resonance, gain, flags, svf=None, V=1):
        D = ctypes.c_double
        self.kind, self.flags, self.V = KIND[kind], int(flags), V
        ec = L.mxg_env_coeff_host
        attack = ec(0, D(attack_ms))
        if attack_ms == 0:
            assert attack == 1.0, "setAttack(0) divides by zero inside pow and gives attack = 1"
        self.pitch = np.full(V, pitch, np.float64)
        self.par = np.repeat(np.array([attack, ec(1, D(decay_ms)), sustain, ec(2, D(release_ms))], np.float64)[:, None], V, 1)
        self.holdtime = np.full(V, 1, np.int64)
        self.shape = np.full(V, distortion, np.float64)
        self.gain = np.full(V, gain, np.float64)
        if kind == "hats":
            cf, rs = svf or (8000.0, 1.0)
            self.coef, a, b = np.zeros((5, V)), np.full(V, cf), np.full(V, rs)
            st = L.mxg_svf_coeffs_host(V, a.ctypes.data, b.ctypes.data, self.coef.ctypes.data)
        else:
            self.coef, a, b = np.zeros((3, V)), np.full(V, float(cutoff)), np.full(V, float(resonance))
            st = L.mxg_filter_coeffs_host(0, V, a.ctypes.data, b.ctypes.data, self.coef.ctypes.data)
        assert st == 0

    @classmethod
    def of_case(cls, L, kind, variant, V=1):
        c, ct = CASES[(kind, variant)], CTOR[kind]
        return cls(L, kind, ct[4] if c["pitch"] is None else c["pitch"], ct[0], ct[1] if c["decay"] is None else c["decay"], ct[2],
                   c["release"], c["distortion"], c["cutoff"], c["resonance"], c["gain"], flags_of(kind, variant), c["svf"], V)

    def interleave(self, other):
        """Even voices self, odd voices other (a second parameter set)."""
        for name in ("pitch", "par", "holdtime", "shape", "gain", "coef"):
            getattr(self, name)[..., 1::2] = getattr(other, name)[..., 1::2]
        return self


def fresh_state(V):
    """phase [V], dst [2][V], ist int64 [6][V], fst [3][V]: all zeros, as the reference's objects in static storage."""
    return [np.zeros(V), np.zeros((2, V)), np.zeros((6, V), np.int64), np.zeros((3, V))]


def state_rows(state, v=0):
    """The 12 values of ROWS of voice v."""
    ph, dst, ist, fst = state
    return np.array([ph[v], dst[0, v], dst[1, v]] + [float(ist[r, v]) for r in range(6)] + [fst[0, v], fst[1, v], fst[2, v]])


def state_from_rows(rows, V=1):
    st = fresh_state(V)
    st[0][:] = rows[0]
    st[1][0], st[1][1] = rows[1], rows[2]
    for r in range(6):
        st[2][r] = int(rows[3 + r])
    for r in range(3):
        st[3][r] = rows[9 + r]
    return st


class HostBackend:
    """mxg_drum_host / mxg_clock_host: mxg_drums.h on the CPU, through the library (no device)."""
    name = "lib"

    def __init__(self):
        import maximilian_amd as m
        self.L = m.lib()
        self.fn = self.L.mxg_drum_host

    def render(self, p, trig, rnd, state, n=None, tpv=None):
        """trig: None, [n] (shared) or [n][V]; rnd: int32 [n][V] or None.  Returns out [n][V] and the new state."""
        V = p.V
        trig = None if trig is None else np.ascontiguousarray(trig, np.float64)
        rnd = None if rnd is None else np.ascontiguousarray(rnd, np.int32)
        n = n if n is not None else (trig.shape[0] if trig is not None else rnd.shape[0])
        tpv = (0 if trig is None or trig.ndim == 1 else 1) if tpv is None else tpv
        st = [np.ascontiguousarray(a).copy() for a in state]
        out = np.zeros((n, V))
        A = lambda a: None if a is None else a.ctypes.data
        s = self.fn(p.kind, p.flags, V, n, A(trig), tpv, A(rnd), A(p.pitch), A(p.par), A(p.holdtime), A(p.shape), A(p.coef), A(p.gain),
                    A(st[0]), A(st[1]), A(st[2]), A(st[3]), A(out))
        assert s == 0, self.L.mxg_last_error()
        return out, st

    def clock(self, bps, clk, last, playhead, n):
        V = len(bps)
        bps, clk = np.ascontiguousarray(bps, np.float64), np.ascontiguousarray(clk, np.float64).copy()
        last = None if last is None else np.ascontiguousarray(last, np.int32)
        ph, cnt, tick = np.ascontiguousarray(playhead, np.int64).copy(), np.zeros(V, np.int32), np.zeros((n, V))
        s = self.L.mxg_clock_host(V, n, bps.ctypes.data, clk.ctypes.data, None if last is None else last.ctypes.data, ph.ctypes.data,
                                  cnt.ctypes.data, tick.ctypes.data)
        assert s == 0, self.L.mxg_last_error()
        return tick, clk, ph, cnt


class GpuBackend:
    """mxg_drum_render / mxg_clock_render on device buffers.  d_out and every state array sit inside a guard band of NaN bit patterns,
    which must come back untouched."""
    name = "gpu"
    GUARD = 64
    PAT = np.uint64(0x7FF8DEADBEEF0001)

    def __init__(self, m):
        self.m, self.L = m, m.lib()

    def _guarded(self, a):
        G = self.GUARD
        raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        band = np.full(G, self.PAT, np.uint64).view(np.uint8)
        return self.m.DeviceBuffer.from_numpy(np.concatenate([band, raw, band]))

    def _back(self, buf, like, what):
        G8 = self.GUARD * 8
        raw = buf.numpy().reshape(-1)
        assert (raw[:G8].view(np.uint64) == self.PAT).all() and (raw[-G8:].view(np.uint64) == self.PAT).all(), \
            "the guard band around %s was written" % what
        return raw[G8:-G8].view(like.dtype).reshape(like.shape).copy()

    def render(self, p, trig, rnd, state, n=None, tpv=None):
        m, V, G8 = self.m, p.V, self.GUARD * 8
        trig = None if trig is None else np.ascontiguousarray(trig, np.float64)
        rnd = None if rnd is None else np.ascontiguousarray(rnd, np.int32)
        n = n if n is not None else (trig.shape[0] if trig is not None else rnd.shape[0])
        tpv = (0 if trig is None or trig.ndim == 1 else 1) if tpv is None else tpv
        dev = lambda a: None if a is None else m.DeviceBuffer.from_numpy(a)
        P = lambda b: None if b is None else b.ptr
        ins = [dev(a) for a in (trig, rnd, p.pitch, p.par, p.holdtime, p.shape, p.coef, p.gain)]
        out_like = np.zeros((n, V))
        sb = [self._guarded(a) for a in state]
        ob = self._guarded(np.full((n, V), -7.5))
        s = self.L.mxg_drum_render(p.kind, p.flags, V, n, P(ins[0]), tpv, *[P(b) for b in ins[1:]], *[b.ptr + G8 for b in sb],
                                   ob.ptr + G8, None)
        assert s == 0, self.L.mxg_last_error()
        m._lib.check(self.L.mxg_stream_sync(None), "mxg_stream_sync")
        st = [self._back(b, np.ascontiguousarray(a), "state array %d" % i) for i, (b, a) in enumerate(zip(sb, state))]
        return self._back(ob, out_like, "d_out"), st

    def clock(self, bps, clk, last, playhead, n):
        m, V, G8 = self.m, len(bps), self.GUARD * 8
        bb = m.DeviceBuffer.from_numpy(np.ascontiguousarray(bps, np.float64))
        lb = None if last is None else m.DeviceBuffer.from_numpy(np.ascontiguousarray(last, np.int32))
        likes = [np.ascontiguousarray(clk, np.float64), np.ascontiguousarray(playhead, np.int64), np.zeros(V + (V & 1), np.int32), np.zeros((n, V))]
        gb = [self._guarded(a) for a in likes]
        s = self.L.mxg_clock_render(V, n, bb.ptr, gb[0].ptr + G8, None if lb is None else lb.ptr, gb[1].ptr + G8, gb[2].ptr + G8,
                                    gb[3].ptr + G8, None)
        assert s == 0, self.L.mxg_last_error()
        m._lib.check(self.L.mxg_stream_sync(None), "mxg_stream_sync")
        c, ph, cnt, tick = [self._back(b, a, "clock array %d" % i) for i, (b, a) in enumerate(zip(gb, likes))]
        if V & 1:   # (the count array was padded to a multiple of 8 bytes: the pad must be untouched as well)
            assert cnt[V] == 0
        return tick, c, ph, cnt[:V]


def play_case(be, g, kind, variant, sr, cuts=(), V=1, tpv=0, upto=N, odd=None):
    """The recorded case through a backend at the CURRENT sample rate `sr` (the caller has set it): blocks at CUTS plus `cuts`, the
    recorded voice repeated V times (odd voices with the parameter set `odd`, a Params of V voices, if given).  Returns out
    [upto][V] and {cut: state} at every block boundary."""
    p = Params.of_case(be.L, kind, variant, V)
    if odd is not None:
        p.interleave(odd)
    allcuts = [c for c in sorted(set(CUTS) | set(cuts) | {upto}) if c <= upto]
    tr = triggers()
    draws = None if kind == "kick" else np.repeat(g["draws"][:, None], V, 1)
    state = fresh_state(V)
    out, states = np.zeros((upto, V)), {0: [a.copy() for a in state]}
    for a, b in zip(allcuts[:-1], allcuts[1:]):
        t = np.repeat(tr[a:b, None], V, 1) if tpv else tr[a:b]
        out[a:b], state = be.render(p, t, None if draws is None else draws[a:b], state, tpv=tpv)
        states[b] = [x.copy() for x in state]
    return out, states


# ---- the kick's derived bound -----------------------------------------------------------------------------------------------------
def fastatan(x):
    return x / (1.0 + 0.28 * (x * x))


def kick_bound(L, variant, env_out, n=N):
    """[n]: the absolute bound of the kick's output at every sample (module docstring); env_out [n] is the envelope's output.
    env_out [n][V] (one envelope per voice, the case's other parameters on every voice) gives the bound [n][V]."""
    c, fl = CASES[("kick", variant)], flags_of("kick", variant)
    u = 2.0 ** -53
    D, ops = 1.0, 1   # ops: roundings after the sine (the product with envOut)
    if fl & DISTORTION:
        s = c["distortion"]
        # d/dx [fastatan(x*s) / fastatan(s)] = s * (1 - 0.28 y^2) / (1 + 0.28 y^2)^2 / fastatan(s), largest at y = 0
        D = s / fastatan(s)
        ops += 6
    e = u * np.abs(env_out) * D
    peak = 1.0 * max(1.0, D)
    if fl & FILTER:
        p = Params.of_case(L, "kick", variant)
        cc, r = p.coef[0, 0], p.coef[1, 0]
        x = y = 0.0
        h = np.zeros(n)
        for k in range(n):   # the impulse response of x += (in - y) * c; y += x; x *= r
            x = x + ((1.0 if k == 0 else 0.0) - y) * cc
            y = y + x
            x = x * r
            h[k] = y
        H = np.abs(h)
        if e.ndim == 1:
            e = np.convolve(e, H)[:n]
        else:   # the same convolution down every column
            e = np.sum([np.concatenate([np.zeros((k,) + e.shape[1:]), H[k] * e[:n - k]]) for k in range(n)], axis=0)
        ops += 5
        peak *= H.sum()
    return (e + ops * u * peak) * c["gain"] + u * peak * c["gain"]


def check_kick(L, g, variant, sr, out, what=""):
    """The kick's output under the bound; where the reference's limiter returned +-1 and the candidate's output*gain lies within the
    bound of +-1 (or the other way round), either value passes: such samples are counted and may be at most 1 % of the case.
    Returns (worst error, its bound there, either-way samples, the bound per sample)."""
    ref = ref_out(g, "kick", variant, sr)[:len(out)]
    env = unshuffle(g["envout/" + key("kick", variant, sr)], (N,))[:len(out)]
    bound = kick_bound(L, variant, env, len(out))
    err = np.abs(out - ref)
    bad = err > bound
    either = 0
    if flags_of("kick", variant) & LIMITER:
        clipped = (np.abs(ref) == 1.0) | (np.abs(out) == 1.0)
        near = clipped & bad & (np.abs(np.abs(out) - 1.0) <= bound) & (np.abs(np.abs(ref) - 1.0) <= bound)
        either = int(near.sum())
        bad &= ~near
    assert not bad.any(), "%s kick %s: %d samples over the bound, worst %.3g against %.3g at %d" % (
        what, variant, bad.sum(), err[bad].max(), bound[np.argmax(err * bad)], int(np.argmax(err * bad)))
    assert either <= 0.01 * len(out), "%s: %d samples within the bound of +-1" % (what, either)
    i = int(np.argmax(err))
    return float(err[i]), float(bound[i]), either, bound


# ---- the numpy model: one step of each drum over V voices -------------------------------------------------------------------------
SINEBUF = None


def sine_buffer():
    """The reference's 514-point sineBuffer, read from the library's table header."""
    global SINEBUF
    if SINEBUF is None:
        import re
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        txt = open(os.path.join(root, "maximilian_amd", "csrc", "maxi_tables.h")).read()
        body = re.search(r"#define MAXI_SINE_TAB_INIT\s*\\?\s*\{(.*?)\}", txt, re.S).group(1)
        vals = np.array([float.fromhex(t) if "x" in t else float(t) for t in re.findall(r"[-+]?(?:0x[0-9a-fA-F.]+p[-+]?\d+|\d[\d.]*(?:[eE][-+]?\d+)?)", body)])
        assert len(vals) == 515 and vals[0] == 0.0
        SINEBUF = vals[1:]   # (entry 0 is the guard in front of sineBuffer[0])
    return SINEBUF


def model_adsr(e, par, holdtime, trig):
    """maxiEnv::adsr(1., trigger) (C:1415-1466) on dict e of [V] arrays (amplitude, output, holdcount, attackphase, decayphase,
    sustainphase, holdphase, releasephase), statement by statement with masks."""
    attack, decay, sustain, release = par
    t1 = trig.astype(bool)
    c1 = t1 & (e["attackphase"] != 1) & (e["holdphase"] != 1) & (e["decayphase"] != 1)
    for k in ("holdcount", "decayphase", "sustainphase", "releasephase"):
        e[k] = np.where(c1, 0, e[k])
    e["attackphase"] = np.where(c1, 1, e["attackphase"])
    a = e["attackphase"] == 1
    e["releasephase"] = np.where(a, 0, e["releasephase"])
    e["amplitude"] = np.where(a, e["amplitude"] + (1 * attack), e["amplitude"])
    e["output"] = np.where(a, 1. * e["amplitude"], e["output"])
    a2 = a & (e["amplitude"] >= 1)
    e["amplitude"] = np.where(a2, 1.0, e["amplitude"])
    e["attackphase"] = np.where(a2, 0, e["attackphase"])
    e["decayphase"] = np.where(a2, 1, e["decayphase"])
    d = e["decayphase"] == 1
    e["amplitude"] = np.where(d, e["amplitude"] * decay, e["amplitude"])
    e["output"] = np.where(d, 1. * e["amplitude"], e["output"])
    d2 = d & (e["amplitude"] <= sustain)
    e["decayphase"] = np.where(d2, 0, e["decayphase"])
    e["holdphase"] = np.where(d2, 1, e["holdphase"])
    h = (e["holdcount"] < holdtime) & (e["holdphase"] == 1)
    e["output"] = np.where(h, 1. * e["amplitude"], e["output"])
    e["holdcount"] = e["holdcount"] + h
    ge = e["holdcount"] >= holdtime
    e["output"] = np.where(ge & t1, 1. * e["amplitude"], e["output"])
    rel = ge & ~t1
    e["holdphase"] = np.where(rel, 0, e["holdphase"])
    e["releasephase"] = np.where(rel, 1, e["releasephase"])
    r = (e["releasephase"] == 1) & (e["amplitude"] > 0.)
    e["amplitude"] = np.where(r, e["amplitude"] * release, e["amplitude"])
    e["output"] = np.where(r, 1. * e["amplitude"], e["output"])
    return e["output"]


def model_noise(rnd):
    r = rnd.astype(np.float32) / np.float32(2147483648.0)
    return (r * np.float32(2.0) - np.float32(1.0)).astype(np.float64)


def model_render(p, trig, rnd, state, sr):
    """The numpy model of snare and hats (and of the kick's phase, envelope and state-machine; its output with numpy's sine).  The
    same interface as the backends' render; trig [n][V] or [n]."""
    with np.errstate(all="ignore"):
        V = p.V
        phase, dst, ist, fst = [np.array(a, copy=True) for a in state]
        e = dict(amplitude=dst[0], output=dst[1], holdcount=ist[0], attackphase=ist[1], decayphase=ist[2], sustainphase=ist[3],
                 holdphase=ist[4], releasephase=ist[5])
        n = len(trig) if trig is not None else len(rnd)
        out = np.zeros((n, V))
        f0, f1, f2 = fst
        sr = float(sr)
        for i in range(n):
            t = np.zeros(V) if trig is None else np.broadcast_to(np.asarray(trig[i]) != 0, (V,))
            env = model_adsr(e, p.par, p.holdtime, t)
            if p.flags & INVERSE:
                env = np.abs(1 - env)
            if p.kind == 0:
                o = np.sin(phase * 6.283185307179586476925286766559)
                phase = np.where(phase >= 1.0, phase - 1.0, phase)
                phase = phase + (1. / (sr / (p.pitch * env)))
                o = o * env
            elif p.kind == 1:
                phase = np.where(phase >= 1.0, phase - 1.0, phase)
                phase = phase + (1. / (sr / (p.pitch * (0.1 + (env * 0.85)))))
                tri = np.where(phase <= 0.5, (phase - 0.25) * 4, ((1.0 - phase) - 0.25) * 4)
                o = (tri + model_noise(rnd[i])) * env
            else:
                sb = sine_buffer()
                phase = phase + 512. / (sr / (p.pitch * 1.0))
                phase = np.where(phase >= 511, phase - 512, phase)
                rem = phase - np.floor(phase)
                idx = np.trunc(phase).astype(np.int64)
                lo = np.where(idx + 1 >= 0, sb[np.clip(idx + 1, 0, 513)], 0.0)
                hi = sb[np.clip(idx + 2, 0, 513)]
                o = ((1 - rem) * lo + rem * hi + model_noise(rnd[i])) * env
            if p.flags & DISTORTION:
                o = (1.0 / fastatan(p.shape)) * fastatan(o * p.shape)
            if p.flags & FILTER:
                if p.kind == 2:
                    g1, g2, g3, g4, k = p.coef
                    v1z, v2z = f1, f2
                    v3 = o + f0 - 2.0 * v2z
                    f1 = f1 + (g1 * v3 - g2 * v1z)
                    f2 = f2 + (g3 * v3 + g4 * v1z)
                    f0 = o
                    high = o - k * f1 - f2
                    notch = o - k * f1
                    o = (f2 * 0.) + (f1 * 0.) + (high * 1.) + (notch * 0.)
                else:
                    f0 = f0 + (o - f1) * p.coef[0]
                    f1 = f1 + f0
                    f0 = f0 * p.coef[1]
                    o = f1
            gq = o * p.gain
            out[i] = np.where(gq > 1, 1., np.where(gq < -1, -1., gq)) if p.flags & LIMITER else gq
        dst = np.array([e["amplitude"], e["output"]])
        ist = np.array([e[k] for k in ("holdcount", "attackphase", "decayphase", "sustainphase", "holdphase", "releasephase")], np.int64)
        return out, [phase, dst, ist, np.array([f0, f1, f2])]


# ---- checks shared by the CPU and the GPU tests -----------------------------------------------------------------------------------
import contextlib  # noqa: E402


@contextlib.contextmanager
def at_rate(L, sr):
    """mxg_settings' sample rate for the duration of the block (the coefficient hosts and the drum calls read it)."""
    prev = L.mxg_sample_rate()
    assert L.mxg_settings(int(sr), 2, 1024) == 0
    try:
        yield
    finally:
        L.mxg_settings(prev, 2, 1024)


def bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    same = a.view(np.uint64) == b.view(np.uint64)
    assert same.all(), "%s: %d of %d values differ, first at %s: %r against %r" % (
        what, (~same).sum(), same.size, np.argwhere(~same)[0].tolist(), a[~same][0], b[~same][0])


def check_case(L, g, kind, variant, sr, out, states, what, v=0):
    """Voice v of a backend's rendering of the recorded case against the file, under the numerics contract: snare and hats and every
    state row BIT FOR BIT, except the kick's output (check_kick) and, with its filter on, the kick's filter state: y is the output
    of the sample in front of the cut before the gain, so it has that sample's bound; x = (y_n - y_n-1) * r the two last bounds
    times |r|.  Returns the kick's (worst error, bound, either-way samples) or None."""
    what = "%s %s" % (what, key(kind, variant, sr))
    rows, res = ref_rows(g, kind, variant, sr), None
    upto = out.shape[0]
    if kind == "kick":
        res = check_kick(L, g, variant, sr, out[:, v], what)
        bound = res[3] / CASES[(kind, variant)]["gain"]
        r = abs(Params.of_case(L, kind, variant).coef[1, 0])
    else:
        bits_equal(out[:, v], ref_out(g, kind, variant, sr)[:upto], what)
    loose = (9, 10) if kind == "kick" and flags_of(kind, variant) & FILTER else ()
    for i, c in enumerate(CUTS):
        if c > upto:
            continue
        got = state_rows(states[c], v)
        exact = [j for j in range(12) if j not in loose]
        bits_equal(got[exact], rows[i][exact], "%s state in front of %d" % (what, c))
        if loose and c >= 2:
            assert abs(got[10] - rows[i][10]) <= bound[c - 1], "%s filter y in front of %d" % (what, c)
            assert abs(got[9] - rows[i][9]) <= (bound[c - 1] + bound[c - 2]) * r, "%s filter x in front of %d" % (what, c)
        elif loose:
            bits_equal(got[[9, 10]], rows[i][[9, 10]], "%s filter state in front of %d" % (what, c))
    return res and res[:3]


def check_clock(g, sr, last, tick, playhead_after, count_after, upto=N):
    ck = "clock/%d/%d/" % (sr, last)
    assert np.array_equal(tick[:, 0] != 0, g[ck + "tick"][:upto] != 0), "tick"
    assert set(np.unique(tick)) <= {0.0, 1.0}
    assert int(playhead_after) == int(g[ck + "playhead"][upto - 1]) and int(count_after) == int(g[ck + "count"][upto - 1])


def denormal_cases(be):
    """An uploaded envelope amplitude of 3 * 2^-1074 in release: it stays with a release coefficient of 0.97 and goes 3 -> 1 -> 0 steps
    with 0.3, on every drum."""
    tiny = 2.0 ** -1074
    for coeff, want in ((0.97, [3, 3, 3, 3, 3, 3]), (0.3, [1, 0, 0, 0, 0, 0])):
        for kind in KINDS:
            p = Params.of_case(be.L, kind, "plain", 2)
            p.par[3] = coeff
            st = fresh_state(2)
            st[1][0] = 3 * tiny
            st[2][0], st[2][5] = 1, 1   # holdcount = holdtime, releasephase
            seen = []
            for _ in range(len(want)):
                out, st = be.render(p, None, None if kind == "kick" else np.full((1, 2), 12345, np.int32), st, n=1)
                assert st[1][0][0] == st[1][0][1]
                seen.append(st[1][0][0] / tiny)
            assert seen == want, (kind, coeff, seen)
