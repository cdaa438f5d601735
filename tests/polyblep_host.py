"""TEST INFRASTRUCTURE shared by the maxiPolyBLEP tests and tools/gen/gen_golden_polyblep.py: the inputs of
tests/golden/polyblep.npz derived from its stored integers (one place for the generator and the tests), mxg_polyblep_host and
mxg_polyblep_render behind ONE numpy interface (HostBackend / GpuBackend), a numpy model that restates the arithmetic of the
phase and of the ten exact waveforms step by step (ModelBackend: IEEE + - * / trunc fmin fmax on arrays), a driver that plays
the file's case through any backend at any cuts, and the numerics contract of DESIGN.md section 4 as one check.

The case: SR = 1000, six voices, N samples, every waveform over the same frequencies.  The frequency block fq / 8.0 Hz is
constant inside each of the stored blocks up to sample PS_FROM (so those blocks also render with one frequency per voice) and
moves per sample after it.  Voice 0 rests at 0 Hz from sample 143 on, voice 1 runs backwards (negative), voice 2 crosses
SR / 4 in both directions (block by block, then inside a block), voice 3 sits just below SR / 4, voices 4 and 5 are a slow and
a mid one.  The pulse widths rotate over the voices at every stored cut; three voices are synced at sample 601."""
import ctypes

import numpy as np

WAVEFORMS = ["SINE", "COSINE", "TRIANGLE", "SQUARE", "RECTANGLE", "SAWTOOTH", "RAMP", "MODIFIED_TRIANGLE", "MODIFIED_SQUARE",
             "HALF_WAVE_RECTIFIED_SINE", "FULL_WAVE_RECTIFIED_SINE", "TRIANGULAR_PULSE", "TRAPEZOID_FIXED", "TRAPEZOID_VARIABLE"]
WF = {n: i for i, n in enumerate(WAVEFORMS)}
EXACT = ["TRIANGLE", "SQUARE", "RECTANGLE", "SAWTOOTH", "RAMP", "MODIFIED_TRIANGLE", "MODIFIED_SQUARE", "TRIANGULAR_PULSE",
         "TRAPEZOID_FIXED", "TRAPEZOID_VARIABLE"]
ULP1 = ["SINE", "COSINE"]                                             # within 1 ULP, like every fallback sample
ABS50 = ["HALF_WAVE_RECTIFIED_SINE", "FULL_WAVE_RECTIFIED_SINE"]      # within 2^-50 absolute
RECT_ABS = 2.0 ** -50
V, N, SR = 6, 1200, 1000
CUTS = [0, 1, 8, 9, 143, 600, 601, 1000, 1193, N]
PS_FROM = 601
PW = [0.0, 0.00005, 0.3, 0.5, 0.99995, 1.0]
PW_Q = [0, 5, 30000, 50000, 99995, 100000]                            # PW = PW_Q / 100000.0
SYNC_AT, SYNC = 601, [(2, 2.75), (4, -0.25), (5, -3.0)]


# the maxiEnvGen edits of the golden: setup(ENV_LEVELS, ENV_TIMES, ENV_CURVES), then (kind: 0 setLevel / 1 setCurve, index, value)
ENV_LEVELS, ENV_TIMES, ENV_CURVES = [0.0, 1.0, 0.25, 0.0], [5.0, 8.0, 11.0], [1.0, 1.0, 2.0]
ENV_OPS = [(0, 0, 0.5), (0, 1, 0.75), (0, 2, -0.125), (0, 3, 0.0625), (0, 4, 9.0), (0, 5, 9.0), (1, 0, 1.5), (1, 2, 0.5), (1, 1, 3.0),
           (0, 1, 0.3), (1, 7, 4.0)]   # (setCurve(3): the reference writes outside its vector -- not called there)
STREAM_FRAMES = 6000
EXAMPLES = {"09a": "9.Envelopes1", "09b": "9.Envelopes2", "09c": "9.Envelopes3"}


def freqs(g):
    return g["fq"].astype(np.float64) / 8.0


def pulse_widths(g, block):
    """The pulse widths of stored block `block`: the six values rotated by one voice per block."""
    pw = g["pw_q"].astype(np.float64) / 100000.0
    return pw[(np.arange(V) + block) % V]


def fallback(freq, sr=SR):
    freq = np.asarray(freq, np.float64)
    return (freq / sr) * sr >= sr / 4.0


def shuffle(a):
    """float64 -> uint8 [8][n]: the bytes of equal weight side by side (the archive compresses them better)."""
    return np.ascontiguousarray(np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint8).reshape(-1, 8).T)


def unshuffle(b, shape):
    return np.ascontiguousarray(b.T).view(np.float64).reshape(shape)


def ref_out(g, wf):
    return unshuffle(g["out/" + wf], (N, V))


def sync_wrap(phase):
    t = np.asarray(phase, np.float64)
    return np.where(t >= 0, t - np.trunc(t), t + (1 - np.trunc(t)))


# ---- the numpy model: the phase and the ten exact waveforms ---------------------------------------------------------------------
def _frac(x):
    return x - np.trunc(x)


def _blep(t, dt):
    a = t / dt - 1
    b = (t - 1) / dt + 1
    return np.where(t < dt, -(a * a), np.where(t > 1 - dt, b * b, 0.0))


def _blamp(t, dt):
    a = t / dt - 1
    b = (t - 1) / dt + 1
    return np.where(t < dt, ((-1 / 3.0) * (a * a)) * a, np.where(t > 1 - dt, ((1 / 3.0) * (b * b)) * b, 0.0))


def _fold4(t):
    y = t * 4
    return np.where(y >= 3, y - 4, np.where(y > 1, 2 - y, y))


def model_wave(wf, t, dt, pw):
    """get() of an exact waveform below the fallback, on arrays."""
    one = np.ones_like(t)
    with np.errstate(all="ignore"):
        if wf == "TRIANGLE":
            y = _fold4(t)
            return 1.0 * (y + (4 * dt) * (_blamp(_frac(t + 0.25), dt) - _blamp(_frac(t + 0.75), dt)))
        if wf == "SQUARE":
            y = np.where(t < 0.5, one, -one)
            return 1.0 * (y + (_blep(t, dt) - _blep(_frac(t + 0.5), dt)))
        if wf == "RECTANGLE":
            y = -2 * pw
            y = np.where(t < pw, y + 2, y)
            return 1.0 * (y + (_blep(t, dt) - _blep(_frac((t + 1) - pw), dt)))
        if wf == "SAWTOOTH":
            u = _frac(t + 0.5)
            return 1.0 * ((2 * u - 1) - _blep(u, dt))
        if wf == "RAMP":
            u = _frac(t)
            return 1.0 * ((1 - 2 * u) + _blep(u, dt))
        if wf == "MODIFIED_TRIANGLE":
            w = np.fmax(0.0001, np.fmin(0.9999, pw))
            y = t * 2
            y = np.where(y >= 2 - w, (y - 2) / w, np.where(y >= w, 1 - (y - w) / (1 - w), y / w))
            return 1.0 * (y + (dt / (w - w * w)) * (_blamp(_frac(t + 0.5 * w), dt) - _blamp(_frac((t + 1) - 0.5 * w), dt)))
        if wf == "MODIFIED_SQUARE":
            t1 = _frac((t + 0.875) + 0.25 * (pw - 0.5))
            t2 = _frac((t + 0.375) + 0.25 * (pw - 0.5))
            y = np.where(t1 < 0.5, one, -one)
            y = y + (_blep(t1, dt) - _blep(t2, dt))
            t1 = _frac(t1 + 0.5 * (1 - pw))
            t2 = _frac(t2 + 0.5 * (1 - pw))
            y = y + np.where(t1 < 0.5, one, -one)
            y = y + (_blep(t1, dt) - _blep(t2, dt))
            return (1.0 * 0.5) * y
        if wf == "TRIANGULAR_PULSE":
            t1 = _frac((t + 0.75) + 0.5 * pw)
            y4 = 4 * t1
            y = np.where(t1 >= pw, -pw, np.where(y4 >= 2 * pw, (4 - y4 / pw) - pw, y4 / pw - pw))
            t2 = _frac((t1 + 1) - 0.5 * pw)
            t3 = _frac((t1 + 1) - pw)
            corr = ((2 * dt) / pw) * ((_blamp(t1, dt) - 2 * _blamp(t2, dt)) + _blamp(t3, dt))
            return 1.0 * np.where(pw > 0, y + corr, y)
        if wf == "TRAPEZOID_FIXED":
            y = np.fmax(-1.0, np.fmin(1.0, 2 * _fold4(t)))
            t1 = _frac(t + 0.125)
            y = y + (4 * dt) * (_blamp(t1, dt) - _blamp(_frac(t1 + 0.5), dt))
            t1 = _frac(t + 0.375)
            y = y + (4 * dt) * (_blamp(t1, dt) - _blamp(_frac(t1 + 0.5), dt))
            return 1.0 * y
        if wf == "TRAPEZOID_VARIABLE":
            w = np.fmin(0.9999, pw)
            scale = 1 / (1 - w)
            y = np.fmax(-1.0, np.fmin(1.0, scale * _fold4(t)))
            t1 = _frac((t + 0.25) - 0.25 * w)
            y = y + ((scale * 2) * dt) * (_blamp(t1, dt) - _blamp(_frac(t1 + 0.5), dt))
            t1 = _frac((t + 0.25) + 0.25 * w)
            y = y + ((scale * 2) * dt) * (_blamp(t1, dt) - _blamp(_frac(t1 + 0.5), dt))
            return 1.0 * y
    raise KeyError(wf)


def arms(wf, t, dt, pw):
    """Which piecewise arm a sample takes, as small integers (the generator asserts that every one occurs)."""
    if wf in ("TRIANGLE", "TRAPEZOID_FIXED", "TRAPEZOID_VARIABLE"):
        y = t * 4
        a = np.where(y >= 3, 0, np.where(y > 1, 1, 2))
        if wf == "TRIANGLE":
            return a, 3
        scale = 2.0 if wf == "TRAPEZOID_FIXED" else 1 / (1 - np.fmin(0.9999, pw))
        z = scale * _fold4(t)
        return a * 3 + np.where(z > 1, 0, np.where(z < -1, 1, 2)), None   # (not every product of the two occurs: see the generator)
    if wf == "MODIFIED_TRIANGLE":
        w = np.fmax(0.0001, np.fmin(0.9999, pw))
        y = t * 2
        return np.where(y >= 2 - w, 0, np.where(y >= w, 1, 2)), 3
    if wf == "TRIANGULAR_PULSE":
        t1 = _frac((t + 0.75) + 0.5 * pw)
        return np.where(t1 >= pw, 0, np.where(4 * t1 >= 2 * pw, 1, 2)) * 2 + (pw > 0), None
    return None, 0


class ModelBackend:
    name = "model"

    def render(self, wf, freq, pw, sr, t, n=None):
        """freq [n][V], or [V] with n; returns out [n][V] (NaN where the fallback is taken, and for a sine waveform), t."""
        freq = np.asarray(freq, np.float64)
        if freq.ndim == 1:
            freq = np.broadcast_to(freq, (n, freq.shape[0]))
        pw = np.full(t.shape, 0.5) if pw is None else np.asarray(pw, np.float64)
        out = np.zeros(freq.shape)
        t = t.copy()
        for n in range(freq.shape[0]):
            dt = freq[n] / sr
            y = model_wave(wf, t, dt, pw) if wf in EXACT else np.full(t.shape, np.nan)
            out[n] = np.where(dt * sr >= sr / 4.0, np.nan, y)
            t = t + dt
            t = t - np.trunc(t)
        return out, t


class HostBackend:
    """mxg_polyblep_host: mxg_polyblep.h on the CPU, through the library (no device)."""
    name = "host"

    def __init__(self):
        import maximilian_amd as m
        self.L = m.lib()

    def render(self, wf, freq, pw, sr, t, n=None):
        freq = np.ascontiguousarray(freq, np.float64)
        fps = freq.ndim == 2
        n = freq.shape[0] if fps else n
        Vv = t.shape[0]
        out, t = np.zeros((n, Vv)), np.ascontiguousarray(t, np.float64).copy()
        pwa = None if pw is None else np.ascontiguousarray(pw, np.float64)
        st = self.L.mxg_polyblep_host(WF[wf], Vv, n, freq.ctypes.data, int(fps), None if pwa is None else pwa.ctypes.data, float(sr),
                                      t.ctypes.data, out.ctypes.data)
        assert st == 0, self.L.mxg_last_error()
        return out, t


class GpuBackend:
    """mxg_polyblep_render on device buffers, a guard band around d_out and d_t checked after every call."""
    name = "gpu"
    GUARD = 64

    def __init__(self, m):
        self.m, self.L = m, m.lib()

    def render(self, wf, freq, pw, sr, t, n=None):
        m, G = self.m, self.GUARD
        freq = np.ascontiguousarray(freq, np.float64)
        fps = freq.ndim == 2
        n = freq.shape[0] if fps else n
        Vv = t.shape[0]
        fill = -7.5
        ob = m.DeviceBuffer.from_numpy(np.full(n * Vv + 2 * G, fill))
        tb = m.DeviceBuffer.from_numpy(np.concatenate([np.full(G, fill), np.asarray(t, np.float64), np.full(G, fill)]))
        fb = m.DeviceBuffer.from_numpy(freq)
        pb = None if pw is None else m.DeviceBuffer.from_numpy(np.ascontiguousarray(pw, np.float64))
        st = self.L.mxg_polyblep_render(WF[wf], Vv, n, fb.ptr, int(fps), None if pb is None else pb.ptr, float(sr), tb.ptr + 8 * G,
                                        ob.ptr + 8 * G, None)
        assert st == 0, self.L.mxg_last_error()
        m._lib.check(self.L.mxg_stream_sync(None), "mxg_stream_sync")
        o, tt = ob.numpy().reshape(-1), tb.numpy().reshape(-1)
        assert (o[:G] == fill).all() and (o[-G:] == fill).all(), "%s: the guard band around d_out was written" % wf
        assert (tt[:G] == fill).all() and (tt[-G:] == fill).all(), "%s: the guard band around d_t was written" % wf
        return o[G:-G].reshape(n, Vv).copy(), tt[G:-G].copy()


def _spread(a, tile, voices):
    """[..][V] -> the six voices repeated `tile` times, the first `voices` columns kept."""
    a = np.tile(a, (1, tile)) if a.ndim == 2 else np.tile(a, tile)
    return a[..., :voices] if voices else a


def play_case(be, g, wf, cuts=None, tile=1, fps=None, voices=None, upto=N, pw_none=False):
    """The stored case through a backend: blocks at `cuts` (a superset of the stored CUTS keeps the stored pulse-width
    rotation and sync; default: the stored ones), the six voices repeated `tile` times and the first `voices` columns kept, the
    first `upto` samples.  fps None / False: one frequency per voice where the block allows it (before PS_FROM), else per sample;
    fps True: always per sample.  Returns out [upto][voices] and the phases at the stored cuts <= upto."""
    f = _spread(freqs(g), tile, voices)
    Vt = f.shape[1]
    cuts = [c for c in sorted(set(CUTS) | set(cuts or ()) | {upto}) if c <= upto]
    t = np.zeros(Vt)
    out = np.zeros((upto, Vt))
    phases = {0: t.copy()}
    block = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a in CUTS:
            block = CUTS.index(a)
        pw = _spread(pulse_widths(g, block), tile, voices)
        if a == SYNC_AT:
            for v, ph in SYNC:
                t[v::V] = sync_wrap(ph)
        if not fps and b <= PS_FROM:
            out[a:b], t = be.render(wf, f[a], pw, SR, t, n=b - a)
        else:
            out[a:b], t = be.render(wf, f[a:b], pw, SR, t)
        if b in CUTS:
            phases[b] = t.copy()
    return out, np.array([phases[c] for c in CUTS if c in phases])


def check_contract(g, wf, out, phases, what="", tile=1, voices=None):
    """DESIGN.md section 4 against the stored reference (its first out.shape[0] samples, the voices spread as in play_case);
    returns the measured maxima {ulp, abs} for the printout."""
    n = out.shape[0]
    return check_against(wf, out, phases, _spread(ref_out(g, wf), tile, voices)[:n],
                         _spread(g["t/" + wf], tile, voices)[:phases.shape[0]], _spread(fallback(freqs(g)), tile, voices)[:n], what)


def check_against(wf, out, phases, ref, ref_phases, fb, what=""):
    """The same contract against any expectation of the same shapes (the stored reference, or mxg_polyblep_host on voices the file
    does not hold): `fb` marks the samples that fall back to the sine.  Returns the measured maxima {ulp, abs}."""
    from conftest import assert_bits_equal, ulp_diff
    assert_bits_equal(phases, ref_phases, "%s %s: phase" % (what, wf))
    res = {"ulp": 0, "abs": 0.0}
    if fb.any():
        res["ulp"] = int(ulp_diff(out[fb], ref[fb]).max())
        assert res["ulp"] <= 1, "%s %s: a fallback sample is %d ULP from the reference" % (what, wf, res["ulp"])
    if wf in EXACT:
        assert_bits_equal(out[~fb], ref[~fb], "%s %s" % (what, wf))
    elif wf in ULP1:
        res["ulp"] = max(res["ulp"], int(ulp_diff(out[~fb], ref[~fb]).max()))
        assert res["ulp"] <= 1, "%s %s: %d ULP from the reference" % (what, wf, res["ulp"])
    else:
        res["abs"] = float(np.abs(out[~fb] - ref[~fb]).max())
        assert res["abs"] <= RECT_ABS, "%s %s: %.3g from the reference (2^-50 = %.3g)" % (what, wf, res["abs"], RECT_ABS)
    return res
