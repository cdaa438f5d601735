"""numpy restatement of maxiFlanger::flange (H:1166-1172) and maxiChorus::chorus (H:1202-1212), vectorised over
voices, one sample at a time.  The checker of the flanger / chorus banks for sizes tests/golden/fx.npz cannot hold;
tests/test_fx_cpu.py pins it to the reference's own output bit for bit.

Every expression keeps the reference's evaluation order (numpy evaluates binary operators as written, in IEEE
double / float).  The one bank-only behaviour: a tap size above `cap` is held to `cap` and counted."""
import numpy as np

INT_MIN = -2147483648


def cvt_i32(d):
    """double -> int as x86-64's cvttsd2si: truncation, INT_MIN for NaN and outside (-2^31-1, 2^31)."""
    ok = (d > -2147483649.0) & (d < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, d, 0.0)), INT_MIN).astype(np.int64)


def noise(rnd):
    """maxiOsc::noise (C:214-220) of the draws: float arithmetic, widened."""
    r = np.asarray(rnd, np.int32).astype(np.float32) / np.float32(2147483648.0)
    return (r * np.float32(2.0) - np.float32(1.0)).astype(np.float64)


def _row(p, n, V, dtype=np.float64):
    a = np.asarray(p)
    if a.ndim == 2:
        return a[n].astype(dtype)
    return np.broadcast_to(a.astype(dtype), (V,))


class _Ring:
    def __init__(self, V, cap):
        self.cap = cap
        self.mem = np.zeros((V, cap))
        self.phase = np.zeros(V, np.int64)
        self.idx = np.arange(V)

    def dl(self, x, size, fb, ovf):
        """maxiDelayline::dl (C:420-429) with the bank's size rule."""
        over = size > self.cap
        ovf += over
        sz = np.where(over, self.cap, np.where(size < 0, 0, size))
        ph = np.where((self.phase < 0) | (self.phase >= sz), 0, self.phase)
        cur = self.mem[self.idx, ph]
        self.mem[self.idx, ph] = (cur * fb) + (x * fb) * 0.5
        self.phase = ph + 1
        return cur


class Flanger:
    def __init__(self, V, cap, sr=44100):
        self.V, self.sr = V, float(sr)
        self.ring = _Ring(V, cap)
        self.lfo_phase = np.zeros(V)
        self.overflow = np.zeros(V, np.int64)

    def flange(self, x, delay, feedback, speed, depth):
        """x [N][V]; parameters scalar / [V] / [N][V]."""
        x = np.asarray(x, np.float64)
        N, V = x.shape
        out = np.empty((N, V))
        with np.errstate(over="ignore", invalid="ignore"):  # feedback > 1 may overflow, as in the reference
            self._run(out, x, N, V, delay, feedback, speed, depth)
        return out

    def _run(self, out, x, N, V, delay, feedback, speed, depth):
        for n in range(N):
            d = _row(delay, n, V, np.uint32).astype(np.float64)
            sp, dp, fb = _row(speed, n, V), _row(depth, n, V), _row(feedback, n, V)
            ph = np.where(self.lfo_phase >= 1.0, self.lfo_phase - 1.0, self.lfo_phase)   # C:364-365
            ph = ph + (1. / (self.sr / sp))
            self.lfo_phase = ph
            lfo = np.where(ph <= 0.5, (ph - 0.25) * 4, ((1.0 - ph) - 0.25) * 4)
            size = cvt_i32((d + ((lfo * dp) * d)) + 1.0)                                   # H:1169
            o = self.ring.dl(x[n], size, fb, self.overflow)
            o = o * (1 - np.abs(o))
            out[n] = (o + x[n]) / 2.0


class Chorus:
    def __init__(self, V, cap):
        self.V = V
        self.rings = (_Ring(V, cap), _Ring(V, cap))
        self.lx = np.zeros(V)
        self.ly = np.zeros(V)
        self.overflow = np.zeros(V, np.int64)

    def chorus(self, x, delay, feedback, coef, depth, rand):
        """x, rand [N][V]; coef (c, r) [2][V] or [N][2][V] (maxiFilter::lores's of the speed, resonance 1)."""
        x = np.asarray(x, np.float64)
        N, V = x.shape
        coef = np.asarray(coef, np.float64)
        out = np.empty((N, V))
        with np.errstate(over="ignore", invalid="ignore"):  # feedback > 1 may overflow, as in the reference
            self._run(out, x, N, V, delay, feedback, coef, depth, rand)
        return out

    def _run(self, out, x, N, V, delay, feedback, coef, depth, rand):
        for n in range(N):
            d = _row(delay, n, V, np.uint32).astype(np.float64)
            dp, fb = _row(depth, n, V), _row(feedback, n, V)
            c, r = (coef[n] if coef.ndim == 3 else coef)
            self.lx = self.lx + (noise(rand[n]) - self.ly) * c                           # C:463-467
            self.ly = self.ly + self.lx
            self.lx = self.lx * r
            lfo = self.ly * 2.0
            s1 = cvt_i32((d + ((lfo * dp) * d)) + 1.0)                                    # H:1207
            s2 = cvt_i32(((d + (((lfo * dp) * d) * 1.02)) + 1.0) * 0.98)                  # H:1208
            o1 = self.rings[0].dl(x[n], s1, fb, self.overflow)
            o2 = self.rings[1].dl(x[n], s2, fb * 0.99, self.overflow)
            o1 = o1 * (1.0 - np.abs(o1))
            o2 = o2 * (1.0 - np.abs(o2))
            out[n] = (o1 + o2 + x[n]) / 3.0
