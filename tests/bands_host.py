"""Shared by tests/test_bands_host.py, tests/test_bands_cabi.py and tests/test_gpu_bands.py: the host build of mxg_bands.h
(tests/host_bands.cpp, g++ under the oracle's FPFLAGS) and the library's K19 entry points behind ONE numpy interface
(HostBackend / GpuBackend), a numpy model that restates the arithmetic (ModelBackend: the Bark limits and the octave map in Python
floats / np.float32, band sums as a double accumulated bin after bin, the octave frame and the peak state machine in float32,
vectorised over frames), the seeded inputs, and the bounds.

Bounds (derived, fixed before any run):
  band sums, averages, peaks, hold counters: equal bits;
  specific: at most ULP_SPECIFIC = 16 ULP from the host pow (OpenCL's ceiling for a double pow, the source K18 used for asymclip);
  relative: |d| <= 33 * 2^-52 * |ref| (two such values divided, plus the two roundings), exactly 1.0 at the frame's maximum;
  total:    |d| <= 39 * 2^-52 * |ref| (16 * 2^-52 from the terms, all >= 0, plus 23 additions rounded on each side);
  frames with NaN, Inf or negative sums: NaN / Inf positions coincide, the finite values are compared."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT

P = ctypes.c_void_p
ULP_SPECIFIC = 16
REL_RELATIVE = 33 * 2.0 ** -52
REL_TOTAL = 39 * 2.0 ** -52
BARK_CONFIGS = [(44100, 1024), (44100, 16), (22050, 1024), (8000, 4096), (96000, 512)]
OCTAVE_CONFIGS = [(44100.0, 512, 12), (44100.0, 512, 3), (44100.0, 8, 1), (44100.0, 2048, 1), (44100.0, 512, 0)]
# the cases of tests/golden/bands.npz (tools/gen/gen_golden_bands.py): inputs from these seeds, runs as (hold time, decay, EQ slope)
BARK_FRAMES, BARK_SEED = 9, 19
OCTAVE_FRAMES, OCTAVE_SEED = 44, 7
OCTAVE_RUNS = [(0, 0.9, 0.0), (2, 0.9, 0.01), (2, 0.0, 0.0), (0, 1.0, -0.001)]
PATCH_FRAMES = 12000
OCTAVE_CUTS = (0, 1, 8, 20, 27, 44)   # calls of 1, 7, 12, 7 and 17 frames


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libbands_host.so")
    flags = [f for f in fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "host_bands.cpp")])
    L = ctypes.CDLL(so)
    S, I, F, U = ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_uint
    L.bnd_host_bark_limits.argtypes = [U, U, P]
    L.bnd_host_octave_map.argtypes = [F, I, I, P]
    L.bnd_host_bark.argtypes = [P, P, S, S, P, P, P, P]
    L.bnd_host_octave.argtypes = [P, I, I, P, S, S, S, F, F, I, F, P, P, P, P]
    return L


def _p(a):
    return None if a is None else a.ctypes.data


# ---- the model ---------------------------------------------------------------------------------------------------------------
def bark_limits_model(sR, bS):
    spec = bS // 2
    scale = []
    for i in range(spec):
        hz = float(((i * sR) & 0xffffffff) // bS)
        scale.append(13.0 * math.atan(hz / 1315.8) + 3.5 * math.atan(math.pow(hz / 7518.0, 2)))
    lim = [0] * 25
    top = scale[spec - 1]
    end, band = int(top / 24), 1
    for i in range(spec):
        while scale[i] > end:
            if band <= 24:
                lim[band] = i
            band += 1
            end = int(band * top / 24)
    lim[24] = spec - 1
    return np.array(lim, np.int32)


def octave_map_model(sr, n, per):
    f = np.float32
    span = f(f(sr) / f(2.0)) / f(n)
    per = per or 1
    inc = f(np.power(f(2.0), f(1.0) / f(per)))
    avgidx, avg_freq, spe_freq, out = 0, f(55.0), span, []
    with np.errstate(over="ignore"):
        for _ in range(n):
            while spe_freq > avg_freq:
                avgidx += 1
                avg_freq = f(avg_freq * inc)
            out.append(avgidx)
            spe_freq = f(spe_freq + span)
    return np.array(out, np.int32), avgidx


class ModelBackend:
    name = "model"

    def bark_limits(self, sR, bS):
        return bark_limits_model(sR, bS)

    def octave_map(self, sr, n, per):
        return octave_map_model(sr, n, per)

    def bark(self, lim, spec):
        """spec [nframes][>= specSize] float32 -> bandsum, specific, relative [nframes][24], total [nframes]."""
        with np.errstate(all="ignore"):
            nf = spec.shape[0]
            sums = np.zeros((nf, 24))
            for b in range(24):
                s = np.zeros(nf)
                for j in range(int(lim[b]), int(lim[b + 1])):
                    s = s + spec[:, j].astype(np.float64)
                sums[:, b] = s
            specific = np.power(sums, 0.23)
            mx = np.zeros(nf)
            total = np.zeros(nf)
            for b in range(24):
                mx = np.where(specific[:, b] > mx, specific[:, b], mx)
                total = total + specific[:, b]
            return sums, specific, specific / mx[:, None], total

    def octave(self, m, nA, mags, S, fps, intercept, slope, hold_time, decay, peak_state=None, hold_state=None):
        """mags [S * fps][>= n] float32 -> averages, peaks [S * fps][nA]; the states [S][nA] are updated in place."""
        f = np.float32
        with np.errstate(all="ignore"):
            nf = S * fps
            avg = np.zeros((nf, nA), f)
            s, count, last = np.zeros(nf, f), 0, 0
            for i in range(len(m)):
                count += 1
                eq = f(f(intercept) + f(f(i) * f(slope)))
                s = (s + (mags[:, i] * eq).astype(f)).astype(f)
                if m[i] != last:
                    avg[:, last:m[i]] = (s / f(count)).astype(f)[:, None]
                    count, s = 0, np.zeros(nf, f)
                last = int(m[i])
            if peak_state is None:
                return avg, None
            peaks = np.zeros((nf, nA), f)
            for st in range(S):
                for k in range(fps):
                    a = avg[st * fps + k]
                    pk, hd = peak_state[st], hold_state[st]
                    up = a >= pk
                    dec = ~up & (hd <= 0)
                    pk[:] = np.where(up, a, np.where(dec, (pk * f(decay)).astype(f), pk))
                    hd[:] = np.where(up, hold_time, np.where(hd > 0, hd - 1, hd))
                    peaks[st * fps + k] = pk
            return avg, peaks


class HostBackend:
    name = "host"

    def __init__(self, L):
        self.L = L

    def bark_limits(self, sR, bS):
        lim = np.zeros(25, np.int32)
        assert self.L.bnd_host_bark_limits(sR, bS, _p(lim)) == 0
        return lim

    def octave_map(self, sr, n, per):
        m = np.zeros(n, np.int32)
        return m, self.L.bnd_host_octave_map(sr, n, per, _p(m))

    def bark(self, lim, spec):
        spec = np.ascontiguousarray(spec, np.float32)
        nf = spec.shape[0]
        lim = np.ascontiguousarray(lim, np.int32)
        a, b, c, t = np.zeros((nf, 24)), np.zeros((nf, 24)), np.zeros((nf, 24)), np.zeros(nf)
        self.L.bnd_host_bark(_p(lim), _p(spec), spec.shape[1], nf, _p(a), _p(b), _p(c), _p(t))
        return a, b, c, t

    def octave(self, m, nA, mags, S, fps, intercept, slope, hold_time, decay, peak_state=None, hold_state=None):
        mags = np.ascontiguousarray(mags, np.float32)
        m = np.ascontiguousarray(m, np.int32)
        avg = np.zeros((S * fps, nA), np.float32)
        pk = np.zeros((S * fps, nA), np.float32) if peak_state is not None else None
        self.L.bnd_host_octave(_p(m), len(m), nA, _p(mags), mags.shape[1], S, fps, intercept, slope, hold_time, decay, _p(avg), _p(pk),
                               _p(peak_state), _p(hold_state))
        return avg, pk


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def bark_spectra(nframes, bins, seed):
    """Magnitudes with a dynamic range of 2^60 inside every band (a reordered double sum then differs from the sequential one);
    frame 1 silent, frame 2 with a NaN bin, frame 3 with a negative band sum, frame 4 with an Inf (where there are that many)."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(0.5, 1.0, (nframes, bins)) * np.exp2(rng.integers(-50, 11, (nframes, bins)))).astype(np.float32)
    if nframes > 4:
        x[1] = 0.0
        x[2, bins // 3] = np.nan
        x[3, : bins // 2] = -x[3, : bins // 2]
        x[4, bins // 2] = np.inf
    return x


def octave_spectra(nframes, bins, seed):
    """Decaying bursts: every band is seen rising, holding, counting down and decaying; one NaN frame."""
    rng = np.random.default_rng(seed)
    env = np.where(np.arange(nframes) % 13 < 3, 1.0, 0.7 ** (np.arange(nframes) % 13))[:, None]
    x = (rng.uniform(0.2, 1.0, (nframes, bins)) * env).astype(np.float32)
    if nframes > 9:
        x[9, bins // 2] = np.nan
    return x


def ulp64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    both_nan = (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
    neq = (a.view(u) != b.view(u)) & ~both_nan
    assert not neq.any(), "%s: %d of %d values differ bitwise, first at %s" % (what, int(neq.sum()), a.size, tuple(np.argwhere(neq)[0]))


def check_loudness(got, ref, what):
    """(specific, relative, total) against the reference triple within the bounds above; returns the measured maxima."""
    (gs, gr, gt), (rs, rr, rt) = got, ref
    worst = {}
    for name, g, r in (("specific", gs, rs), ("relative", gr, rr), ("total", gt, rt)):
        assert np.array_equal(np.isnan(g), np.isnan(r)), "%s %s: NaN positions differ" % (what, name)
        assert np.array_equal(np.isinf(g), np.isinf(r)), "%s %s: Inf positions differ" % (what, name)
        fin = np.isfinite(r)
        if name == "specific":
            worst[name] = int(ulp64(g[fin], r[fin]).max()) if fin.any() else 0
            assert worst[name] <= ULP_SPECIFIC, (what, name, worst[name])
        else:
            rel = np.abs(g[fin] - r[fin]) / np.maximum(np.abs(r[fin]), 1e-300)
            worst[name] = float(rel.max()) if fin.any() else 0.0
            assert worst[name] <= (REL_RELATIVE if name == "relative" else REL_TOTAL), (what, name, worst[name])
    at = np.isfinite(gs).all(axis=1) & (gs.max(axis=1) > 0)   # relative is exactly 1.0 at each such frame's maximum
    assert (gr[at].max(axis=1) == 1.0).all(), what
    return worst


# ---- the library behind the same interface, and the drivers of tests/golden/bands.npz ---------------------------------------------
class GpuBackend:
    """mxg_bark_batch / mxg_octave_batch on device copies; `m` is the maximilian_amd package on a GPU box."""
    name = "gpu"

    def __init__(self, m):
        self.m, self.lib = m, m.lib()
        self.bark_plans, self.oct_plans = {}, {}

    def bark_limits(self, sR, bS):
        p = self.bark_plans.setdefault((sR, bS), self.lib.mxg_bark_plan_create(sR, bS))
        lim = np.zeros(25, np.int32)
        assert p and self.lib.mxg_bark_plan_limits(p, _p(lim)) == 0
        self._bark = p
        return lim

    def octave_map(self, sr, n, per):
        p = self.oct_plans.setdefault((sr, n, per), self.lib.mxg_octave_plan_create(sr, n, per))
        assert p
        m = np.zeros(n, np.int32)
        assert self.lib.mxg_octave_plan_map(p, _p(m)) == 0
        self._oct = p
        return m, self.lib.mxg_octave_plan_averages(p)

    def bark(self, lim, spec):
        """(the plan of the last bark_limits call)"""
        D = self.m.DeviceBuffer
        spec = np.ascontiguousarray(spec, np.float32)
        nf = spec.shape[0]
        src = D.from_numpy(spec)
        outs = [D((nf, 24), np.float64), D((nf, 24), np.float64), D((nf, 24), np.float64), D(nf, np.float64)]
        self.m._lib.check(self.lib.mxg_bark_batch(self._bark, src.ptr, spec.shape[1], nf, *[o.ptr for o in outs], None), "mxg_bark_batch")
        return tuple(o.numpy() for o in outs)

    def octave(self, m, nA, mags, S, fps, intercept, slope, hold_time, decay, peak_state=None, hold_state=None):
        D = self.m.DeviceBuffer
        mags = np.ascontiguousarray(mags, np.float32)
        src = D.from_numpy(mags)
        avg = D((S * fps, nA), np.float32)
        pk = ps = hs = None
        if peak_state is not None:
            pk, ps, hs = D((S * fps, nA), np.float32), D.from_numpy(peak_state), D.from_numpy(hold_state)
        self.m._lib.check(self.lib.mxg_octave_batch(self._oct, src.ptr, mags.shape[1], S, fps, intercept, slope, hold_time, decay, avg.ptr,
                                                    pk.ptr if pk else None, ps.ptr if ps else None, hs.ptr if hs else None, None),
                          "mxg_octave_batch")
        if peak_state is not None:
            peak_state[:], hold_state[:] = ps.numpy(), hs.numpy()
        return avg.numpy(), pk.numpy() if pk else None


def play_bark_cases(be, g, exact):
    """Every Bark case of bands.npz through a backend: the limits bit for bit; specific / relative / total bit for bit where the
    backend calls the reference's own pow (`exact`: the host build), else within the bounds above.  Returns the measured maxima."""
    worst = {}
    for i, (sR, bS) in enumerate(BARK_CONFIGS):
        lim = be.bark_limits(sR, bS)
        assert lim.tolist() == g["bark/%d/limits" % i].tolist(), (be.name, sR, bS)
        x = bark_spectra(BARK_FRAMES, bS // 2, BARK_SEED)
        _, sp, rl, tt = be.bark(lim, x)
        ref = (g["bark/%d/specific" % i], g["bark/%d/relative" % i], g["bark/%d/total" % i])
        if exact:
            for name, a, b in zip(("specific", "relative", "total"), (sp, rl, tt), ref):
                bits_equal(a, b, "%s %s of (%d, %d) against the reference" % (be.name, name, sR, bS))
        w = check_loudness((sp, rl, tt), ref, "%s (%d, %d) against the reference" % (be.name, sR, bS))
        worst = {k: max(v, worst.get(k, 0)) for k, v in w.items()}
    return worst


def play_octave_cases(be, g, cuts=OCTAVE_CUTS):
    """Every octave case of bands.npz through a backend, the 44 frames cut into calls at `cuts`, state carried: all bit for bit."""
    for i, (sr, n, per) in enumerate(OCTAVE_CONFIGS):
        m, nA = be.octave_map(sr, n, per)
        assert nA == int(g["oct/%d/nAverages" % i]) and m.tolist() == g["oct/%d/map" % i].tolist(), (be.name, sr, n, per)
        x = octave_spectra(OCTAVE_FRAMES, n, OCTAVE_SEED)
        for r, (hold, decay, slope) in enumerate(OCTAVE_RUNS):
            ps, hs = np.zeros((1, nA), np.float32), np.zeros((1, nA), np.int32)
            for a, b in zip(cuts[:-1], cuts[1:]):
                av, pk = be.octave(m, nA, x[a:b], 1, b - a, 1.0, slope, hold, decay, ps, hs)
                what = "%s (%g, %d, %d) run %d frames %d..%d" % (be.name, sr, n, per, r, a, b)
                bits_equal(av, g["oct/%d/%d/averages" % (i, r)][a:b], what + ": averages")
                bits_equal(pk, g["oct/%d/%d/peaks" % (i, r)][a:b], what + ": peaks")
                assert hs[0].tolist() == g["oct/%d/%d/holds" % (i, r)][b - 1].tolist(), what + ": hold counters"
