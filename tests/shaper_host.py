"""Shared by tests/test_shaper_host.py, tests/test_gpu_shaper.py and tools/gen/gen_golden_shaper.py: the host build of
mxg_shaper.h (tests/host_shaper.cpp, g++ under the oracle's FPFLAGS) and the library's K18 entry points behind ONE numpy
interface (HostBackend / GpuBackend), a numpy model that restates the arithmetic (ModelBackend: IEEE + - * / sqrt floor on
arrays, the line's state machine step by step in Python floats), the inputs of tests/golden/shaper.npz that are derived from its
stored integers (one place for the generator and the tests), and drivers that play the file's cases through any backend.

The model and the host build are pinned to shaper.npz by test_shaper_host.py; the model is then the checker of the GPU tests on
shapes the file does not hold.  The model's atanDist / asymclip use numpy's own atan / pow and are only ever compared within
the tolerance of those two modes."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT, assert_bits_equal, ulp_diff

P = ctypes.c_void_p
MODES = {"hardclip": 0, "softclip": 1, "fastatan": 2, "fastAtanDist": 3, "atanDist": 4, "asymclip": 5}
EXACT_MODES = ("hardclip", "fastatan", "fastAtanDist")
PARAM_MODES = ("fastAtanDist", "atanDist", "asymclip")
# ---- tolerances -------------------------------------------------------------------------------
# softclip: (x * x) * x against pow(x, 3): the cubes differ by at most 1 ULP of a value below 1 (2^-53); the rounding of
# x - c / 3 and the one of the product by 2 / 3 may each pass that on once: 2^-52 absolute.
SOFTCLIP_ABS = 2.0 ** -52
# atanDist / asymclip: no error figure for the device library's functions is documented on the build machine, so the OpenCL
# double-precision ceilings stand in: atan 5 ULP, pow 16 ULP; glibc's are within 1.  Two results can then be (E + 1) ULP of the
# function's value apart.  asymclip returns that value (negated): E_POW + 1.  atanDist multiplies it by the factor: the same
# relative distance is up to twice as many ULPs of the product (the position inside the binade), plus half an ULP from each
# rounding of the product: 2 * (E_ATAN + 1) + 1.  With the factor 1.0 / atan(shape) formed on the device too the second atan
# brings the same again and the division one more rounding: 2 * 2 * (E_ATAN + 1) + 2.
E_ATAN, E_POW = 5, 16
ULP_ASYMCLIP = E_POW + 1
ULP_ATANDIST_PV = 2 * (E_ATAN + 1) + 1
ULP_ATANDIST_PS = 2 * 2 * (E_ATAN + 1) + 2
LINE_FRESH_PAR = (0.0, 0.0, 0.0, 1.0, 0.0)   # lineStart, lineEnd, inc, oneShot, trigEnable
LINE_FRESH_ST = (0.0, -1.0, 0.0, 0.0)        # lineValue, lastTrigVal, triggered, lineComplete


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libshaper_host.so")
    flags = [f for f in fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "host_shaper.cpp")])
    L = ctypes.CDLL(so)
    S, I, D = ctypes.c_size_t, ctypes.c_int, ctypes.c_double
    L.shp_host_shape.argtypes = [I, S, S, P, P, P, I, P]
    L.shp_host_atan_norm.restype = D
    L.shp_host_atan_norm.argtypes = [D]
    L.shp_host_xfade.argtypes = [S, S, S, P, P, P, I, P]
    L.shp_host_select.argtypes = [I, S, S, S, P, P, I, I, P, P]
    L.shp_host_line.argtypes = [S, S, P, D, P, P, P]
    L.shp_host_line_prepare.argtypes = [S, P, P, P, P, P, D, P, P]
    return L


def _p(a):
    return None if a is None else a.ctypes.data


def _c(a, t=np.float64):
    return None if a is None else np.ascontiguousarray(a, t)


def line_fresh(V):
    par = np.repeat(np.array(LINE_FRESH_PAR)[:, None], V, axis=1)
    st = np.repeat(np.array(LINE_FRESH_ST)[:, None], V, axis=1)
    return np.ascontiguousarray(par), np.ascontiguousarray(st)


class HostBackend:
    """numpy in, numpy out; `st` of the line is updated in place."""
    name = "host"

    def __init__(self, L):
        self.L = L

    def atan_norm(self, shape):
        return np.array([self.L.shp_host_atan_norm(float(s)) for s in np.asarray(shape).reshape(-1)]).reshape(np.shape(shape))

    def shape(self, mode, x, a=None, b=None):
        """a, b: [V], or [N][V] for one value per sample (both alike).  atanDist per voice: b is the factor, None = formed here."""
        N, V = x.shape
        ps = int(a is not None and np.ndim(a) == 2)
        if mode == "atanDist" and not ps and b is None:
            b = self.atan_norm(a)
        x, a, b = _c(x), _c(a), _c(b)
        out = np.zeros((N, V))
        assert self.L.shp_host_shape(MODES[mode], V, N, _p(x), _p(a), _p(b), ps, _p(out)) == 0
        return out

    def xfade(self, ch1, ch2, xf):
        ch1, ch2, xf = _c(ch1), _c(ch2), _c(xf)
        N, V = ch1.shape[-2:]
        C = 1 if ch1.ndim == 2 else ch1.shape[0]
        out = np.zeros(ch1.shape)
        self.L.shp_host_xfade(C, V, N, _p(ch1), _p(ch2), _p(xf), int(xf.ndim == 2), _p(out))
        return out

    def select(self, interpolate, index, values, normalised):
        """values [K][V] constants or [K][N][V] signals -> (out, nan_count [V])."""
        index, values = _c(index), _c(values)
        N, V = index.shape
        out, cnt = np.zeros((N, V)), np.zeros(V, np.uint32)
        self.L.shp_host_select(int(interpolate), values.shape[0], V, N, _p(index), _p(values), int(values.ndim == 3), int(normalised),
                               _p(cnt), _p(out))
        return out, cnt

    def line(self, trig, N, par, st):
        """trig: [N][V], or a number played on N samples."""
        V = par.shape[1]
        blk = None if np.ndim(trig) == 0 else _c(trig)
        out = np.zeros((N, V))
        self.L.shp_host_line(V, N, _p(blk), 0.0 if blk is not None else float(trig), _p(par), _p(st), _p(out))
        return out


class ModelBackend:
    name = "model"

    def atan_norm(self, shape):
        return 1.0 / np.arctan(np.asarray(shape, np.float64))

    def shape(self, mode, x, a=None, b=None):
        with np.errstate(all="ignore"):
            x = np.asarray(x, np.float64)
            if a is not None:
                a = np.broadcast_to(np.asarray(a, np.float64), x.shape)
            if b is not None:
                b = np.broadcast_to(np.asarray(b, np.float64), x.shape)
            fa = lambda t: t / (1.0 + 0.28 * (t * t))  # noqa: E731
            if mode == "hardclip":
                return np.where(x >= 1, 1.0, np.where(x <= -1, -1.0, x))
            if mode == "softclip":
                return np.where(x >= 1, 1.0, np.where(x <= -1, -1.0, (2 / 3.0) * (x - ((x * x) * x) / 3.0)))
            if mode == "fastatan":
                return fa(x)
            if mode == "fastAtanDist":
                return (1.0 / fa(a)) * fa(x * a)
            if mode == "atanDist":
                return (1.0 / np.arctan(a) if b is None else b) * np.arctan(x * a)
            neg = -np.power(np.where(x < 0, -x, 1.0), a)
            pos = np.power(np.where(x < 0, 1.0, x), b)
            return np.where(x >= 1, 1.0, np.where(x <= -1, -1.0, np.where(x < 0, neg, pos)))

    def xfade(self, ch1, ch2, xf):
        with np.errstate(all="ignore"):
            ch1, ch2 = np.asarray(ch1, np.float64), np.asarray(ch2, np.float64)
            xf = np.broadcast_to(np.asarray(xf, np.float64), ch1.shape[-2:])
            xf = np.where(xf > 1, 1.0, np.where(xf < -1, -1.0, xf))
            val = np.where(1.0 < xf, 1.0, xf)
            val = np.where(val < -1.0, -1.0, val)
            n = ((val - -1.0) / (1.0 - -1.0) * (1.0 - 0.0)) + 0.0
            return (ch1 * np.sqrt(1.0 - n)) + (ch2 * np.sqrt(n))

    def select(self, interpolate, index, values, normalised):
        with np.errstate(all="ignore"):
            index, values = np.array(index, np.float64), np.asarray(values, np.float64)
            N, V = index.shape
            K = values.shape[0]
            vals = values if values.ndim == 3 else np.broadcast_to(values[:, None, :], (K, N, V))
            if normalised:
                index = index * (float(K) - 1e-9)
            index = np.where(index < 0, 0.0, np.where(index >= K, float(K - 1), index))
            nan = np.isnan(index)
            index = np.where(nan, 0.0, index)
            nn, vv = np.meshgrid(np.arange(N), np.arange(V), indexing="ij")
            if not interpolate:
                return vals[index.astype(np.int64), nn, vv], nan.sum(axis=0).astype(np.uint32)
            a1 = np.floor(index).astype(np.int64)
            mix = index - a1.astype(np.float64)
            a2 = np.where(a1 + 1 == K, 0, a1 + 1)
            return (vals[a1, nn, vv] * (1.0 - mix)) + (vals[a2, nn, vv] * mix), nan.sum(axis=0).astype(np.uint32)

    def line(self, trig, N, par, st):
        V = par.shape[1]
        out = np.zeros((N, V))
        for v in range(V):
            start, end, inc = (float(par[i, v]) for i in range(3))
            one, en = par[3, v] != 0, par[4, v] != 0
            val, last, trg, done = float(st[0, v]), float(st[1, v]), st[2, v] != 0, st[3, v] != 0
            ts = [float(trig)] * N if np.ndim(trig) == 0 else trig[:, v].tolist()
            res = []
            for t in ts:
                if not done:
                    if en and not trg:
                        trg = t > 0.0 and last <= 0.0
                        val = start
                    if trg:
                        val = float(np.float64(val) + np.float64(inc))
                        done = (val <= end) if inc <= 0 else (val >= end)
                        if done and not one:
                            trg = done = False
                    last = t
                res.append(val)
            out[:, v] = res
            st[:, v] = [val, last, float(trg), float(done)]
        return out


def line_prepare_model(par, st, v, start, end, ms, oneshot, sr):
    """maxiLine::prepare on voice v: lineValue takes the previous lineStart."""
    with np.errstate(all="ignore"):
        st[0, v] = par[0, v]
        par[0, v], par[1, v] = start, end
        par[2, v] = (np.float64(end) - np.float64(start)) / (np.float64(ms) / 1000.0 * np.float64(sr))
        par[3, v] = 1.0 if oneshot else 0.0
        st[2, v] = st[3, v] = 0.0


class GpuBackend:
    """The library's entry points; everything is uploaded before and downloaded after every call."""
    name = "gpu"

    def __init__(self, mx):
        self.mx = mx

    def atan_norm(self, shape):
        return self.mx.atan_norm(shape)

    def shape(self, mode, x, a=None, b=None):
        mx, D = self.mx, self.mx.DeviceBuffer
        N, V = x.shape
        ps = int(a is not None and np.ndim(a) == 2)
        if mode == "atanDist" and not ps and b is None:
            b = self.atan_norm(a)
        dx, out = D.from_numpy(_c(x)), D((N, V))
        da, db = (None if t is None else D.from_numpy(_c(t)) for t in (a, b))
        mx._lib.check(mx.lib().mxg_shape_render(MODES[mode], V, N, dx.ptr, da and da.ptr, db and db.ptr, ps, out.ptr, None), "mxg_shape_render")
        return out.numpy()

    def xfade(self, ch1, ch2, xf):
        mx, D = self.mx, self.mx.DeviceBuffer
        ch1, ch2, xf = _c(ch1), _c(ch2), _c(xf)
        N, V = ch1.shape[-2:]
        C = 1 if ch1.ndim == 2 else ch1.shape[0]
        d1, d2, dxf, out = D.from_numpy(ch1), D.from_numpy(ch2), D.from_numpy(xf), D(ch1.shape)
        mx._lib.check(mx.lib().mxg_xfade_render(C, V, N, d1.ptr, d2.ptr, dxf.ptr, int(xf.ndim == 2), out.ptr, None), "mxg_xfade_render")
        return out.numpy()

    def select(self, interpolate, index, values, normalised):
        mx, D = self.mx, self.mx.DeviceBuffer
        index, values = _c(index), _c(values)
        N, V = index.shape
        di, dv, out, cnt = D.from_numpy(index), D.from_numpy(values), D((N, V)), D(V, np.uint32)
        mx._lib.check(mx.lib().mxg_select_render(int(interpolate), values.shape[0], V, N, di.ptr, dv.ptr, int(values.ndim == 3),
                                                 int(normalised), cnt.ptr, out.ptr, None), "mxg_select_render")
        return out.numpy(), cnt.numpy()

    def line(self, trig, N, par, st):
        mx, D = self.mx, self.mx.DeviceBuffer
        V = par.shape[1]
        blk = None if np.ndim(trig) == 0 else D.from_numpy(_c(trig))
        dpar, dst, out = D.from_numpy(_c(par)), D.from_numpy(_c(st)), D((N, V))
        mx._lib.check(mx.lib().mxg_line_render(V, N, blk and blk.ptr, 0.0 if blk is not None else float(trig), dpar.ptr, dst.ptr, out.ptr,
                                               None), "mxg_line_render")
        st[...] = dst.numpy()
        assert dpar.numpy().tobytes() == _c(par).tobytes()   # parameters are read only
        return out.numpy()


# ---- the inputs of tests/golden/shaper.npz that are derived from its stored integers -----------------------------------
NPS = 400    # samples of the cases with a parameter per sample
NX = 600     # samples of the xfade and select cases
NXV = 200    # samples of the xfade case with a per-voice xfader
ASYM_V = 2   # asymclip plays voices 0 and 1: the patched -0.0 samples are in voice 2 (pow(-0.0, b) has a sign rule of its own)


def signal(g):
    """[N][3] in [-1.5, 1.5], with the patched exact +-1, 0.0, -0.0 and the one NaN."""
    x = g["q"] / 16384.0
    for n, v, val in g["patches"]:
        x[int(n), int(v)] = val
    return np.ascontiguousarray(x)


def unit(pq):
    return (pq.astype(np.float64) + 32768.0) / 65535.0


def per_sample_params(g):
    """shape in [0.5, 50] [NPS][3]; a, b in [0.25, 8] [NPS][2]."""
    u = unit(g["pq"])
    return (np.ascontiguousarray(0.5 + 49.5 * u), np.ascontiguousarray(0.25 + 7.75 * u[:, :ASYM_V]),
            np.ascontiguousarray(0.25 + 7.75 * u[::-1, :ASYM_V]))


def xfade_inputs(g):
    x = signal(g)
    ch1 = np.stack([x[0:NX], x[NX:2 * NX]])
    ch2 = np.stack([x[2 * NX:3 * NX], x[1400:1400 + NX]])
    return ch1, ch2, np.ascontiguousarray(x[300:300 + NX])   # the xfader passes both clamps: the signal reaches +-1.5


def select_inputs(g):
    """(index, values, normalised) of the two cases: K = 5 constants, index in [-0.5, 5.5]; K = 4 signals, normalised index in
    [-0.1, 1.1]."""
    x = signal(g)[:NX]
    assert not np.isnan(x).any()
    return {"const": ((x + 1.5) / 3.0 * 6.0 - 0.5, g["sel/const/values"], False),
            "sig": ((x + 1.5) / 3.0 * 1.2 - 0.1, g["sel/sig/vq"] / 16384.0, True)}


def line_trigger(g):
    return np.ascontiguousarray(g["line/tq"] / 4.0)


# ---- drivers ---------------------------------------------------------------------------------------------------------------
def cut_list(g, N, extra=()):
    return sorted(set(c for c in list(g["cuts"].tolist()) + list(extra) if c <= N) | {0, N})


def play_blocks(fn, N, cuts):
    return np.concatenate([fn(a, b) for a, b in zip(cuts[:-1], cuts[1:])], axis=-2)


def check_shape(name, mode, got, ref, ps, xin=None):
    """One shaping mode against the reference's stream: bits, the softclip bound, or ULPs of the reference value.  xin: the
    input, for the modes with clipped branches (|x| >= 1 gives exactly +-1)."""
    what = "%s: %s" % (name, mode)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN positions"
    if mode in EXACT_MODES:
        assert_bits_equal(got, ref, what)
        return 0
    x = np.where(np.isnan(ref), 0.0, ref)
    y = np.where(np.isnan(ref), 0.0, got)
    if mode in ("softclip", "asymclip"):
        clipped = np.abs(xin) >= 1.0
        assert (np.abs(x[clipped]) == 1.0).all()
        assert_bits_equal(y[clipped], x[clipped], what + ": clipped branches")
    if mode == "softclip":
        err = float(np.abs(y - x).max())
        print("%s: max abs error %.3e (bound %.3e)" % (what, err, SOFTCLIP_ABS))
        assert err <= SOFTCLIP_ABS, what
        return err
    bound = ULP_ASYMCLIP if mode == "asymclip" else (ULP_ATANDIST_PS if ps else ULP_ATANDIST_PV)
    worst = int(ulp_diff(y, x).max())
    print("%s: max %d ULP (bound %d)" % (what, worst, bound))
    assert worst <= bound, what
    return worst


def play_shape_cases(be, g, extra=()):
    """Every mode with per-voice and per-sample parameters, cut as stored and at `extra`; -> {(mode, ps): measured figure}."""
    x = signal(g)
    res = {}
    shape_ps, a_ps, b_ps = per_sample_params(g)
    for mode in MODES:
        xs = x[:, :ASYM_V] if mode == "asymclip" else x
        if mode == "asymclip":
            a, b = g["shape/pv/asym_a"], g["shape/pv/asym_b"]
        elif mode in PARAM_MODES:
            a, b = g["shape/pv/shape"], (g["shape/pv/norm"] if mode == "atanDist" else None)
        else:
            a = b = None
        cuts = cut_list(g, x.shape[0], extra)
        got = play_blocks(lambda s, e: be.shape(mode, np.ascontiguousarray(xs[s:e]), a, b), x.shape[0], cuts)
        res[(mode, 0)] = check_shape("per voice", mode, got, g["shape/pv/" + mode].astype(np.float64), 0, xs)
        if mode in PARAM_MODES:
            a, b = (a_ps, b_ps) if mode == "asymclip" else (shape_ps[:, :xs.shape[1]], None)
            cuts = cut_list(g, NPS, extra)
            got = play_blocks(lambda s, e: be.shape(mode, np.ascontiguousarray(xs[s:e]), a[s:e], None if b is None else b[s:e]), NPS, cuts)
            res[(mode, 1)] = check_shape("per sample", mode, got, g["shape/ps/" + mode], 1, xs[:NPS])
    res[("softclip_u", 0)] = check_shape("uniform draws", "softclip", be.shape("softclip", g["softclip_u/x"]), g["softclip_u/out"], 0, g["softclip_u/x"])
    z = be.shape("asymclip", g["asym_zero/x"], g["asym_zero/a"], g["asym_zero/b"])
    assert_bits_equal(z, g["asym_zero/out"], "asymclip of -0.0")
    assert np.array_equal(np.signbit(z), np.signbit(g["asym_zero/out"])), "asymclip of -0.0: the sign of zero"
    return res


def play_xfade_cases(be, g, extra=()):
    ch1, ch2, xf = xfade_inputs(g)
    cuts = cut_list(g, NX, extra)
    got = play_blocks(lambda s, e: be.xfade(ch1[:, s:e], ch2[:, s:e], xf[s:e]), NX, cuts)
    assert_bits_equal(got, g["xfade/ps"], "xfade, an xfader per sample, C = 2")
    got = play_blocks(lambda s, e: be.xfade(ch1[0, s:e], ch2[0, s:e], xf[s:e]), NX, cuts)
    assert_bits_equal(got, g["xfade/ps"][0], "xfade, an xfader per sample, C = 1")
    cuts = cut_list(g, NXV, extra)
    got = play_blocks(lambda s, e: be.xfade(ch1[:, s:e], ch2[:, s:e], g["xfade/pv_xf"]), NXV, cuts)
    assert_bits_equal(got, g["xfade/pv"], "xfade, an xfader per voice")


def play_select_cases(be, g, extra=()):
    cuts = cut_list(g, NX, extra)
    for name, (index, values, normalised) in select_inputs(g).items():
        for interp, key in ((0, "select"), (1, "selectx")):
            def blk(s, e):
                out, cnt = be.select(interp, index[s:e], values[:, s:e] if values.ndim == 3 else values, normalised)
                assert not cnt.any()
                return out
            assert_bits_equal(play_blocks(blk, NX, cuts), g["sel/%s/%s" % (name, key)], "select %s %s" % (name, key))


def line_events(g):
    """{sample: [(kind, voice, start / on, end, ms, oneshot)]}: kind 0 = prepare, 1 = triggerEnable."""
    ev = {}
    for n, kind, v, a, b, ms, one in g["line/events"].tolist():
        ev.setdefault(int(n), []).append((int(kind), int(v), a, b, ms, int(one)))
    return ev


def play_line_case(be, g, prepare, extra=()):
    """The line case: events applied at their cuts through `prepare(par, st, v, start, end, ms, oneshot, sr)`; the output and
    the state arrays at every stored cut are the reference's bits."""
    trig = line_trigger(g)
    N, V = trig.shape
    sr = float(g["sr"])
    ev = line_events(g)
    par, st = line_fresh(V)
    cuts = cut_list(g, N, extra)
    stored = g["cuts"].tolist()
    out = np.zeros((N, V))
    for a, b in zip(cuts[:-1], cuts[1:]):
        for kind, v, p0, p1, ms, one in ev.get(a, []):
            if kind == 0:
                prepare(par, st, v, p0, p1, ms, one, sr)
            else:
                par[4, v] = 1.0 if p0 > 0.0 else 0.0
        out[a:b] = be.line(trig[a:b], b - a, par, st)
        if b in stored:
            i = stored.index(b) - 1
            assert_bits_equal(par, g["line/snap%d/par" % i], "line: parameters at cut %d" % b)
            assert_bits_equal(st, g["line/snap%d/st" % i], "line: state at cut %d" % b)
    assert_bits_equal(out, g["line/out"], "line")
    # the line.play(1) idiom: fresh lines prepared with the same first events, a constant trigger
    par, st = line_fresh(V)
    for kind, v, p0, p1, ms, one in ev[0]:
        if kind == 0:
            prepare(par, st, v, p0, p1, ms, one, sr)
        else:
            par[4, v] = 1.0 if p0 > 0.0 else 0.0
    n = g["line_const/out"].shape[0]
    got = np.concatenate([be.line(1.0, 7, par, st), be.line(1.0, n - 7, par, st)])
    assert_bits_equal(got, g["line_const/out"], "line.play(1)")
    assert_bits_equal(st, g["line_const/st"], "line.play(1): state")
