"""Shared by tests/test_classic_host.py, tests/test_gpu_classic.py and tools/gen/gen_golden_classic.py: the host build of
mxg_classic.h (tests/host_classic.cpp, g++ under the oracle's FPFLAGS) and the library's K23 entry points behind ONE numpy
interface (HostBackend / GpuBackend), a numpy / Python-float model that restates the arithmetic (ModelBackend), the inputs of
tests/golden/classic.npz that are derived from its stored integers (one place for the generator and the tests), the a-priori
tolerances of the four transcendental map modes, and drivers that play the file's cases through any backend.

The model and the host build are pinned to classic.npz by test_classic_host.py; the host build is then the checker of the GPU
tests on shapes the file does not hold."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT, assert_bits_equal, ulp_diff

P = ctypes.c_void_p
MAP_MODES = {"linlin": 0, "linexp": 1, "explin": 2, "clamp": 3, "ampToDbs": 4, "dbsToAmp": 5}
EXACT_MAPS = ("linlin", "clamp")
PS_THRESHOLD, PS_ATTACK, PS_RELEASE, PS_RATIO = 1, 2, 4, 8
# ---- tolerances of the transcendental map modes, fixed before the first GPU run -----------------
# No error figure for the device library's functions is documented, so the OpenCL double-precision ceilings stand in: pow 16 ULP,
# log / log10 3 ULP; glibc's are within 1.  Two results of one function on the same operand can then be (E + 1) ULP of the
# function's value apart.  Every operand of a transcendental is formed by the same IEEE operations on both sides (the clip, val -
# inMin, the quotients), so it is the same double.
E_POW, E_LOG = 16, 3
# dbsToAmp = pow(10.0, dbs * 0.05): the function's value itself.
ULP_DBSTOAMP = E_POW + 1
# linexp = pow(outMax / outMin, t) * outMin: the same relative distance is up to twice as many ULPs of the product (the position
# inside the binade), plus half an ULP from each side's rounding of the product.
ULP_LINEXP = 2 * (E_POW + 1) + 1


def amptodbs_bound(ref):
    """|got - ref| for ampToDbs = log10(amp) * 20.0, per element: the two log10 values L are (E_LOG + 1) ULP(L) apart, the
    product by 20.0 carries that times 20 and rounds once on each side (half an ULP of the result each)."""
    y = np.abs(np.where(np.isfinite(ref), ref, 0.0))
    return (E_LOG + 1) * np.spacing(y / 20.0) * 20.0 + np.spacing(y)


def explin_bound(x, rng, aux):
    """|got - ref| for explin = (log(val / inMin) / den * span) + outMin, per element, from the inputs alone: l = log(q) differs
    by (E_LOG + 1) ULP(l); the division by den (the same double on both sides) and the product by span scale that; each of the
    three later roundings (quotient, product, sum) adds half an ULP of its own result per side."""
    with np.errstate(all="ignore"):
        i0, i1, o0, o1 = (np.broadcast_to(r, x.shape) for r in rng)
        den = np.broadcast_to(aux, x.shape)
        val = np.where(i1 < x, i1, x)
        val = np.where(val < i0, i0, val)
        l = np.abs(np.log(val / i0))
        span = np.abs(o1 - o0)
        a = l / np.abs(den)
        b = a * span
        y = np.abs((np.log(val / i0) / den * (o1 - o0)) + o0)
        bound = (E_LOG + 1) * np.spacing(l) / np.abs(den) * span + np.spacing(a) * span + np.spacing(b) + np.spacing(y)
        return np.where(np.isfinite(bound), bound, 0.0)


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libclassic_host.so")
    flags = [f for f in fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "host_classic.cpp")])
    L = ctypes.CDLL(so)
    S, I, D = ctypes.c_size_t, ctypes.c_int, ctypes.c_double
    L.cls_h_gate.argtypes = [S, S, P, P, P, P, I, P, P, P, P]
    L.cls_h_compress.argtypes = [S, S, P, P, P, P, P, P, I, P, P, P]
    L.cls_h_line.argtypes = [S, S, S, P, P, P, P, P, D, P, P, P]
    L.cls_h_lag.argtypes = [S, S, P, P, P, I, P, P]
    L.cls_h_map.argtypes = [I, S, S, P, P, P, P]
    for f in (L.cls_h_makeup, L.cls_h_coeff, L.cls_h_explin_den):
        f.restype = D
    L.cls_h_makeup.argtypes = [D]
    L.cls_h_coeff.argtypes = [D, D]
    L.cls_h_explin_den.argtypes = [D, D]
    return L


def _p(a):
    return None if a is None else a.ctypes.data


def _c(a, t=np.float64):
    return None if a is None else np.ascontiguousarray(a, t)


def dyn_fresh(V):
    return np.zeros((3, V)), np.zeros((4, V), np.int64)


def env_fresh(V):
    return np.zeros((2, V)), np.zeros((2, V), np.int32)


def ps_flags(thr, att, rel, ratio=None):
    return (PS_THRESHOLD * (np.ndim(thr) == 2) + PS_ATTACK * (np.ndim(att) == 2) + PS_RELEASE * (np.ndim(rel) == 2) +
            PS_RATIO * (ratio is not None and np.ndim(ratio) == 2))


class HostBackend:
    """numpy in, numpy out; the state arrays are updated in place.  A parameter is [V], or [N][V] for one value per sample."""
    name = "host"

    def __init__(self, L):
        self.L = L

    def makeup(self, ratio):
        return np.array([self.L.cls_h_makeup(float(r)) for r in np.asarray(ratio).reshape(-1)]).reshape(np.shape(ratio))

    def coeff(self, ms, sr):
        return self.L.cls_h_coeff(float(ms), float(sr))

    def explin_den(self, rng):
        return np.array([self.L.cls_h_explin_den(float(a), float(b)) for a, b in zip(rng[0], rng[1])])

    def gate(self, x, thr, hold, att, rel, dst, ist):
        N, V = x.shape
        x, thr, att, rel, hold = _c(x), _c(thr), _c(att), _c(rel), _c(hold, np.int64)
        out = np.zeros((N, V))
        self.L.cls_h_gate(V, N, _p(x), _p(thr), _p(att), _p(rel), ps_flags(thr, att, rel), _p(hold), _p(dst), _p(ist), _p(out))
        return out

    def compress(self, x, ratio, thr, att, rel, dst, ist, makeup=None):
        N, V = x.shape
        makeup = self.makeup(ratio) if makeup is None else makeup
        x, ratio, makeup, thr, att, rel = _c(x), _c(ratio), _c(makeup), _c(thr), _c(att), _c(rel)
        out = np.zeros((N, V))
        self.L.cls_h_compress(V, N, _p(x), _p(ratio), _p(makeup), _p(thr), _p(att), _p(rel), ps_flags(thr, att, rel, ratio), _p(dst), _p(ist), _p(out))
        return out

    def line(self, N, seg, count, trig, tindex, tamp, sr, dst, ist):
        S, V = seg.shape
        seg, count, trig, tindex, tamp = _c(seg), _c(count, np.int32), _c(trig), _c(tindex, np.int32), _c(tamp)
        out = np.zeros((N, V))
        self.L.cls_h_line(V, N, S, _p(seg), _p(count), _p(trig), _p(tindex), _p(tamp), float(sr), _p(dst), _p(ist), _p(out))
        return out

    def lag(self, x, alpha, recip, val):
        N, V = x.shape
        x, alpha, recip = _c(x), _c(alpha), _c(recip)
        out = np.zeros((N, V))
        self.L.cls_h_lag(V, N, _p(x), _p(alpha), _p(recip), int(alpha.ndim == 2), _p(val), _p(out))
        return out

    def map(self, mode, x, rng=None, aux=None):
        N, V = x.shape
        if mode == "explin" and aux is None:
            aux = self.explin_den(rng)
        x, rng, aux = _c(x), _c(rng), _c(aux)
        out = np.zeros((N, V))
        assert self.L.cls_h_map(MAP_MODES[mode], V, N, _p(x), _p(rng), _p(aux), _p(out)) == 0
        return out


def _col(p, N, v):
    """The N values voice v sees of a parameter that is [V] or [N][V], as Python floats."""
    p = np.asarray(p, np.float64)
    return [float(p[v])] * N if p.ndim == 1 else p[:, v].tolist()


class ModelBackend:
    """The state machines statement by statement in Python floats (IEEE doubles), the maps on numpy arrays."""
    name = "model"

    def makeup(self, ratio):
        with np.errstate(all="ignore"):
            return 1 + np.log(np.asarray(ratio, np.float64))

    def coeff(self, ms, sr):
        return float(np.power(0.01, 1.0 / (np.float64(ms) * np.float64(sr) * 0.001)))

    def explin_den(self, rng):
        with np.errstate(all="ignore"):
            return np.log(np.asarray(rng[1], np.float64) / np.asarray(rng[0], np.float64))

    def gate(self, x, thr, hold, att, rel, dst, ist):
        N, V = x.shape
        out = np.zeros((N, V))
        for v in range(V):
            amp, cur, o = (float(t) for t in dst[:, v])
            hc, ap, hp, rp = (int(t) for t in ist[:, v])
            ht = int(hold[v])
            res = []
            for xi, th, at, re_ in zip(x[:, v].tolist(), _col(thr, N, v), _col(att, N, v), _col(rel, N, v)):
                if abs(xi) > th and ap != 1:
                    hc, rp, ap = 0, 0, 1
                    if amp == 0:
                        amp = 0.01
                if ap == 1 and amp < 1:
                    amp *= (1 + at)
                    o = xi * amp
                if amp >= 1:
                    ap, hp = 0, 1
                if hc < ht and hp == 1:
                    o = xi
                    hc += 1
                if hc == ht:
                    hp, rp = 0, 1
                if rp == 1 and amp > 0.:
                    amp *= re_
                    o = xi * amp
                res.append(o)
            out[:, v] = res
            dst[:, v] = [amp, cur, o]
            ist[:, v] = [hc, ap, hp, rp]
        return out

    def compress(self, x, ratio, thr, att, rel, dst, ist, makeup=None):
        N, V = x.shape
        makeup = self.makeup(ratio) if makeup is None else makeup
        out = np.zeros((N, V))
        with np.errstate(all="ignore"):
            for v in range(V):
                amp, cur, o = (float(t) for t in dst[:, v])
                hc, ap, hp, rp = (int(t) for t in ist[:, v])
                res = []
                for xi, ra, mk, th, at, re_ in zip(x[:, v].tolist(), _col(ratio, N, v), _col(makeup, N, v), _col(thr, N, v), _col(att, N, v), _col(rel, N, v)):
                    if abs(xi) > th and ap != 1:
                        hc, rp, ap = 0, 0, 1
                        if cur == 0:
                            cur = ra
                    if ap == 1 and cur < ra - 1:
                        cur *= (1 + at)
                    if cur >= ra - 1:
                        ap, rp = 0, 1
                    if rp == 1 and cur > 0.:
                        cur *= re_
                    o = float(np.float64(xi) / np.float64(1. + cur))
                    res.append(float(np.float64(o) * np.float64(mk)))
                out[:, v] = res
                dst[:, v] = [amp, cur, o]
                ist[:, v] = [hc, ap, hp, rp]
        return out

    def line(self, N, seg, count, trig, tindex, tamp, sr, dst, ist):
        S, V = seg.shape
        out = np.zeros((N, V))
        f = np.float64
        with np.errstate(all="ignore"):
            for v in range(V):
                n = min(max(int(count[v]), 1), S)
                tab = seg[:, v].tolist()
                amp, start = float(dst[0, v]), float(dst[1, v])
                vi, playing = int(ist[0, v]), int(ist[1, v])
                ts = None if trig is None else trig[:, v].tolist()
                res = []
                for i in range(N):
                    if ts is not None and ts[i] != 0.0:
                        playing, vi, amp = 1, min(max(int(tindex[v]), 0), max(n - 2, 0)), float(tamp[v])
                    if playing == 1:
                        a = min(max(vi, 0), n - 1)
                        period = f(4.) / (f(tab[min(a + 1, n - 1)]) * f(0.0044))
                        cur = tab[a]
                        if cur - amp > 0.0000001 and vi < n:
                            amp = float(f(amp) + ((f(cur) - f(start)) / (f(sr) / period)))
                        elif cur - amp < -0.0000001 and vi < n:
                            amp = float(f(amp) - (((f(cur) - f(start)) * f(-1)) / (f(sr) / period)))
                        elif vi > n - 1:
                            vi = n - 2
                        else:
                            vi += 2
                            start = cur
                        res.append(amp)
                    else:
                        res.append(0.0)
                out[:, v] = res
                dst[:, v] = [amp, start]
                ist[:, v] = [vi, playing]
        return out

    def lag(self, x, alpha, recip, val):
        N, V = x.shape
        out = np.zeros((N, V))
        with np.errstate(all="ignore"):
            a = np.broadcast_to(np.asarray(alpha, np.float64), (N, V))
            r = np.broadcast_to(np.asarray(recip, np.float64), (N, V))
            y = np.array(val, np.float64)
            for n in range(N):
                y = (a[n] * x[n]) + (r[n] * y)
                out[n] = y
            val[...] = y
        return out

    def map(self, mode, x, rng=None, aux=None):
        with np.errstate(all="ignore"):
            x = np.asarray(x, np.float64)
            if mode == "ampToDbs":
                return np.log10(x) * 20.0
            if mode == "dbsToAmp":
                return np.power(10.0, x * 0.05)
            i0, i1 = (np.broadcast_to(r, x.shape) for r in rng[:2])
            if mode == "clamp":
                return np.where(x > i1, i1, np.where(x < i0, i0, x))
            o0, o1 = (np.broadcast_to(r, x.shape) for r in rng[2:4])
            val = np.where(i1 < x, i1, x)
            val = np.where(val < i0, i0, val)
            if mode == "linlin":
                return ((val - i0) / (i1 - i0) * (o1 - o0)) + o0
            if mode == "linexp":
                return np.power((o1 / o0), (val - i0) / (i1 - i0)) * o0
            den = np.broadcast_to(self.explin_den(rng) if aux is None else aux, x.shape)
            return (np.log(val / i0) / den * (o1 - o0)) + o0


class GpuBackend:
    """The library's entry points; everything is uploaded before and downloaded after every call."""
    name = "gpu"

    def __init__(self, mx):
        self.mx = mx
        self.lib = mx.lib()

    def makeup(self, ratio):
        return np.array([self.lib.mxg_dyn_makeup_host(float(r)) for r in np.asarray(ratio).reshape(-1)]).reshape(np.shape(ratio))

    def coeff(self, ms, sr):
        return self.lib.mxg_dyn_coeff_host(float(ms), float(sr))

    def explin_den(self, rng):
        rng = _c(rng)
        aux = np.zeros(rng.shape[1])
        self.mx._lib.check(self.lib.mxg_map_range_host(MAP_MODES["explin"], rng.shape[1], _p(rng), _p(aux)), "mxg_map_range_host")
        return aux

    def _dev(self, *arrays):
        D = self.mx.DeviceBuffer
        return [None if a is None else D.from_numpy(a) for a in arrays]

    def gate(self, x, thr, hold, att, rel, dst, ist):
        N, V = x.shape
        thr, att, rel = _c(thr), _c(att), _c(rel)
        dx, dt, da, dr, dh, dd, di = self._dev(_c(x), thr, att, rel, _c(hold, np.int64), _c(dst), _c(ist, np.int64))
        out = self.mx.DeviceBuffer((N, V))
        self.mx._lib.check(self.lib.mxg_dyn_gate_render(V, N, dx.ptr, dt.ptr, da.ptr, dr.ptr, ps_flags(thr, att, rel), dh.ptr, dd.ptr, di.ptr, out.ptr,
                                                        None), "mxg_dyn_gate_render")
        dst[...], ist[...] = dd.numpy(), di.numpy()
        return out.numpy()

    def compress(self, x, ratio, thr, att, rel, dst, ist, makeup=None):
        N, V = x.shape
        makeup = self.makeup(ratio) if makeup is None else makeup
        ratio, thr, att, rel = _c(ratio), _c(thr), _c(att), _c(rel)
        dx, dq, dm, dt, da, dr, dd, di = self._dev(_c(x), ratio, _c(makeup), thr, att, rel, _c(dst), _c(ist, np.int64))
        out = self.mx.DeviceBuffer((N, V))
        self.mx._lib.check(self.lib.mxg_dyn_compress_render(V, N, dx.ptr, dq.ptr, dm.ptr, dt.ptr, da.ptr, dr.ptr, ps_flags(thr, att, rel, ratio),
                                                            dd.ptr, di.ptr, out.ptr, None), "mxg_dyn_compress_render")
        dst[...], ist[...] = dd.numpy(), di.numpy()
        return out.numpy()

    def line(self, N, seg, count, trig, tindex, tamp, sr, dst, ist):
        S, V = seg.shape
        assert int(self.lib.mxg_sample_rate()) == int(sr), "the sample rate in force is mxg_settings's"
        ds, dc, dt, dx, da, dd, di = self._dev(_c(seg), _c(count, np.int32), _c(trig), _c(tindex, np.int32), _c(tamp), _c(dst), _c(ist, np.int32))
        out = self.mx.DeviceBuffer((N, V))
        self.mx._lib.check(self.lib.mxg_envelope_line_render(V, N, S, ds.ptr, dc.ptr, dt and dt.ptr, dx and dx.ptr, da and da.ptr, dd.ptr, di.ptr,
                                                             out.ptr, None), "mxg_envelope_line_render")
        dst[...], ist[...] = dd.numpy(), di.numpy()
        assert ds.numpy().tobytes() == _c(seg).tobytes()   # the tables are read only
        return out.numpy()

    def lag(self, x, alpha, recip, val):
        N, V = x.shape
        alpha, recip = _c(alpha), _c(recip)
        dx, da, dr, dv = self._dev(_c(x), alpha, recip, _c(val))
        out = self.mx.DeviceBuffer((N, V))
        self.mx._lib.check(self.lib.mxg_lag_render(V, N, dx.ptr, da.ptr, dr.ptr, int(alpha.ndim == 2), dv.ptr, out.ptr, None), "mxg_lag_render")
        val[...] = dv.numpy()
        return out.numpy()

    def map(self, mode, x, rng=None, aux=None):
        N, V = x.shape
        if mode == "explin" and aux is None:
            aux = self.explin_den(rng)
        dx, dr, da = self._dev(_c(x), _c(rng), _c(aux))
        out = self.mx.DeviceBuffer((N, V))
        self.mx._lib.check(self.lib.mxg_map_render(MAP_MODES[mode], V, N, dx.ptr, dr and dr.ptr, da and da.ptr, out.ptr, None), "mxg_map_render")
        return out.numpy()


# ---- the inputs of tests/golden/classic.npz that are derived from its stored integers --------------------------------------
def signal(q):
    """int16 -> doubles in [-2, 2) with full use of the grid q / 16384."""
    return np.ascontiguousarray(q.astype(np.float64) / 16384.0)


def patched(q, patches):
    x = signal(q)
    for n, v, val in np.asarray(patches).reshape(-1, 3):
        x[int(n), int(v)] = val
    return x


def env_trigger_block(g):
    return np.ascontiguousarray(g["env/tq"].astype(np.float64) / 2.0)


# ---- drivers ---------------------------------------------------------------------------------------------------------------
def cut_list(g, N, extra=()):
    return sorted(set(c for c in list(g["cuts"].tolist()) + list(extra) if c <= N) | {0, N})


def play_gate_case(be, g, extra=()):
    x = signal(g["gate/q"])
    N, V = x.shape
    thr, att, rel, hold = g["gate/thr"], g["gate/att"], g["gate/rel"], g["gate/hold"]
    dst, ist = dyn_fresh(V)
    stored = g["cuts"].tolist()
    cuts = cut_list(g, N, extra)
    out = np.zeros((N, V))
    for a, b in zip(cuts[:-1], cuts[1:]):
        out[a:b] = be.gate(x[a:b], thr, hold, att, rel, dst, ist)
        if b in stored:
            i = stored.index(b) - 1
            assert_bits_equal(dst, g["gate/snap%d/dst" % i], "gate: dst at cut %d" % b)
            assert np.array_equal(ist, g["gate/snap%d/ist" % i]), "gate: ist at cut %d" % b
    assert_bits_equal(out, g["gate/out"], "gate")


def play_compress_case(be, g, extra=()):
    """Bank A: three voices through compressor(), the ratio of voice 2 changes at a cut.  Bank B: one voice through compress(),
    whose parameters are the members its setters left (stored; the coefficients are also what coeff() gives)."""
    x = signal(g["comp/q"])
    N = x.shape[0]
    stored = g["cuts"].tolist()
    cuts = cut_list(g, N, extra)
    change = int(g["comp/change_at"])
    assert change in cuts
    xa, V = x[:, :3], 3
    dst, ist = dyn_fresh(V)
    out = np.zeros((N, V))
    for a, b in zip(cuts[:-1], cuts[1:]):
        ratio = g["comp/ratio_late" if a >= change else "comp/ratio"]
        out[a:b] = be.compress(xa[a:b], ratio, g["comp/thr"], g["comp/att"], g["comp/rel"], dst, ist, g["comp/makeup_late" if a >= change else "comp/makeup"])
        if b in stored:
            i = stored.index(b) - 1
            assert_bits_equal(dst, g["comp/snap%d/dst" % i], "compressor: dst at cut %d" % b)
            assert np.array_equal(ist, g["comp/snap%d/ist" % i]), "compressor: ist at cut %d" % b
    assert_bits_equal(out, g["comp/out"], "compressor")
    ratio, thr, att, rel = (np.array([t]) for t in g["comp/members"])
    dst, ist = dyn_fresh(1)
    xb = np.ascontiguousarray(x[:, 3:4])
    got = np.concatenate([be.compress(xb[a:b], ratio, thr, att, rel, dst, ist, g["comp/members_makeup"]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert_bits_equal(got, g["comp/out_members"], "compress() with the setters")
    assert_bits_equal(dst, g["comp/members_dst"], "compress(): dst")
    assert np.array_equal(ist, g["comp/members_ist"]), "compress(): ist"


def env_events(g):
    ev = {}
    for n, v, index, amp in g["env/events"].tolist():
        ev.setdefault(int(n), []).append((int(v), int(index), amp))
    return ev


def play_env_case(be, g, trigger, extra=(), key="env", sr=None):
    """The envelope case: triggers inside blocks through the trigger block, triggers between launches at their cuts through
    `trigger(v, index, amp, count, dst, ist)`; the output and the state arrays at every stored cut are the reference's bits."""
    seg, count = g["env/seg"], g["env/count"]
    trig = env_trigger_block(g)
    N, V = trig.shape
    sr = float(g["sr"]) if sr is None else sr
    ev = env_events(g)
    dst, ist = env_fresh(V)
    stored = g["cuts"].tolist()
    cuts = cut_list(g, N, extra)
    out = np.zeros((N, V))
    for a, b in zip(cuts[:-1], cuts[1:]):
        for v, index, amp in ev.get(a, []):
            trigger(v, index, amp, count, dst, ist)
        blk = trig[a:b] if (a // 7) % 2 == 0 or trig[a:b].any() else None   # a block without a trigger may also run without the block
        out[a:b] = be.line(b - a, seg, count, blk, g["env/tindex"], g["env/tamp"], sr, dst, ist)
        if b in stored:
            i = stored.index(b) - 1
            assert_bits_equal(dst, g["%s/snap%d/dst" % (key, i)], "%s: dst at cut %d" % (key, b))
            assert np.array_equal(ist, g["%s/snap%d/ist" % (key, i)]), "%s: ist at cut %d" % (key, b)
    assert_bits_equal(out, g[key + "/out"], key)


def model_trigger(v, index, amp, count, dst, ist):
    assert 0 <= index <= count[v] - 2
    ist[1, v], ist[0, v], dst[0, v] = 1, index, amp


def play_lag_case(be, g, extra=()):
    x = patched(g["lag/q"], g["lag/patches"])
    N, V = x.shape
    alpha, recip, val = g["lag/alpha"], g["lag/recip"], g["lag/val0"].copy()
    stored = g["cuts"].tolist()
    cuts = cut_list(g, N, extra)
    out = np.zeros((N, V))
    for a, b in zip(cuts[:-1], cuts[1:]):
        out[a:b] = be.lag(x[a:b], alpha, recip, val)
        if b in stored:
            assert_bits_equal(val, g["lag/snap%d/val" % (stored.index(b) - 1)], "lag: val at cut %d" % b)
    assert_bits_equal(out, g["lag/out"], "lag")
    # alpha per sample: the block that repeats the per-voice pair gives the same bits
    val = g["lag/val0"].copy()
    blk = lambda p: np.ascontiguousarray(np.broadcast_to(p, (N, V)))  # noqa: E731
    assert_bits_equal(be.lag(x, blk(alpha), blk(recip), val), g["lag/out"], "lag, alpha per sample")


def check_map(name, mode, got, ref, x, rng, aux):
    """One map mode against the reference's stream: bits, ULPs of the reference value, or the absolute bound per element; the
    positions of NaN and +-Inf agree exactly.  -> the measured worst case (in the unit of its bound)."""
    what = "%s: %s" % (name, mode)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN positions"
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]), what + ": Inf positions"
    if mode in EXACT_MAPS:
        assert_bits_equal(got, ref, what)
        return 0
    fin = np.isfinite(ref)
    if mode in ("linexp", "dbsToAmp"):
        bound = ULP_LINEXP if mode == "linexp" else ULP_DBSTOAMP
        worst = int(ulp_diff(got[fin], ref[fin]).max()) if fin.any() else 0
        print("%s: max %d ULP (bound %d)" % (what, worst, bound))
        assert worst <= bound, what
        return worst
    bound = amptodbs_bound(ref) if mode == "ampToDbs" else explin_bound(x, rng, aux)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    ratio = float((err[fin] / bound[fin]).max()) if fin.any() else 0.0
    print("%s: max abs error %.3e; worst error / bound %.3f (bound per element, largest %.3e)" % (what, float(err.max()), ratio, float(bound[fin].max()) if fin.any() else 0.0))
    assert (err <= bound)[fin].all(), what
    return ratio


def map_input(g, mode):
    x = patched(g["map/q"], g["map/patches"])
    return np.ascontiguousarray(x * 40.0) if mode == "dbsToAmp" else x


def play_map_cases(be, g, extra=()):
    """Every mode, cut as stored and at `extra`; -> {mode: measured figure}."""
    rng, aux = g["map/range"], g["map/aux"]
    res = {}
    for mode in MAP_MODES:
        x = map_input(g, mode)
        N = x.shape[0]
        cuts = cut_list(g, N, extra)
        r = rng if mode in ("linlin", "linexp", "explin", "clamp") else None
        got = np.concatenate([be.map(mode, x[a:b], r, aux if mode == "explin" else None) for a, b in zip(cuts[:-1], cuts[1:])])
        res[mode] = check_map("golden", mode, got, g["map/" + mode], x, rng, aux)
    return res
