"""Shared by tests/test_seq_host.py and tests/test_gpu_seq.py: the host build of mxg_seq.h (tests/host_seq.cpp, g++ under the
oracle's FPFLAGS) and the library's mxg_seq_render / mxg_seq_signal behind ONE numpy interface (HostBackend / GpuBackend), and
drivers that play the cases of tests/golden/seq.npz through either.

The host build is pinned bit for bit to seq.npz by test_seq_host.py and is then the checker of the randomized GPU tests."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT

P = ctypes.c_void_p
ONZX, COUNTER, STEP, INDEX, ZXTOPULSE = range(5)
KIND_NAMES = {ONZX: "onzx", COUNTER: "counter", STEP: "step", INDEX: "index", ZXTOPULSE: "zxtopulse"}
VAL_VALUES, VAL_STEP = 0, 1
FUSED_CASES = ["values", "step", "extphase"]


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libseq_host.so")
    flags = [f for f in fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "host_seq.cpp")])
    L = ctypes.CDLL(so)
    L.seq_host_ratio.argtypes = [ctypes.c_size_t, ctypes.c_size_t, P, P, P]
    L.seq_host_render.argtypes = ([ctypes.c_double, ctypes.c_size_t, ctypes.c_size_t, P, P, P, ctypes.c_int, P, P, ctypes.c_size_t,
                                   ctypes.c_size_t, P, ctypes.c_int, P, P, ctypes.c_size_t, ctypes.c_size_t] + [P] * 8)
    L.seq_host_signal.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, P, P, P, P, ctypes.c_size_t, ctypes.c_size_t] + [P] * 5
    L.seq_host_saw.argtypes = [ctypes.c_double, ctypes.c_size_t, ctypes.c_size_t, P, P, P]
    return L


def build_envgen(tmpdir):
    """tests/host_envgen.cpp: maxiEnvGen::play as a lane of envgen.hip runs it (pinned to the oracle by tests/test_envgen_host.py)."""
    so = os.path.join(str(tmpdir), "libenvgen_host.so")
    subprocess.check_call(["g++", "-std=c++17"] + HOST_OPT + ["-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "host_envgen.cpp")])
    E = ctypes.CDLL(so)
    E.envgen_host.restype = ctypes.c_int
    E.envgen_host.argtypes = [ctypes.c_size_t, ctypes.c_size_t, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P,
                              ctypes.c_int]
    return E


# ---- fresh states (include/maxigpu.h) ----------------------------------------------------------------------------------
def fresh_seq(V):
    dst, ist = np.zeros((5, V)), np.zeros((6, V), np.int64)
    dst[[1, 3]] = 1.0
    ist[[0, 3, 4, 5]] = 1
    return dst, ist


def fresh_sig(kind, V):
    dst, ist = np.zeros((3, V)), np.zeros((2, V), np.int64)
    if kind == COUNTER:
        dst[[1, 2]] = 1.0
        ist[:] = 1
    else:
        dst[0] = 1.0
        ist[0] = 1
        if kind == STEP:
            ist[1] = 1
    return dst, ist


def table(rows, width):
    t = np.zeros((len(rows), width))
    for i, r in enumerate(rows):
        t[i, :len(r)] = r
    return t, np.array([len(r) for r in rows], np.int32)


def _c(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def _p(a):
    return None if a is None else a.ctypes.data


class HostBackend:
    """numpy in, numpy out; clk / dst / ist are updated in place."""
    name = "host"

    def __init__(self, L):
        self.L = L

    def render(self, sr, V, N, freq, clk, phase, norm, plen, pat, mode, values, vlen, vpat, step, hold, dst, ist, want):
        wt, wv, wg = want
        freq, phase, norm, values, step, hold = (_c(a, np.float64) for a in (freq, phase, norm, values, step, hold))
        plen, pat, vlen, vpat = (_c(a, np.int32) for a in (plen, pat, vlen, vpat))
        out = [np.zeros((N, V)) if w else None for w in (wt, wv, wg)]
        pv = 0 if phase is None else int(phase.ndim == 2)
        self.L.seq_host_render(float(sr), V, N, _p(freq), _p(clk) if freq is not None else None, _p(phase), pv, _p(norm), _p(plen),
                               norm.shape[0], norm.shape[1], _p(pat), mode, _p(values), _p(vlen),
                               0 if values is None else values.shape[0], 0 if values is None else values.shape[1], _p(vpat), _p(step),
                               _p(hold), _p(dst), _p(ist), *[_p(o) for o in out])
        return out

    def signal(self, kind, V, N, a, b, values, vlen, vpat, par, dst, ist):
        a, b, values, par = (_c(x, np.float64) for x in (a, b, values, par))
        vlen, vpat = _c(vlen, np.int32), _c(vpat, np.int32)
        out = np.zeros((N, V))
        self.L.seq_host_signal(kind, V, N, _p(a), _p(b), _p(values), _p(vlen), 0 if values is None else values.shape[0],
                               0 if values is None else values.shape[1], _p(vpat), _p(par), _p(dst), _p(ist), _p(out))
        return out


class GpuBackend:
    """The same interface over the C-ABI: every array is uploaded, the state arrays are read back into the caller's."""
    name = "gpu"

    def __init__(self, mx):
        self.mx = mx

    def _up(self, a, dtype):
        return None if a is None else self.mx.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype))

    @staticmethod
    def _d(b):
        return None if b is None else b.ptr

    def render(self, sr, V, N, freq, clk, phase, norm, plen, pat, mode, values, vlen, vpat, step, hold, dst, ist, want):
        mx, D = self.mx, self.mx.DeviceBuffer
        f64, i32 = np.float64, np.int32
        d = {k: self._up(a, f64) for k, a in dict(freq=freq, phase=phase, norm=norm, values=values, step=step, hold=hold, dst=dst).items()}
        d.update({k: self._up(a, i32) for k, a in dict(plen=plen, pat=pat, vlen=vlen, vpat=vpat).items()})
        d["clk"] = self._up(clk, f64) if freq is not None else None
        d["ist"] = self._up(ist, np.int64)
        out = [D((N, V), f64) if w else None for w in want]
        pv = 0 if phase is None else int(np.ndim(phase) == 2)
        old = mx.maxiSettings.sampleRate
        mx.maxiSettings.setup(int(sr), 2, 1024)
        try:
            mx._lib.check(mx.lib().mxg_seq_render(V, N, self._d(d["freq"]), self._d(d["clk"]), self._d(d["phase"]), pv, d["norm"].ptr,
                                                   d["plen"].ptr, norm.shape[0], norm.shape[1], self._d(d["pat"]), mode,
                                                   self._d(d["values"]), self._d(d["vlen"]), 0 if values is None else values.shape[0],
                                                   0 if values is None else values.shape[1], self._d(d["vpat"]), self._d(d["step"]),
                                                   self._d(d["hold"]), d["dst"].ptr, d["ist"].ptr, *[self._d(o) for o in out], None),
                          "mxg_seq_render")
            res = [None if o is None else o.numpy() for o in out]
            dst[...] = d["dst"].numpy()
            ist[...] = d["ist"].numpy()
            if freq is not None:
                clk[...] = d["clk"].numpy()
        finally:
            mx.maxiSettings.setup(old, 2, 1024)
        return res

    def signal(self, kind, V, N, a, b, values, vlen, vpat, par, dst, ist):
        mx, D = self.mx, self.mx.DeviceBuffer
        f64, i32 = np.float64, np.int32
        da, db, dv, dp, dd = (self._up(x, f64) for x in (a, b, values, par, dst))
        dl, dr, di = self._up(vlen, i32), self._up(vpat, i32), self._up(ist, np.int64)
        out = D((N, V), f64)
        mx._lib.check(mx.lib().mxg_seq_signal(kind, V, N, da.ptr, self._d(db), self._d(dv), self._d(dl), 0 if values is None else values.shape[0],
                                              0 if values is None else values.shape[1], self._d(dr), self._d(dp), dd.ptr, di.ptr, out.ptr,
                                              None), "mxg_seq_signal")
        res = out.numpy()
        dst[...] = dd.numpy()
        ist[...] = di.numpy()
        return res


def ratio_tables(times, plen):
    """mxg_seq_ratio_host (host arithmetic of the library: no device needed)."""
    import maximilian_amd as mx
    times, plen = np.ascontiguousarray(times, np.float64), np.ascontiguousarray(plen, np.int32)
    norm = np.zeros_like(times)
    mx._lib.check(mx.lib().mxg_seq_ratio_host(times.shape[0], times.shape[1], plen.ctypes.data, times.ctypes.data, norm.ctypes.data),
                  "mxg_seq_ratio_host")
    return norm


# ---- golden cases -----------------------------------------------------------------------------------------------------
def load_case(g, name):
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}


def block_of(cuts, n):
    """index of the stored block that holds sample n"""
    return int(np.searchsorted(np.asarray(cuts), n, side="right") - 1)


def play_fused(be, c, extra_cuts=(), want=(True, True, True)):
    """Plays a fused golden case block by block (stored cuts plus `extra_cuts`).  Returns (trig, val, gate, {stored cut index:
    (dst, ist, clk)}): numpy [N][V] each (None where not wanted)."""
    stored = [int(x) for x in c["cuts"]]
    N, V = c["trig"].shape
    cuts = sorted(set(stored) | {int(x) for x in extra_cuts if 0 < int(x) < N})
    norm = ratio_tables(c["times"], c["len"])
    internal = "freq" in c
    dst, ist = fresh_seq(V)
    clk = np.zeros(V)
    outs = [np.zeros((N, V)) if w else None for w in want]
    states = {}
    for a, b in zip(cuts[:-1], cuts[1:]):
        i = block_of(stored, a)
        res = be.render(int(c["sr"]), V, b - a, c["freq"] if internal else None, clk, None if internal else c["phase"][a:b], norm, c["len"],
                        c["pat"], int(c["mode"]), c["values%d" % i], c["vlen%d" % i], c["vpat"], c["step%d" % i], c["hold"], dst, ist, want)
        for o, r in zip(outs, res):
            if o is not None:
                o[a:b] = r
        if b in stored:
            states[stored.index(b) - 1] = (dst.copy(), ist.copy(), clk.copy())
    return outs[0], outs[1], outs[2], states


def expected_values(c):
    """The stored indices back to doubles through each block's lists."""
    stored = [int(x) for x in c["cuts"]]
    N, V = c["trig"].shape
    out = np.zeros((N, V))
    for i, (a, b) in enumerate(zip(stored[:-1], stored[1:])):
        tab = c["values%d" % i]
        out[a:b] = tab[c["vpat"][None, :], c["val_idx"][a:b]]
    return out


def sig_inputs(g, kind):
    """(first input, second input, parameter) of a signal case, as the generator formed them."""
    trig = g["sig/trig"].astype(np.float64)
    saw, sine, noise = (g["sig/%s_q" % k] / 32768.0 for k in ("saw", "sine", "noise"))
    if kind == ONZX:
        return np.ascontiguousarray(sine + 0.3 * noise), None, None
    if kind == COUNTER:
        return trig, saw, None
    if kind == STEP:
        return trig, None, g["sig/step"]
    if kind == INDEX:
        return trig, np.ascontiguousarray(sine * 0.7 + 0.5), None
    return trig, None, g["sig/hold"]


def sig_expected(g, kind):
    name = KIND_NAMES[kind]
    if kind in (ONZX, COUNTER, ZXTOPULSE):
        return g["sig/%s/out" % name].astype(np.float64)
    idx = g["sig/%s/out_idx" % name]
    vals = g["sig/values"][g["sig/vpat"][None, :], np.minimum(idx, g["sig/values"].shape[1] - 1)]
    return np.where(idx == 255, 0.0, vals)


def play_signal(be, g, kind, extra_cuts=()):
    a, b, par = sig_inputs(g, kind)
    N, V = a.shape
    stored = [int(x) for x in g["sig/cuts"]]
    cuts = sorted(set(stored) | {int(x) for x in extra_cuts if 0 < int(x) < N})
    tab = kind in (STEP, INDEX)
    dst, ist = fresh_sig(kind, V)
    out, states = np.zeros((N, V)), {}
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        out[c0:c1] = be.signal(kind, V, c1 - c0, a[c0:c1], None if b is None else b[c0:c1], g["sig/values"] if tab else None,
                               g["sig/vlen"] if tab else None, g["sig/vpat"] if tab else None, par, dst, ist)
        if c1 in stored:
            states[stored.index(c1) - 1] = (dst.copy(), ist.copy())
    return out, states


# ---- the comparisons (bit for bit) -------------------------------------------------------------------------------------
def assert_same(a, b, what):
    from conftest import assert_bits_equal
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        assert_bits_equal(a, b, what)
    else:
        assert np.array_equal(a, b), what


def check_fused(c, name, trig, val, gate, states):
    assert_same(trig, c["trig"].astype(np.float64), name + " trig")
    assert_same(val, expected_values(c), name + " val")
    assert_same(gate, c["gate"].astype(np.float64), name + " gate")
    ncut = len(c["cuts"]) - 1
    assert sorted(states) == list(range(ncut))
    for i in range(ncut):
        dst, ist, clk = states[i]
        assert_same(dst, c["snap%d/dst" % i], "%s cut %d dst" % (name, i))
        assert_same(ist, c["snap%d/ist" % i], "%s cut %d ist" % (name, i))
        if "freq" in c:
            assert_same(clk, c["snap%d/clk" % i], "%s cut %d clk" % (name, i))


def check_signal(g, kind, out, states):
    exp = sig_expected(g, kind)
    assert exp.any()
    name = KIND_NAMES[kind]
    assert_same(out, exp, name)
    ncut = len(g["sig/cuts"]) - 1
    assert sorted(states) == list(range(ncut))
    for i in range(ncut):
        assert_same(states[i][0], g["sig/%s/snap%d/dst" % (name, i)], "%s cut %d dst" % (name, i))
        assert_same(states[i][1], g["sig/%s/snap%d/ist" % (name, i)], "%s cut %d ist" % (name, i))
