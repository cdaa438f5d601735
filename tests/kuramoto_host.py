"""Shared by tests/test_kuramoto_host.py and tests/test_gpu_kuramoto.py: the host build of mxg_kuramoto.h (tests/host_kuramoto.cpp,
g++ under the oracle's FPFLAGS) and the library's mxg_kuramoto_render behind ONE numpy interface (HostBackend / GpuBackend), a
numpy model that restates the reference step by step with numpy's sine (ModelBackend), and a driver that plays the cases of
tests/golden/kuramoto.npz through any of them.

The host build is held to kuramoto.npz within each case's `tol` by test_kuramoto_host.py; it is then the bit-for-bit checker of the
GPU tests, on the file's cases and on shapes the file does not hold."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT

P = ctypes.c_void_p
MEANFIELD, ASYNC = 1, 2
MIX, PHASES = 1, 2
TWOPI = 6.283185307179586476925286766559


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libkuramoto_host.so")
    flags = [f for f in fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "host_kuramoto.cpp")])
    L = ctypes.CDLL(so)
    L.kura_host_render.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, P, ctypes.c_int, P,
                                   ctypes.c_int, P, P, P, ctypes.c_int, P, P]
    for f in (L.kura_host_sin, L.kura_host_cos):
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.c_double]
    L.kura_host_sin_error.restype = ctypes.c_double
    L.kura_host_sin_error.argtypes = [ctypes.c_size_t]
    return L


def fresh(S, N, phase=None):
    """Fresh sets in the layouts of include/maxigpu.h: phases 0 (or `phase`), gathered phases 0, flags down."""
    st = {"phase": np.zeros((S, N)), "gathered": np.zeros((S, N)), "update": np.zeros(S, np.int32)}
    if phase is not None:
        st["phase"][...] = phase
    return st


def _p(a):
    return None if a is None else a.ctypes.data


def _par(a, S):
    """freq / K: scalar or [S] -> ([S], 0); [B][S] -> (itself, 1)."""
    a = np.asarray(a, np.float64)
    if a.ndim == 2:
        return np.ascontiguousarray(a), 1
    return np.ascontiguousarray(np.broadcast_to(a, (S,))), 0


class HostBackend:
    """numpy in, numpy out; the state arrays of `st` are updated in place."""
    name = "host"

    def __init__(self, L):
        self.L = L

    def render(self, sr, mode, st, B, freq, K, want=MIX | PHASES):
        S, N = st["phase"].shape
        f, fps = _par(freq, S)
        k, kps = _par(K, S)
        mix = np.zeros((B, S)) if want & MIX else None
        ph = np.zeros((B, S, N)) if want & PHASES else None
        r = self.L.kura_host_render(float(sr), mode, S, N, B, _p(f), fps, _p(k), kps, _p(st["phase"]), _p(st["gathered"]), _p(st["update"]),
                                    want, _p(mix), _p(ph))
        assert r == 0
        return {"mix": mix, "phases": ph}


class ModelBackend:
    """The reference restated in numpy, all sets at once: the sums run sequentially over j (and the mix over i), the sine is
    numpy's.  The mean-field form sums S and C in j order."""
    name = "model"

    def render(self, sr, mode, st, B, freq, K, want=MIX | PHASES):
        S, N = st["phase"].shape
        f, fps = _par(freq, S)
        k, kps = _par(K, S)
        dt = TWOPI / float(sr)
        mix, ph = np.zeros((B, S)), np.zeros((B, S, N))
        p, g, up = st["phase"], st["gathered"], st["update"]
        with np.errstate(invalid="ignore"):
            for b in range(B):
                if mode & ASYNC:
                    fl = up != 0
                    g[fl] = p[fl]
                    up[...] = 0
                else:   # a sync set gathers at every sample and owns neither array
                    fl, g = np.ones(S, bool), p.copy()
                keff = np.where(fl, k[b] if kps else k, 0.0)
                adj = np.zeros((S, N))
                if mode & MEANFIELD:
                    Ssum, Csum = np.zeros(S), np.zeros(S)
                    for j in range(N):
                        Ssum = Ssum + np.sin(g[:, j])
                        Csum = Csum + np.cos(g[:, j])
                    adj = np.cos(p) * Ssum[:, None] - np.sin(p) * Csum[:, None]
                else:
                    for j in range(N):
                        adj = adj + np.sin(g[:, j, None] - p)
                q = p + dt * ((f[b] if fps else f)[:, None] + ((keff / float(N))[:, None] * adj))
                q = np.where(q >= TWOPI, q - TWOPI, np.where(q < 0, q + TWOPI, q))
                p[...] = q
                m = np.zeros(S)
                for i in range(N):
                    m = m + q[:, i]
                mix[b] = m / float(N)
                ph[b] = q
        return {"mix": mix if want & MIX else None, "phases": ph if want & PHASES else None}


class GpuBackend:
    """The library's mxg_kuramoto_render; `st` is uploaded before and downloaded after every call.  Unwanted outputs, and the
    async arrays of a sync call, are NULL when `nulls` is set; otherwise an unwanted output is a poisoned block that must come
    back untouched."""
    name = "gpu"
    POISON = -12345.5

    def __init__(self, mx, nulls=True):
        self.mx, self.nulls = mx, nulls

    def render(self, sr, mode, st, B, freq, K, want=MIX | PHASES):
        mx = self.mx
        mx.maxiSettings.setup(int(sr), 2, 1024)
        try:
            S, N = st["phase"].shape
            D = mx.DeviceBuffer
            f, fps = _par(freq, S)
            k, kps = _par(K, S)
            df, dk = D.from_numpy(f), D.from_numpy(k)
            dp = D.from_numpy(st["phase"])
            use_async = bool(mode & ASYNC) or not self.nulls
            dg = D.from_numpy(st["gathered"]) if use_async else None
            du = D.from_numpy(st["update"]) if use_async else None
            out = {}
            for bit, name, shape in ((MIX, "mix", (B, S)), (PHASES, "phases", (B, S, N))):
                if want & bit or not self.nulls:
                    out[name] = D.from_numpy(np.full(shape, self.POISON))
            g = lambda d: None if d is None else d.ptr  # noqa: E731
            mx._lib.check(mx.lib().mxg_kuramoto_render(mode, S, N, B, df.ptr, fps, dk.ptr, kps, dp.ptr, g(dg), g(du), want,
                                                       g(out.get("mix")), g(out.get("phases")), None), "mxg_kuramoto_render")
            st["phase"][...] = dp.numpy().reshape(S, N)
            if use_async:
                gathered, update = dg.numpy().reshape(S, N), du.numpy().reshape(S)
                if mode & ASYNC:
                    st["gathered"][...], st["update"][...] = gathered, update
                else:   # a sync call leaves the async arrays alone
                    assert np.array_equal(gathered, st["gathered"]) and np.array_equal(update, st["update"])
            res = {}
            for bit, name, shape in ((MIX, "mix", (B, S)), (PHASES, "phases", (B, S, N))):
                a = out[name].numpy().reshape(shape) if name in out else None
                if a is not None and not want & bit:
                    assert (a == self.POISON).all(), "the unwanted block %s was written" % name
                    a = None
                res[name] = a
            return res
        finally:
            mx.maxiSettings.setup(44100, 2, 1024)


# ---- the cases of tests/golden/kuramoto.npz ----------------------------------------------------------------------------------
def case(g, name):
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}


def case_params(c):
    n = int(c["cuts"][-1])
    if "freq_q" in c:
        return c["freq_q"] / 256.0, c["K_q"] / 256.0, True
    return np.full(n, float(c["freq"])), np.full(n, float(c["K"])), False


def play_case(be, c, mode=0, extra=(), want=MIX | PHASES):
    """One golden case (mode: the case's own ASYNC bit is added) in the file's blocks, cut further at `extra`.  Returns mix [n],
    phases [n][N] and {cut: state}."""
    N, sr = int(c["N"]), int(c["sr"])
    mode |= ASYNC if int(c["async"]) else 0
    f, k, ps = case_params(c)
    n = int(c["cuts"][-1])
    cuts = sorted(set(c["cuts"].tolist()) | set(extra))
    st = fresh(1, N, c["phase0"])
    st["update"][:] = int(c["raise0"])
    mix, ph, states = np.zeros(n), np.zeros((n, N)), {}
    for a, b in zip(cuts[:-1], cuts[1:]):
        for cut, idx, val in c["events"]:
            if int(cut) == a:
                st["phase"][0, int(idx)] = val
                if mode & ASYNC:
                    st["update"][0] = 1
        o = be.render(sr, mode, st, b - a, f[a:b, None] if ps else f[a], k[a:b, None] if ps else k[a], want)
        if want & MIX:
            mix[a:b] = o["mix"][:, 0]
        if want & PHASES:
            ph[a:b] = o["phases"][:, 0]
        states[b] = {key: v.copy() for key, v in st.items()}
    return mix, ph, states


def case_deviation(c, mix, ph, states):
    """The largest |difference| from the file (plain, not on the circle: the file's wrap margin rules a differing wrap out): the
    mix at every sample, the phases (async: and the gathered phases) at every cut, the whole phase streams where the file has
    them.  The flags must match."""
    dev = float(np.abs(mix - c["mix"]).max())
    for i, cut in enumerate(c["cuts"].tolist()[1:]):
        s = states[cut]
        dev = max(dev, float(np.abs(s["phase"][0] - c["snap_phase"][i]).max()))
        if int(c["async"]):
            dev = max(dev, float(np.abs(s["gathered"][0] - c["snap_gathered"][i]).max()))
            assert int(s["update"][0]) == int(c["snap_update"][i]) == 0
    if "phases" in c:
        dev = max(dev, float(np.abs(ph - c["phases"]).max()))
    return dev
