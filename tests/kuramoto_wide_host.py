"""Shared by tests/test_kuramoto_wide_host.py and tests/test_gpu_kuramoto_wide.py: the host build of mxg_kuramoto.h for sets of up
to 1024 oscillators (tests/host_kuramoto_wide.cpp, g++ under the oracle's FPFLAGS) and the library's mxg_kuramoto_wide_render
behind the numpy interface of tests/kuramoto_host.py (render(sr, mode, st, B, freq, K, want)), so that its driver (play_case,
case_deviation) plays the cases of tests/golden/kuramoto_wide.npz through either.

The host build is held to kuramoto_wide.npz within each case's `tol`, and to tests/host_kuramoto.cpp bit for bit for N <= 64, by
test_kuramoto_wide_host.py; it is then the bit-for-bit checker of the GPU tests."""
import ctypes
import os
import subprocess

import numpy as np

import kuramoto_host as kh
from conftest import HOST_OPT, ROOT

P = ctypes.c_void_p
SRC = os.path.join(ROOT, "tests", "host_kuramoto_wide.cpp")
INC = "-I" + os.path.join(ROOT, "maximilian_amd", "csrc")
CASES = ["n65", "n128", "n129", "ps1000", "desync1024", "sync1024", "async_raise", "async_never"]


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libkuramoto_wide_host.so")
    flags = [f for f in kh.fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", INC, "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.kura_wide_host_render.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, P, ctypes.c_int,
                                        P, ctypes.c_int, P, P, P, ctypes.c_int, P, P]
    return L


class WideHostBackend:
    """numpy in, numpy out; the state arrays of `st` are updated in place."""
    name = "host (wide)"

    def __init__(self, L):
        self.L = L

    def render(self, sr, mode, st, B, freq, K, want=kh.MIX | kh.PHASES):
        S, N = st["phase"].shape
        f, fps = kh._par(freq, S)
        k, kps = kh._par(K, S)
        mix = np.zeros((B, S)) if want & kh.MIX else None
        ph = np.zeros((B, S, N)) if want & kh.PHASES else None
        r = self.L.kura_wide_host_render(float(sr), mode, S, N, B, kh._p(f), fps, kh._p(k), kps, kh._p(st["phase"]), kh._p(st["gathered"]),
                                         kh._p(st["update"]), want, kh._p(mix), kh._p(ph))
        assert r == 0
        return {"mix": mix, "phases": ph}


class WideGpuBackend:
    """The library's mxg_kuramoto_wide_render (or, entry="mxg_kuramoto_render", K17's entry point through the same plumbing); `st`
    is uploaded before and downloaded after every call.  Unwanted outputs, and the async arrays of a sync call, are NULL when
    `nulls` is set; otherwise an unwanted output is a poisoned block that must come back untouched."""
    name = "gpu (wide)"
    POISON = -12345.5

    def __init__(self, mx, nulls=True, entry="mxg_kuramoto_wide_render"):
        self.mx, self.nulls, self.entry = mx, nulls, entry

    def render(self, sr, mode, st, B, freq, K, want=kh.MIX | kh.PHASES):
        mx = self.mx
        mx.maxiSettings.setup(int(sr), 2, 1024)
        try:
            S, N = st["phase"].shape
            D = mx.DeviceBuffer
            f, fps = kh._par(freq, S)
            k, kps = kh._par(K, S)
            df, dk = D.from_numpy(f), D.from_numpy(k)
            dp = D.from_numpy(st["phase"])
            use_async = bool(mode & kh.ASYNC) or not self.nulls
            dg = D.from_numpy(st["gathered"]) if use_async else None
            du = D.from_numpy(st["update"]) if use_async else None
            out = {}
            for bit, name, shape in ((kh.MIX, "mix", (B, S)), (kh.PHASES, "phases", (B, S, N))):
                if want & bit or not self.nulls:
                    out[name] = D.from_numpy(np.full(shape, self.POISON))
            g = lambda d: None if d is None else d.ptr  # noqa: E731
            mx._lib.check(getattr(mx.lib(), self.entry)(mode, S, N, B, df.ptr, fps, dk.ptr, kps, dp.ptr, g(dg), g(du), want,
                                                        g(out.get("mix")), g(out.get("phases")), None), self.entry)
            st["phase"][...] = dp.numpy().reshape(S, N)
            if use_async:
                gathered, update = dg.numpy().reshape(S, N), du.numpy().reshape(S)
                if mode & kh.ASYNC:
                    st["gathered"][...], st["update"][...] = gathered, update
                else:   # a sync call leaves the async arrays alone
                    assert np.array_equal(gathered, st["gathered"]) and np.array_equal(update, st["update"])
            res = {}
            for bit, name, shape in ((kh.MIX, "mix", (B, S)), (kh.PHASES, "phases", (B, S, N))):
                a = out[name].numpy().reshape(shape) if name in out else None
                if a is not None and not want & bit:
                    assert (a == self.POISON).all(), "the unwanted block %s was written" % name
                    a = None
                res[name] = a
            return res
        finally:
            mx.maxiSettings.setup(44100, 2, 1024)
