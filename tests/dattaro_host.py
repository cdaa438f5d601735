"""Helpers of the maxiDattaroReverb tests: the host build of maximilian_amd/csrc/mxg_dattaro.h (tests/host_dattaro.cpp) as a bank
renderer over the state layout of mxg_dattaro_render, the state itself, and the replay of a golden case."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

import dattaro_cases as dc
from conftest import GOLDEN, HOST_OPT, ROOT

P = ctypes.c_void_p
THREADS = 16


def build(tmp):
    so = str(tmp / "libdattaro_host.so")
    subprocess.check_call(["g++", "-std=c++17"] + HOST_OPT + ["-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "host_dattaro.cpp")])
    L = ctypes.CDLL(so)
    L.dt_host_render.restype = ctypes.c_int
    L.dt_host_render.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, P, P, P, P, P, ctypes.c_int]
    L.dt_host_layout.restype = ctypes.c_int
    L.dt_host_layout.argtypes = [ctypes.c_uint32, P, P, P, P]
    L.dt_tile_fuzz.restype = ctypes.c_int
    L.dt_tile_fuzz.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t, P, P, P, P]
    return L


class State:
    """The carried state of a bank of V maxiDattaroReverb constructed at `rate`: all zero."""

    def __init__(self, rate, V):
        self.lens, self.offs, S = dc.layout(rate)
        self.rate, self.V = int(rate), V
        self.rings = np.zeros((V, S))
        self.idx = np.zeros((V, dc.RINGS), np.int32)
        self.state = np.zeros((V, dc.STATE))

    def parts(self):
        return [("rings", self.rings), ("idx", self.idx), ("state", self.state)]


def host_render(L, st, x):
    """One block through the host build; x [N][V].  Returns out [2][N][V]."""
    N, V = x.shape
    assert V == st.V and x.flags.c_contiguous
    out = np.zeros((2, N, V))
    rcode = L.dt_host_render(st.rate, V, N, x.ctypes.data, st.rings.ctypes.data, st.idx.ctypes.data, st.state.ctypes.data,
                             out.ctypes.data, THREADS)
    assert rcode == 0
    return out


def load_golden():
    return np.load(os.path.join(GOLDEN, "dattaro.npz"))


def case_inputs(case, g):
    """The case's input, its digest checked against the file."""
    x = dc.inputs(case)
    assert dc.inputs_digest(x) == str(g[case["name"] + "/in_sha256"]), \
        "the regenerated inputs of %s are not the ones the golden file was made from" % case["name"]
    return x


def check_case_state(case, g, st, what):
    """Every piece of final state against the golden file, bit for bit."""
    from conftest import assert_bits_equal
    name = case["name"]
    assert np.array_equal(st.idx, g[name + "/idx"]), what + ": ring indices"
    assert hashlib.sha256(np.ascontiguousarray(st.rings).tobytes()).hexdigest() == str(g[name + "/ring_sha256"]), what + ": ring contents"
    if name + "/rings" in g.files:
        assert_bits_equal(st.rings, g[name + "/rings"], what + ": ring contents")
    assert_bits_equal(st.state, g[name + "/state"], what + ": lp0 lp1 lp2 sigl sigr")
