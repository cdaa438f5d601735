"""Helpers of the reverb tests: the host build of maximilian_amd/csrc/mxg_reverb.h (tests/host_reverb.cpp) as a bank renderer over
the state layout of mxg_reverb_render, the state itself, and the replay of a golden case."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

import reverb_cases as rc
from conftest import GOLDEN, HOST_OPT, ROOT

P = ctypes.c_void_p
THREADS = 16


def build(tmp):
    so = str(tmp / "libreverb_host.so")
    subprocess.check_call(["g++", "-std=c++17"] + HOST_OPT + ["-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "host_reverb.cpp")])
    L = ctypes.CDLL(so)
    L.rv_host_render.restype = ctypes.c_int
    L.rv_host_render.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, P, P, P, ctypes.c_int, P, P, P, P, P,
                                 ctypes.c_int]
    L.rv_layout.restype = ctypes.c_int
    L.rv_layout.argtypes = [ctypes.c_int, P, P]
    L.rv_tile_fuzz.restype = ctypes.c_int
    L.rv_tile_fuzz.argtypes = [ctypes.c_int] * 5 + [P]
    return L


class State:
    """The carried state of a bank of V reverbs, as the constructors leave it."""

    def __init__(self, kind, V):
        lens, _, S = rc.layout(kind)
        self.kind, self.V = kind, V
        self.rings = np.zeros((V, S))
        self.idx = np.zeros((V, len(lens)), np.int32)
        self.lp = np.zeros((V, 8))
        self.wc = np.tile(np.array([0.84, 0.2]), (V, 1))

    def parts(self):
        p = [("rings", self.rings), ("idx", self.idx)]
        if self.kind == rc.FREEVERB:
            p += [("lp", self.lp), ("wc", self.wc)]
        return p


def ptr(a):
    return None if a is None else a.ctypes.data


def host_render(L, st, mode, x, room=None, absorb=None, ps=0):
    """One block through the host build; x [N][V].  Returns out [N][V] ([2][N][V] for the stereo kind)."""
    N, V = x.shape
    assert V == st.V and x.flags.c_contiguous
    out = np.zeros((rc.CHANNELS[st.kind], N, V))
    rcode = L.rv_host_render(st.kind, mode, V, N, ptr(x), ptr(room), ptr(absorb), ps, ptr(st.rings), ptr(st.idx), ptr(st.lp),
                             ptr(st.wc), ptr(out), THREADS)
    assert rcode == 0
    return out if st.kind == rc.STEREO else out[0]


def load_golden():
    return np.load(os.path.join(GOLDEN, "reverb.npz"))


def case_blocks(case, g):
    """The case's inputs (digest checked against the file) cut into the blocks a bank replays it in: runs of equal mode.
    Yields (start, stop, mode, x, room, absorb, ps): parameters [V] where the case is block-rate, else [n][V]."""
    x, mode, room, absorb = rc.inputs(case)
    assert rc.inputs_digest(x, mode, room, absorb) == str(g[case["name"] + "/in_sha256"]), \
        "the regenerated inputs of %s are not the ones the golden file was made from" % case["name"]
    per_sample = case["params"] == "ps"
    for a, b, m in rc.runs(mode):
        if per_sample:
            yield a, b, m, np.ascontiguousarray(x[a:b]), np.ascontiguousarray(room[a:b]), np.ascontiguousarray(absorb[a:b]), 3
        else:
            yield a, b, m, np.ascontiguousarray(x[a:b]), room[0].copy(), absorb[0].copy(), 0


def check_case_state(case, g, st, what):
    """Every piece of final state against the golden file, bit for bit."""
    from conftest import assert_bits_equal
    name = case["name"]
    assert np.array_equal(st.idx, g[name + "/idx"]), what + ": ring indices"
    assert hashlib.sha256(st.rings.tobytes()).hexdigest() == str(g[name + "/ring_sha256"]), what + ": ring contents"
    if name + "/rings" in g.files:
        assert_bits_equal(st.rings, g[name + "/rings"], what + ": ring contents")
    if case["kind"] == rc.FREEVERB:
        assert_bits_equal(st.lp, g[name + "/lp"], what + ": low-pass states")
        assert_bits_equal(st.wc, g[name + "/wc"], what + ": (w, cut)")
