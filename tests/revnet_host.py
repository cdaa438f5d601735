"""Helpers of the reverb-network tests: the host build of maximilian_amd/csrc/mxg_revfilt.h (tests/host_revnet.cpp) as a bank
renderer over the state layout of mxg_revnet_render, the state itself, and the replay of a golden case."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

import revnet_cases as rc
from conftest import GOLDEN, HOST_OPT, ROOT

P = ctypes.c_void_p
THREADS = 16


def build(tmp):
    so = str(tmp / "librevnet_host.so")
    subprocess.check_call(["g++", "-std=c++17"] + HOST_OPT + ["-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-Wall",
                           "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "host_revnet.cpp")])
    L = ctypes.CDLL(so)
    render = [ctypes.c_uint32, ctypes.c_uint32, P, P, P, ctypes.c_size_t, ctypes.c_size_t] + [P] * 8
    L.rn_host_render.restype = ctypes.c_int
    L.rn_host_render.argtypes = render + [ctypes.c_int]
    L.rn_host_tiled.restype = ctypes.c_int
    L.rn_host_tiled.argtypes = render
    L.rn_host_layout.restype = ctypes.c_int
    L.rn_host_layout.argtypes = [ctypes.c_uint32, ctypes.c_uint32, P, P, P, P, P]
    return L


class Net:
    """A bank of V networks of one topology: the carried state as fresh objects leave it, and the parameters."""

    def __init__(self, V, combs, aps, lowpass=None, comb_fb=0.85, comb_cut=0.2, ap_fb=0.85):
        self.V, self.combs, self.aps = V, list(combs), list(aps)
        self.lowpass = [0] * len(self.combs) if lowpass is None else [int(bool(f)) for f in lowpass]
        self.P, self.A = len(self.combs), len(self.aps)
        self.lengths = self.combs + self.aps
        self.offsets, self.S = rc.layout(self.combs, self.aps)
        self.rings = np.zeros((V, self.S))
        self.idx = np.zeros((V, self.P + self.A), np.int32)
        self.lp = np.zeros((V, self.P))
        self.comb_fb = np.ascontiguousarray(np.broadcast_to(np.asarray(comb_fb, np.float64), (V, self.P)))
        self.comb_cut = np.ascontiguousarray(np.broadcast_to(np.asarray(comb_cut, np.float64), (V, self.P)))
        self.ap_fb = np.ascontiguousarray(np.broadcast_to(np.asarray(ap_fb, np.float64), (V, self.A)))

    def randomise(self, rng):
        """Rings full, indices anywhere, low-pass states of the low-pass combs set."""
        self.rings = rng.uniform(-1, 1, (self.V, self.S))
        self.idx = (rng.integers(0, 1 << 30, (self.V, self.P + self.A)) % np.array(self.lengths)).astype(np.int32)
        self.lp = rng.uniform(-1, 1, (self.V, self.P)) * np.array(self.lowpass, np.float64)
        return self

    def _topo(self):
        return (np.asarray(self.combs + [0], np.uint32), np.asarray(self.aps + [0], np.uint32), np.asarray(self.lowpass + [0], np.uint32))

    def parts(self):
        return [("rings", self.rings), ("idx", self.idx), ("lp", self.lp)]


def _call(fn, net, x, extra=()):
    N, V = x.shape
    assert V == net.V and x.flags.c_contiguous and x.dtype == np.float64
    out = np.zeros((N, V))
    cs, aps, lowp = net._topo()
    for a in (net.rings, net.idx, net.lp, net.comb_fb, net.comb_cut, net.ap_fb):
        assert a.flags.c_contiguous
    r = fn(net.P, net.A, cs.ctypes.data, aps.ctypes.data, lowp.ctypes.data, V, N, x.ctypes.data, net.comb_fb.ctypes.data,
           net.comb_cut.ctypes.data, net.ap_fb.ctypes.data, net.rings.ctypes.data, net.idx.ctypes.data, net.lp.ctypes.data,
           out.ctypes.data, *extra)
    return r, out


def host_render(L, net, x):
    """One block through the step-by-step walk; x [N][V].  Returns out [N][V]; the state of `net` moves on."""
    r, out = _call(L.rn_host_render, net, x, (THREADS,))
    assert r == 0
    return out


def host_tiled(L, net, x):
    """One block the kernel's way.  Returns (out, collisions)."""
    r, out = _call(L.rn_host_tiled, net, x)
    assert r >= 0
    return out, r


def load_golden():
    return np.load(os.path.join(GOLDEN, "revnet.npz"))


def case_net(case, g):
    """(fresh Net, x) of a golden case; the regenerated inputs are checked against the digest in the file."""
    x, comb_fb, comb_cut, ap_fb = rc.inputs(case)
    assert rc.inputs_digest(case, x, comb_fb, comb_cut, ap_fb) == str(g[case["name"] + "/in_sha256"]), \
        "the regenerated inputs of %s are not the ones the golden file was made from" % case["name"]
    combs, aps, lowp = rc.topology(case)
    return Net(case["V"], combs, aps, lowp, comb_fb, comb_cut, ap_fb), x


def check_case_state(case, g, rings, idx, lp, what):
    """Every piece of final state against the golden file, bit for bit."""
    from conftest import assert_bits_equal
    name = case["name"]
    assert np.array_equal(idx, g[name + "/idx"]), what + ": ring indices"
    assert hashlib.sha256(np.ascontiguousarray(rings).tobytes()).hexdigest() == str(g[name + "/ring_sha256"]), what + ": ring contents"
    if name + "/rings" in g.files:
        assert_bits_equal(rings, g[name + "/rings"], what + ": ring contents")
    assert_bits_equal(lp, g[name + "/lp"], what + ": low-pass states")


def assert_state_equal(got_parts, exp_parts, what):
    from conftest import assert_bits_equal
    for (name, a), (_, e) in zip(got_parts, exp_parts):
        if name == "idx":
            assert np.array_equal(a, e), what + ": ring indices"
        else:
            assert_bits_equal(a, e, "%s: %s" % (what, name))
