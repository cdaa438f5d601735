"""Shared by tests/test_analysis_host.py and tests/test_gpu_analysis.py: the host build of mxg_analysis.h (tests/host_analysis.cpp,
g++ under the oracle's FPFLAGS) and the library's mxg_analysis_render behind ONE numpy interface (HostBackend / GpuBackend), a
numpy model that restates the reference step by step with a ring of DOUBLES exactly like maxiRingBuf (ModelBackend), and a
driver that plays the cases of tests/golden/analysis.npz through any of them.

The model and the host build are pinned bit for bit to analysis.npz by test_analysis_host.py; the model is then the checker of
the GPU tests on shapes the file does not hold."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT, assert_bits_equal

P = ctypes.c_void_p
ZX, ZCR, ENV, SAH, ALL = 1, 2, 4, 8, 15
NAMES = {ZX: "zx", ZCR: "zcr", ENV: "env", SAH: "sah"}
STATE_KEYS = ("prev_x", "zring", "zpos", "zcount", "overflow", "env", "sah_phase", "sah_value")
STAGE_STATE = {ZX: ("prev_x",), ZCR: ("prev_x", "zring", "zpos", "zcount", "overflow"), ENV: ("env",), SAH: ("sah_phase", "sah_value")}


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libanalysis_host.so")
    flags = [f for f in fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "host_analysis.cpp")])
    L = ctypes.CDLL(so)
    L.ana_host_render.argtypes = ([ctypes.c_double, ctypes.c_size_t, ctypes.c_size_t, P, ctypes.c_int, P, P, P, ctypes.c_size_t] + [P] * 7 +
                                  [ctypes.c_int] + [P] * 6)
    L.ana_host_follow_f.restype = ctypes.c_float
    L.ana_host_follow_f.argtypes = [P, ctypes.c_float, ctypes.c_float, ctypes.c_float]
    return L


def words(cap):
    return (int(cap) + 63) // 64


def fresh(V, cap):
    """Fresh objects, in the layouts of include/maxigpu.h."""
    return {"prev_x": np.zeros(V), "zring": np.zeros((words(cap), V), np.uint64), "zpos": np.zeros(V, np.int32),
            "zcount": np.zeros(V, np.int64), "overflow": np.zeros(V, np.uint32), "env": np.zeros(V), "sah_phase": np.zeros(V),
            "sah_value": np.zeros(V)}


def pack_ring(slots):
    """[cap][V] of 0 / 1 -> u64 [ceil(cap/64)][V]: slot s is bit s & 63 of word s >> 6."""
    cap, V = slots.shape
    b = np.zeros((words(cap) * 64, V), np.uint8)
    b[:cap] = slots != 0
    by = np.packbits(b, axis=0, bitorder="little")                      # [nw * 8][V]
    return np.ascontiguousarray(np.ascontiguousarray(by.T).view("<u8").T)  # [nw][V]


def unpack_ring(ring, cap):
    by = np.ascontiguousarray(np.ascontiguousarray(ring.T).view(np.uint8).T)   # [nw * 8][V]
    return np.unpackbits(by, axis=0, bitorder="little")[:cap].astype(np.float64)


def golden_ring(packed, cap):
    """The file's packbits(axis=0, 'little') of the reference's ring [cap][V] -> the device layout."""
    return pack_ring(np.unpackbits(packed, axis=0, bitorder="little")[:cap])


def _p(a):
    return None if a is None else a.ctypes.data


class HostBackend:
    """numpy in, numpy out; the state arrays of `st` are updated in place."""
    name = "host"

    def __init__(self, L):
        self.L = L

    def render(self, sr, x, want, st, window, cap, attack, release, hold):
        N, V = x.shape
        x = np.ascontiguousarray(x, np.float64)
        out = {n: np.zeros((N, V)) for b, n in NAMES.items() if want & b}
        hold = None if hold is None else np.ascontiguousarray(hold, np.float64)
        win = None if window is None else np.ascontiguousarray(window, np.uint32)
        att, rel = (None if a is None else np.ascontiguousarray(a, np.float64) for a in (attack, release))
        self.L.ana_host_render(float(sr), V, N, _p(x), want, _p(st["prev_x"]), _p(win), _p(st["zring"]), int(cap), _p(st["zpos"]),
                               _p(st["zcount"]), _p(st["overflow"]), _p(att), _p(rel), _p(st["env"]), _p(hold),
                               0 if hold is None else int(hold.ndim == 2), _p(st["sah_phase"]), _p(st["sah_value"]),
                               *[_p(out.get(n)) for n in ("zx", "zcr", "env", "sah")])
        return out


class ModelBackend:
    """The reference restated step by step in Python floats: the ring is [cap] doubles per voice holding 0.0 / 1.0, pushed and
    read as maxiRingBuf::push / tail do (H:434-458); it is packed into the device layout only to carry it in `st`."""
    name = "model"

    def render(self, sr, x, want, st, window, cap, attack, release, hold):
        N, V = x.shape
        cap = int(cap)
        out = {n: np.zeros((N, V)) for b, n in NAMES.items() if want & b}
        ring = unpack_ring(st["zring"], cap) if want & ZCR else None
        for v in range(V):
            xs = x[:, v].tolist()
            if want & (ZX | ZCR):
                prev = float(st["prev_x"][v])
                bits = []
                for s in xs:
                    bits.append(1.0 if (prev <= 0 and s > 0) else 0.0)
                    prev = s
                st["prev_x"][v] = prev
                if want & ZX:
                    out["zx"][:, v] = bits
                if want & ZCR:
                    buf = ring[:, v].tolist()
                    idx = int(st["zpos"][v])
                    if not 0 <= idx < cap:
                        idx = 0
                    W = int(window[v])
                    if W > cap:
                        W = cap
                        st["overflow"][v] += 1
                    count = int(st["zcount"][v])
                    res = []
                    for b in bits:
                        buf[idx] = b                      # push
                        idx += 1
                        if idx == cap:
                            idx = 0
                        if b:
                            count += 1
                        count -= int(buf[idx - W] if idx >= W else buf[cap - (W - idx)])   # tail(W)
                        res.append(float(count))
                    out["zcr"][:, v] = res
                    ring[:, v] = buf
                    st["zpos"][v], st["zcount"][v] = idx, count
            if want & ENV:
                env, att, rel = float(st["env"][v]), float(attack[v]), float(release[v])
                res = []
                for s in xs:
                    a = abs(s)
                    env = (att if a > env else rel) * (env - a) + a
                    res.append(env)
                out["env"][:, v] = res
                st["env"][v] = env
            if want & SAH:
                ph, hv = float(st["sah_phase"][v]), float(st["sah_value"][v])
                hs = np.broadcast_to(hold[:, v] if np.ndim(hold) == 2 else hold[v], (N,)).tolist()
                res = []
                for s, ms in zip(xs, hs):
                    t = ms / 1000.0 * float(sr)
                    h = float(np.trunc(t)) if t >= 1.0 else 0.0   # (double)(size_t)t; negative or NaN: 0 samples
                    if ph >= h:
                        ph -= h
                    if ph < 1.0:
                        hv = s
                    ph += 1.0
                    res.append(hv)
                out["sah"][:, v] = res
                st["sah_phase"][v], st["sah_value"][v] = ph, hv
        if want & ZCR:
            st["zring"][:] = pack_ring(ring)
        return out


class GpuBackend:
    """The library's mxg_analysis_render; `st` is uploaded before and downloaded after every call.  Stages that are not wanted get
    NULL for their arrays when `nulls` is set."""
    name = "gpu"

    def __init__(self, mx, nulls=True):
        self.mx, self.nulls = mx, nulls

    def render(self, sr, x, want, st, window, cap, attack, release, hold):
        mx = self.mx
        mx.maxiSettings.setup(int(sr), 2, 1024)
        try:
            N, V = x.shape
            D = mx.DeviceBuffer
            dx = D.from_numpy(np.ascontiguousarray(x, np.float64))
            need = set()
            for b, keys in STAGE_STATE.items():
                if want & b or not self.nulls:
                    need |= set(keys)
            dev = {k: D.from_numpy(st[k]) for k in STATE_KEYS if k in need}
            par = {"window": (window, np.uint32, ZCR), "attack": (attack, np.float64, ENV), "release": (release, np.float64, ENV),
                   "hold": (hold, np.float64, SAH)}
            dpar = {k: D.from_numpy(np.ascontiguousarray(a, t)) for k, (a, t, b) in par.items() if a is not None and (want & b or not self.nulls)}
            out = {n: D((N, V), np.float64) for b, n in NAMES.items() if want & b}
            g = lambda d, k: d[k].ptr if k in d else None  # noqa: E731
            mx._lib.check(mx.lib().mxg_analysis_render(
                V, N, dx.ptr, want, g(dev, "prev_x"), g(dpar, "window"), g(dev, "zring"), int(cap), g(dev, "zpos"), g(dev, "zcount"),
                g(dev, "overflow"), g(dpar, "attack"), g(dpar, "release"), g(dev, "env"), g(dpar, "hold"),
                int(hold is not None and np.ndim(hold) == 2), g(dev, "sah_phase"), g(dev, "sah_value"), g(out, "zx"), g(out, "zcr"),
                g(out, "env"), g(out, "sah"), None), "mxg_analysis_render")
            for k, d in dev.items():
                st[k][...] = d.numpy()
            return {n: d.numpy() for n, d in out.items()}
        finally:
            mx.maxiSettings.setup(44100, 2, 1024)


# ---- the cases of tests/golden/analysis.npz ------------------------------------------------------------------------------
def signal(g):
    x = g["q"] / 32768.0
    for n, v, val in g["patches"]:
        x[int(n), int(v)] = val
    return np.ascontiguousarray(x)


def play_case(be, g, name, extra=(), want=ALL):
    """The case in the file's blocks, cut further at `extra`; returns the outputs and {cut position: state}."""
    c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}
    x = signal(g)
    N, V = x.shape
    cap, sr = int(c["cap"]), int(c["sr"])
    cuts = sorted(set(c["cuts"].tolist()) | set(extra))
    st = fresh(V, cap)
    outs = {n: np.zeros((N, V)) for b, n in NAMES.items() if want & b}
    states = {}
    hold = c["hold"]
    for a, b in zip(cuts[:-1], cuts[1:]):
        o = be.render(sr, x[a:b], want, st, c["window"], cap, c["attack"], c["release"], hold[a:b] if hold.ndim == 2 else hold)
        for n in outs:
            outs[n][a:b] = o[n]
        states[b] = {k: v.copy() for k, v in st.items()}
    return c, outs, states


def check_case(c, name, outs, states, want=ALL):
    exp = {"zx": c["zx"].astype(np.float64), "zcr": c["zcr"].astype(np.float64), "sah": c["sah"].astype(np.float64)}
    if "env" in c:
        exp["env"] = c["env"]
    for b, n in NAMES.items():
        if want & b and n in exp:
            assert_bits_equal(outs[n], exp[n], "%s: %s" % (name, n))
    cap = int(c["cap"])
    for i, cut in enumerate(c["cuts"].tolist()[1:]):
        s = states[cut]
        what = "%s: state at cut %d, " % (name, cut)
        if want & (ZX | ZCR):
            assert_bits_equal(s["prev_x"], c["snap%d/prev_x" % i], what + "prev_x")
        if want & ZCR:
            assert np.array_equal(s["zring"], golden_ring(c["snap%d/ring" % i], cap)), what + "ring"
            assert np.array_equal(s["zpos"], c["snap%d/pos" % i]) and np.array_equal(s["zcount"], c["snap%d/count" % i]), what + "pos / count"
            assert not s["overflow"].any()
        dst = c["snap%d/dst" % i]
        if want & ENV:
            assert_bits_equal(s["env"], dst[0], what + "env")
        if want & SAH:
            assert_bits_equal(s["sah_phase"], dst[1], what + "sah phase")
            assert_bits_equal(s["sah_value"], dst[2], what + "sah value")


def edge_case(cap, W, V=3, seed=0):
    """Ring edge matrix: V voices at staggered start positions (one of them cap - 1), N = 2 * cap + 5 in blocks of 1, 7, 64 and the
    rest, a signal that crosses often."""
    rng = np.random.default_rng(1000 * cap + W + seed)
    N = 2 * cap + 5
    x = rng.choice([-0.5, 0.25, 0.75, -0.125, 0.0], (N, V))
    st = fresh(V, cap)
    st["zpos"][:] = [(cap - 1, 0, cap // 2)[v % 3] for v in range(V)]
    cuts = [c for c in (0, 1, 8, 72) if c < N] + [N]
    return x, st, np.full(V, W, np.uint32), cuts
