"""Shared by tests/test_dyn_host.py and tests/test_gpu_dyn.py: the host build of mxg_dyn.h (tests/host_dyn.cpp, g++ under
the oracle's FPFLAGS, so log10 / pow / sqrt are glibc's as in the reference) behind the same control interface as
maxiDynamicsBank, a driver that plays a case of tests/golden/dyn.npz through either, and the near-tie rule.

The host build is pinned bit for bit to dyn.npz by test_dyn_host.py and is then the checker of the randomized GPU tests
(numpy's log10 / power are not glibc's and are not used)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT

P = ctypes.c_void_p
NEAR_DB = 1e-9  # a detector level this close to a compared boundary may take the other branch on the device
SETTERS = ["setAttackHigh", "setReleaseHigh", "setAttackLow", "setReleaseLow", "setLookAhead", "setRMSWindowSize", "setInputAnalyser"]
STATE = ["rms_ring", "la_ring", "rms_pos", "la_pos", "running", "dst_h", "ist_h", "dst_l", "ist_l", "overflow"]


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libdyn_host.so")
    flags = [f for f in fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "host_dyn.cpp")])
    L = ctypes.CDLL(so)
    L.dyn_host_render.argtypes = ([ctypes.c_size_t] * 2 + [P] * 8 + [ctypes.c_int] + [P] * 5 + [ctypes.c_int, P, ctypes.c_size_t, P,
                                                                                            ctypes.c_size_t] + [P] * 10)
    L.rms_host_render.argtypes = [ctypes.c_size_t] * 2 + [P, P, P, ctypes.c_size_t, P, P, P, P]
    L.dyn_host_set_time.argtypes = [P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, ctypes.c_double]
    for f in (L.dyn_host_ring_advance, L.dyn_host_ring_head):
        f.argtypes = [ctypes.c_int, ctypes.c_int]
    L.dyn_host_ring_tail.argtypes = [ctypes.c_int] * 3
    return L


def fresh_env(V):
    d = np.zeros((5, V))
    d[2:5] = 1.0
    i = np.zeros((7, V), np.int64)
    i[4:7] = 1
    return d, i


def host_bank(L, V, cap_rms=None, cap_lookahead=None):
    """maxiDynamicsBank's control interface over numpy state and the host build."""
    from maximilian_amd.banks import _DynControl

    class HostDynamicsBank(_DynControl):
        def __init__(self):
            self._init_control(V, cap_rms, cap_lookahead)
            self.rms_ring, self.la_ring = np.zeros((self.cap_rms, V)), np.zeros((self.cap_lookahead, V))
            self.rms_pos, self.la_pos = np.zeros(V, np.int32), np.zeros(V, np.int32)
            self.running, self.overflow = np.zeros(V), np.zeros(V, np.uint32)
            (self.dst_h, self.ist_h), (self.dst_l, self.ist_l) = fresh_env(V), fresh_env(V)

        def play(self, sig, control, *pars):
            """numpy in; returns (out, level_db)."""
            N = sig.shape[0]
            self.running[self._zero_running] = 0.0
            self._zero_running[:] = False
            sig = np.ascontiguousarray(sig, np.float64)
            control = sig if control is None else np.ascontiguousarray(control, np.float64)
            bufs, ps = [], 0
            for k, x in enumerate(pars):
                a = np.asarray(x, np.float64)
                if a.ndim == 2:
                    ps |= 1 << k
                    a = np.ascontiguousarray(a.reshape(N, V))
                else:
                    a = np.ascontiguousarray(np.broadcast_to(a, (V,)))
                bufs.append(a)
            out, lvl = np.zeros((N, V)), np.zeros((N, V))
            L.dyn_host_render(V, N, sig.ctypes.data, control.ctypes.data, *[b.ctypes.data for b in bufs], ps,
                              self.window.ctypes.data, self.lookahead.ctypes.data, self.analyser.ctypes.data,
                              self.stages_high.ctypes.data, self.stages_low.ctypes.data, 3, self.rms_ring.ctypes.data, self.cap_rms,
                              self.la_ring.ctypes.data, self.cap_lookahead, self.rms_pos.ctypes.data, self.la_pos.ctypes.data,
                              self.running.ctypes.data, self.dst_h.ctypes.data, self.ist_h.ctypes.data, self.dst_l.ctypes.data,
                              self.ist_l.ctypes.data, self.overflow.ctypes.data, out.ctypes.data, lvl.ctypes.data)
            return out, lvl

        def state(self):
            return {k: getattr(self, k).copy() for k in STATE}

    return HostDynamicsBank()


class GpuBank:
    """The same play / state interface over maxiDynamicsBank (numpy in and out)."""

    def __init__(self, mx, V, cap_rms=None, cap_lookahead=None, stream=None):
        self.mx, self.b = mx, mx.maxiDynamicsBank(V, cap_rms=cap_rms, cap_lookahead=cap_lookahead, stream=stream)

    def __getattr__(self, name):
        return getattr(self.b, name)

    def play(self, sig, control, *pars):
        D = self.mx.DeviceBuffer
        ds = D.from_numpy(np.ascontiguousarray(sig, np.float64))
        dc = None if control is None else D.from_numpy(np.ascontiguousarray(control, np.float64))
        out = self.b.play(ds, dc, *pars, want_level=True)
        return out.numpy(), self.b.level_db.numpy()

    def state(self):
        b = self.b
        return {"rms_ring": b.rms_ring.numpy(), "la_ring": b.la_ring.numpy(), "rms_pos": b.rms_pos.numpy(), "la_pos": b.la_pos.numpy(),
                "running": b.running.numpy(), "dst_h": b.env_high[0].numpy(), "ist_h": b.env_high[1].numpy(),
                "dst_l": b.env_low[0].numpy(), "ist_l": b.env_low[1].numpy(), "overflow": b.overflow.numpy()}


# ---- golden cases -----------------------------------------------------------------------------------------------------
def load_case(g, name):
    c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}
    c["sig"] = c["sig_q"] / 32768.0
    c["control"] = c["control_q"] / 32768.0 if "control_q" in c else None
    c["pars"] = [c["par%d" % k] for k in range(6)]
    return c


def construct(c, factory):
    """A bank for a golden case, constructed -- like the reference's objects -- under the sample rate the case names (ring sizes, the
    50 ms window and the two setupASR(10, 10) tables come from it); everything afterwards runs at 44100."""
    import maximilian_amd as mx
    mx.maxiSettings.setup(int(c["sr_ctor"]), 2, 1024)
    try:
        bank = factory(c["sig"].shape[1])
    finally:
        mx.maxiSettings.setup(44100, 2, 1024)
    assert (bank.cap_rms, bank.cap_lookahead) == (int(c["cap_rms"]), int(c["cap_la"]))
    return bank


def play_case(bank, c, extra_cuts=()):
    """Plays a golden case: the analysers first, then block by block (cut at the stored cuts plus `extra_cuts`) with the setter
    calls at their positions.  Returns (out, level_db, {cut index: state}) -- states at the stored cuts."""
    N, V = c["sig"].shape
    bank.setInputAnalyser(c["analyser"])
    stored = [int(x) for x in c["cuts"]]
    cuts = sorted(set(stored) | {int(x) for x in extra_cuts})
    out, lvl, states = np.zeros((N, V)), np.zeros((N, V)), {}
    for a, b in zip(cuts[:-1], cuts[1:]):
        for n, what, v, val in c["ops"]:
            if int(n) == a:
                f = getattr(bank, SETTERS[int(what)])
                if int(what) < 4:
                    f(val)  # the envelope times: one shape per bank (the generator made the call on every voice)
                else:
                    f(val, voices=[int(v)])
        pars = [p[a:b] if p.ndim == 2 else p for p in c["pars"]]
        o, l = bank.play(c["sig"][a:b], None if c["control"] is None else c["control"][a:b], *pars)
        out[a:b], lvl[a:b] = o, l
        if b in stored:
            states[stored.index(b) - 1] = bank.state()
    return out, lvl, states


def expected_state(c, i, last):
    s = {k: c["snap%d/%s" % (i, k)] for k in ("running", "dst_h", "ist_h", "dst_l", "ist_l")}
    s["rms_pos"], s["la_pos"] = c["snap%d/rpos" % i], c["snap%d/lpos" % i]
    if last:
        s["rms_ring"], s["la_ring"] = c["snap%d/rring" % i], c["snap%d/lring" % i]
    return s


# ---- the near-tie rule ------------------------------------------------------------------------------------------------
def tie_start(level, pars):
    """Per voice, the first sample at which the CHECKER's detector level lies within NEAR_DB of a boundary it is compared with
    (lowerKnee / higherKnee of a section with a knee, the bare threshold of one without), or N where there is none.  From that
    sample on the voice may have taken the other branch on the device and is left out of the comparison."""
    N, V = level.shape
    th, rh, kh, tl, rl, kl = [np.broadcast_to(np.asarray(p, np.float64), (N, V)) for p in pars]
    near = np.zeros((N, V), bool)
    with np.errstate(invalid="ignore"):
        for t, r, k in ((th, rh, kh), (tl, rl, kl)):
            on, knee = r > 0, k > 0
            for b, use in ((t - k / 2.0, on & knee), (t + k / 2.0, on & knee), (t, on & ~knee)):
                near |= use & (np.abs(level - b) <= NEAR_DB)
    return np.where(near.any(axis=0), near.argmax(axis=0), N)


def compare_output(got, exp, valid, what=""):
    """Positions of NaN and of exact 0.0 must agree where `valid`; returns the largest relative error of the rest."""
    g, e = got[valid], exp[valid]
    assert np.array_equal(np.isnan(g), np.isnan(e)), "%s: NaN positions differ" % what
    assert np.array_equal(g == 0.0, e == 0.0), "%s: positions of exact 0.0 differ (%d)" % (what, int(((g == 0.0) != (e == 0.0)).sum()))
    assert np.array_equal(np.isinf(g), np.isinf(e)) and np.array_equal(g[np.isinf(e)], e[np.isinf(e)]), "%s: infinities differ" % what
    m = np.isfinite(e) & (e != 0.0)
    if not m.any():
        return 0.0
    return float((np.abs(g[m] - e[m]) / np.abs(e[m])).max())
