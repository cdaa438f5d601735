"""The cases of tests/golden/grainpool.npz (K27: granular streams over pool slots) and everything derived from them -- one place for
tools/gen/gen_golden_grainpool.py, tests/test_grainpool_host.py and tests/test_gpu_grainpool.py.  Every input follows from the
small integers below.

A bank call has one mode, one overlaps, one window, one set of MXG_GPOOL_PS_* bits and rand() draws or none: the streams of the
table are played in GROUPS of equal (mode, overlaps, window, ps, rnd), every group cut at the same CUTS."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT, assert_bits_equal

P = ctypes.c_void_p
SR, GRAIN_LENGTH, SAMPLE_DUR = 44100, 0.01, 441
T = 2000
CUTS = [0, 1, 8, 143, 600, 601, 1429, 1993, 2000]
LENS = [130, 300, 777, 2048, 4096]      # the pool: slots 0 and 1 are shorter than a grain (sampleEndPos = len, the grain wraps)
R, CAP = len(LENS), max(LENS)
STRIDE = CAP + 32                       # doubles between slots in the host arrays (any value >= cap is a valid layout)
GUARD = 8                               # doubles in front of slot 0 in the host array
RN = 64                                 # rand() draws per stream
WINDOWS = {"hann": 0, "rect": 3, "gaussian": 8}
PS_A, PS_B, PS_POSMOD = 1, 2, 4
PATCH_SL_FRAMES = 10500               # tests/patches/stretch_loop_patch.cpp: 9000 samples of play(), 1500 of playAtPosition


def tri(n):
    """A triangle LFO that crosses zero: period 400, range [-1.5625, 1.5625]."""
    return (np.abs((n % 400) - 200) - 100) / 64.0


def saw(mul, mod, den):
    return lambda n: ((n * mul) % mod) / float(den)


def const(v):
    return lambda n: np.full(n.shape, float(v))


# mode, overlaps, window, rnd, ps, slot, a, b, posMod, start position (raw), loop (start01, end01) or None
STREAMS = [
    # ---- maxiTimeStretch::play, rand() draws given
    (0, 2, "hann", True, 0, 3, const(1.0), None, None, 0.0, None),              # 0  the plain case
    (0, 2, "hann", True, 0, 0, const(0.25), None, None, 0.0, None),             # 1  timestretch 0.25 on the 130-sample slot: every grain wraps
    (0, 2, "hann", True, 0, 2, const(-1.0), None, None, 0.0, None),             # 2  negative speed: position walks down, grains read backwards
    # ---- maxiTimeStretch::play, no draws, overlaps 3, rect; speed at every sample (PS_A)
    (0, 3, "rect", False, PS_A, 1, const(0.5), None, const(0.1), 0.0, None),    # 3  a constant column in a per-sample block; posMod [S]; 300-sample slot
    (0, 3, "rect", False, PS_A, 4, tri, None, const(0.0), 100.0, None),         # 4  speed from the LFO: its sign flips the grains' direction (:349)
    # ---- maxiStretch::play with loop points, draws given
    (1, 2, "hann", True, 0, 4, const(1.0), const(2.0), None, 0.0, (0.25, 0.5)),             # 5  loop [0.25, 0.5] of the 4096 slot, walks in in one step
    (1, 2, "hann", True, 0, 4, const(0.5), const(0.25), None, 0.0, (1000 / 4096.0, 1001 / 4096.0)),  # 6  pitch 0.5, timestretch 0.25, a loop of ONE sample; walks in by 1 a sample
    (1, 2, "hann", True, 0, 4, const(1.7), const(-1.0), None, 3900.0, (0.25, 0.5)),          # 7  pitch 1.7, timestretch -1, starts above its loop
    (1, 2, "hann", True, 0, 3, const(1.0), const(1.0), None, 0.0, (0.5, 0.5 + 16 / 2048.0)),  # 8  starts below a loop of 16: walks in by 16 a sample
    (1, 2, "hann", True, 0, 2, const(-1.0), const(1.5), None, 0.0, None),                    # 9  negative pitch; setLoopStart(0.25) at cut 601
    (1, 2, "hann", True, 0, 1, const(1.0), const(1.0), None, 0.0, None),                     # 10 setSlot(2) at cut 1429 (setSample :466-478)
    # ---- maxiStretch::play, overlaps 6, gaussian, no draws; timestretch and posMod at every sample
    (1, 6, "gaussian", False, PS_B | PS_POSMOD, 4, const(1.0), tri, saw(7, 64, 512), 0.0, None),      # 11 the LFO on the rate crosses zero; posMod moves
    (1, 6, "gaussian", False, PS_B | PS_POSMOD, 0, const(0.5), const(1.0), const(0.0), 0.0, None),     # 12 six live grains on the 130-sample slot
    # ---- maxiTimeStretch::playAtPosition
    (2, 3, "rect", False, 0, 3, saw(3, 1000, 1024), None, None, 0.0, None),     # 13
    (2, 3, "rect", False, 0, 0, saw(5, 900, 1024), None, None, 0.0, None),      # 14 on the 130-sample slot
    # ---- maxiPitchShift::play
    (3, 2, "hann", False, 0, 4, const(1.7), None, const(0.0), 0.0, None),       # 15 pitch 1.7
    (3, 2, "hann", False, 0, 1, const(0.5), None, const(0.05), 0.0, None),      # 16 pitch 0.5 on the 300-sample slot (position resets at len)
    # ---- maxiStretch::playAtPosition
    (4, 3, "hann", False, PS_B, 3, const(1.0), saw(5, 900, 1024), None, 0.0, None),    # 17 the position at every sample
    (4, 3, "hann", False, PS_B, 2, const(-0.5), saw(3, 1000, 1024), None, 0.0, None),  # 18 a negative pitchstretch
    (4, 2, "gaussian", False, 0, 4, const(1.7), const(0.3), None, 0.0, None),          # 19 one position for the call
]
NS = len(STREAMS)
LOOP_STREAMS = [5, 6, 7, 8]           # a loop from the start
EVENTS = {601: ("loopStart", 9, 0.25), 1429: ("slot", 10, 2)}


def pool_content():
    """[R] arrays: the "16-bit" integer ramp of the sampler patches plus a sine in eighths."""
    out = []
    for r, n in enumerate(LENS):
        i = np.arange(n)
        out.append(((i * 53 + 11 * r) % 601 - 300).astype(np.float64) + np.round(1000.0 * np.sin(2.0 * np.pi * i / 97.0)) / 8.0)
    return out


def pool_array():
    """The host pool: (the whole array, the offset of element 0 of slot 0)."""
    mem = np.zeros(GUARD + R * STRIDE)
    for r, a in enumerate(pool_content()):
        mem[GUARD + r * STRIDE:GUARD + r * STRIDE + a.size] = a
    return mem


def rnd_draws(i):
    return ((i * 7 + np.arange(RN) * 3) % 10).astype(np.int32)


def loop_samples(n, start01, end01):
    """setLoopStart / setLoopEnd: (unsigned long)(val * len)."""
    return int(start01 * n), int(end01 * n)


def groups():
    """[(key, [stream indices])] in table order; key = (mode, overlaps, window, rnd, ps)."""
    out = []
    for i, s in enumerate(STREAMS):
        key = s[:5]
        for k, idx in out:
            if k == key:
                idx.append(i)
                break
        else:
            out.append((key, [i]))
    return out


class GroupState:
    """One group's arrays as the entry points take them."""

    def __init__(self, key, idx):
        self.key, self.idx = key, idx
        self.mode, self.ov, self.win, self.has_rnd, self.ps = key
        S = self.S = len(idx)
        n = np.arange(T)
        self.slot = np.array([STREAMS[i][5] for i in idx], np.uint32)
        self.loop = np.zeros((2, S), np.uint64)
        self.st, self.gst = np.zeros((4, S)), np.zeros((4, 8, S))
        cols = {"a": [], "b": [], "pm": []}
        for j, i in enumerate(idx):
            s = STREAMS[i]
            ln = LENS[s[5]]
            self.loop[:, j] = (0, ln) if s[10] is None else loop_samples(ln, *s[10])
            self.st[0, j] = s[9]
            for name, f in (("a", s[6]), ("b", s[7]), ("pm", s[8])):
                cols[name].append(None if f is None else np.asarray(f(n), np.float64))
        self.a = np.stack(cols["a"], 1)
        self.b = None if cols["b"][0] is None else np.stack(cols["b"], 1)
        self.pm = None if cols["pm"][0] is None else np.stack(cols["pm"], 1)
        self.rnd = np.stack([rnd_draws(i) for i in idx]) if self.has_rnd else None

    def block(self, name, n0, n1):
        """The argument for samples [n0, n1): [n][S] where the entry point reads it at every sample, else [S]."""
        x = getattr(self, name)
        if x is None:
            return None
        ps = (name == "a" and (self.mode == 2 or self.ps & PS_A)) or (name == "b" and self.ps & PS_B) or (name == "pm" and self.ps & PS_POSMOD)
        return np.ascontiguousarray(x[n0:n1]) if ps else np.ascontiguousarray(x[0])

    def apply_event(self, ev):
        kind, i = ev[0], ev[1]
        if i not in self.idx:
            return
        j = self.idx.index(i)
        ln = LENS[int(self.slot[j])]
        if kind == "loopStart":      # setLoopStart :493-496
            self.loop[0, j] = int(ev[2] * ln)
        else:                        # maxiStretch::setSample :466-478: no grains, the whole new slot, position = looper = 0
            self.slot[j] = ev[2]
            self.gst[:, :, j] = 0.0
            self.loop[:, j] = (0, LENS[ev[2]])
            self.st[0, j] = self.st[1, j] = 0.0


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libgrainpool_host.so")
    flags = [f for f in fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "host_grainpool.cpp")])
    L = ctypes.CDLL(so)
    Z, I, D = ctypes.c_size_t, ctypes.c_int, ctypes.c_double
    L.gp_h_render.argtypes = [I, Z, Z, P, Z, Z, Z, P, P, P, P, I, D, D, I, P, P, P, I, P, Z, P, P, P]
    L.gp_h_loop.argtypes = [ctypes.c_uint64, D, D, P, P]
    L.gp_h_loop.restype = ctypes.c_char_p
    for f in (L.gp_h_advance, L.gp_h_advance_plain):
        f.restype = D
        f.argtypes = [D, D, D, I]
    return L


def _p(a):
    return None if a is None else a.ctypes.data


class HostBackend:
    """tests/host_grainpool.cpp: mxg_grainpool.h built by g++ under the oracle's flags.  The window tables are the reference's own
    (stored in the golden file)."""
    name = "host"

    def __init__(self, L, windows):
        self.L, self.windows = L, windows

    def call(self, mode, ov, win, n, mem, lens, slot, loop, a, b, pm, ps, rnd, st, gst):
        S = st.shape[1]
        out = np.zeros((n, S))
        w = np.ascontiguousarray(self.windows[win])
        rc = self.L.gp_h_render(mode, S, n, mem.ctypes.data + 8 * GUARD, STRIDE, CAP, len(lens), lens.ctypes.data, _p(slot), _p(loop), w.ctypes.data,
                                w.size, GRAIN_LENGTH, float(SR), ov, _p(a), _p(b), _p(pm), ps, _p(rnd), 0 if rnd is None else rnd.shape[1],
                                st.ctypes.data, gst.ctypes.data, out.ctypes.data)
        return out, rc


class TilesBackend(HostBackend):
    """tests/host_grainpool.cpp: the call as K27's tile form cuts it -- the scheduler pass with its birth lists, then every sample on
    its own from an anchor and a line (gp_tile_sched, gp_tile_sample), on the host."""
    name = "tiles"

    def call(self, *args):
        self.L.gp_h_tiles(1)
        try:
            return HostBackend.call(self, *args)
        finally:
            self.L.gp_h_tiles(0)


class TwinBackend:
    """The library's mxg_granular_pool_host (no device): its own plan, its own window table."""
    name = "twin"

    def __init__(self, m):
        self.m, self.lib, self.plans = m, m.lib(), {}

    def plan(self, win):
        if win not in self.plans:
            p = self.lib.mxg_grain_plan_create(WINDOWS[win], GRAIN_LENGTH, SR)
            assert p, self.lib.mxg_last_error().decode()
            self.plans[win] = p
        return self.plans[win]

    def call(self, mode, ov, win, n, mem, lens, slot, loop, a, b, pm, ps, rnd, st, gst):
        S = st.shape[1]
        out = np.zeros((n, S))
        rc = self.lib.mxg_granular_pool_host(self.plan(win), mode, S, n, mem.ctypes.data + 8 * GUARD, STRIDE, CAP, len(lens), lens.ctypes.data,
                                             _p(slot), _p(loop), ov, _p(a), _p(b), _p(pm), ps, _p(rnd), 0 if rnd is None else rnd.shape[1],
                                             st.ctypes.data, gst.ctypes.data, out.ctypes.data)
        return out, rc


class GpuBackend:
    """mxg_granular_pool_render over a pool from mxg_sample_pool_alloc; everything goes up before a call and comes back after it."""
    name = "gpu"

    def __init__(self, m):
        self.m, self.lib, self.plans = m, m.lib(), {}
        self.pool = None

    plan = TwinBackend.plan

    def _pool(self, mem, lens):
        key = (mem.tobytes(), lens.tobytes())
        if self.pool is None or self.pool[0] != key:
            st = ctypes.c_size_t(0)
            p = self.lib.mxg_sample_pool_alloc(len(lens), CAP, ctypes.byref(st))
            assert p, self.lib.mxg_last_error().decode()
            for r in range(len(lens)):
                a = np.ascontiguousarray(mem[GUARD + r * STRIDE:GUARD + r * STRIDE + CAP])
                self.m._lib.check(self.lib.mxg_memcpy_h2d(p + 8 * st.value * r, a.ctypes.data, a.nbytes, None), "h2d")
            dl = self.m.DeviceBuffer.from_numpy(lens)
            self.pool = (key, p, st.value, dl)
        return self.pool[1:]

    def call(self, mode, ov, win, n, mem, lens, slot, loop, a, b, pm, ps, rnd, st, gst):
        D = self.m.DeviceBuffer
        S = st.shape[1]
        p, stride, dl = self._pool(mem, lens)
        up = lambda x: None if x is None else D.from_numpy(np.ascontiguousarray(x))
        d = [up(x) for x in (slot, loop, a, b, pm, rnd)]
        dst, dgst, out = D.from_numpy(st), D.from_numpy(gst), D((n, S))
        ptr = lambda x: None if x is None else x.ptr
        rc = self.lib.mxg_granular_pool_render(self.plan(win), mode, S, n, p, stride, CAP, len(lens), dl.ptr, ptr(d[0]), ptr(d[1]), ov, ptr(d[2]),
                                               ptr(d[3]), ptr(d[4]), ps, ptr(d[5]), 0 if rnd is None else rnd.shape[1], dst.ptr, dgst.ptr,
                                               out.ptr, None)
        if rc == 0:
            rc = self.lib.mxg_sync()     # (what the device found while it rendered is the status of the next synchronising call)
        if rc == 0:
            rc = self.lib.mxg_last_async_error()
        o = out.numpy()
        st[...] = dst.numpy()
        gst[...] = dgst.numpy()
        return o, rc


def random_case(rng, mode, S, T):
    """Random streams over the table's pool: (ps, a, b, posMod, slot, loop, rnd, st); blocks [T][S] where a PS bit is set."""
    ps = int(rng.integers(0, 8)) & {0: 5, 1: 7, 2: 0, 3: 5, 4: 3}[mode]
    col = lambda lo, hi, per: rng.uniform(lo, hi, (T, S)) if per else rng.uniform(lo, hi, S)
    a = rng.uniform(0, 1, (T, S)) if mode == 2 else col(-1.5, 1.5, ps & 1)
    b = col(-2.0, 2.0, ps & 2) if mode == 1 else (col(0.0, 1.0, ps & 2) if mode == 4 else None)
    pm = col(0.0, 0.2, ps & 4) if mode in (0, 1, 3) and rng.integers(0, 2) else None
    if pm is None:
        ps &= ~4
    slot = rng.integers(0, R, S).astype(np.uint32)
    loop = np.zeros((2, S), np.uint64)
    for j in range(S):
        n = LENS[slot[j]]
        lo = int(rng.integers(0, n - 1))
        loop[:, j] = (lo, int(rng.integers(lo + 1, n + 1)))
    rnd = rng.integers(0, 10, (S, 200)).astype(np.int32) if rng.integers(0, 2) else None
    st = np.zeros((4, S))
    st[0] = rng.uniform(0, 1, S) * np.array(LENS)[slot]
    return ps, a, b, pm, slot, loop, rnd, st


def run_table(be, cuts=CUTS, only=None):
    """Plays the table through backend be, cut at `cuts` (the events' positions are added).  Returns (out [T][NS], {cut: (st [3][NS],
    gst [4][8][NS])})."""
    cuts = sorted(set(cuts) | set(EVENTS) | {0, T})
    mem, lens = pool_array(), np.array(LENS, np.uint64)
    out = np.zeros((T, NS))
    snaps = {c: (np.zeros((3, NS)), np.zeros((4, 8, NS))) for c in cuts[1:]}
    for key, idx in groups():
        if only is not None and key[0] not in only:
            continue
        gs = GroupState(key, idx)
        for n0, n1 in zip(cuts[:-1], cuts[1:]):
            if n0 in EVENTS:
                gs.apply_event(EVENTS[n0])
            rnd = gs.rnd
            o, rc = be.call(gs.mode, gs.ov, gs.win, n1 - n0, mem, lens, gs.slot, gs.loop if gs.mode == 1 else None, gs.block("a", n0, n1),
                            gs.block("b", n0, n1), gs.block("pm", n0, n1), gs.ps, rnd, gs.st, gs.gst)
            assert rc == 0, (be.name, key, n0, rc)
            out[n0:n1, idx] = o
            snaps[n1][0][:, idx] = gs.st[:3]
            snaps[n1][1][:, :, idx] = gs.gst
    return out, snaps


def check_table(be, g, extra=(), only=None):
    """run_table against the golden file, at every stored cut and for every stored array."""
    out, snaps = run_table(be, list(CUTS) + list(extra), only)
    cols = [i for i, s in enumerate(STREAMS) if only is None or s[0] in only]
    assert_bits_equal(out[:, cols], g["out"][:, cols], be.name + ": output")
    for ci, c in enumerate(CUTS[1:]):
        assert_bits_equal(snaps[c][0][:, cols], g["snap%d/st" % (ci + 1)][:, cols], "%s: position, looper, randomOffset at cut %d" % (be.name, c))
        assert_bits_equal(snaps[c][1][:, :, cols], g["snap%d/gst" % (ci + 1)][:, :, cols], "%s: live grains at cut %d" % (be.name, c))
