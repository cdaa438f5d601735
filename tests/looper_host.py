"""Shared by tests/test_looper_host.py, tests/test_gpu_looper.py and tools/gen/gen_golden_looper.py: the cases of
tests/golden/looper.npz (the table below; every input is derived HERE from small integers, for the generator and the tests alike),
numpy pools in the layout of mxg_sample_pool_alloc, three backends behind one interface -- the host build of mxg_looper.h
(tests/host_looper.cpp, g++ under the oracle's FPFLAGS), the library's _host twins and the library's device entry points -- and
drivers that play the file's cases through any of them and compare every stored cut bit for bit.

The host build and the _host twins are pinned to looper.npz by test_looper_host.py; the twin is then the checker of the GPU tests
on shapes the file does not hold."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT, assert_bits_equal

P = ctypes.c_void_p
PLAY_NONE, PLAY, PLAYLOOP = -1, 0, 2
GUARD_LO, GUARD_HI = 4, 22          # mxg_smp.h: kSmpGuardLo, kSmpGuardHi (checked against the host build in test_looper_host.py)
N, CUTS = 2000, [0, 1, 8, 143, 600, 601, 1429, 1993, 2000]
NAN = float("nan")

# ---- the golden bank: one row per slot -----------------------------------------------------------------------------------
# (len, start, end, mix, enable, prefill, recpos0, play): enable = "on" | "off" | ("burst", period) | "flip"; prefill: the "16-bit"
# ramp or zeros; recpos0: recordPosition at sample 0; play = (offset of the play head from the record head at sample 0 or None:
# position len - 1 as setSample leaves it, pstart, pend) with pstart / pend None = the record loop's own bounds.
ROWS = [
    (4096, 0.25, 0.2501, 0.5, "on", True, 0.0, (None, None, None)),         # 0  a span under one sample: one index
    (300, 0.5, 0.5, 0.0, ("burst", 7), False, 0.0, (None, None, None)),      # 1  start == end: one index; the lag never settles
    (300, 0.7, 0.2, 1.0, "on", True, 0.0, (None, None, None)),               # 2  start > end: one index; mix 1 keeps (cur / 32767 * lag) * 32767
    (777, 0.1003, 0.1503, 0.5, ("burst", 97), True, 0.0, (None, None, None)),  # 3  39 indices, fractional bounds
    (1000, 0.1, 0.3, 0.5, "on", False, 0.0, (None, None, None)),             # 4  200 indices: between 64 and a cut's length
    (1000, 0.1, 0.6, 0.5, "on", True, 0.0, (None, None, None)),              # 5  500 indices
    (50, 0.0, 1.0, 0.5, ("burst", 300), True, 0.0, (None, None, None)),      # 6  the whole sample, shorter than most cuts; lag reaches 1.0
    (4096, 0.0, 1.0, 0.0, "on", False, 0.0, (None, None, None)),             # 7  the whole sample, never wraps
    (1000, 0.25, 0.5, 1.0, "on", True, 0.0, (None, None, None)),             # 8  end * len = 500 exactly
    (101, 0.0, 0.995, 0.5, "off", True, 0.0, (None, 0.0, 1.0)),              # 9  never on; play() starts at len - 1
    (2, 0.0, 1.0, 0.5, "on", False, 0.0, (None, None, None)),                # 10 the shortest sample
    (101, 0.0, 1.0, 0.5, "flip", True, 0.0, (None, None, None)),             # 11 the enable flips inside cuts
    (50, 0.0, 1.0, 0.0, "on", False, 0.0, (None, None, None)),               # 12 a NaN and a -0.0 input sample
    (777, 0.0, 1.0, 0.5, "on", True, 0.0, (None, None, None)),               # 13 start -> 0.9003 at cut 601: the clamp, integer head, fractional bound
    (300, 0.0, 1.0, 0.5, ("burst", 97), True, 0.0, (None, None, None)),      # 14 trigger() at cut 1429
    (300, 0.0, 1.0, 0.5, "on", True, 5.0, (0, 0.0, 1.0)),                    # 15 the play head on the record head's index
    (300, 0.0, 1.0, 0.5, "on", True, 5.0, (1, 0.0, 1.0)),                    # 16 one ahead: old content
    (300, 0.0, 1.0, 0.5, "on", True, 5.0, (-1, 0.0, 1.0)),                   # 17 one behind: the sample before
    (4096, 0.75, 1.0, 0.5, "on", True, 0.0, (0, 0.0, 0.25)),                 # 18 a region the record head never reaches
]
R = len(ROWS)
LENS = np.array([r[0] for r in ROWS], np.uint64)
CAP = int(LENS.max())
SPECIAL_IN = {(700, 12): NAN, (701, 12): -0.0, (3, 12): NAN}          # (sample, slot): the input there
EVENTS = {601: ("bounds", 13, 0.9003, 1.0), 1429: ("trigger", 14)}   # at a cut, between two calls
PLAY_SLOTS = [9, 15, 16, 17, 18]   # the rows the play() run keeps (the playLoop run has all of them)
# normalise: (len, kind, maxLevel)
NORM_ROWS = [(300, "peak", 1.0), (101, "negpeak", 0.5), (1000, "ramp", 200.0), (50, "zero", 1.0)]


def ramp(n):
    """The patch's "16-bit" sample (tests/patches/sampler_zx_patch.cpp): integers in [-300, 300]."""
    i = np.arange(n)
    return ((i * 53) % 601 - 300).astype(np.float64)


def input_q(rows=R, seed=2500):
    """int16 [N][rows]: the input is q / 16384.0 (a carrier per slot plus noise: no two samples alike)."""
    rng = np.random.default_rng(seed)
    n = np.arange(N)[:, None]
    x = 0.8 * np.sin(2 * np.pi * n * (0.0131 + 0.0037 * np.arange(rows)[None, :])) + 0.05 * rng.standard_normal((N, rows))
    q = np.round(np.clip(x, -1.0, 1.0) * 16384).astype(np.int16)
    if rows == R:
        q[:, 16] = q[:, 17] = q[:, 15]    # the three play-head placements record the same signal
    return q


def signal(q):
    x = q.astype(np.float64) / 16384.0
    for (n, r), v in SPECIAL_IN.items():
        if r < x.shape[1]:
            x[n, r] = v
    return x


def enable_u8():
    """uint8 [N][R] from the rows' patterns.  A burst of period p is on for the first 60 % of it."""
    n = np.arange(N)
    e = np.zeros((N, R), np.uint8)
    for r, row in enumerate(ROWS):
        k = row[4]
        if k == "on":
            e[:, r] = 1
        elif k == "flip":   # flips inside the cuts 143..600, 601..1429 and 1993..2000
            e[:, r] = ((n >= 300) & (n < 450)) | ((n >= 700) & (n < 1100)) | (n == 1995) | (n == 1997)
        elif k != "off":
            e[:, r] = (n % k[1]) < (k[1] * 6) // 10
    return e


def enable_block(u8):
    """The doubles a gate block would hold: any non-zero value means true (2.5, -1 and a denormal among them)."""
    vals = np.array([1.0, 2.5, -1.0, 1e-300])
    n = np.arange(u8.shape[0])[:, None] + np.arange(u8.shape[1])[None, :]
    return np.where(u8 != 0, vals[n % 4], 0.0)


def play_start(mode, rows=None):
    """position at sample 0 for every row: play() reads its head and then moves, playLoop moves and then reads."""
    rows = ROWS if rows is None else rows
    pos = np.zeros(len(rows))
    for r, row in enumerate(rows):
        off = row[7][0]
        pos[r] = row[0] - 1 if off is None else row[6] + off - (1 if mode == PLAYLOOP else 0)
    return pos


def play_bounds(rows=None):
    rows = ROWS if rows is None else rows
    ps = np.array([row[1] if row[7][1] is None else row[7][1] for row in rows])
    pe = np.array([row[2] if row[7][2] is None else row[7][2] for row in rows])
    return ps, pe


def stride_of(cap):
    return (cap + GUARD_LO + GUARD_HI + 15) // 16 * 16


class Bank:
    """A pool in the layout of mxg_sample_pool_alloc as one numpy array, with the per-slot members."""

    def __init__(self, lens, cap=None):
        self.len = np.ascontiguousarray(lens, np.uint64)
        self.R = len(self.len)
        self.cap = int(cap if cap is not None else self.len.max())
        self.stride = stride_of(self.cap)
        self.mem = np.zeros(self.R * self.stride)
        self.recpos, self.lag, self.position = np.zeros(self.R), np.zeros(self.R), self.len.astype(np.float64) - 1
        self.mix, self.start, self.end = np.full(self.R, 0.5), np.zeros(self.R), np.ones(self.R)
        self.pstart, self.pend = np.zeros(self.R), np.ones(self.R)
        self.dropped = np.zeros(self.R, np.uint32)

    @property
    def pool_ptr(self):
        return self.mem.ctypes.data + 8 * GUARD_LO

    def slot(self, r):
        o = r * self.stride + GUARD_LO
        return self.mem[o:o + int(self.len[r])]

    def set_sample(self, r, data):
        o = r * self.stride + GUARD_LO
        self.mem[o:o + self.cap] = 0.0
        self.mem[o:o + len(data)] = data
        self.position[r] = len(data) - 1      # setSample (H:670-678)

    def trigger(self, r=None):
        r = slice(None) if r is None else r
        self.position[r] = 0.0
        self.recpos[r] = 0.0

    def outside(self):
        """Everything that is not inside [0, len) of a slot: guards, tails, padding."""
        m = np.ones(self.mem.size, bool)
        for r in range(self.R):
            o = r * self.stride + GUARD_LO
            m[o:o + int(self.len[r])] = False
        return self.mem[m]

    def copy(self):
        b = Bank(self.len, self.cap)
        for k in ("mem", "recpos", "lag", "position", "mix", "start", "end", "pstart", "pend", "dropped"):
            setattr(b, k, getattr(self, k).copy())
        return b


def golden_bank(mode, rows=None):
    rows = list(range(R)) if rows is None else rows
    sel = [ROWS[r] for r in rows]
    b = Bank([row[0] for row in sel], CAP)
    for i, row in enumerate(sel):
        if row[5]:
            b.set_sample(i, ramp(row[0]))
        b.mix[i], b.start[i], b.end[i], b.recpos[i] = row[3], row[1], row[2], row[6]
    b.position[:] = play_start(mode, sel)
    b.pstart[:], b.pend[:] = play_bounds(sel)
    return b


def norm_bank():
    b = Bank([row[0] for row in NORM_ROWS])
    for i, (n, kind, _) in enumerate(NORM_ROWS):
        a = ramp(n)
        if kind == "peak":
            a[n // 3] = 4711.0
        elif kind == "negpeak":
            a[n // 2] = -3000.5
        elif kind == "zero":
            a[:] = 0.0
            a[1::2] = -0.0
        b.set_sample(i, a)
    return b, np.array([row[2] for row in NORM_ROWS])


def apply_event(b, ev, rows):
    if ev[1] not in rows:
        return
    i = rows.index(ev[1])
    if ev[0] == "bounds":
        b.start[i], b.end[i] = ev[2], ev[3]
    else:
        b.trigger(i)


# ---- backends --------------------------------------------------------------------------------------------------------------
def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "liblooper_host.so")
    flags = [f for f in fpflags() if not f.startswith("-O")] + HOST_OPT
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "host_looper.cpp")])
    L = ctypes.CDLL(so)
    S, I, D = ctypes.c_size_t, ctypes.c_int, ctypes.c_double
    L.lp_h_render.argtypes = [S, S, P, S, P, P, P, I] + [P] * 5 + [I] + [P] * 5
    L.lp_h_render_pieces.argtypes = [I, I] + L.lp_h_render.argtypes
    L.lp_h_normalise.argtypes = [S, P, S, P, P]
    for f in (L.lp_h_play_step, L.lp_h_smp_step):
        f.restype = ctypes.c_longlong
        f.argtypes = [I, P, D, D, S]
    L.lp_h_guards.argtypes = [P, P]
    return L


def _c(a):
    return None if a is None else np.ascontiguousarray(a, np.float64)


def _p(a):
    return None if a is None else a.ctypes.data


class HostBackend:
    """tests/host_looper.cpp: the bank's arrays are updated in place."""
    name = "host"

    def __init__(self, L):
        self.L = L

    def render(self, b, x, enable, mode=PLAY_NONE):
        x, enable = _c(x), _c(enable)
        n = x.shape[0]
        out = np.zeros((n, b.R)) if mode != PLAY_NONE else None
        self.L.lp_h_render(b.R, n, b.pool_ptr, b.stride, _p(b.len), _p(x), _p(enable), int(enable.ndim == 2), _p(b.mix), _p(b.start), _p(b.end),
                           _p(b.recpos), _p(b.lag), mode, _p(b.pstart), _p(b.pend), _p(b.position), _p(out), _p(b.dropped))
        return out

    def normalise(self, b, level):
        level = _c(level)
        self.L.lp_h_normalise(b.R, b.pool_ptr, b.stride, _p(b.len), _p(level))


class PiecesBackend(HostBackend):
    """tests/host_looper.cpp: the call as K25 cuts it into pieces and tiles (lp_plan_slot, lp_walk_element), on the host."""

    def __init__(self, L, piece, tile):
        self.L, self.piece, self.tile, self.name = L, piece, tile, "pieces(%d, %d)" % (piece, tile)

    def render(self, b, x, enable, mode=PLAY_NONE):
        x, enable = _c(x), _c(enable)
        n = x.shape[0]
        out = np.zeros((n, b.R)) if mode != PLAY_NONE else None
        self.L.lp_h_render_pieces(self.piece, self.tile, b.R, n, b.pool_ptr, b.stride, _p(b.len), _p(x), _p(enable), int(enable.ndim == 2), _p(b.mix),
                                  _p(b.start), _p(b.end), _p(b.recpos), _p(b.lag), mode, _p(b.pstart), _p(b.pend), _p(b.position), _p(out),
                                  _p(b.dropped))
        return out


class TwinBackend:
    """The library's _host twins (no device)."""
    name = "twin"

    def __init__(self, mx):
        self.mx, self.lib = mx, mx.lib()

    def render(self, b, x, enable, mode=PLAY_NONE):
        x, enable = _c(x), _c(enable)
        n = x.shape[0]
        out = np.zeros((n, b.R)) if mode != PLAY_NONE else None
        self.mx._lib.check(self.lib.mxg_looprec_host(b.R, n, b.pool_ptr, b.stride, b.cap, _p(b.len), _p(x), _p(enable), int(enable.ndim == 2),
                                                     _p(b.mix), _p(b.start), _p(b.end), _p(b.recpos), _p(b.lag), mode, _p(b.pstart), _p(b.pend),
                                                     _p(b.position), _p(out), _p(b.dropped)), "mxg_looprec_host")
        return out

    def normalise(self, b, level):
        level = _c(level)
        self.mx._lib.check(self.lib.mxg_sample_pool_normalise_host(b.R, b.pool_ptr, b.stride, b.cap, _p(b.len), _p(level)),
                           "mxg_sample_pool_normalise_host")


class _Prefix:
    """The first R slots of a bank, as the entry points address them."""

    def __init__(self, b, R):
        self.full, self.R, self.cap, self.stride = b, R, b.cap, b.stride


class GpuBackend:
    """The device entry points over a pool from mxg_sample_pool_alloc: the numpy bank goes up before a call and comes back after it
    (guards, tails and padding included), so a test sees every byte the kernel could have touched."""
    name = "gpu"

    def __init__(self, mx):
        self.mx, self.lib = mx, mx.lib()

    def _up(self, b):
        mx, L = self.mx, self.lib
        b = getattr(b, "full", b)
        st = ctypes.c_size_t(0)
        pool = L.mxg_sample_pool_alloc(b.R, b.cap, ctypes.byref(st))
        assert pool and st.value == b.stride, (pool, st.value, b.stride)
        mx._lib.check(L.mxg_memcpy_h2d(pool - 8 * GUARD_LO, b.mem.ctypes.data, b.mem.nbytes, None), "h2d")
        D = mx.DeviceBuffer
        d = {k: D.from_numpy(getattr(b, k)) for k in ("recpos", "lag", "position", "mix", "start", "end", "pstart", "pend", "dropped")}
        d["len"] = D(b.R, np.uint64)
        mx._lib.check(L.mxg_sample_pool_lengths(b.R, b.cap, _p(b.len), d["len"].ptr), "mxg_sample_pool_lengths")
        return pool, d

    def _down(self, b, pool, d):
        mx, L = self.mx, self.lib
        mx._lib.check(L.mxg_sync(), "mxg_sync")
        mx._lib.check(L.mxg_memcpy_d2h(b.mem.ctypes.data, pool - 8 * GUARD_LO, b.mem.nbytes, None), "d2h")
        for k in ("recpos", "lag", "position", "dropped"):
            getattr(b, k)[:] = d[k].numpy()
        mx._lib.check(L.mxg_sample_pool_free(pool), "mxg_sample_pool_free")

    def render(self, b, x, enable, mode=PLAY_NONE, band=0, R=None):
        """band > 0: the output block lies inside a larger allocation filled with a sentinel, which must come back intact.
        R: address only the first R slots of the bank (x, enable and the output are [n][R])."""
        mx, L = self.mx, self.lib
        x, enable = _c(x), _c(enable)
        n = x.shape[0]
        full, b = b, (b if R is None else _Prefix(b, R))
        pool, d = self._up(b)
        dx, de = mx.DeviceBuffer.from_numpy(x), mx.DeviceBuffer.from_numpy(enable)
        SENT = -7.25
        dout = mx.DeviceBuffer.from_numpy(np.full(n * b.R + 2 * band, SENT)) if mode != PLAY_NONE else None
        mx._lib.check(L.mxg_looprec_render(b.R, n, pool, b.stride, b.cap, d["len"].ptr, dx.ptr, de.ptr, int(enable.ndim == 2), d["mix"].ptr,
                                           d["start"].ptr, d["end"].ptr, d["recpos"].ptr, d["lag"].ptr, mode, d["pstart"].ptr, d["pend"].ptr,
                                           d["position"].ptr, (dout.ptr + 8 * band) if dout else None, d["dropped"].ptr, None),
                      "mxg_looprec_render")
        self._down(full, pool, d)
        if dout is None:
            return None
        o = dout.numpy()
        if band:
            assert (o[:band] == SENT).all() and (o[band + n * b.R:] == SENT).all(), "the output block's bands were written"
        return o[band:band + n * b.R].reshape(n, b.R)

    def normalise(self, b, level):
        mx, L = self.mx, self.lib
        pool, d = self._up(b)
        dl = mx.DeviceBuffer.from_numpy(_c(level))
        mx._lib.check(L.mxg_sample_pool_normalise(b.R, pool, b.stride, b.cap, d["len"].ptr, dl.ptr, None), "mxg_sample_pool_normalise")
        self._down(b, pool, d)


# ---- drivers ---------------------------------------------------------------------------------------------------------------
def run_case(be, g, key, cuts):
    """Plays the stored run `key` ("loop": every row under playLoop; "play": PLAY_SLOTS under play()) through backend be, cut at
    `cuts` (the events' positions are added).  Returns (out, bank)."""
    mode, rows = (PLAYLOOP, list(range(R))) if key == "loop" else (PLAY, PLAY_SLOTS)
    cuts = sorted(set(cuts) | set(EVENTS) | {0, N})
    x = signal(g["inq"])[:, rows]
    en = enable_block(g["en"])[:, rows]
    b = golden_bank(mode, rows)
    outs = []
    for a, c in zip(cuts[:-1], cuts[1:]):
        if a in EVENTS:
            apply_event(b, EVENTS[a], rows)
        outs.append(be.render(b, x[a:c], en[a:c], mode))
    return np.concatenate(outs), b


def check_cuts(be, g, key, extra=()):
    """run_case, comparing at every stored cut: recordPosition, the lag's val, position and the content of every slot."""
    mode, rows = (PLAYLOOP, list(range(R))) if key == "loop" else (PLAY, PLAY_SLOTS)
    stored = [int(c) for c in g["cuts"]]
    cuts = sorted(set(stored) | set(extra))
    x = signal(g["inq"])[:, rows]
    en = enable_block(g["en"])[:, rows]
    b = golden_bank(mode, rows)
    ref = golden_bank(mode, rows)
    outs = []
    for a, c in zip(cuts[:-1], cuts[1:]):
        if a in EVENTS:
            apply_event(b, EVENTS[a], rows)
        outs.append(be.render(b, x[a:c], en[a:c], mode))
        if c in stored:
            i = stored.index(c)
            what = "%s: %s at cut %d" % (be.name, key, c)
            flat, val = g["%s/snap%d/idx" % (key, i)], g["%s/snap%d/val" % (key, i)]
            for f, v in zip(flat, val):     # flat = slot * CAP + element
                ref.slot(int(f) // CAP)[int(f) % CAP] = v
            assert_bits_equal(b.recpos, g["%s/snap%d/recpos" % (key, i)], what + " recordPosition")
            assert_bits_equal(b.lag, g["%s/snap%d/lag" % (key, i)], what + " lag")
            assert_bits_equal(b.position, g["%s/snap%d/position" % (key, i)], what + " position")
            assert_bits_equal(b.mem, ref.mem, what + " slot contents, guards and tails")
    assert_bits_equal(np.concatenate(outs), g[key + "/out"], "%s: %s output" % (be.name, key))
    assert not b.dropped.any(), "a golden case counted a dropped sample"
    return b


def check_normalise(be, g):
    b, level = norm_bank()
    be.normalise(b, level)
    for i in range(b.R):
        assert_bits_equal(b.slot(i), g["norm/after%d" % i], "%s: normalise slot %d" % (be.name, i))
    assert not b.outside().any()
    return b


def random_case(rng, Rr, Nn, cap=None, domain=True):
    """A bank with random contents, lengths, bounds and members, an input block and an enable block (per sample or per slot)."""
    cap = int(cap if cap is not None else rng.integers(2, 601))
    lens = rng.integers(2, cap + 1, Rr)
    lens[rng.integers(0, Rr)] = cap
    b = Bank(lens, cap)
    for r in range(Rr):
        if rng.integers(0, 3):
            b.set_sample(r, np.round(rng.uniform(-3e4, 3e4, int(lens[r]))))
    kind = rng.integers(0, 5, Rr)
    s, e = rng.uniform(0, 0.999, Rr), rng.uniform(0, 1, Rr)
    e = np.where(kind == 0, 1.0, np.where(kind == 1, s, np.where(kind == 2, np.minimum(1.0, s + rng.uniform(0, 0.1, Rr)), e)))
    s = np.where(kind == 0, 0.0, s)
    b.start[:], b.end[:] = s, e
    b.mix[:] = rng.choice([0.0, 0.5, 1.0, 0.3], Rr)
    b.recpos[:] = np.floor(rng.uniform(0, 1, Rr) * lens)
    b.lag[:] = rng.choice([0.0, 1.0, 0.37], Rr)
    b.position[:] = np.floor(rng.uniform(0, 1, Rr) * lens)
    ps = rng.uniform(0, 0.999, Rr)
    b.pstart[:], b.pend[:] = ps, np.minimum(1.0, ps + rng.uniform(0, 1, Rr))
    x = rng.uniform(-1, 1, (Nn, Rr))
    if rng.integers(0, 2):
        en = (rng.uniform(0, 1, (Nn, Rr)) < rng.choice([0.1, 0.5, 0.9, 1.0])).astype(np.float64) * rng.choice([1.0, -2.0])
    else:
        en = rng.integers(0, 2, Rr).astype(np.float64)
    return b, x, en


def same_bank(a, b, what):
    assert_bits_equal(a.mem, b.mem, what + ": pool (contents, guards, tails)")
    for k in ("recpos", "lag", "position"):
        assert_bits_equal(getattr(a, k), getattr(b, k), what + ": " + k)
    assert np.array_equal(a.dropped, b.dropped), what + ": dropped"
