"""Host-side mirror of maxiTimeStretch / maxiStretch (src/libs/maxiGrains.h) as banks of streams."""
import ctypes

import numpy as np

from ._lib import check, lib
from .banks import DeviceBuffer, _Bank, _as_dev, _ptr

WINDOWS = {"hann": 0, "hamming": 1, "cosine": 2, "rect": 3, "triangle": 4, "triangleNZ": 5,
           "blackmanHarris": 6, "blackmanNutall": 7, "gaussian": 8}


class _GranularBank(_Bank):
    MODE = 0

    def __init__(self, streams, sample_bank, window="hann", stream=None):
        """`sample_bank`: a maxiSampleBank holding the shared maxiSample (setSample done)."""
        super().__init__(streams, stream)
        self.sample = sample_bank
        self.window_kind = WINDOWS[window] if isinstance(window, str) else int(window)
        self.state = DeviceBuffer((4, self.V))      # position, looper, randomOffset, rand cursor
        self.grains = DeviceBuffer((4, 8, self.V))  # live grains, creation order
        self._plans = {}

    def setPosition(self, pos):
        """maxiTimeStretch::setPosition (L/maxiGrains.h:335-338): clamp(pos*len, 0, len-1)."""
        st = self.state.numpy()
        n = self.sample.getLength()
        st[0] = np.clip(np.broadcast_to(np.asarray(pos, np.float64), (self.V,)) * n, 0, n - 1)
        self.state.upload(st)

    def getPosition(self):
        return self.state.numpy()[0]

    def getNormalisedPosition(self):
        return self.getPosition() / float(self.sample.getLength())

    def _plan(self, grainLength):
        key = (float(grainLength), self.sample.mySampleRate)
        if key not in self._plans:
            p = lib().mxg_grain_plan_create(self.window_kind, float(grainLength), self.sample.mySampleRate)
            if not p:
                raise ValueError(lib().mxg_last_error().decode())
            self._plans[key] = p
        return self._plans[key]

    def _render(self, a, b, grainLength, overlaps, posMod, N, rnd, out, mode=None):
        mode = self.MODE if mode is None else mode
        if mode == 2:   # per-sample position signal [N][S]
            da = a if (isinstance(a, DeviceBuffer) or hasattr(a, "data_ptr")) else \
                DeviceBuffer.from_numpy(np.ascontiguousarray(a, np.float64).reshape(N, self.V))
        else:
            da = _as_dev(a, self.V)
        db = None if b is None else _as_dev(b, self.V)
        dp = None if posMod is None else _as_dev(posMod, self.V)
        dr, R = None, 0
        if rnd is not None:
            r = np.ascontiguousarray(rnd, np.int32).reshape(self.V, -1)
            dr, R = DeviceBuffer.from_numpy(r), r.shape[1]
        out = self._out(N, out)
        check(lib().mxg_granular_render(self._plan(grainLength), mode, self.V, N, self.sample.d_samples,
                                        self.sample.getLength(), int(overlaps), _ptr(da), _ptr(db), _ptr(dp),
                                        _ptr(dr), R, self.state.ptr, self.grains.ptr, _ptr(out), self.stream),
              "mxg_granular_render")
        return out

    def close(self):
        for p in self._plans.values():
            lib().mxg_grain_plan_destroy(p)
        self._plans = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class maxiTimeStretchBank(_GranularBank):
    """S x maxiTimeStretch<F> (L/maxiGrains.h:287-368)."""
    MODE = 0

    def play(self, speed, grainLength, overlaps, N, posMod=None, rnd=None, out=None):
        return self._render(speed, None, grainLength, overlaps, posMod, N, rnd, out)

    def playAtPosition(self, pos, grainLength, overlaps, out=None):
        """maxiTimeStretch::playAtPosition (L/maxiGrains.h:359-367): `pos` is the [N][S] per-sample
        normalised position signal the caller iterates itself."""
        return self._render(pos, None, grainLength, overlaps, None, pos.shape[0], None, out, mode=2)


class maxiPitchShiftBank(_GranularBank):
    """S x maxiPitchShift<F> (L/maxiGrains.h:374-432).  state[1] is the member `cycles`."""
    MODE = 3

    def play(self, speed, grainLength, overlaps, N, posMod=None, out=None):
        return self._render(speed, None, grainLength, overlaps, posMod, N, None, out)


class maxiStretchBank(_GranularBank):
    """S x maxiStretch<F> (L/maxiGrains.h:436-542), default loop points."""
    MODE = 1

    def play(self, pitchstretch, timestretch, grainLength, overlaps, N, posMod=None, rnd=None, out=None):
        return self._render(pitchstretch, timestretch, grainLength, overlaps, posMod, N, rnd, out)


PS_A, PS_B, PS_POSMOD = 1, 2, 4   # MXG_GPOOL_PS_* (include/maxigpu.h)


class maxiGrainPoolBank(_Bank):
    """S granular streams that each read their OWN slot of a sample pool (K27, mxg_granular_pool_render): the reference's
    maxiTimeStretch / maxiPitchShift / maxiStretch objects after setSample(), maxiStretch with its loop points
    (L/maxiGrains.h:445, :493-509) and playAtPosition (:531-539).  `pool`: a maxiLooperBank -- the loops it recorded are stretched
    where they lie -- or a tuple (d_pool, stride, cap, lengths).  Parameters are scalars, arrays [S], or blocks [N][S] (numpy or a
    device block another bank wrote): a block is read at every sample, as a patch that hands play() a changing argument.  A render
    only enqueues while stream s reads slot s (the default with streams <= slots); with any other assignment the C-ABI reads the slot
    indices back before it launches, so the call waits for the stream and cannot be captured into a graph.  Every render returns the [N][S] block maxiMixBank.stereo takes.  Bit-exact; independent of how the samples are split into calls."""

    def __init__(self, streams, pool, window="hann", stream=None):
        super().__init__(streams, stream)
        self.window_kind = WINDOWS[window] if isinstance(window, str) else int(window)
        if isinstance(pool, tuple):
            self._d_pool, self.stride, self.cap, lengths = pool
            self._lengths = np.ascontiguousarray(lengths, np.uint64).reshape(-1)
            self._len = DeviceBuffer.from_numpy(self._lengths)
            self._bank = None
        else:
            self._bank, self.stride, self.cap = pool, pool.stride, pool.cap
        self.R = int(self.lengths.size)
        self.mySampleRate = 44100                       # maxiSample::setSample (H:676)
        self.state = DeviceBuffer((4, self.V))          # position, looper (maxiPitchShift: cycles), randomOffset, rand cursor
        self.grains = DeviceBuffer((4, 8, self.V))      # live grains, creation order
        self.slot = (np.arange(self.V) % self.R).astype(np.uint32)
        self.loop = np.stack([np.zeros(self.V, np.uint64), self.lengths[self.slot]])
        self._whole = np.ones(self.V, bool)             # the stream's loop is its whole slot: loopEnd follows the slot's length
        self._d_slot, self._d_loop = DeviceBuffer(self.V, np.uint32), DeviceBuffer((2, self.V), np.uint64)
        self._dirty = True
        self._plans = {}

    @property
    def lengths(self):
        return self._lengths if self._bank is None else self._bank.lengths

    def getLength(self, s):
        """The length of the slot stream s reads."""
        return int(self.lengths[self.slot[s]])

    def _streams(self, s):
        return range(self.V) if s is None else [int(s)]

    def setSlot(self, s, r, stretch=True):
        """setSample() of stream s: it reads slot r from now on and its live grains are gone.  stretch=True is
        maxiStretch::setSample (:466-478), which also resets position, looper and the loop to the whole slot."""
        s, r = int(s), int(r)
        if not 0 <= r < self.R:
            raise ValueError("maxiGrainPoolBank.setSlot: slot %d is outside the pool of %d slots" % (r, self.R))
        if not 0 <= s < self.V:
            raise ValueError("maxiGrainPoolBank.setSlot: stream %d of %d" % (s, self.V))
        self.slot[s] = r
        g = self.grains.numpy()
        g[:, :, s] = 0.0
        self.grains.upload(g)
        if stretch:
            st = self.state.numpy()
            st[0, s] = st[1, s] = 0.0
            self.state.upload(st)
            self.loop[:, s] = (0, self.lengths[r])
            self._whole[s] = True
        self._dirty = True

    def _set_loop(self, s, start01, end01):
        ls, le = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib().mxg_stretch_loop_host(self.getLength(s), float(start01), float(end01), ctypes.byref(ls), ctypes.byref(le)),
              "mxg_stretch_loop_host")
        return ls.value, le.value

    def setLoop(self, start01, end01, s=None):
        """setLoopStart and setLoopEnd together.  NaN, a negative value, loopStart >= loopEnd and loopEnd > len are refused."""
        for i in self._streams(s):
            self.loop[:, i] = self._set_loop(i, start01, end01)
            self._whole[i] = False
        self._dirty = True

    def setLoopStart(self, val, s=None):
        """maxiStretch::setLoopStart (:493-496): loopStart = (unsigned long)(val * len).  A start at or above the stream's loopEnd is
        refused (the reference's unsigned loopLength would wrap): move the end first."""
        for i in self._streams(s):
            ls, _ = self._set_loop(i, val, 1.0)
            if ls >= self.loop[1, i]:
                raise ValueError("maxiGrainPoolBank.setLoopStart: loopStart >= loopEnd (stream %d: %d >= %d)" % (i, ls, self.loop[1, i]))
            self.loop[0, i] = ls
            self._whole[i] = False
        self._dirty = True

    def setLoopEnd(self, val, s=None):
        """maxiStretch::setLoopEnd (:498-501)."""
        for i in self._streams(s):
            _, le = self._set_loop(i, 0.0, val)      # the conversion and its refusals are mxg_stretch_loop_host's alone
            if le <= self.loop[0, i]:
                raise ValueError("maxiGrainPoolBank.setLoopEnd: loopStart >= loopEnd (stream %d: %d >= %d)" % (i, self.loop[0, i], le))
            self.loop[1, i] = le
            self._whole[i] = False
        self._dirty = True

    def _follow_lengths(self):
        """A stream on its whole slot has loopEnd = the slot's length NOW (the pool's setSample / setLength may have changed it), as
        the reference's setSample re-derives it; a loop that was set stays as set."""
        cur = self.lengths[self.slot].astype(np.uint64)
        stale = self._whole & (self.loop[1] != cur)
        if stale.any():
            self.loop[1, stale] = cur[stale]
            self._dirty = True

    def getLoopEnd(self):
        self._follow_lengths()
        return self.loop[1].copy()

    def setPosition(self, pos):
        """setPosition (:488-491): clamp(pos * len, 0, len - 1), each stream with the length of its own slot."""
        st = self.state.numpy()
        n = self.lengths[self.slot].astype(np.float64)
        st[0] = np.clip(np.broadcast_to(np.asarray(pos, np.float64), (self.V,)) * n, 0, n - 1)
        self.state.upload(st)

    def getPosition(self):
        return self.state.numpy()[0]

    def getNormalisedPosition(self):
        return self.getPosition() / self.lengths[self.slot].astype(np.float64)

    def _plan(self, grainLength):
        key = float(grainLength)
        if key not in self._plans:
            p = lib().mxg_grain_plan_create(self.window_kind, key, self.mySampleRate)
            if not p:
                raise ValueError(lib().mxg_last_error().decode())
            self._plans[key] = p
        return self._plans[key]

    def _param(self, x, N):
        """-> (device object or None, read at every sample?)"""
        if x is None:
            return None, False
        if isinstance(x, DeviceBuffer) or hasattr(x, "data_ptr"):
            shape = tuple(x.shape)
            if shape == (N, self.V):
                return x, True
            if shape != (self.V,):
                raise ValueError("maxiGrainPoolBank: a device parameter is [S] or [N][S], not %r" % (shape,))
            return x, False
        a = np.asarray(x, np.float64)
        if a.ndim == 2:
            if a.shape != (N, self.V):
                raise ValueError("maxiGrainPoolBank: a parameter block is [N][S] = (%d, %d), not %r" % (N, self.V, a.shape))
            return DeviceBuffer.from_numpy(np.ascontiguousarray(a)), True
        return DeviceBuffer.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (self.V,)))), False

    def _render(self, mode, a, b, grainLength, overlaps, posMod, N, rnd, out):
        N = int(N)
        da, psa = self._param(a, N)
        db, psb = self._param(b, N)
        dp, psp = self._param(posMod, N)
        if mode == 2 and not psa:
            raise ValueError("maxiGrainPoolBank.playAtPosition: pos is the [N][S] position signal")
        ps = (PS_A if psa and mode != 2 else 0) | (PS_B if psb else 0) | (PS_POSMOD if psp else 0)
        dr, Rn = None, 0
        if rnd is not None:
            r = np.ascontiguousarray(rnd, np.int32).reshape(self.V, -1)
            dr, Rn = DeviceBuffer.from_numpy(r), r.shape[1]
        self._follow_lengths()
        if self._dirty:
            self._d_slot.upload(self.slot)
            self._d_loop.upload(self.loop)
            self._dirty = False
        out = self._out(N, out)
        d_pool, d_len = (self._d_pool, self._len.ptr) if self._bank is None else (self._bank.pool, self._bank.len.ptr)
        # the indices were checked in setSlot.  Stream s on slot s needs no d_slot at all, and then the call only enqueues; any other
        # assignment hands the C-ABI the device array, which it reads back before it launches (that call waits for the stream)
        identity = self.V <= self.R and bool((self.slot == np.arange(self.V)).all())
        check(lib().mxg_granular_pool_render(self._plan(grainLength), mode, self.V, N, d_pool, self.stride, self.cap, self.R, d_len,
                                             None if identity else self._d_slot.ptr, self._d_loop.ptr if mode == 1 else None, int(overlaps), _ptr(da), _ptr(db),
                                             _ptr(dp), ps, _ptr(dr), Rn, self.state.ptr, self.grains.ptr, _ptr(out), self.stream),
              "mxg_granular_pool_render")
        self._keep = (da, db, dp, dr)   # (alive until the stream has run the launch)
        return out

    def timestretch(self, speed, grainLength, overlaps, N, posMod=None, rnd=None, out=None):
        """maxiTimeStretch::play (:341-355)."""
        return self._render(0, speed, None, grainLength, overlaps, posMod, N, rnd, out)

    def pitchshift(self, speed, grainLength, overlaps, N, posMod=None, out=None):
        """maxiPitchShift::play (:412-430); state[1] is the member `cycles`."""
        return self._render(3, speed, None, grainLength, overlaps, posMod, N, None, out)

    def stretch(self, pitchstretch, timestretch, grainLength, overlaps, N, posMod=None, rnd=None, out=None):
        """maxiStretch::play (:512-530) inside each stream's loop points."""
        return self._render(1, pitchstretch, timestretch, grainLength, overlaps, posMod, N, rnd, out)

    def playAtPosition(self, pos, grainLength, overlaps, out=None):
        """maxiTimeStretch::playAtPosition (:359-367): pos is the [N][S] normalised position signal."""
        return self._render(2, pos, None, grainLength, overlaps, None, pos.shape[0], None, out)

    def stretchAtPosition(self, pitchstretch, pos, grainLength, overlaps, N=None, out=None):
        """maxiStretch::playAtPosition (:531-539): pos a scalar / [S] for the call, or the [N][S] position signal."""
        if N is None:
            N = pos.shape[0]
        return self._render(4, pitchstretch, pos, grainLength, overlaps, None, N, None, out)

    def close(self):
        for p in self._plans.values():
            lib().mxg_grain_plan_destroy(p)
        self._plans = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
