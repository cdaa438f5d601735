"""Host-side mirror of the reference's operator API, one *bank* of V instances per object.

Names follow the reference (src/maximilian.h): `maxiOscBank.sinebuf(freq, N)` renders what N
consecutive calls of `maxiOsc::sinebuf(freq[v])` on each of the V oscillators would return,
as an [N, V] sample-major block that stays on the device.  State (phase, filter memories,
envelope flags ...) lives in device SoA arrays owned by the bank and carries from block to
block, exactly like consecutive `play()` callbacks.  Everything here is plumbing over the
C-ABI (maximilian_amd/_lib.py); no arithmetic on signals happens in Python.
"""
import ctypes
import os

import numpy as np

from ._lib import check, lib

OSC_WAVEFORMS = {
    "sinewave": 0, "coswave": 1, "phasor": 2, "saw": 3, "triangle": 4, "square": 5, "pulse": 6,
    "impulse": 7, "sinebuf": 8, "sinebuf4": 9, "sawn": 10, "phasorBetween": 11,
}
FILTER_KINDS = {"lores": 0, "hires": 1, "bandpass": 2, "lopass": 3, "hipass": 4}


class DeviceBuffer:
    """A typed device allocation (hipMalloc via mxg_malloc) with numpy upload/download.

    Stream contract: banks launch on their own `stream`, while allocation-time zeroing and the
    copies here go through the library's default stream.  So the zeroing is complete before the
    constructor returns, upload() is synchronous (mxg_memcpy_h2d waits), and numpy() waits for ALL
    outstanding device work (mxg_sync) before it copies -- a block a kernel on any stream is still
    writing is never read half-finished, and a first render never races the zero fill."""

    def __init__(self, shape, dtype=np.float64, zero=True):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.ptr = lib().mxg_malloc(max(self.nbytes, 8))
        if not self.ptr:
            raise MemoryError("mxg_malloc(%d): %s" % (self.nbytes, lib().mxg_last_error().decode()))
        if zero and self.nbytes:
            check(lib().mxg_memset(self.ptr, 0, self.nbytes, None), "mxg_memset")
            check(lib().mxg_stream_sync(None), "mxg_stream_sync")

    @classmethod
    def from_numpy(cls, a, dtype=None):
        a = np.ascontiguousarray(a, dtype=dtype if dtype is not None else a.dtype)
        b = cls(a.shape, a.dtype, zero=False)
        b.upload(a)
        return b

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.nbytes == self.nbytes, (a.shape, self.shape)
        if self.nbytes:
            check(lib().mxg_memcpy_h2d(self.ptr, a.ctypes.data, self.nbytes, None), "mxg_memcpy_h2d")
        return self

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            check(lib().mxg_sync(), "mxg_sync")  # the producer may have run on any stream
            check(lib().mxg_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes, None), "mxg_memcpy_d2h")
        return out

    def free(self):
        if getattr(self, "ptr", None):
            lib().mxg_free(self.ptr)
            self.ptr = None

    def __del__(self):  # best effort
        try:
            self.free()
        except Exception:
            pass


def _ptr(x):
    """Device pointer of a DeviceBuffer / torch tensor / raw int / None."""
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


def _as_dev(x, V, dtype=np.float64):
    """Per-voice parameter: scalar / array-like -> DeviceBuffer [V]; device objects pass through."""
    if isinstance(x, DeviceBuffer) or hasattr(x, "data_ptr"):
        return x
    a = np.asarray(x, dtype=dtype)
    if a.ndim == 0:
        a = np.full(V, a, dtype=dtype)
    return DeviceBuffer.from_numpy(a)


class maxiSettings:
    """maxiSettings (H:117-163): global sampleRate / channels / bufferSize."""
    sampleRate, channels, bufferSize = 44100, 2, 1024

    @classmethod
    def setup(cls, sampleRate, channels, bufferSize):
        check(lib().mxg_settings(sampleRate, channels, bufferSize), "mxg_settings")
        cls.sampleRate, cls.channels, cls.bufferSize = sampleRate, channels, bufferSize


class _Bank:
    def __init__(self, voices, stream=None):
        check(lib().mxg_init(-1), "mxg_init")
        self.V = int(voices)
        self.stream = stream

    def _out(self, N, out):
        return out if out is not None else DeviceBuffer((N, self.V), np.float64, zero=False)

    def sync(self):
        check(lib().mxg_stream_sync(self.stream), "mxg_stream_sync")


class maxiOscBank(_Bank):
    """V x maxiOsc (H:169-215).  Methods: one per reference waveform, `(freq, N)` -> [N, V]."""

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.phase = DeviceBuffer(self.V)   # maxiOsc::phase  (ctor sets 0, C:209-212)
        self.output = DeviceBuffer(self.V)  # maxiOsc::output (held by square/pulse)

    def phaseReset(self, phaseIn):
        """maxiOsc::phaseReset (C:222-226), per voice."""
        self.phase.upload(np.broadcast_to(np.asarray(phaseIn, np.float64), (self.V,)))

    def render(self, waveform, freq, N, p1=None, p2=None, out=None, per_sample=False, pitch=None):
        """`pitch`: row pitch of the output in DOUBLES (mxg_osc_render_pitch): the block is then a [N, pitch] buffer whose first V
        columns are the voices (the rest is padding nobody writes); None = V."""
        wf = OSC_WAVEFORMS[waveform] if isinstance(waveform, str) else int(waveform)
        if per_sample:
            f = freq if (isinstance(freq, DeviceBuffer) or hasattr(freq, "data_ptr")) else \
                DeviceBuffer.from_numpy(np.asarray(freq, np.float64).reshape(N, self.V))
        else:
            f = _as_dev(freq, self.V)
        a = None if p1 is None else _as_dev(p1, self.V)
        b = None if p2 is None else _as_dev(p2, self.V)
        if pitch is not None and int(pitch) != self.V:
            out = out if out is not None else DeviceBuffer((N, int(pitch)), np.float64)
            check(lib().mxg_osc_render_pitch(wf, self.V, N, _ptr(f), 1 if per_sample else 0, _ptr(a), _ptr(b), self.phase.ptr,
                                             self.output.ptr, _ptr(out), int(pitch) * 8, self.stream), "mxg_osc_render_pitch")
            self._keep = (f, a, b)
            return out
        out = self._out(N, out)
        check(lib().mxg_osc_render(wf, self.V, N, _ptr(f), 1 if per_sample else 0, _ptr(a), _ptr(b),
                                   self.phase.ptr, self.output.ptr, _ptr(out), self.stream),
              "mxg_osc_render")
        self._keep = (f, a, b)  # keep parameter buffers alive until the next call
        return out

    def render_mix(self, waveform, freq, pan, N, p1=None, p2=None, out=None, store=True, mix=None, rows=None):
        """Render + fused maxiMix::stereo mixdown in one pass (mxg_osc_render_mix).
        Returns (out [N,V] or None, mix [N,2]).  rows: a device pointer / buffer [mxg_osc_mix_groups(V)][N][2] (e.g. a
        grouped mix queue's slot) -- then the per-workgroup rows are left there (mxg_osc_render_mix_rows) and no mix is
        formed here; returns (out, None)."""
        wf = OSC_WAVEFORMS[waveform] if isinstance(waveform, str) else int(waveform)
        f, pn = _as_dev(freq, self.V), _as_dev(pan, self.V)
        a = None if p1 is None else _as_dev(p1, self.V)
        b = None if p2 is None else _as_dev(p2, self.V)
        out = (self._out(N, out) if store else None)
        if rows is not None:
            check(lib().mxg_osc_render_mix_rows(wf, self.V, N, _ptr(f), _ptr(a), _ptr(b), self.phase.ptr,
                                                self.output.ptr, _ptr(out), _ptr(pn), _ptr(rows), self.stream),
                  "mxg_osc_render_mix_rows")
            self._keep = (f, a, b, pn)
            return out, None
        mix = mix if mix is not None else DeviceBuffer((N, 2), np.float64, zero=False)
        check(lib().mxg_osc_render_mix(wf, self.V, N, _ptr(f), _ptr(a), _ptr(b), self.phase.ptr,
                                       self.output.ptr, _ptr(out), _ptr(pn), _ptr(mix), self.stream),
              "mxg_osc_render_mix")
        self._keep = (f, a, b, pn)
        return out, mix

    def sinebuf_tables(self, freq, tables, N, pan=None, store=True, out=None, ahead=False, fused_sum=False):
        """EXTENSION: sinebuf with a 514-entry table per voice (mxg_osc_render_tables).  tables: [V][514] (numpy or device).
        Returns (out [N,V] or None, mix [N,2] or None): the mix is formed from the kernel's partial rows with mxg_mix_rows_sum, or
        (fused_sum) inside the render kernel.  ahead: the pipelined form (MXG_TABLES_AHEAD): freq / pan must then be the SAME device
        buffers from call to call (pass DeviceBuffers) and self.phase untouched in between."""
        if ahead or fused_sum:
            f = _as_dev(freq, self.V)
            tb = tables if isinstance(tables, DeviceBuffer) or hasattr(tables, "data_ptr") else DeviceBuffer.from_numpy(
                np.ascontiguousarray(tables, np.float64))
            out = self._out(N, out) if store else None
            pn = rows = mix = None
            if pan is not None:
                pn = _as_dev(pan, self.V)
                G = lib().mxg_osc_tables_groups(self.V)
                rows = DeviceBuffer((G, N, 2), np.float64)
                mix = DeviceBuffer((N, 2), np.float64, zero=False)
            check(lib().mxg_osc_render_tables_ex(self.V, N, _ptr(f), _ptr(tb), self.phase.ptr, self.output.ptr, _ptr(out), _ptr(pn), _ptr(rows),
                                                 _ptr(mix) if (fused_sum and mix is not None) else None, 1 if ahead else 0, self.stream),
                  "mxg_osc_render_tables_ex")
            if pan is not None and not fused_sum:
                check(lib().mxg_mix_rows_sum(G, N * 2, rows.ptr, mix.ptr, self.stream), "mxg_mix_rows_sum")
            self._keep = (f, tb, pn, rows)
            self.last_rows = rows
            return out, mix
        f = _as_dev(freq, self.V)
        tb = tables if isinstance(tables, DeviceBuffer) or hasattr(tables, "data_ptr") else DeviceBuffer.from_numpy(
            np.ascontiguousarray(tables, np.float64))
        out = self._out(N, out) if store else None
        pn = rows = mix = None
        if pan is not None:
            pn = _as_dev(pan, self.V)
            G = lib().mxg_osc_tables_groups(self.V)
            rows = DeviceBuffer((G, N, 2), np.float64)
        check(lib().mxg_osc_render_tables(self.V, N, _ptr(f), _ptr(tb), self.phase.ptr, self.output.ptr, _ptr(out), _ptr(pn), _ptr(rows),
                                          self.stream), "mxg_osc_render_tables")
        if pan is not None:
            mix = DeviceBuffer((N, 2), np.float64, zero=False)
            check(lib().mxg_mix_rows_sum(G, N * 2, rows.ptr, mix.ptr, self.stream), "mxg_mix_rows_sum")
        self._keep = (f, tb, pn, rows)
        return out, mix

    def noise(self, rand, out=None):
        """maxiOsc::noise (C:214-220) from caller-supplied rand() draws, int32 [N][V] (draw n*V+v is the
        one a voice-inner per-sample loop hands to voice v at sample n)."""
        if not (isinstance(rand, DeviceBuffer) or hasattr(rand, "data_ptr")):
            rand = DeviceBuffer.from_numpy(np.ascontiguousarray(rand, np.int32))
        N = rand.shape[0]
        out = self._out(N, out)
        check(lib().mxg_osc_noise(self.V, N, _ptr(rand), self.output.ptr, _ptr(out), self.stream),
              "mxg_osc_noise")
        self._keep = rand
        return out

    def sinewave(self, freq, N, **kw): return self.render("sinewave", freq, N, **kw)
    def coswave(self, freq, N, **kw): return self.render("coswave", freq, N, **kw)
    def phasor(self, freq, N, **kw): return self.render("phasor", freq, N, **kw)
    def saw(self, freq, N, **kw): return self.render("saw", freq, N, **kw)
    def triangle(self, freq, N, **kw): return self.render("triangle", freq, N, **kw)
    def square(self, freq, N, **kw): return self.render("square", freq, N, **kw)
    def pulse(self, freq, duty, N, **kw): return self.render("pulse", freq, N, p1=duty, **kw)
    def impulse(self, freq, N, **kw): return self.render("impulse", freq, N, **kw)
    def sinebuf(self, freq, N, **kw): return self.render("sinebuf", freq, N, **kw)
    def sinebuf4(self, freq, N, **kw): return self.render("sinebuf4", freq, N, **kw)
    def sawn(self, freq, N, **kw): return self.render("sawn", freq, N, **kw)

    def phasorBetween(self, freq, startphase, endphase, N, **kw):
        return self.render("phasorBetween", freq, N, p1=startphase, p2=endphase, **kw)


def filter_coeffs(kind, cutoff, res):
    """Host-libm coefficients [3][V] of maxiFilter::lores/hires (c, r; C:456-461) or bandpass
    (inputs[0..2]; C:489-495), per voice."""
    k = FILTER_KINDS[kind] if isinstance(kind, str) else int(kind)
    cutoff = np.ascontiguousarray(cutoff, np.float64)
    res = np.ascontiguousarray(np.broadcast_to(np.asarray(res, np.float64), cutoff.shape))
    coef = np.zeros((3, cutoff.size))
    check(lib().mxg_filter_coeffs_host(k, cutoff.size, cutoff.ctypes.data, res.ctypes.data,
                                       coef.ctypes.data), "mxg_filter_coeffs_host")
    return coef


class maxiFilterBank(_Bank):
    """V x maxiFilter (H:289-366)."""

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.state = DeviceBuffer((5, self.V))  # x, y, outputs[0..2]  (ctor zeros, C:1517)

    def render(self, kind, x, cutoff, resonance=None, out=None, cutoff_per_sample=False,
               res_per_sample=False):
        k = FILTER_KINDS[kind] if isinstance(kind, str) else int(kind)
        N = x.shape[0]
        coef = None
        if k in (0, 1, 2) and not (cutoff_per_sample or res_per_sample):
            cu = np.broadcast_to(np.asarray(cutoff, np.float64), (self.V,))
            coef = DeviceBuffer.from_numpy(filter_coeffs(k, cu, resonance))
        cut = cutoff if cutoff_per_sample and not isinstance(cutoff, np.ndarray) else (
            DeviceBuffer.from_numpy(np.asarray(cutoff, np.float64).reshape(N, self.V))
            if cutoff_per_sample else _as_dev(cutoff, self.V))
        rs = None
        if resonance is not None:
            rs = (DeviceBuffer.from_numpy(np.asarray(resonance, np.float64).reshape(N, self.V))
                  if res_per_sample and isinstance(resonance, np.ndarray)
                  else (resonance if res_per_sample else _as_dev(resonance, self.V)))
        out = self._out(N, out)
        check(lib().mxg_filter_render(k, self.V, N, _ptr(x), _ptr(cut), int(cutoff_per_sample),
                                      _ptr(rs), int(res_per_sample), _ptr(coef), self.state.ptr,
                                      _ptr(out), self.stream), "mxg_filter_render")
        self._keep = (cut, rs, coef)
        return out

    def lores(self, x, cutoff, resonance, **kw): return self.render("lores", x, cutoff, resonance, **kw)
    def hires(self, x, cutoff, resonance, **kw): return self.render("hires", x, cutoff, resonance, **kw)
    def bandpass(self, x, cutoff, resonance, **kw): return self.render("bandpass", x, cutoff, resonance, **kw)
    def lopass(self, x, cutoff, **kw): return self.render("lopass", x, cutoff, None, **kw)
    def hipass(self, x, cutoff, **kw): return self.render("hipass", x, cutoff, None, **kw)


class maxiEnvGenBank(_Bank):
    """V x maxiEnvGen (H:2268-2547) sharing one envelope shape; per-voice (or shared) trigger signals."""
    HOLD = -46692.0

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.stages = None
        self.loop = self.retrigger = False
        self._arm()

    def _arm(self):
        d = np.zeros((5, self.V))
        d[2:5] = 1.0                                   # maxiTrigger::previousValue (H:593)
        i = np.zeros((7, self.V), np.int64)
        i[4:7] = 1                                     # firstTrigger (H:594); state WAITING (resetAndArm)
        self.dstate, self.istate = DeviceBuffer.from_numpy(d), DeviceBuffer.from_numpy(i)

    def setup(self, levels, times, curves, looping, allowRetrigger=False):
        levels, times, curves = (np.ascontiguousarray(a, np.float64) for a in (levels, times, curves))
        if not (levels.size == times.size + 1 and levels.size == curves.size + 1):
            return False                               # H:2395-2398
        st = np.zeros((times.size, 6))
        rc = lib().mxg_envgen_stages_host(levels.size, levels.ctypes.data, times.ctypes.data, curves.ctypes.data,
                                          st.ctypes.data)
        if rc < 0:
            return False
        self.host_stages, self.stages = st, DeviceBuffer.from_numpy(st)
        self.loop, self.retrigger = bool(looping), bool(allowRetrigger)
        self._arm()
        return True

    def setupAR(self, attack, release): return self.setup([0, 1, 0], [attack, release], [1, 1], False, False)

    def setupASR(self, attack, release):
        return self.setup([0, 1, 1, 0], [attack, self.HOLD, release], [1, 1, 1], False, False)

    def setupADSR(self, attack, decay, sustain, release):
        return self.setup([0, 1, sustain, sustain, 0], [attack, decay, self.HOLD, release], [1, 1, 1, 1], False, False)

    def setRetrigger(self, val): self.retrigger = bool(val)
    def setLoop(self, val): self.loop = bool(val)

    def play(self, trigger, out=None):
        """trigger: [N][V] per voice, or [N] shared."""
        if not (isinstance(trigger, DeviceBuffer) or hasattr(trigger, "data_ptr")):
            trigger = DeviceBuffer.from_numpy(np.ascontiguousarray(trigger, np.float64))
        tpv = len(trigger.shape) == 2
        N = trigger.shape[0]
        out = self._out(N, out)
        check(lib().mxg_envgen_render(self.V, N, _ptr(trigger), int(tpv), self.stages.ptr, self.host_stages.shape[0],
                                      int(self.loop), int(self.retrigger), self.dstate.ptr, self.istate.ptr, _ptr(out),
                                      self.stream), "mxg_envgen_render")
        self._keep = trigger
        return out


class maxiSamplerBank(_Bank):
    """NS x maxiSampler (L/maxiSynths.h:137-187) of `voices` slots each, all playing one sample.  The control
    methods mirror the reference (they edit host copies of the slot state between renders); play(N) renders N
    calls of maxiSampler::play() for every sampler."""

    def __init__(self, samplers, voices=32, stream=None):
        super().__init__(samplers * voices, stream)
        self.NS, self.voices = int(samplers), int(voices)
        self.sample = maxiSampleBank(1, stream)
        V = self.V
        self.sustain = True
        self.currentVoice = np.zeros(self.NS, np.int64)
        self.pitch = np.zeros(V)                      # ctor, maxiSynths.cpp:262-283
        self.gain = np.zeros(V)                       # envOutGain (uninitialised in the reference: 0 here)
        self.env = maxiEnvBank(V, stream)
        self.env.setAttack(0); self.env.setDecay(1); self.env.setSustain(1.0); self.env.setRelease(2000)
        self.position = np.zeros(V)
        self.trigger_state = np.zeros(V, np.int32)
        self.outhold = np.zeros(V)
        self._state_dirty = True

    # -- control side (host), maxiSynths.cpp:303-491 ------------------------------------------------------
    def load(self, fileName):
        ok = self.sample.load(fileName)
        self.position[:] = float(self.sample.getLength()) if ok else self.position
        self._state_dirty = True
        return ok

    def setSample(self, samples):
        self.sample.setSample(samples)
        self.position[:] = self.sample.getLength() - 1.0      # maxiSample::setSample (H:677)
        self._state_dirty = True

    def _slots(self, setall):
        if setall:
            return np.arange(self.V)
        return np.arange(self.NS) * self.voices + self.currentVoice

    def _pull(self):
        if not self._state_dirty:
            self.position, self.trigger_state, self.outhold = self._dpos.numpy(), self._dtrig.numpy(), self._dout.numpy()

    def setPitch(self, pitch, setall=False):
        self.pitch[self._slots(setall)] = pitch

    def midiNoteOn(self, pitch, velocity, setall=False):
        sl = self._slots(setall)
        self.pitch[sl] = pitch
        if not setall:
            self.gain[sl] = velocity / 128

    def midiNoteOff(self, pitch, velocity=0):
        self._pull()
        self.trigger_state[self.pitch == pitch] = 0
        self._state_dirty = True

    def trigger(self):
        self._pull()
        sl = self._slots(False)
        self.trigger_state[sl] = 1
        self.position[sl] = 0.0
        self.currentVoice = (self.currentVoice + 1) % self.voices
        self._state_dirty = True

    def play(self, N, want_outputs=False):
        V = self.V
        if self._state_dirty:
            self._dpos = DeviceBuffer.from_numpy(self.position)
            self._dtrig = DeviceBuffer.from_numpy(self.trigger_state)
            self._dout = DeviceBuffer.from_numpy(self.outhold)
            self._state_dirty = False
        freq = np.zeros(V)
        check(lib().mxg_sampler_freq_host(V, self.pitch.ctypes.data, self.sample.getLength(), freq.ctypes.data),
              "mxg_sampler_freq_host")
        dfreq, dgain = DeviceBuffer.from_numpy(freq), DeviceBuffer.from_numpy(self.gain)
        dpar, dhold = self.env._params()
        mix = DeviceBuffer((N, self.NS), zero=False)
        self.outputs = DeviceBuffer((N, V), zero=False) if want_outputs else None
        check(lib().mxg_sampler_render(V, N, self.voices, int(self.sustain), self.sample.d_samples, self.sample.getLength(),
                                       dfreq.ptr, dgain.ptr, dpar.ptr, dhold.ptr, self._dpos.ptr, self._dtrig.ptr,
                                       self._dout.ptr, self.env.dstate.ptr, self.env.istate.ptr, mix.ptr,
                                       _ptr(self.outputs), self.stream), "mxg_sampler_render")
        self._keep = (dfreq, dgain)
        return mix


class _Filter2Bank(_Bank):
    KIND = 0

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.state = DeviceBuffer((3, self.V))
        self.coef = None

    def _play(self, x, out):
        N = x.shape[0]
        out = self._out(N, out)
        check(lib().mxg_filter2_render(self.KIND, self.V, N, _ptr(x), self.coef.ptr, self.state.ptr, _ptr(out),
                                       self.stream), "mxg_filter2_render")
        return out


class maxiDCBlockerBank(_Filter2Bank):
    """V x maxiDCBlocker (H:1255-1267)."""
    KIND = 0

    def play(self, x, R, out=None):
        self.coef = _as_dev(R, self.V)
        return self._play(x, out)


class maxiSVFBank(_Filter2Bank):
    """V x maxiSVF (H:1281-1338); the ctor's setParams(1000, 1) (H:1284)."""
    KIND = 1

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.freq = np.full(self.V, 1000.0)
        self.res = np.full(self.V, 1.0)
        self._host = None

    def setCutoff(self, cutoff):
        self.freq = np.ascontiguousarray(np.broadcast_to(np.asarray(cutoff, np.float64), (self.V,)))
        self._host = None

    def setResonance(self, q):
        self.res = np.ascontiguousarray(np.broadcast_to(np.asarray(q, np.float64), (self.V,)))
        self._host = None

    def coefficients(self):
        if self._host is None:
            c = np.zeros((5, self.V))
            check(lib().mxg_svf_coeffs_host(self.V, self.freq.ctypes.data, self.res.ctypes.data, c.ctypes.data),
                  "mxg_svf_coeffs_host")
            self._host = c
        return self._host

    def play(self, w, lpmix, bpmix, hpmix, notchmix, out=None):
        mix = np.stack([np.broadcast_to(np.asarray(m, np.float64), (self.V,)) for m in (lpmix, bpmix, hpmix, notchmix)])
        self.coef = DeviceBuffer.from_numpy(np.concatenate([self.coefficients(), mix]))
        return self._play(w, out)


class maxiBiquadBank(_Filter2Bank):
    """V x maxiBiquad (H:1343-1486)."""
    KIND = 2
    LOWPASS, HIGHPASS, BANDPASS, NOTCH, PEAK, LOWSHELF, HIGHSHELF = range(7)

    def set(self, filtType, cutoff, Q, peakGain):
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(filtType, np.int32), (self.V,)))
        cu, q, g = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (self.V,))) for a in (cutoff, Q, peakGain))
        c = np.zeros((5, self.V))
        check(lib().mxg_biquad_coeffs_host(self.V, t.ctypes.data, cu.ctypes.data, q.ctypes.data, g.ctypes.data,
                                           c.ctypes.data), "mxg_biquad_coeffs_host")
        self.host_coef = c
        self.coef = DeviceBuffer.from_numpy(c)

    def play(self, x, out=None):
        return self._play(x, out)


class maxiEnvBank(_Bank):
    """V x maxiEnv (H:888-932).  No constructor in the reference: all state starts at zero
    (static-storage objects), holdtime defaults to 1 (H:915)."""

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.par = np.zeros((4, self.V))  # attack, decay, sustain, release
        self.holdtime = np.ones(self.V, np.int64)
        self.dstate = DeviceBuffer((2, self.V))            # amplitude, output
        self.istate = DeviceBuffer((6, self.V), np.int64)  # holdcount + 5 phase flags
        self._dirty = True

    def _coeff(self, which, ms):
        ms = np.broadcast_to(np.asarray(ms, np.float64), (self.V,))
        f = lib().mxg_env_coeff_host
        cache = {}
        return np.array([cache.setdefault(m, f(which, m)) for m in ms.tolist()])

    def setAttack(self, ms): self.par[0] = self._coeff(0, ms); self._dirty = True      # C:1480-1482
    def setAttackMS(self, ms): self.par[0] = self._coeff(3, ms); self._dirty = True    # C:1486-1488
    def setDecay(self, ms): self.par[1] = self._coeff(1, ms); self._dirty = True       # C:1475-1477
    def setSustain(self, level): self.par[2] = np.asarray(level, np.float64); self._dirty = True
    def setRelease(self, ms): self.par[3] = self._coeff(2, ms); self._dirty = True     # C:1470-1472

    def _params(self):
        if self._dirty:
            self._dpar = DeviceBuffer.from_numpy(self.par)
            self._dhold = DeviceBuffer.from_numpy(self.holdtime)
            self._dirty = False
        return self._dpar, self._dhold

    def render(self, mode, x, trigger, N, out=None):
        dpar, dhold = self._params()
        trig = trigger
        tpv = 0
        if not (isinstance(trigger, DeviceBuffer) or hasattr(trigger, "data_ptr")):
            t = np.ascontiguousarray(trigger, np.int32)
            tpv = 1 if t.ndim == 2 else 0
            trig = DeviceBuffer.from_numpy(t)
        else:
            tpv = 1 if len(trigger.shape) == 2 else 0
        out = self._out(N, out)
        check(lib().mxg_env_render(mode, self.V, N, _ptr(x), _ptr(trig), tpv, dpar.ptr, dhold.ptr,
                                   self.dstate.ptr, self.istate.ptr, _ptr(out), self.stream),
              "mxg_env_render")
        self._keep = trig
        return out

    def adsr(self, x, trigger, N, **kw): return self.render(0, x, trigger, N, **kw)
    def ar(self, x, trigger, N, **kw): return self.render(1, x, trigger, N, **kw)


class maxiVoiceBank(_Bank):
    """V fused subtractive voices: maxiOsc::saw -> maxiFilter::lores -> maxiEnv::adsr
    (config 3; the per-voice body of 14.monosynth / 15.polysynth), one kernel, one store/sample."""

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.env = maxiEnvBank(voices, stream)
        self.osc_state = DeviceBuffer((2, self.V))
        self.flt_state = DeviceBuffer((5, self.V))

    def render(self, mode, freq, cutoff, resonance, trigger, N, out=None):
        f = _as_dev(freq, self.V)
        cu = np.broadcast_to(np.asarray(cutoff, np.float64), (self.V,))
        rs = np.broadcast_to(np.asarray(resonance, np.float64), (self.V,))
        coef = None
        if mode == 0:
            coef = DeviceBuffer.from_numpy(filter_coeffs(0, cu, rs))
        dcu, drs = DeviceBuffer.from_numpy(cu), DeviceBuffer.from_numpy(rs)
        dpar, dhold = self.env._params()
        trig = trigger
        if not (isinstance(trigger, DeviceBuffer) or hasattr(trigger, "data_ptr")):
            trig = DeviceBuffer.from_numpy(np.ascontiguousarray(trigger, np.int32))
        tpv = 1 if len(trig.shape) == 2 else 0
        out = self._out(N, out)
        check(lib().mxg_voice_render(mode, self.V, N, _ptr(f), dcu.ptr, drs.ptr, _ptr(coef), _ptr(trig),
                                     tpv, dpar.ptr, dhold.ptr, self.osc_state.ptr, self.flt_state.ptr,
                                     self.env.dstate.ptr, self.env.istate.ptr, _ptr(out), self.stream),
              "mxg_voice_render")
        self._keep = (f, dcu, drs, coef, trig)
        return out

    def render_mix(self, mode, freq, cutoff, resonance, trigger, pan, N, out=None, store=True, mix=None, rows=None):
        """render() + the fused maxiMix::stereo mixdown of the bank in the same kernel (mxg_voice_render_mix).
        Returns (out [N,V] or None, mix [N,2]).  rows: a device pointer / buffer [mxg_osc_mix_groups(V)][N][2] (e.g. a grouped
        mix queue's slot) -- then the per-workgroup rows are left there (mxg_voice_render_mix_rows); returns (out, None)."""
        f, pn = _as_dev(freq, self.V), _as_dev(pan, self.V)
        cu = np.broadcast_to(np.asarray(cutoff, np.float64), (self.V,))
        rs = np.broadcast_to(np.asarray(resonance, np.float64), (self.V,))
        coef = DeviceBuffer.from_numpy(filter_coeffs(0, cu, rs)) if mode == 0 else None
        dcu, drs = DeviceBuffer.from_numpy(cu), DeviceBuffer.from_numpy(rs)
        dpar, dhold = self.env._params()
        trig = trigger
        if not (isinstance(trigger, DeviceBuffer) or hasattr(trigger, "data_ptr")):
            trig = DeviceBuffer.from_numpy(np.ascontiguousarray(trigger, np.int32))
        tpv = 1 if len(trig.shape) == 2 else 0
        out = self._out(N, out) if store else None
        args = (mode, self.V, N, _ptr(f), dcu.ptr, drs.ptr, _ptr(coef), _ptr(trig), tpv, dpar.ptr, dhold.ptr, self.osc_state.ptr,
                self.flt_state.ptr, self.env.dstate.ptr, self.env.istate.ptr, _ptr(out), _ptr(pn))
        self._keep = (f, dcu, drs, coef, trig, pn)
        if rows is not None:
            check(lib().mxg_voice_render_mix_rows(*args, _ptr(rows), self.stream), "mxg_voice_render_mix_rows")
            return out, None
        mix = mix if mix is not None else DeviceBuffer((N, 2), np.float64, zero=False)
        check(lib().mxg_voice_render_mix(*args, _ptr(mix), self.stream), "mxg_voice_render_mix")
        return out, mix


class maxiMixBank(_Bank):
    """maxiMix::stereo over a bank + the mixdown over voices (C:503-509)."""

    def stereo(self, x, pan, out=None):
        N = x.shape[0]
        p = _as_dev(pan, self.V)
        out = out if out is not None else DeviceBuffer((N, 2), np.float64, zero=False)
        check(lib().mxg_mix_stereo(self.V, N, _ptr(x), _ptr(p), _ptr(out), self.stream),
              "mxg_mix_stereo")
        self._keep = p
        return out

    def bus(self, channels, x, px, py=None, pz=None, out=None, bus=None):
        """stereo (2) / quad (4, C:512-522) / ambisonic (8, C:525-541): mix [N][channels]; `bus`, if a
        DeviceBuffer [N][channels][V], also receives the per-voice two/four/eight signals."""
        N = x.shape[0]
        dx = _as_dev(px, self.V)
        dy = None if py is None else _as_dev(py, self.V)
        dz = None if pz is None else _as_dev(pz, self.V)
        out = out if out is not None else DeviceBuffer((N, channels), np.float64, zero=False)
        check(lib().mxg_mix_bus(channels, self.V, N, _ptr(x), _ptr(dx), _ptr(dy), _ptr(dz), _ptr(bus),
                                _ptr(out), self.stream), "mxg_mix_bus")
        self._keep = (dx, dy, dz)
        return out

    def quad(self, x, px, py, **kw): return self.bus(4, x, px, py, **kw)
    def ambisonic(self, x, px, py, pz, **kw): return self.bus(8, x, px, py, pz, **kw)


class maxiDelaylineBank(_Bank):
    """V x maxiDelayline (H:266-284).  The ring is `cap` slots per voice (slot-major on device)
    instead of the reference's fixed 88200*8; `size` <= cap."""

    def __init__(self, voices, cap, stream=None):
        super().__init__(voices, stream)
        self.cap = int(cap)
        self.memory = DeviceBuffer((self.cap, self.V))    # ctor memset 0, C:415-417
        self.phase = DeviceBuffer(self.V, np.int32)       # static-storage objects start at 0

    def _render(self, mode, x, size, feedback, position, out):
        N = x.shape[0]
        sz = _as_dev(size, self.V, np.int32)
        fb = _as_dev(feedback, self.V)
        ps = None if position is None else _as_dev(position, self.V, np.int32)
        out = self._out(N, out)
        check(lib().mxg_delay_render(mode, self.V, N, _ptr(x), _ptr(sz), _ptr(fb), _ptr(ps),
                                     self.memory.ptr, self.cap, self.phase.ptr, _ptr(out), self.stream),
              "mxg_delay_render")
        self._keep = (sz, fb, ps)
        return out

    def dl(self, x, size, feedback, out=None):
        return self._render(0, x, size, feedback, None, out)

    def dlFromPosition(self, x, size, feedback, position, out=None):
        return self._render(1, x, size, feedback, position, out)


FX_PS = {"delay": 1, "feedback": 2, "speed": 4, "depth": 8}  # MXG_FX_PS_* (include/maxigpu.h)


def _fx_dev(x, dtype, what, counts):
    """A device input of an effect bank: its element type must be `dtype`, a torch tensor must be contiguous, and its
    element count one of `counts` -- the kernels read raw memory."""
    want = np.dtype(dtype)
    if isinstance(x, DeviceBuffer):
        ok, n = x.dtype == want, int(np.prod(x.shape))
    else:
        ok = str(x.dtype).replace("torch.", "") == want.name and x.is_contiguous()
        n = int(x.numel())
    if not ok:
        raise TypeError("%s: needs a contiguous %s device array, got %s" % (what, want.name, x.dtype))
    if n not in counts:
        raise ValueError("%s: %d elements, expected one of %s" % (what, n, sorted(set(counts))))
    return n


def _fx_param(x, V, N, dtype, what="parameter"):
    """An effect parameter: scalar / [V] -> ([V] buffer, 0); [N][V] -> ([N][V] buffer, 1); device objects are
    [V] unless their element count is N*V."""
    if isinstance(x, DeviceBuffer) or hasattr(x, "data_ptr"):
        n = _fx_dev(x, dtype, what, (V, N * V))
        return x, int(n == N * V and N > 1)
    a = np.asarray(x, dtype=dtype)
    if a.ndim == 2:
        return DeviceBuffer.from_numpy(a.reshape(N, V)), 1
    return _as_dev(a, V, dtype), 0


def _fx_input(x, V, N):
    _fx_dev(x, np.float64, "input", (N * V,))


class _FxBank(_Bank):
    RINGS = 1

    def __init__(self, voices, cap, stream=None):
        super().__init__(voices, stream)
        self.cap = int(cap)
        self.memory = DeviceBuffer((self.RINGS, self.V, self.cap))  # voice-major rings, ctor memset 0 (C:415-417)
        self.phase = DeviceBuffer((self.RINGS, self.V), np.int32)   # maxiDelayline::phase of value-initialised objects
        self.overflow = DeviceBuffer(self.V, np.uint32)              # taps held to `cap` so far (not in the reference)

    def _params(self, N, delay, feedback, depth):
        d, pd = _fx_param(delay, self.V, N, np.uint32, "delay")
        f, pf = _fx_param(feedback, self.V, N, np.float64, "feedback")
        p, pp = _fx_param(depth, self.V, N, np.float64, "depth")
        return (d, f, p), pd * FX_PS["delay"] | pf * FX_PS["feedback"] | pp * FX_PS["depth"]


class maxiFlangerBank(_FxBank):
    """V x maxiFlanger (H:1144-1172).  `flange(x, delay, feedback, speed, depth)` -> [N, V]; each parameter is a
    scalar, [V] (held for the block) or [N, V] (per sample).  State: memory [1][V][cap], phase [1][V] (the delay
    line), lfo_phase [V] (the triangle LFO), overflow [V]."""

    def __init__(self, voices, cap, stream=None):
        super().__init__(voices, cap, stream)
        self.lfo_phase = DeviceBuffer(self.V)  # maxiOsc::phase (ctor 0, C:209-212)

    def flange(self, x, delay, feedback, speed, depth, out=None):
        N = x.shape[0]
        (d, f, p), ps = self._params(N, delay, feedback, depth)
        _fx_input(x, self.V, N)
        s, pspd = _fx_param(speed, self.V, N, np.float64, "speed")
        ps |= pspd * FX_PS["speed"]
        out = self._out(N, out)
        check(lib().mxg_flanger_render(self.V, N, _ptr(x), _ptr(d), _ptr(f), _ptr(s), _ptr(p), ps,
                                       self.memory.ptr, self.cap, self.phase.ptr, self.lfo_phase.ptr,
                                       self.overflow.ptr, _ptr(out), self.stream), "mxg_flanger_render")
        self._keep = (d, f, s, p)
        return out


def chorus_coeffs(speed):
    """(c, r) of maxiChorus's lopass.lores(noise, speed, 1.0) (C:455-468) on the host libm: [2][V] for a [V]
    speed, [N][2][V] for an [N][V] one."""
    sp = np.asarray(speed, np.float64)
    flat = np.ascontiguousarray(sp.reshape(-1))
    c = filter_coeffs(0, flat, np.ones_like(flat))[:2]
    if sp.ndim == 2:
        return np.ascontiguousarray(c.reshape(2, sp.shape[0], sp.shape[1]).transpose(1, 0, 2))
    return np.ascontiguousarray(c)


class maxiChorusBank(_FxBank):
    """V x maxiChorus (H:1179-1212).  `chorus(x, delay, feedback, speed, depth, rand)` -> [N, V]; `rand` is the
    int32 [N, V] rand() draw each voice's lfo.noise() takes (C:214-220).  `speed` is a scalar / [V] / [N, V]
    (the lores cutoff; its coefficients are computed on the host), or pass `coef` ([2][V] / [N][2][V])
    directly.  State: memory [2][V][cap], phase [2][V], lp [2][V] (lores x, y), overflow [V]."""
    RINGS = 2

    def __init__(self, voices, cap, stream=None):
        super().__init__(voices, cap, stream)
        self.lp = DeviceBuffer((2, self.V))  # maxiFilter::x, y (ctor 0)

    def chorus(self, x, delay, feedback, speed, depth, rand, coef=None, out=None):
        N = x.shape[0]
        (d, f, p), ps = self._params(N, delay, feedback, depth)
        if coef is None:
            sp = np.asarray(speed, np.float64)
            coef = chorus_coeffs(sp if sp.ndim == 2 else np.broadcast_to(sp, (self.V,)))
        coef_ps = int(np.prod(coef.shape)) == 2 * N * self.V and N > 1
        _fx_input(x, self.V, N)
        if isinstance(coef, np.ndarray):
            cf = DeviceBuffer.from_numpy(np.ascontiguousarray(coef, np.float64))
        else:
            cf = coef
        _fx_dev(cf, np.float64, "coef", (2 * self.V, 2 * N * self.V))
        if isinstance(rand, np.ndarray):
            rd = DeviceBuffer.from_numpy(np.ascontiguousarray(rand, np.int32).reshape(N, self.V))
        else:
            rd = rand
        _fx_dev(rd, np.int32, "rand", (N * self.V,))
        out = self._out(N, out)
        check(lib().mxg_chorus_render(self.V, N, _ptr(x), _ptr(d), _ptr(f), _ptr(p), ps, _ptr(rd), _ptr(cf),
                                      int(coef_ps), self.memory.ptr, self.cap, self.phase.ptr, self.lp.ptr,
                                      self.overflow.ptr, _ptr(out), self.stream), "mxg_chorus_render")
        self._keep = (d, f, p, cf, rd)
        return out


REVERB_KINDS = {"sat": 0, "freeverb": 1, "freeverb_stereo": 2}  # MXG_REVERB_* (include/maxigpu.h)
REVERB_PS = {"roomsize": 1, "absorbtion": 2}                    # MXG_REVERB_PS_*


def reverb_layout(kind):
    """(combs, allpasses, ring doubles per voice, lengths, offsets) of a reverb kind (mxg_reverb_layout_host)."""
    nc, na, S = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    lens, offs = np.zeros(39, np.uint32), np.zeros(39, np.uint32)
    check(lib().mxg_reverb_layout_host(int(kind), ctypes.addressof(nc), ctypes.addressof(na), ctypes.addressof(S),
                                       lens.ctypes.data, offs.ctypes.data), "mxg_reverb_layout_host")
    F = nc.value + na.value
    return nc.value, na.value, S.value, lens[:F].astype(int).tolist(), offs[:F].astype(int).tolist()


class _ReverbBank(_Bank):
    """State of V reverbs (libs/maxiReverb.h): rings [V][ring doubles] (voice-major), idx int32 [V][filters]; the
    constructors' zeros.  Ring state per voice: 3 992 / 18 905 / 12 587 doubles."""
    KIND = 0

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.ncombs, self.nallpasses, self.ring_doubles, self.lengths, self.offsets = reverb_layout(self.KIND)
        self.rings = DeviceBuffer((self.V, self.ring_doubles))
        self.idx = DeviceBuffer((self.V, self.ncombs + self.nallpasses), np.int32)
        self.lp = self.wc = None

    def _render(self, mode, x, room, absorb, ps, channels, out):
        N = x.shape[0]
        _fx_input(x, self.V, N)
        if out is None:
            out = DeviceBuffer((N, self.V) if channels == 1 else (channels, N, self.V), np.float64, zero=False)
        check(lib().mxg_reverb_render(self.KIND, mode, self.V, N, _ptr(x), _ptr(room), _ptr(absorb), ps, self.rings.ptr,
                                      self.idx.ptr, _ptr(self.lp), _ptr(self.wc), _ptr(out), self.stream), "mxg_reverb_render")
        self._keep = (room, absorb)
        return out


class maxiSatReverbBank(_ReverbBank):
    """V x maxiSatReverb: 4 plain combs into 3 allpasses.  `play(x)` -> [N, V] (playStereo is (b, -b))."""
    KIND = REVERB_KINDS["sat"]

    def play(self, x, out=None):
        return self._render(0, x, None, None, 0, 1, out)


class maxiFreeVerbBank(_ReverbBank):
    """V x maxiFreeVerb: 8 low-pass combs into 4 (`play(x)`) or 31 (`play(x, roomsize, absorbtion)`) allpasses, both on
    the same rings.  The parameters are scalars, [V] or [N, V]; they set the comb weight and cutoff for good.  State
    besides the rings: lp [V][8] (the combs' low-pass states), wc [V][2] = (w, cut), 0.84 and 0.2 in a fresh object."""
    KIND = REVERB_KINDS["freeverb"]

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.lp = DeviceBuffer((self.V, 8))
        self.wc = DeviceBuffer.from_numpy(np.tile(np.array([0.84, 0.2]), (self.V, 1)))

    def play(self, x, roomsize=None, absorbtion=None, out=None):
        if roomsize is None and absorbtion is None:
            return self._render(0, x, None, None, 0, 1, out)
        if roomsize is None or absorbtion is None:
            raise TypeError("play(x, roomsize, absorbtion) takes both parameters")
        N = x.shape[0]
        r, pr = _fx_param(roomsize, self.V, N, np.float64, "roomsize")
        a, pa = _fx_param(absorbtion, self.V, N, np.float64, "absorbtion")
        return self._render(1, x, r, a, pr * REVERB_PS["roomsize"] | pa * REVERB_PS["absorbtion"], 1, out)


class maxiFreeVerbStereoBank(_ReverbBank):
    """V x maxiFreeVerbStereo.  `playStereo(x)` -> [2, N, V]: left = 8 plain combs into 4 allpasses, right = the same four
    allpass rings stepped a second time with 0.0 (what the reference computes; its roomsize / absorbtion are read by nothing
    and are accepted here only to be ignored)."""
    KIND = REVERB_KINDS["freeverb_stereo"]

    def playStereo(self, x, roomsize=None, absorbtion=None, out=None):
        return self._render(0, x, None, None, 0, 2, out)


def dattaro_layout(sample_rate=44100):
    """(lengths [10], offsets [10], ring doubles per voice, tap positions [14], tap rings [14]) of a maxiDattaroReverb
    constructed at `sample_rate` (mxg_dattaro_layout_host; needs no device).  Raises for a rate outside the accepted range."""
    S = ctypes.c_uint32()
    lens, offs = np.zeros(10, np.uint32), np.zeros(10, np.uint32)
    taps, rings = np.zeros(14, np.uint32), np.zeros(14, np.uint32)
    check(lib().mxg_dattaro_layout_host(int(sample_rate), lens.ctypes.data, offs.ctypes.data, ctypes.addressof(S),
                                        taps.ctypes.data, rings.ctypes.data), "mxg_dattaro_layout_host")
    return (lens.astype(int).tolist(), offs.astype(int).tolist(), S.value, taps.astype(int).tolist(),
            rings.astype(int).tolist())


class maxiDattaroReverbBank(_Bank):
    """V x maxiDattaroReverb (libs/maxiReverb.h, K14), every delay length fixed from `sample_rate` at construction as the
    reference's constructor does.  `playStereo(x)` -> [2, N, V] (left, right).  State: rings [V][ring_doubles]
    (voice-major, ring r at offsets[r]), idx int32 [V][10], state [V][5] = lp0 lp1 lp2 sigl sigr; all zero when fresh.
    The reference's unobservable pre-delay ring is not carried."""

    def __init__(self, voices, sample_rate=44100, stream=None):
        super().__init__(voices, stream)
        self.sample_rate = int(sample_rate)
        self.lengths, self.offsets, self.ring_doubles, self.tap_positions, self.tap_rings = dattaro_layout(self.sample_rate)
        self.rings = DeviceBuffer((self.V, self.ring_doubles))
        self.idx = DeviceBuffer((self.V, 10), np.int32)
        self.state = DeviceBuffer((self.V, 5))

    def playStereo(self, x, out=None):
        N = x.shape[0]
        _fx_input(x, self.V, N)
        if out is None:
            out = DeviceBuffer((2, N, self.V), np.float64, zero=False)
        check(lib().mxg_dattaro_render(self.sample_rate, self.V, N, _ptr(x), self.rings.ptr, self.idx.ptr, self.state.ptr,
                                       _ptr(out), self.stream), "mxg_dattaro_render")
        return out


def _revnet_sizes(sizes, what):
    a = np.asarray(list(sizes), dtype=np.float64).reshape(-1)
    if a.size and (not np.all(np.isfinite(a)) or np.any(a != np.floor(a)) or np.any(a < 0) or np.any(a > 0xffffffff)):
        raise ValueError("%s: the delay lengths are whole numbers of samples" % what)
    return np.ascontiguousarray(a, dtype=np.uint32)


def revnet_layout(comb_sizes, ap_sizes, comb_lowpass=None):
    """(offsets [combs + allpasses], ring doubles per voice) of a reverb network (mxg_revnet_layout_host; needs no device).
    Raises for a topology the kernel does not take: a count beyond 32, no stage at all, a length outside [1, 44100], a
    low-pass comb shorter than 64."""
    cs, aps = _revnet_sizes(comb_sizes, "comb_sizes"), _revnet_sizes(ap_sizes, "ap_sizes")
    lowp = None
    if comb_lowpass is not None:
        lowp = np.ascontiguousarray(np.asarray(list(comb_lowpass)).reshape(-1) != 0, dtype=np.uint32)
        if lowp.size != cs.size:
            raise ValueError("comb_lowpass: one flag per comb")
    S = ctypes.c_uint32()
    offs = np.zeros(max(cs.size + aps.size, 1), np.uint32)
    check(lib().mxg_revnet_layout_host(cs.size, aps.size, cs.ctypes.data, aps.ctypes.data, None if lowp is None else lowp.ctypes.data,
                                       offs.ctypes.data if cs.size + aps.size <= 64 else None, ctypes.addressof(S)),
          "mxg_revnet_layout_host")
    return offs[:cs.size + aps.size].astype(int).tolist(), S.value


class maxiReverbNetBank(_Bank):
    """V custom reverbs out of maxiReverbFilters stages (libs/maxiReverb.h, K30), one topology per bank: the parallel combs
    `comb_sizes` summed in order -- combfb, or lpcombfb where `comb_lowpass` flags it -- into the serial allpasses `ap_sizes`.
    Lengths are whole samples in [1, 44100], at most 32 of each kind, a low-pass comb at least 64.  `play(x)` -> [N, V].
    Feedbacks and cutoffs are per voice and stage (a scalar, [stages] or [V][stages]), constant within a call, and nothing
    clamps them.  State: rings [V][ring_doubles] (voice-major, stage f at offsets[f], combs first), idx int32
    [V][combs + allpasses], lp [V][combs] (the low-pass combs' filter states); all zero when fresh."""

    def __init__(self, voices, comb_sizes, ap_sizes, comb_lowpass=None, comb_fb=0.85, comb_cut=0.2, ap_fb=0.85, stream=None):
        super().__init__(voices, stream)
        self._cs, self._as = _revnet_sizes(comb_sizes, "comb_sizes"), _revnet_sizes(ap_sizes, "ap_sizes")
        self.ncombs, self.nallpasses = int(self._cs.size), int(self._as.size)
        self.comb_lowpass = [False] * self.ncombs if comb_lowpass is None else [bool(f) for f in comb_lowpass]
        self.offsets, self.ring_doubles = revnet_layout(self._cs, self._as, self.comb_lowpass)
        self._lowp = np.asarray(self.comb_lowpass, dtype=np.uint32)
        self.lengths = self._cs.astype(int).tolist() + self._as.astype(int).tolist()
        self.rings = DeviceBuffer((self.V, self.ring_doubles))
        self.idx = DeviceBuffer((self.V, self.ncombs + self.nallpasses), np.int32)
        self.lp = DeviceBuffer((self.V, self.ncombs))
        self.comb_fb = DeviceBuffer((self.V, self.ncombs))
        self.comb_cut = DeviceBuffer((self.V, self.ncombs))
        self.ap_fb = DeviceBuffer((self.V, self.nallpasses))
        self.set_comb_fb(comb_fb)
        self.set_comb_cut(comb_cut)
        self.set_ap_fb(ap_fb)

    def _set(self, buf, value, stages, what):
        a = np.asarray(value, dtype=np.float64)
        if a.ndim > 2 or (a.ndim == 1 and a.shape != (stages,)) or (a.ndim == 2 and a.shape != (self.V, stages)):
            raise ValueError("%s: a scalar, [%d] or [%d][%d], got %s" % (what, stages, self.V, stages, a.shape))
        self.sync()  # a call still running reads the old values
        buf.upload(np.broadcast_to(a, (self.V, stages)))

    def set_comb_fb(self, fb):
        self._set(self.comb_fb, fb, self.ncombs, "comb_fb")

    def set_comb_cut(self, cutoff):
        self._set(self.comb_cut, cutoff, self.ncombs, "comb_cut")

    def set_ap_fb(self, fb):
        self._set(self.ap_fb, fb, self.nallpasses, "ap_fb")

    def clear(self):
        """Back to fresh objects: rings, indices and low-pass states zero; the parameters stay."""
        self.sync()
        for b in (self.rings, self.idx, self.lp):
            if b.nbytes:
                check(lib().mxg_memset(b.ptr, 0, b.nbytes, None), "mxg_memset")
        check(lib().mxg_stream_sync(None), "mxg_stream_sync")

    def play(self, x, out=None):
        N = x.shape[0]
        _fx_input(x, self.V, N)
        out = self._out(N, out)
        check(lib().mxg_revnet_render(self.ncombs, self.nallpasses, self._cs.ctypes.data, self._as.ctypes.data, self._lowp.ctypes.data,
                                      self.V, N, _ptr(x), self.comb_fb.ptr, self.comb_cut.ptr, self.ap_fb.ptr, self.rings.ptr,
                                      self.idx.ptr, self.lp.ptr, _ptr(out), self.stream), "mxg_revnet_render")
        return out


DYN_PS = {"thresholdHigh": 1, "ratioHigh": 2, "kneeHigh": 4, "thresholdLow": 8, "ratioLow": 16, "kneeLow": 32}  # MXG_DYN_PS_*


def ms_to_samps(ms):
    """maxiConvert::msToSamps (H:944-947): truncation to size_t."""
    return int(float(ms) / 1000.0 * maxiSettings.sampleRate)


class _DynControl:
    """The host side of maxiDynamics (H:2625-2897): what its constructor and setters leave behind, as the arrays
    mxg_dynamics_render reads.  Per voice: window / lookahead (samples) and analyser; per bank: the two setupASR(10, 10)
    stage tables.  No device work here (tests/dyn_host.py drives the host build of the kernel's arithmetic with it)."""
    PEAK, RMS = 0, 1

    def _init_control(self, V, cap_rms, cap_lookahead):
        self.V = int(V)
        # both rings are sized from the sample rate in force at construction (H:2637, H:2651)
        self.cap_rms = int(cap_rms) if cap_rms is not None else ms_to_samps(500)
        self.cap_lookahead = int(cap_lookahead) if cap_lookahead is not None else int(maxiSettings.sampleRate)
        self.window = np.zeros(self.V, np.uint32)       # maxiRMS::windowSize = 0 until setup()
        self.lookahead = np.zeros(self.V, np.uint32)    # lookAheadSize = 0
        self.analyser = np.full(self.V, self.RMS, np.int32)
        self._zero_running = np.zeros(self.V, bool)
        self._set_window(50.0)                          # rms.setup(500, 50)
        self._zero_running[:] = False
        self.stages_high, self.stages_low = self._asr(), self._asr()
        self._dirty = True

    @staticmethod
    def _asr():
        levels, times, curves = np.array([0.0, 1, 1, 0]), np.array([10.0, -46692.0, 10.0]), np.ones(3)
        st = np.zeros((3, 6))
        check(lib().mxg_envgen_stages_host(4, levels.ctypes.data, times.ctypes.data, curves.ctypes.data, st.ctypes.data),
              "mxg_envgen_stages_host")
        return st

    def _select(self, x, voices, dtype=np.float64):
        """(indices, values) of a setter call made on `voices` (None = every voice) with a scalar or one value per voice."""
        idx = np.arange(self.V)[slice(None) if voices is None else voices].reshape(-1)
        a = np.asarray(x, dtype)
        if a.ndim and a.shape != idx.shape:
            raise ValueError("expected a scalar or %d values, got shape %s" % (idx.size, a.shape))
        return idx, np.broadcast_to(a, idx.shape)

    def _set_time(self, table, index, ms):
        check(lib().mxg_envgen_set_time_host(table.ctypes.data, table.shape[0], index, float(ms)), "mxg_envgen_set_time_host")
        self._dirty = True

    def invalidate(self):
        """Call after editing window / lookahead / analyser / stages_high / stages_low in place (all host arrays, in samples)."""
        self._dirty = True

    def setAttackHigh(self, attack): self._set_time(self.stages_high, 0, attack)    # H:2815-2817
    def setReleaseHigh(self, release): self._set_time(self.stages_high, 2, release)  # H:2822-2824
    def setAttackLow(self, attack): self._set_time(self.stages_low, 0, attack)      # H:2829-2831
    def setReleaseLow(self, release): self._set_time(self.stages_low, 2, release)    # H:2836-2838

    def setLookAhead(self, length, voices=None):
        """H:2844-2847: msToSamps, held at the ring's size.  Scalar or one value per voice of `voices` (None = all)."""
        idx, ms = self._select(length, voices)
        for v, m in zip(idx.tolist(), ms.tolist()):
            self.lookahead[v] = min(ms_to_samps(m), self.cap_lookahead)
        self._dirty = True

    def getLookAhead(self):
        """H:2851-2853: sampsToMs divides two integers (H:949-952)."""
        return (self.lookahead.astype(np.int64) // int(maxiSettings.sampleRate)) * 1000.0

    def _set_window(self, ms, voices=None):
        idx, ms = self._select(ms, voices)
        for v, m in zip(idx.tolist(), ms.tolist()):
            s = ms_to_samps(m)
            if s <= self.cap_rms:         # maxiRMS::setWindowSize H:2590-2596: a request above the ring is ignored ...
                self.window[v] = s
            self._zero_running[v] = True  # ... but the running sum is zeroed either way (the ring is not)
        self._dirty = True

    def setRMSWindowSize(self, winSize, voices=None):
        """H:2859-2861: min(winSize, 500) ms."""
        self._set_window(np.minimum(np.asarray(winSize, np.float64), 500.0), voices)

    def setInputAnalyser(self, mode, voices=None):
        idx, m = self._select(mode, voices, np.int64)
        self.analyser[idx] = np.where(m == self.PEAK, self.PEAK, self.RMS)
        self._dirty = True


class maxiDynamicsBank(_Bank, _DynControl):
    """V x maxiDynamics (H:2625-2897).  `play(sig, control, thresholdHigh, ratioHigh, kneeHigh, thresholdLow, ratioLow,
    kneeLow)` -> [N, V]; each parameter is a scalar, [V] or [N, V].  The setters take scalars or [V] arrays (the four
    attack / release times are one value per bank: the envelopes share one shape).  State, all device buffers that can
    be read and uploaded between blocks: rms_ring [cap_rms][V], la_ring [cap_lookahead][V], rms_pos / la_pos [V],
    running [V], env_high / env_low = (dstate [5][V], istate [7][V]) as maxiEnvGenBank keeps them, overflow [V]."""

    def __init__(self, voices, cap_rms=None, cap_lookahead=None, stream=None):
        _Bank.__init__(self, voices, stream)
        self._init_control(self.V, cap_rms, cap_lookahead)
        self.rms_ring = DeviceBuffer((self.cap_rms, self.V))
        self.la_ring = DeviceBuffer((self.cap_lookahead, self.V))
        self.rms_pos = DeviceBuffer(self.V, np.int32)
        self.la_pos = DeviceBuffer(self.V, np.int32)
        self.running = DeviceBuffer(self.V)
        self.overflow = DeviceBuffer(self.V, np.uint32)
        d = np.zeros((5, self.V))
        d[2:5] = 1.0
        i = np.zeros((7, self.V), np.int64)
        i[4:7] = 1
        self.env_high = (DeviceBuffer.from_numpy(d), DeviceBuffer.from_numpy(i))
        self.env_low = (DeviceBuffer.from_numpy(d), DeviceBuffer.from_numpy(i))
        self.level_db = None

    def _upload_control(self):
        if self._zero_running.any():  # setWindowSize zeroes runningRMS of the voices it was called on
            r = self.running.numpy()
            r[self._zero_running] = 0.0
            self.running.upload(r)
            self._zero_running[:] = False
        if self._dirty:
            self._dwin, self._dla = DeviceBuffer.from_numpy(self.window), DeviceBuffer.from_numpy(self.lookahead)
            self._dan = DeviceBuffer.from_numpy(self.analyser)
            self._dsh, self._dsl = DeviceBuffer.from_numpy(self.stages_high), DeviceBuffer.from_numpy(self.stages_low)
            self._dirty = False

    def play(self, sig, control, thresholdHigh, ratioHigh, kneeHigh, thresholdLow, ratioLow, kneeLow, out=None,
             want_level=False):
        N = sig.shape[0]
        _fx_dev(sig, np.float64, "sig", (N * self.V,))
        if control is None:
            control = sig
        else:
            _fx_dev(control, np.float64, "control", (N * self.V,))
        pars, ps = [], 0
        for name, x in zip(DYN_PS, (thresholdHigh, ratioHigh, kneeHigh, thresholdLow, ratioLow, kneeLow)):
            b, per = _fx_param(x, self.V, N, np.float64, name)
            pars.append(b)
            ps |= per * DYN_PS[name]
        self._upload_control()
        out = self._out(N, out)
        self.level_db = DeviceBuffer((N, self.V), zero=False) if want_level else None
        check(lib().mxg_dynamics_render(self.V, N, _ptr(sig), _ptr(control), *[_ptr(b) for b in pars], ps,
                                        self._dwin.ptr, self._dla.ptr, self._dan.ptr, self._dsh.ptr, self._dsl.ptr,
                                        self.stages_high.shape[0], self.rms_ring.ptr, self.cap_rms, self.la_ring.ptr,
                                        self.cap_lookahead, self.rms_pos.ptr, self.la_pos.ptr, self.running.ptr,
                                        self.env_high[0].ptr, self.env_high[1].ptr, self.env_low[0].ptr,
                                        self.env_low[1].ptr, self.overflow.ptr, _ptr(out), _ptr(self.level_db), self.stream),
              "mxg_dynamics_render")
        self._keep = (pars, sig, control)
        return out

    def compress(self, sig, threshold, ratio, knee, **kw):                    # H:2771-2773
        return self.play(sig, None, threshold, ratio, knee, 0, 0, 0, **kw)

    def sidechainCompress(self, sig, control, threshold, ratio, knee, **kw):  # H:2783-2785
        return self.play(sig, control, threshold, ratio, knee, 0, 0, 0, **kw)

    def compandAbove(self, sig, control, threshold, ratio, knee, **kw):       # H:2795-2797
        return self.play(sig, control, threshold, ratio, knee, 0, 0, 0, **kw)

    def compandBelow(self, sig, control, threshold, ratio, knee, **kw):       # H:2807-2809
        return self.play(sig, control, 0, 0, 0, threshold, ratio, knee, **kw)


class maxiRMSBank(_Bank):
    """V x maxiRMS (H:2579-2616).  `cap` is the ring's size in samples (the reference's setup(maxLength, ...) in ms:
    ms_to_samps).  State: ring [cap][V], pos [V], running [V], overflow [V]."""

    def __init__(self, voices, cap, stream=None):
        super().__init__(voices, stream)
        self.cap = int(cap)
        self.ring = DeviceBuffer((self.cap, self.V))
        self.pos = DeviceBuffer(self.V, np.int32)
        self.running = DeviceBuffer(self.V)
        self.overflow = DeviceBuffer(self.V, np.uint32)
        self.window = np.zeros(self.V, np.uint32)
        self._dwin = None

    def setup(self, maxLength, windowSize):
        """H:2584-2587: a new zeroed ring of msToSamps(maxLength) slots, then setWindowSize."""
        self.cap = ms_to_samps(maxLength)
        self.ring = DeviceBuffer((self.cap, self.V))
        self.pos = DeviceBuffer(self.V, np.int32)
        self.setWindowSize(windowSize)

    def setWindowSize(self, newWindowSize, voices=None):
        """H:2590-2596; scalar or one value per voice of `voices` (None = all)."""
        idx = np.arange(self.V)[slice(None) if voices is None else voices].reshape(-1)
        ms = np.broadcast_to(np.asarray(newWindowSize, np.float64), idx.shape)
        r = self.running.numpy()
        for v, m in zip(idx.tolist(), ms.tolist()):
            s = ms_to_samps(m)
            if s <= self.cap:
                self.window[v] = s
            r[v] = 0.0
        self.running.upload(r)
        self._dwin = None

    def play(self, x, out=None):
        N = x.shape[0]
        _fx_dev(x, np.float64, "input", (N * self.V,))
        if self._dwin is None:
            self._dwin = DeviceBuffer.from_numpy(self.window)
        out = self._out(N, out)
        check(lib().mxg_rms_render(self.V, N, _ptr(x), self._dwin.ptr, self.ring.ptr, self.cap, self.pos.ptr,
                                   self.running.ptr, self.overflow.ptr, _ptr(out), self.stream), "mxg_rms_render")
        return out


ANALYSIS_WANT = {"zx": 1, "zcr": 2, "env": 4, "sah": 8}


def analysis_want(want):
    """Names ('zx', 'zcr', 'env', 'sah'), an iterable of them or MXG_ANA_WANT_* bits -> the bits."""
    if isinstance(want, (int, np.integer)):
        return int(want)
    names = [want] if isinstance(want, str) else list(want)
    bad = [n for n in names if n not in ANALYSIS_WANT]
    if bad:
        raise ValueError("want: unknown output %r (one of %s)" % (bad[0], ", ".join(ANALYSIS_WANT)))
    return sum(ANALYSIS_WANT[n] for n in set(names))


def envfollow_coeff(ms, sample_rate=None):
    """maxiEnvelopeFollower::setAttack / setRelease (H:1224-1231): pow(0.01, 1.0 / (ms * sampleRate * 0.001)), host libm."""
    sr = float(maxiSettings.sampleRate if sample_rate is None else sample_rate)
    f = lib().mxg_envfollow_coeff_host
    return np.array([f(float(m), sr) for m in np.atleast_1d(np.asarray(ms, np.float64)).reshape(-1)]).reshape(np.shape(ms))


class maxiAnalysisBank(_Bank):
    """V x (maxiZeroCrossingDetector, maxiZeroCrossingRate, maxiEnvelopeFollower, maxiSampleAndHold) over one input block
    (H:969-1040, 1214-1250; mxg_analysis_render, K16).  `cap` is the size of the ring of crossings in samples (None: the
    sample rate in force now, as the reference's constructor sizes it).  The window defaults to `cap`; the follower to
    setAttack(100), setRelease(100).  State: prev_x [V], zring u64 [ceil(cap/64)][V] (one bit per slot), zpos [V], zcount
    [V], overflow [V], env [V], sah_phase [V], sah_value [V]."""

    def __init__(self, voices, cap=None, stream=None):
        super().__init__(voices, stream)
        self.cap = int(maxiSettings.sampleRate if cap is None else cap)
        if self.cap < 1:
            raise ValueError("cap: the ring needs at least one slot")
        self.window = np.full(self.V, self.cap, np.uint32)
        self._dwin = None
        self.attack = DeviceBuffer.from_numpy(np.full(self.V, envfollow_coeff(100.0)))
        self.release = DeviceBuffer.from_numpy(np.full(self.V, envfollow_coeff(100.0)))
        self.hold_ms = DeviceBuffer(self.V)
        self.reset()

    def reset(self):
        """Fresh objects: everything zero (the window and the follower's coefficients stay)."""
        V = self.V
        self.prev_x = DeviceBuffer(V)
        self.zring = DeviceBuffer(((self.cap + 63) // 64, V), np.uint64)
        self.zpos = DeviceBuffer(V, np.int32)
        self.zcount = DeviceBuffer(V, np.int64)
        self.overflow = DeviceBuffer(V, np.uint32)
        self.env = DeviceBuffer(V)
        self.sah_phase = DeviceBuffer(V)
        self.sah_value = DeviceBuffer(V)

    def setWindow(self, samples):
        """The rate's window in samples, scalar or [V] (the reference: maxiSettings::sampleRate at play time).  0 is refused;
        above cap it is held at cap by the kernel and counted in `overflow`."""
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(samples, np.uint32), (self.V,)))
        check(lib().mxg_analysis_window_host(self.V, w.ctypes.data, self.cap), "mxg_analysis_window_host")
        self.window = w.copy()
        self._dwin = None

    def setAttack(self, attackMS):
        self.attack = DeviceBuffer.from_numpy(np.broadcast_to(envfollow_coeff(attackMS), (self.V,)))

    def setRelease(self, releaseMS):
        self.release = DeviceBuffer.from_numpy(np.broadcast_to(envfollow_coeff(releaseMS), (self.V,)))

    def render(self, x, want=("zx", "zcr", "env", "sah"), hold_ms=None, out=None):
        """x: device [N][V].  hold_ms: scalar / [V], or a device or host [N][V] array (a hold time per sample); None keeps the
        last one.  Returns {name: [N][V] device block} for the requested outputs; `out` may supply some of them."""
        bits = analysis_want(want)
        N = x.shape[0]
        _fx_dev(x, np.float64, "input", (N * self.V,))
        per_sample = 0
        hold = self.hold_ms
        if hold_ms is not None:
            if isinstance(hold_ms, DeviceBuffer) or hasattr(hold_ms, "data_ptr"):
                per_sample = 1 if _fx_dev(hold_ms, np.float64, "hold_ms", (self.V, N * self.V)) == N * self.V else 0
                hold = hold_ms
            else:
                a = np.asarray(hold_ms, np.float64)
                if a.ndim == 2:
                    hold, per_sample = DeviceBuffer.from_numpy(a.reshape(N, self.V)), 1
                else:
                    hold = self.hold_ms = DeviceBuffer.from_numpy(np.broadcast_to(a, (self.V,)))
        if self._dwin is None:
            self._dwin = DeviceBuffer.from_numpy(self.window)
        out = dict(out or {})
        res = {n: out[n] if n in out else DeviceBuffer((N, self.V), np.float64, zero=False) for n, b in ANALYSIS_WANT.items() if bits & b}
        check(lib().mxg_analysis_render(self.V, N, _ptr(x), bits, self.prev_x.ptr, self._dwin.ptr, self.zring.ptr, self.cap,
                                        self.zpos.ptr, self.zcount.ptr, self.overflow.ptr, self.attack.ptr, self.release.ptr,
                                        self.env.ptr, _ptr(hold), per_sample, self.sah_phase.ptr, self.sah_value.ptr,
                                        _ptr(res.get("zx")), _ptr(res.get("zcr")), _ptr(res.get("env")), _ptr(res.get("sah")),
                                        self.stream), "mxg_analysis_render")
        return res


SHAPE_MODES = {"hardclip": 0, "softclip": 1, "fastatan": 2, "fastAtanDist": 3, "atanDist": 4, "asymclip": 5}
SELECT_MAX_K = 64
XFADE_MAX_C = 8


def atan_norm(shape):
    """1.0 / atan(shape) with the host libm (mxg_atan_norm_host): atanDist's factor, the reference's own expression (H:1128)."""
    f = lib().mxg_atan_norm_host
    return np.array([f(float(s)) for s in np.atleast_1d(np.asarray(shape, np.float64)).reshape(-1)]).reshape(np.shape(shape))


class maxiShaperBank(_Bank):
    """V x maxiNonlinearity / maxiDistortion over one block [N][V] (H:1046-1139; mxg_shape_render, K18).  One method per
    reference call; parameters are scalar / [V], or a device or host [N][V] block (one value per sample).  out may be x (in
    place).  hardclip, fastatan and fastAtanDist are the reference's bits; softclip is within 2^-52 of it; atanDist and asymclip
    use the device's atan / pow (tolerance)."""

    def _render(self, mode, x, a=None, b=None, out=None):
        N = x.shape[0]
        _fx_input(x, self.V, N)
        pa = pb = None
        ps = 0
        if a is not None:
            pa, ps = _fx_param(a, self.V, N, np.float64, "shape" if b is None else "a")
        if mode == "asymclip":
            pb, psb = _fx_param(b, self.V, N, np.float64, "b")
            if psb != ps:   # one flag for both: the per-voice one is spread over the block
                if ps:
                    pb = DeviceBuffer.from_numpy(np.broadcast_to(pb.numpy(), (N, self.V)))
                else:
                    pa, ps = DeviceBuffer.from_numpy(np.broadcast_to(pa.numpy(), (N, self.V))), 1
        elif mode == "atanDist" and not ps:
            pb = DeviceBuffer.from_numpy(atan_norm(pa.numpy() if isinstance(pa, DeviceBuffer) else pa.cpu().numpy()))
        out = self._out(N, out)
        check(lib().mxg_shape_render(SHAPE_MODES[mode], self.V, N, _ptr(x), _ptr(pa), _ptr(pb), ps, _ptr(out), self.stream),
              "mxg_shape_render")
        return out

    def hardclip(self, x, out=None):
        return self._render("hardclip", x, out=out)

    def softclip(self, x, out=None):
        return self._render("softclip", x, out=out)

    def fastatan(self, x, out=None):
        return self._render("fastatan", x, out=out)

    def fastAtanDist(self, x, shape, out=None):
        return self._render("fastAtanDist", x, shape, out=out)

    def atanDist(self, x, shape, out=None):
        return self._render("atanDist", x, shape, out=out)

    def asymclip(self, x, a, b, out=None):
        return self._render("asymclip", x, a, b, out=out)


class maxiXFadeBank(_Bank):
    """V x maxiXFade::xfade over C = 1 .. 8 channels (H:1491-1527; mxg_xfade_render, K18): ch1, ch2 are device [C][N][V] (or
    [N][V] for C = 1), xfader scalar / [V] or a device or host [N][V] block.  Bit-exact."""

    def xfade(self, ch1, ch2, xfader, out=None):
        shape = tuple(ch1.shape)
        C, N = (1, shape[0]) if len(shape) == 2 else (shape[0], shape[1])
        if not 1 <= C <= XFADE_MAX_C:
            raise ValueError("C: 1 .. %d channels, got %d" % (XFADE_MAX_C, C))
        for c, what in ((ch1, "ch1"), (ch2, "ch2")):
            _fx_dev(c, np.float64, what, (C * N * self.V,))
        xf, ps = _fx_param(xfader, self.V, N, np.float64, "xfader")
        if out is None:
            out = DeviceBuffer(shape, np.float64, zero=False)
        check(lib().mxg_xfade_render(C, self.V, N, _ptr(ch1), _ptr(ch2), _ptr(xf), ps, _ptr(out), self.stream), "mxg_xfade_render")
        return out


class maxiSelectBank(_Bank):
    """V x maxiSelect (interpolate=False) / maxiSelectX (True) over K = 1 .. 64 values (H:2018-2088; mxg_select_render, K18).
    values: host [K] / [K][V] constants (kept on the device), or a device [K][N][V] block of signals.  A NaN index is undefined
    in the reference; here it reads element 0 and is counted per voice in `nan_count`.  Bit-exact."""

    def __init__(self, voices, interpolate=False, stream=None):
        super().__init__(voices, stream)
        self.interpolate = bool(interpolate)
        self.nan_count = DeviceBuffer(self.V, np.uint32)

    def play(self, index, values, normalised=False, out=None):
        N = index.shape[0]
        _fx_dev(index, np.float64, "index", (N * self.V,))
        if isinstance(values, DeviceBuffer) or hasattr(values, "data_ptr"):
            K = int(values.shape[0])
            n = _fx_dev(values, np.float64, "values", (K * self.V, K * N * self.V))
            sig = int(n == K * N * self.V and (N > 1 or len(values.shape) == 3))
        else:
            a = np.asarray(values, np.float64)
            K = a.shape[0]
            values = DeviceBuffer.from_numpy(np.broadcast_to(a.reshape(K, -1), (K, self.V)))
            sig = 0
        if not 1 <= K <= SELECT_MAX_K:
            raise ValueError("K: 1 .. %d values, got %d" % (SELECT_MAX_K, K))
        out = self._out(N, out)
        check(lib().mxg_select_render(int(self.interpolate), K, self.V, N, _ptr(index), _ptr(values), sig, int(bool(normalised)),
                                      self.nan_count.ptr, _ptr(out), self.stream), "mxg_select_render")
        return out


class maxiLineBank(_Bank):
    """V x maxiLine (H:1532-1617; mxg_line_render, K18).  par [5][V] = lineStart, lineEnd, inc, oneShot, trigEnable; state
    [4][V] = lineValue, lastTrigVal, triggered, lineComplete.  prepare() keeps the reference's quirk: lineValue takes the
    previous lineStart.  Bit-exact, the state included."""

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.par = DeviceBuffer((5, self.V))
        self.reset()

    def reset(self):
        """Fresh objects: lineValue 0, lastTrigVal -1, inc 0, one-shot, triggers disabled."""
        par = np.zeros((5, self.V))
        par[3] = 1.0
        self.par.upload(par)
        st = np.zeros((4, self.V))
        st[1] = -1.0
        self.state = DeviceBuffer.from_numpy(st)

    def prepare(self, start, end, durationMs, isOneShot, voices=None):
        """maxiLine::prepare on every voice, or on `voices` (indices); arguments scalar or [V]."""
        V = self.V
        par, st = self.par.numpy(), self.state.numpy()
        s, e, ms = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (V,))) for a in (start, end, durationMs))
        one = np.ascontiguousarray(np.broadcast_to(np.asarray(isOneShot), (V,)).astype(np.int32))
        mask = None
        if voices is not None:
            mask = np.zeros(V, np.int32)
            mask[np.atleast_1d(np.asarray(voices, np.int64))] = 1
        check(lib().mxg_line_prepare_host(V, s.ctypes.data, e.ctypes.data, ms.ctypes.data, one.ctypes.data,
                                          None if mask is None else mask.ctypes.data, float(maxiSettings.sampleRate),
                                          par.ctypes.data, st.ctypes.data), "mxg_line_prepare_host")
        self.par.upload(par)
        self.state.upload(st)

    def triggerEnable(self, on):
        par = self.par.numpy()
        par[4] = (np.broadcast_to(np.asarray(on, np.float64), (self.V,)) > 0.0).astype(np.float64)
        self.par.upload(par)

    def isLineComplete(self):
        return self.state.numpy()[3] != 0.0

    def play(self, trigger, N=None, out=None):
        """trigger: a device [N][V] block, or a number played on N samples (line.play(1))."""
        if isinstance(trigger, DeviceBuffer) or hasattr(trigger, "data_ptr"):
            N = trigger.shape[0]
            _fx_dev(trigger, np.float64, "trigger", (N * self.V,))
            tp, tc = _ptr(trigger), 0.0
        else:
            if N is None:
                raise ValueError("N: a constant trigger needs the number of samples")
            tp, tc = None, float(trigger)
        out = self._out(int(N), out)
        check(lib().mxg_line_render(self.V, int(N), tp, tc, self.par.ptr, self.state.ptr, _ptr(out), self.stream), "mxg_line_render")
        return out


MAP_MODES = {"linlin": 0, "linexp": 1, "explin": 2, "clamp": 3, "ampToDbs": 4, "dbsToAmp": 5}  # MXG_MAP_* (include/maxigpu.h)
CLASSIC_PS = {"threshold": 1, "attack": 2, "release": 4, "ratio": 8}                          # MXG_CLASSIC_PS_*
ENVELOPE_MAX_S = 64


def dyn_coeff(ms, sample_rate=None):
    """maxiDyn::setAttack / setRelease: pow(0.01, 1.0 / (ms * sampleRate * 0.001)) with the host libm (mxg_dyn_coeff_host)."""
    return lib().mxg_dyn_coeff_host(float(ms), float(maxiSettings.sampleRate if sample_rate is None else sample_rate))


def dyn_makeup(ratio):
    """1 + log(ratio) with the host libm (mxg_dyn_makeup_host): the compressor's make-up factor; scalar / array alike."""
    f = lib().mxg_dyn_makeup_host
    return np.array([f(float(r)) for r in np.atleast_1d(np.asarray(ratio, np.float64)).reshape(-1)]).reshape(np.shape(ratio))


class maxiDynBank(_Bank):
    """V x maxiDyn (src/maximilian.cpp:1200-1314; mxg_dyn_gate_render / mxg_dyn_compress_render, K23).  gate() and compressor()
    take the reference's arguments: scalar / [V], or a device or host [N][V] block (one value per sample); compress() runs the
    same step on the members the four setters left (setAttack / setRelease in ms: the stored value is pow(0.01, ...), which
    compress() uses as 1 + attack -- the reference's quirk).  State: dst [3][V] = amplitude, currentRatio, output; ist int64
    [4][V] = holdcount, attackphase, holdphase, releasephase; gate and compressor share it, as the members of one maxiDyn are.
    Bit-exact, the state included; out is distinct from x."""

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.dst = DeviceBuffer((3, self.V))
        self.ist = DeviceBuffer((4, self.V), np.int64)
        self.ratio, self.threshold, self.attack, self.release = (np.zeros(self.V) for _ in range(4))

    def _params(self, N, **named):
        ptrs, flags = [], 0
        for name, x in named.items():
            p, ps = _fx_param(x, self.V, N, np.float64, name)
            ptrs.append(p)
            flags |= CLASSIC_PS[name] * ps
        return ptrs, flags

    def gate(self, x, threshold=0.9, holdtime=1, attack=1, release=0.9995, out=None):
        N = x.shape[0]
        _fx_input(x, self.V, N)
        (thr, att, rel), flags = self._params(N, threshold=threshold, attack=attack, release=release)
        hold = _as_dev(holdtime, self.V, np.int64)
        out = self._out(N, out)
        check(lib().mxg_dyn_gate_render(self.V, N, _ptr(x), _ptr(thr), _ptr(att), _ptr(rel), flags, _ptr(hold), self.dst.ptr, self.ist.ptr,
                                        _ptr(out), self.stream), "mxg_dyn_gate_render")
        return out

    def compressor(self, x, ratio, threshold=0.9, attack=1, release=0.9995, out=None, makeup=None):
        """makeup: the make-up factors 1 + log(ratio) of `ratio`, in its layout (dyn_makeup: the host libm's, as in the reference).
        None: they are formed here from a host ratio.  A ratio that lives on the device comes with its make-up block, which its
        producer formed once on the host; nothing is then copied back."""
        N = x.shape[0]
        _fx_input(x, self.V, N)
        on_device = isinstance(ratio, DeviceBuffer) or hasattr(ratio, "data_ptr")
        if on_device and makeup is None:
            raise ValueError("ratio: a device-resident ratio needs makeup= (dyn_makeup of the same values, in the same layout)")
        (thr, att, rel, rat), flags = self._params(N, threshold=threshold, attack=attack, release=release, ratio=ratio)
        if makeup is None:
            makeup = dyn_makeup(np.asarray(ratio, np.float64))
        mk, mk_ps = _fx_param(makeup, self.V, N, np.float64, "makeup")
        if mk_ps != (1 if flags & CLASSIC_PS["ratio"] else 0):
            raise ValueError("makeup: ratio and makeup travel together, both [V] or both [N][V]")
        out = self._out(N, out)
        check(lib().mxg_dyn_compress_render(self.V, N, _ptr(x), _ptr(rat), _ptr(mk), _ptr(thr), _ptr(att), _ptr(rel), flags, self.dst.ptr,
                                            self.ist.ptr, _ptr(out), self.stream), "mxg_dyn_compress_render")
        return out

    def compress(self, x, out=None):
        return self.compressor(x, self.ratio, self.threshold, self.attack, self.release, out=out)

    def _set(self, name, value):
        setattr(self, name, np.ascontiguousarray(np.broadcast_to(np.asarray(value, np.float64), (self.V,))))

    def setAttack(self, attackMS):
        self._set("attack", [dyn_coeff(ms) for ms in np.broadcast_to(np.asarray(attackMS, np.float64), (self.V,))])

    def setRelease(self, releaseMS):
        self._set("release", [dyn_coeff(ms) for ms in np.broadcast_to(np.asarray(releaseMS, np.float64), (self.V,))])

    def setThreshold(self, thresholdI):
        self._set("threshold", thresholdI)

    def setRatio(self, ratioF):
        self._set("ratio", ratioF)


class maxiEnvelopeBank(_Bank):
    """V x maxiEnvelope (src/maximilian.cpp:377-412; mxg_envelope_line_render, K23).  segments: one table for every voice ([S]) or
    a table per voice ([S][V], `count` entries of voice v in use): value, time, value, time ...  State: dst [2][V] = amplitude,
    startval; ist int32 [2][V] = valindex, isPlaying.  trigger() between blocks writes the state; a device trigger block in
    line() performs trigger(trig_index, trig_amp) before the samples where it is non-zero.  Bit-exact, the state included.  A
    trigger index outside [0, count - 2] is refused (the reference indexes out of its vector there)."""

    def __init__(self, voices, segments, count=None, stream=None):
        super().__init__(voices, stream)
        seg = np.asarray(segments, np.float64)
        if seg.ndim == 1:
            seg = np.repeat(seg[:, None], self.V, axis=1)
        self.S = seg.shape[0]
        if not 2 <= self.S <= ENVELOPE_MAX_S or seg.shape != (self.S, self.V):
            raise ValueError("segments: [S] or [S][V] with S in 2 .. %d, got %s" % (ENVELOPE_MAX_S, seg.shape))
        self._count = np.ascontiguousarray(np.broadcast_to(np.asarray(self.S if count is None else count, np.int32), (self.V,)))
        if (self._count < 2).any() or (self._count > self.S).any():
            raise ValueError("count: 2 .. S entries per voice")
        self.segments = DeviceBuffer.from_numpy(seg)
        self.count = DeviceBuffer.from_numpy(self._count)
        self.dst = DeviceBuffer((2, self.V))
        self.ist = DeviceBuffer((2, self.V), np.int32)
        self.trig_index = DeviceBuffer(self.V, np.int32)
        self.trig_amp = DeviceBuffer(self.V)

    def trigger(self, index, amp, voices=None):
        """maxiEnvelope::trigger(index, amp) on every voice, or on `voices` (indices); arguments scalar or [V]."""
        V = self.V
        dst, ist = self.dst.numpy(), self.ist.numpy()
        ix = np.ascontiguousarray(np.broadcast_to(np.asarray(index, np.int32), (V,)))
        am = np.ascontiguousarray(np.broadcast_to(np.asarray(amp, np.float64), (V,)))
        mask = None
        if voices is not None:
            mask = np.zeros(V, np.int32)
            mask[np.atleast_1d(np.asarray(voices, np.int64))] = 1
        check(lib().mxg_envelope_trigger_host(V, ix.ctypes.data, am.ctypes.data, None if mask is None else mask.ctypes.data,
                                              self._count.ctypes.data, dst.ctypes.data, ist.ctypes.data), "mxg_envelope_trigger_host")
        self.dst.upload(dst)
        self.ist.upload(ist)

    def line(self, N=None, trigger=None, trig_index=0, trig_amp=0.0, out=None):
        """N samples of line(); trigger: a device [N][V] block whose non-zero values trigger (trig_index, trig_amp: scalar / [V])."""
        if trigger is not None:
            N = trigger.shape[0]
            _fx_dev(trigger, np.float64, "trigger", (N * self.V,))
            ix = np.ascontiguousarray(np.broadcast_to(np.asarray(trig_index, np.int32), (self.V,)))
            if (ix < 0).any() or (ix > self._count - 2).any():
                raise ValueError("trig_index: outside [0, count - 2]")
            self.trig_index.upload(ix)
            self.trig_amp.upload(np.broadcast_to(np.asarray(trig_amp, np.float64), (self.V,)))
        elif N is None:
            raise ValueError("N: without a trigger block the number of samples is needed")
        out = self._out(int(N), out)
        check(lib().mxg_envelope_line_render(self.V, int(N), self.S, self.segments.ptr, self.count.ptr, _ptr(trigger), self.trig_index.ptr,
                                             self.trig_amp.ptr, self.dst.ptr, self.ist.ptr, _ptr(out), self.stream), "mxg_envelope_line_render")
        return out

    @property
    def valindex(self):
        return self.ist.numpy()[0]

    @property
    def amplitude(self):
        return self.dst.numpy()[0]


class maxiLagExpBank(_Bank):
    """V x maxiLagExp<double> (H:499-560; mxg_lag_render, K23): val = (alpha * x) + (alphaReciprocal * val) over a block.
    alpha and alphaReciprocal are independent, as in the reference: init() sets both, setAlpha() only alpha.  Bit-exact."""

    def __init__(self, voices, alpha=0.5, val=0.0, stream=None):
        super().__init__(voices, stream)
        self.init(alpha, val)

    def init(self, alpha, val):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, np.float64), (self.V,)))
        self.alpha, self.alphaReciprocal = DeviceBuffer.from_numpy(a), DeviceBuffer.from_numpy(1.0 - a)
        self.val = DeviceBuffer.from_numpy(np.broadcast_to(np.asarray(val, np.float64), (self.V,)))

    def setAlpha(self, alpha):
        self.alpha.upload(np.broadcast_to(np.asarray(alpha, np.float64), (self.V,)))

    def setAlphaReciprocal(self, alphaReciprocal):
        self.alphaReciprocal.upload(np.broadcast_to(np.asarray(alphaReciprocal, np.float64), (self.V,)))

    def setVal(self, val):
        self.val.upload(np.broadcast_to(np.asarray(val, np.float64), (self.V,)))

    def addSample(self, x, alpha=None, alphaReciprocal=None, out=None):
        """A block [N][V] of samples -> the value after each; alpha / alphaReciprocal: device [N][V] blocks for a pair per sample."""
        N = x.shape[0]
        _fx_input(x, self.V, N)
        a, r, ps = self.alpha, self.alphaReciprocal, 0
        if alpha is not None:
            _fx_dev(alpha, np.float64, "alpha", (N * self.V,))
            _fx_dev(alphaReciprocal, np.float64, "alphaReciprocal", (N * self.V,))
            a, r, ps = alpha, alphaReciprocal, 1
        out = self._out(N, out)
        check(lib().mxg_lag_render(self.V, N, _ptr(x), _ptr(a), _ptr(r), ps, self.val.ptr, _ptr(out), self.stream), "mxg_lag_render")
        return out

    def value(self):
        return self.val.numpy()


class maxiMapBank(_Bank):
    """V x maxiMap / maxiConvert over one block [N][V] (H:801-854, 955-961; mxg_map_render, K23).  Ranges are scalar / [V].  out
    may be x (in place).  linlin and clamp are the reference's bits; linexp, explin, ampToDbs and dbsToAmp use the device's pow /
    log / log10 (tolerance); explin's log(inMax / inMin) comes from the host libm."""

    def _render(self, mode, x, rng=(), out=None):
        N = x.shape[0]
        _fx_input(x, self.V, N)
        dr = da = None
        if rng:
            r = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(t, np.float64), (self.V,)) for t in rng]))
            dr = DeviceBuffer.from_numpy(r)
            if mode == "explin":
                aux = np.zeros(self.V)
                check(lib().mxg_map_range_host(MAP_MODES[mode], self.V, r.ctypes.data, aux.ctypes.data), "mxg_map_range_host")
                da = DeviceBuffer.from_numpy(aux)
        out = self._out(N, out)
        check(lib().mxg_map_render(MAP_MODES[mode], self.V, N, _ptr(x), _ptr(dr), _ptr(da), _ptr(out), self.stream), "mxg_map_render")
        return out

    def linlin(self, x, inMin, inMax, outMin, outMax, out=None):
        return self._render("linlin", x, (inMin, inMax, outMin, outMax), out)

    def linexp(self, x, inMin, inMax, outMin, outMax, out=None):
        return self._render("linexp", x, (inMin, inMax, outMin, outMax), out)

    def explin(self, x, inMin, inMax, outMin, outMax, out=None):
        return self._render("explin", x, (inMin, inMax, outMin, outMax), out)

    def clamp(self, x, low, high, out=None):
        return self._render("clamp", x, (low, high), out)

    def ampToDbs(self, x, out=None):
        return self._render("ampToDbs", x, (), out)

    def dbsToAmp(self, x, out=None):
        return self._render("dbsToAmp", x, (), out)


POLYBLEP_WAVEFORMS = {"SINE": 0, "COSINE": 1, "TRIANGLE": 2, "SQUARE": 3, "RECTANGLE": 4, "SAWTOOTH": 5, "RAMP": 6, "MODIFIED_TRIANGLE": 7,
                      "MODIFIED_SQUARE": 8, "HALF_WAVE_RECTIFIED_SINE": 9, "FULL_WAVE_RECTIFIED_SINE": 10, "TRIANGULAR_PULSE": 11,
                      "TRAPEZOID_FIXED": 12, "TRAPEZOID_VARIABLE": 13}


def polyblep_sync(phase):
    """PolyBLEP::sync's wrap (P:101-108) on the host: t - (int64)t, a negative phase t + (1 - (int64)t)."""
    t = np.asarray(phase, np.float64)
    return np.where(t >= 0, t - np.trunc(t), t + (1 - np.trunc(t)))


class maxiPolyBLEPBank(_Bank):
    """V x maxiPolyBLEP (src/libs/maxiPolyBLEP.h; mxg_polyblep_render, K20): one waveform for the bank, a pulse width and a
    phase per voice, the phase carried from call to call.  The phase and the ten arithmetic waveforms are the reference's
    bits; the sine waveforms and the sine fallback at freq >= sampleRate / 4 are within the bounds of DESIGN.md section 4."""

    def __init__(self, voices, sampleRate=None, stream=None):
        super().__init__(voices, stream)
        self.sampleRate = float(maxiSettings.sampleRate if sampleRate is None else sampleRate)
        self.waveform = 0                     # the reference's constructor: SINE, pulse width 0.5, t = 0
        self.pw = None                        # None: 0.5 on every voice
        self.t = DeviceBuffer(self.V)

    def set_waveform(self, waveform):
        wf = POLYBLEP_WAVEFORMS[waveform] if isinstance(waveform, str) else int(waveform)
        if not 0 <= wf < len(POLYBLEP_WAVEFORMS):
            raise ValueError("waveform: one of POLYBLEP_WAVEFORMS")
        self.waveform = wf

    def set_pulse_width(self, pw):
        """Per voice: scalar or [V]."""
        self.pw = _as_dev(pw, self.V)

    def set_sample_rate(self, sampleRate):
        self.sampleRate = float(sampleRate)

    def sync(self, phases=None, voices=None):
        """maxiPolyBLEP::sync(phase) on every voice, or on `voices` (indices); phases scalar or one per synced voice.  Without an
        argument: wait for the stream, as every bank does."""
        if phases is None:
            return super().sync()
        if voices is None:
            self.t.upload(np.ascontiguousarray(np.broadcast_to(polyblep_sync(phases), (self.V,))))
            return
        t = self.t.numpy()
        t[np.atleast_1d(np.asarray(voices, np.int64))] = polyblep_sync(phases)
        self.t.upload(t)

    def render(self, freq, N=None, out=None, per_sample=False):
        """freq: scalar / [V] with N, or per_sample a host or device [N][V] block."""
        if per_sample:
            f = freq if (isinstance(freq, DeviceBuffer) or hasattr(freq, "data_ptr")) else \
                DeviceBuffer.from_numpy(np.ascontiguousarray(freq, np.float64))
            N = f.shape[0]
            _fx_dev(f, np.float64, "freq", (N * self.V,))
        else:
            if N is None:
                raise ValueError("N: block-constant frequencies need the number of samples")
            f = _as_dev(freq, self.V)
        out = self._out(int(N), out)
        check(lib().mxg_polyblep_render(self.waveform, self.V, int(N), _ptr(f), 1 if per_sample else 0, _ptr(self.pw), self.sampleRate,
                                        self.t.ptr, _ptr(out), self.stream), "mxg_polyblep_render")
        self._keep = f  # keep the parameter buffer alive until the next call
        return out


KURAMOTO_WANT = {"mix": 1, "phases": 2}
KURAMOTO_MAX_N = 64


class maxiKuramotoBank(_Bank):
    """S x maxiKuramotoOscillatorSet (asynchronous=True: maxiAsyncKuramotoOscillator) of N = 1 .. 64 phase-coupled oscillators
    each (H:1628-1808; mxg_kuramoto_render, K17).  meanfield=True selects the tolerance mode that forms the coupling sum from
    the set's summed sines and cosines (N pairs per sample instead of N * N sines).  State: phase [S][N]; asynchronous sets
    also gathered [S][N] and update i32 [S].  dt is TWOPI / maxiSettings.sampleRate at each call.  set_phase / set_phases are
    the reference's setPhase / setPhases between two blocks; on asynchronous sets they raise the set's flag."""
    MAX_N = KURAMOTO_MAX_N
    ENTRY = "mxg_kuramoto_render"

    def __init__(self, sets, N, meanfield=False, asynchronous=False, stream=None):
        self.S, self.N = int(sets), int(N)
        if not 1 <= self.N <= self.MAX_N:   # (before the device is touched, as the entry point refuses it)
            raise ValueError("N: a set has 1 .. %d oscillators, got %d" % (self.MAX_N, self.N))
        super().__init__(sets, stream)
        self.mode = (1 if meanfield else 0) | (2 if asynchronous else 0)
        self.asynchronous = bool(asynchronous)
        self.freq = DeviceBuffer(self.S)
        self.K = DeviceBuffer(self.S)
        self.reset()

    def reset(self):
        """Fresh sets: phases 0, gathered phases 0, flags down."""
        self.phase = DeviceBuffer((self.S, self.N))
        self.gathered = DeviceBuffer((self.S, self.N)) if self.asynchronous else None
        self.update = DeviceBuffer(self.S, np.int32) if self.asynchronous else None

    def phases(self):
        """getPhase(i) of every set: host [S][N]."""
        return self.phase.numpy()

    def set_phases(self, phases, sets=None):
        """setPhases: [N] for every set, or [S][N]; `sets` restricts it to those sets (rows of `phases` then match them)."""
        cur = self.phase.numpy()
        idx = np.arange(self.S) if sets is None else np.atleast_1d(np.asarray(sets, np.int64))
        cur[idx] = np.broadcast_to(np.asarray(phases, np.float64), (len(idx), self.N))
        self.phase.upload(cur)
        self._raise(idx)

    def set_phase(self, phase, oscillatorIdx, sets=None):
        """setPhase(phase, oscillatorIdx) on every set, or on `sets` (phase: scalar or one per set)."""
        if not 0 <= int(oscillatorIdx) < self.N:
            raise IndexError("oscillatorIdx %d outside a set of %d" % (oscillatorIdx, self.N))
        cur = self.phase.numpy()
        idx = np.arange(self.S) if sets is None else np.atleast_1d(np.asarray(sets, np.int64))
        cur[idx, int(oscillatorIdx)] = np.broadcast_to(np.asarray(phase, np.float64), (len(idx),))
        self.phase.upload(cur)
        self._raise(idx)

    def _raise(self, idx):
        if self.asynchronous:
            up = self.update.numpy()
            up[idx] = 1
            self.update.upload(up)

    def _param(self, x, B, keep, what):
        """scalar / [S] (kept for the next call) or a device / host [B][S] block -> (buffer, per_sample)."""
        if isinstance(x, DeviceBuffer) or hasattr(x, "data_ptr"):
            n = _fx_dev(x, np.float64, what, (self.S, B * self.S))
            return x, (1 if n == B * self.S and B > 1 else 0)   # (B == 1: [S] and [1][S] are the same memory)
        a = np.asarray(x, np.float64)
        if a.ndim == 2:
            return DeviceBuffer.from_numpy(a.reshape(B, self.S)), 1
        keep.upload(np.broadcast_to(a, (self.S,)))
        return keep, 0

    def render(self, B, freq, K, want=("mix",), out=None):
        """B samples.  freq, K: scalar / [S], or a device or host [B][S] block (one value per sample).  Returns {name: device
        block} for the wanted outputs: "mix" [B][S], "phases" [B][S][N]; `out` may supply them."""
        names = [want] if isinstance(want, str) else list(want)
        bad = [n for n in names if n not in KURAMOTO_WANT]
        if bad:
            raise ValueError("want: unknown output %r (one of %s)" % (bad[0], ", ".join(KURAMOTO_WANT)))
        bits = sum(KURAMOTO_WANT[n] for n in set(names))
        B = int(B)
        f, fps = self._param(freq, B, self.freq, "freq")
        k, kps = self._param(K, B, self.K, "K")
        out = dict(out or {})
        shapes = {"mix": (B, self.S), "phases": (B, self.S, self.N)}
        res = {n: out[n] if n in out else DeviceBuffer(shapes[n], np.float64, zero=False) for n, b in KURAMOTO_WANT.items() if bits & b}
        check(getattr(lib(), self.ENTRY)(self.mode, self.S, self.N, B, _ptr(f), fps, _ptr(k), kps, self.phase.ptr, _ptr(self.gathered),
                                         _ptr(self.update), bits, _ptr(res.get("mix")), _ptr(res.get("phases")), self.stream),
              self.ENTRY)
        return res

    def play(self, freq, K, B=None, out=None):
        """play(freq, K) for B samples -> the mix block, device [B][S].  B defaults to the rows of a [B][S] freq or K."""
        if B is None:
            for x in (freq, K):
                if len(getattr(x, "shape", ())) == 2:
                    B = int(x.shape[0])
            if B is None:
                raise ValueError("play: B is needed when freq and K are per set")
        return self.render(B, freq, K, ("mix",), None if out is None else {"mix": out})["mix"]

    def render_phases(self, freq, K, B=None, out=None):
        """As play(), returning (mix [B][S], phases [B][S][N])."""
        if B is None:
            for x in (freq, K):
                if len(getattr(x, "shape", ())) == 2:
                    B = int(x.shape[0])
            if B is None:
                raise ValueError("render_phases: B is needed when freq and K are per set")
        r = self.render(B, freq, K, ("mix", "phases"), out)
        return r["mix"], r["phases"]


KURAMOTO_WIDE_MAX_N = 1024


class maxiKuramotoWideBank(maxiKuramotoBank):
    """maxiKuramotoBank for sets of N = 1 .. 1024 oscillators (mxg_kuramoto_wide_render, K26: one workgroup per set, one lane per
    oscillator).  The same methods, state and modes; it pays from N = 65 on -- up to 64 maxiKuramotoBank packs several sets into
    a wavefront and gives the same bits.  The exact form is N * N sines per set and sample: a set of 1024 is about a million, and
    only meanfield=True (N sine / cosine pairs) brings a set that wide near real time."""
    MAX_N = KURAMOTO_WIDE_MAX_N
    ENTRY = "mxg_kuramoto_wide_render"


SAMPLE_MODES = {"play": 0, "playOnce": 1, "playLoop": 2, "playUntil": 3, "playAtSpeed": 4,
                "playOnceAtSpeed": 5, "playUntilAtSpeed": 6, "play4": 7, "playAtSpeedBetweenPoints": 8,
                # trigger-driven (mxg_sample_render_trig)
                "playOnZX": 9, "playOnZXAtSpeed": 10, "playOnZXAtSpeedFromOffset": 11,
                "playOnZXAtSpeedBetweenPoints": 12, "loopSetPosOnZX": 13, "playWithPhasor": 14}


def seq_table(rows, width=None):
    """Ragged lists -> (doubles [P][L], int32 lengths [P]): the table form of mxg_seq_render / mxg_seq_signal."""
    rows = [list(np.atleast_1d(np.asarray(r, np.float64))) for r in rows]
    if not rows or min(len(r) for r in rows) < 1:
        raise ValueError("a table needs at least one list and every list at least one entry")
    width = max(len(r) for r in rows) if width is None else int(width)
    tab = np.zeros((len(rows), width))
    for i, r in enumerate(rows):
        tab[i, :len(r)] = r
    return tab, np.array([len(r) for r in rows], np.int32)


def seq_ratio_tables(times):
    """maxiRatioSeq::playTrig's boundary tables for a list of ratio lists (mxg_seq_ratio_host: host arithmetic, the reference's
    operations in the reference's order).  Returns (norm [P][L], lengths [P])."""
    tab, lens = seq_table(times)
    norm = np.zeros_like(tab)
    check(lib().mxg_seq_ratio_host(tab.shape[0], tab.shape[1], lens.ctypes.data, tab.ctypes.data, norm.ctypes.data), "mxg_seq_ratio_host")
    return norm, lens


class _SeqTables:
    """Value lists on the device: `values` = a list of lists; a voice picks its list with `select`."""

    def _set_values(self, values):
        if values is None:
            self.values = self.vlen = None
            self.values_shape = (0, 0)
            return
        tab, lens = seq_table(values)
        self.values, self.vlen, self.values_shape = DeviceBuffer.from_numpy(tab), DeviceBuffer.from_numpy(lens), tab.shape

    def _select(self, sel):
        return None if sel is None else DeviceBuffer.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(sel, np.int32), (self.V,))))


class maxiSeqBank(_Bank, _SeqTables):
    """V fused sequencers (kernel K15, mxg_seq_render): a clock per voice -> maxiRatioSeq::playTrig against the voice's ratio
    pattern -> playValues or maxiStep::pull over the voice's value list -> maxiZXToPulse::play.  `times` is a list of ratio lists
    (at most 64 ratios each), `values` a list of value lists; setPattern / setValueList pick one per voice (default: list 0).
    Patterns and lists are block-constant: change them between renders (setTimes / setValues).  The blocks render() returns stay
    on the device and are what maxiEnvGenBank.play (trigger, gate) and maxiOscBank.render(per_sample=True) (value) accept."""

    def __init__(self, voices, times=((1,),), values=None, stream=None):
        super().__init__(voices, stream)
        self.clock = DeviceBuffer(self.V)  # maxiOsc::phase of the internal clock
        d = np.zeros((5, self.V))
        d[[1, 3]] = 1.0                     # maxiTrigger::previousValue of maxiStep and maxiZXToPulse (H:594)
        i = np.zeros((6, self.V), np.int64)
        i[[0, 3, 4, 5]] = 1                 # maxiRatioSeq::first, the two firstTrigger, maxiStep::first
        self.dstate, self.istate = DeviceBuffer.from_numpy(d), DeviceBuffer.from_numpy(i)
        self.pattern = self.value_list = self.step = self.hold = None
        self.setTimes(times)
        self._set_values(values)

    def setTimes(self, times):
        norm, lens = seq_ratio_tables(times)
        self.host_norm = norm
        self.norm, self.len = DeviceBuffer.from_numpy(norm), DeviceBuffer.from_numpy(lens)

    def setValues(self, values): self._set_values(values)
    def setPattern(self, sel): self.pattern = self._select(sel)
    def setValueList(self, sel): self.value_list = self._select(sel)
    def setStep(self, step): self.step = _as_dev(step, self.V)
    def setHold(self, samples): self.hold = _as_dev(samples, self.V)

    def render(self, N, freq=None, phase=None, trig=True, val=None, gate=False):
        """freq [V]: the internal clock maxiOsc::phasor(freq[v]); or phase: a device / numpy phase signal [N][V] or shared [N].
        val: None, "values" (playValues) or "step" (maxiStep::pull).  Returns (trig, val, gate) device blocks [N][V], None where
        not asked for; a stage that is not asked for does not run."""
        if (freq is None) == (phase is None):
            raise ValueError("give freq (internal clock) or phase (external), not both")
        if val not in (None, "values", "step"):
            raise ValueError("val must be None, 'values' or 'step'")
        if val is not None and self.values is None:
            raise ValueError("no value lists: pass values= or call setValues")
        f = ph = None
        pv = 0
        if freq is not None:
            f = _as_dev(freq, self.V)
        else:
            ph = phase if (isinstance(phase, DeviceBuffer) or hasattr(phase, "data_ptr")) else \
                DeviceBuffer.from_numpy(np.ascontiguousarray(phase, np.float64))
            pv = int(len(ph.shape) == 2)
        outs = [DeviceBuffer((N, self.V), np.float64, zero=False) if w else None for w in (trig, val is not None, gate)]
        check(lib().mxg_seq_render(self.V, N, _ptr(f), self.clock.ptr if f is not None else None, _ptr(ph), pv, self.norm.ptr, self.len.ptr,
                                   self.host_norm.shape[0], self.host_norm.shape[1], _ptr(self.pattern), 1 if val == "step" else 0,
                                   _ptr(self.values), _ptr(self.vlen), self.values_shape[0], self.values_shape[1], _ptr(self.value_list),
                                   _ptr(self.step), _ptr(self.hold), self.dstate.ptr, self.istate.ptr, _ptr(outs[0]), _ptr(outs[1]),
                                   _ptr(outs[2]), self.stream), "mxg_seq_render")
        self._keep = (f, ph)
        return tuple(outs)


class _SeqSignalBank(_Bank, _SeqTables):
    """One of the reference's sequencing classes driven by device signals [N][V] (mxg_seq_signal)."""
    KIND = 0

    def __init__(self, voices, values=None, stream=None):
        super().__init__(voices, stream)
        d, i = np.zeros((3, self.V)), np.zeros((2, self.V), np.int64)
        self._fresh(d, i)
        self.dstate, self.istate = DeviceBuffer.from_numpy(d), DeviceBuffer.from_numpy(i)
        self.value_list = None
        self._set_values(values)

    def _fresh(self, d, i):
        d[0] = 1.0  # maxiTrigger::previousValue
        i[0] = 1    # firstTrigger

    def setValues(self, values): self._set_values(values)
    def setValueList(self, sel): self.value_list = self._select(sel)

    def _dev(self, x, N):
        if x is None or isinstance(x, DeviceBuffer) or hasattr(x, "data_ptr"):
            return x
        return DeviceBuffer.from_numpy(np.ascontiguousarray(x, np.float64).reshape(N, self.V))

    def _run(self, a, b=None, par=None, out=None):
        N = a.shape[0] if hasattr(a, "shape") else len(a)
        a, b = self._dev(a, N), self._dev(b, N)
        par = None if par is None else _as_dev(par, self.V)
        out = self._out(N, out)
        check(lib().mxg_seq_signal(self.KIND, self.V, N, _ptr(a), _ptr(b), _ptr(self.values), _ptr(self.vlen), self.values_shape[0],
                                   self.values_shape[1], _ptr(self.value_list), _ptr(par), self.dstate.ptr, self.istate.ptr, _ptr(out),
                                   self.stream), "mxg_seq_signal")
        self._keep = (a, b, par)
        return out


class maxiTriggerBank(_SeqSignalBank):
    """V x maxiTrigger (H:564-596)."""
    KIND = 0

    def onZX(self, input, out=None): return self._run(input, out=out)


class maxiCounterBank(_SeqSignalBank):
    """V x maxiCounter (H:1953-1977)."""
    KIND = 1

    def _fresh(self, d, i):
        d[1:3] = 1.0
        i[:] = 1

    def count(self, incTrigger, resetTrigger, out=None): return self._run(incTrigger, resetTrigger, out=out)


class maxiStepBank(_SeqSignalBank):
    """V x maxiStep (H:2093-2141) over the value lists of the bank."""
    KIND = 2

    def _fresh(self, d, i):
        d[0] = 1.0
        i[:] = 1  # trig.firstTrigger, first

    def pull(self, trigSig, step=1.0, out=None): return self._run(trigSig, par=step, out=out)


class maxiIndexBank(_SeqSignalBank):
    """V x maxiIndex (H:1982-2013) over the value lists of the bank."""
    KIND = 3

    def pull(self, trigSig, indexSig, out=None): return self._run(trigSig, indexSig, out=out)


class maxiZXToPulseBank(_SeqSignalBank):
    """V x maxiZXToPulse (H:2235-2262)."""
    KIND = 4

    def play(self, input, holdTimeInSamples, out=None): return self._run(input, par=holdTimeInSamples, out=out)


class maxiSampleBank(_Bank):
    """V play heads over one maxiSample (H:602-783): the bank shares the sample data the way
    maxiGrains alias one maxiSample (L/maxiGrains.h:162)."""

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        self.d_samples = None
        self.length = 0
        self.mySampleRate = int(maxiSettings.sampleRate)  # ctor, C:546
        self.position = DeviceBuffer(self.V)
        # maxiTrigger zxTrig (H:593-594: previousValue = 1, firstTrigger = 1), phasorPrev/First (H:731-732)
        self.zx_prev = DeviceBuffer.from_numpy(np.ones(self.V))
        self.zx_first = DeviceBuffer.from_numpy(np.ones(self.V, np.int32))
        self.phasor_prev = DeviceBuffer(self.V)
        self.phasor_first = DeviceBuffer.from_numpy(np.ones(self.V, np.int32))

    def setSample(self, samples):
        """maxiSample::setSample (H:670-678): copies the data, mySampleRate=44100, position=len-1."""
        a = np.ascontiguousarray(samples, np.float64)
        self.clear()
        p = lib().mxg_sample_upload(a.ctypes.data, a.size)
        if not p:
            raise MemoryError(lib().mxg_last_error().decode())
        self.d_samples, self.length = p, a.size
        self.mySampleRate = 44100
        self.position.upload(np.full(self.V, a.size - 1.0))

    def load(self, fileName, channel=0):
        """maxiSample::load (C:605-692): 16-bit PCM WAV -> device amplitudes (de-interleave + /32767.0 on
        the device).  Returns False if the file cannot be read (the reference's bool).  position = size."""
        n = ctypes.c_size_t(0)
        hdr = np.zeros(8, np.int32)
        p = lib().mxg_sample_load_wav(os.fsencode(fileName), int(channel), ctypes.byref(n), hdr.ctypes.data)
        if not p:
            return False
        self.clear()
        self.d_samples, self.length = p, n.value
        self.wav_header = hdr
        self.mySampleRate = int(hdr[4])
        self.position.upload(np.full(self.V, float(n.value)))   # C:681
        return True

    def save(self, fileName):
        """maxiSample::save (C:698-725) with the header fields of the loaded file (or a mono 16-bit default)."""
        hdr = getattr(self, "wav_header", None)
        if hdr is None:
            hdr = np.array([36 + 2 * self.length, 16, 1, 1, self.mySampleRate, 2 * self.mySampleRate, 2, 16], np.int32)
        check(lib().mxg_sample_save_wav(os.fsencode(fileName), self.d_samples, self.length, hdr.ctypes.data,
                                        self.stream), "mxg_sample_save_wav")
        return True

    def amplitudes(self):
        """The device sample buffer as a numpy array (for tests)."""
        out = np.empty(self.length)
        check(lib().mxg_memcpy_d2h(out.ctypes.data, self.d_samples, out.nbytes, self.stream), "mxg_memcpy_d2h")
        return out

    def setSampleAndRate(self, samples, sampleRate):
        self.setSample(samples)
        self.mySampleRate = int(sampleRate)

    def trigger(self):
        """maxiSample::trigger (C:597-600)."""
        self.position.upload(np.zeros(self.V))

    def setPosition(self, newPos):
        """maxiSample::setPosition (C:749-751): clamp(newPos,0,1)*length."""
        p = np.clip(np.broadcast_to(np.asarray(newPos, np.float64), (self.V,)), 0.0, 1.0) * self.length
        self.position.upload(p)

    def getLength(self):
        return self.length

    def clear(self):
        if self.d_samples:
            lib().mxg_sample_free(self.d_samples)
            self.d_samples = None

    def render(self, mode, N, a=None, start=None, end=None, out=None, per_sample=False):
        m = SAMPLE_MODES[mode] if isinstance(mode, str) else int(mode)
        if per_sample and not (isinstance(a, DeviceBuffer) or hasattr(a, "data_ptr")):
            a = DeviceBuffer.from_numpy(np.asarray(a, np.float64).reshape(N, self.V))
        da = None if a is None else (a if per_sample else _as_dev(a, self.V))
        ds = None if start is None else _as_dev(start, self.V)
        de = None if end is None else _as_dev(end, self.V)
        out = self._out(N, out)
        check(lib().mxg_sample_render(m, self.V, N, self.d_samples, self.length, self.mySampleRate,
                                      _ptr(da), int(per_sample), _ptr(ds), _ptr(de), self.position.ptr,
                                      _ptr(out), self.stream), "mxg_sample_render")
        self._keep = (da, ds, de)
        return out

    def render_trig(self, mode, trig, a=None, p0=None, p1=None, out=None, per_sample=False):
        """Modes 9-14: `trig` is the per-sample [N][V] trigger (or phasor) signal."""
        m = SAMPLE_MODES[mode] if isinstance(mode, str) else int(mode)
        if not (isinstance(trig, DeviceBuffer) or hasattr(trig, "data_ptr")):
            trig = DeviceBuffer.from_numpy(np.ascontiguousarray(trig, np.float64))
        N = trig.shape[0]
        if per_sample and not (isinstance(a, DeviceBuffer) or hasattr(a, "data_ptr")):
            a = DeviceBuffer.from_numpy(np.asarray(a, np.float64).reshape(N, self.V))
        da = None if a is None else (a if per_sample else _as_dev(a, self.V))
        d0 = None if p0 is None else _as_dev(p0, self.V)
        d1 = None if p1 is None else _as_dev(p1, self.V)
        tprev, tfirst = (self.phasor_prev, self.phasor_first) if m == 14 else (self.zx_prev, self.zx_first)
        out = self._out(N, out)
        check(lib().mxg_sample_render_trig(m, self.V, N, self.d_samples, self.length, self.mySampleRate,
                                           _ptr(trig), _ptr(da), int(per_sample), _ptr(d0), _ptr(d1),
                                           self.position.ptr, tprev.ptr, tfirst.ptr, _ptr(out), self.stream),
              "mxg_sample_render_trig")
        self._keep = (trig, da, d0, d1)
        return out

    def playOnZX(self, trig, **kw): return self.render_trig("playOnZX", trig, **kw)
    def playOnZXAtSpeed(self, trig, speed, **kw): return self.render_trig("playOnZXAtSpeed", trig, a=speed, **kw)

    def playOnZXAtSpeedFromOffset(self, trig, speed, offset, **kw):
        return self.render_trig("playOnZXAtSpeedFromOffset", trig, a=speed, p0=offset, **kw)

    def playOnZXAtSpeedBetweenPoints(self, trig, speed, offset, length, **kw):
        return self.render_trig("playOnZXAtSpeedBetweenPoints", trig, a=speed, p0=offset, p1=length, **kw)

    def loopSetPosOnZX(self, trig, pos, **kw): return self.render_trig("loopSetPosOnZX", trig, p0=pos, **kw)
    def playWithPhasor(self, pha, **kw): return self.render_trig("playWithPhasor", pha, **kw)

    def play(self, N, **kw): return self.render("play", N, **kw)
    def playOnce(self, N, **kw): return self.render("playOnce", N, **kw)
    def playLoop(self, start, end, N, **kw): return self.render("playLoop", N, start=start, end=end, **kw)
    def playUntil(self, end, N, **kw): return self.render("playUntil", N, end=end, **kw)
    def playAtSpeed(self, speed, N, **kw): return self.render("playAtSpeed", N, a=speed, **kw)
    def playOnceAtSpeed(self, speed, N, **kw): return self.render("playOnceAtSpeed", N, a=speed, **kw)

    def playUntilAtSpeed(self, end, speed, N, **kw):
        return self.render("playUntilAtSpeed", N, a=speed, end=end, **kw)

    def play4(self, frequency, start, end, N, **kw):
        return self.render("play4", N, a=frequency, start=start, end=end, **kw)

    def playAtSpeedBetweenPoints(self, frequency, start, end, N, **kw):
        return self.render("playAtSpeedBetweenPoints", N, a=frequency, start=start, end=end, **kw)

    def __del__(self):
        try:
            self.clear()
        except Exception:
            pass


DRUM_KINDS = {"kick": 0, "snare": 1, "hats": 2}
DRUM_INVERSE, DRUM_DISTORTION, DRUM_FILTER, DRUM_LIMITER = 1, 2, 4, 8


class _DrumBank(_Bank):
    """V x one drum class of src/libs/maxiSynths.h (mxg_drum_render, K21).  The setters take the reference's units; the members
    inverse / useDistortion / useFilter / useLimiter are one value for the bank (constant per launch).  State, carried from call to
    call (DeviceBuffers: numpy() / upload() go through mxg_memcpy_*): phase [V], dstate [2][V] and istate int64 [6][V] as
    maxiEnvBank's, fstate [3][V] (lores x, y | SVF v0z, v1, v2).  cutoff / resonance start at 0.0 where the reference leaves them
    uninitialised: lores clamps them to 10 Hz and 1."""
    KIND = None
    CTOR = None  # setAttack, setDecay (ms), setSustain, setRelease (ms), pitch
    USE_FILTER = False

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        V = self.V
        self.inverse, self.useDistortion, self.useFilter, self.useLimiter = False, False, self.USE_FILTER, False
        self.env = np.zeros((4, V))
        self.holdtime = np.ones(V, np.int64)
        self.pitch, self.distortion, self.gain = np.full(V, float(self.CTOR[4])), np.zeros(V), np.ones(V)
        self.cutoff, self.resonance = np.zeros(V), np.zeros(V)
        self.phase = DeviceBuffer(V)
        self.dstate = DeviceBuffer((2, V))
        self.istate = DeviceBuffer((6, V), np.int64)
        self.fstate = DeviceBuffer((3, V))
        self._dev = None
        self.setAttack(self.CTOR[0])
        self.setDecay(self.CTOR[1])
        self.setSustain(self.CTOR[2])
        self.setRelease(self.CTOR[3])

    def _set(self, name, value):
        getattr(self, name)[...] = np.asarray(value, getattr(self, name).dtype)
        self._dev = None

    def _coeff(self, which, ms):
        f = lib().mxg_env_coeff_host
        return np.array([f(which, m) for m in np.broadcast_to(np.asarray(ms, np.float64), (self.V,)).tolist()])

    def setAttack(self, ms): self.env[0] = self._coeff(0, ms); self._dev = None    # (0: divides by zero inside pow, attack = 1)
    def setDecay(self, ms): self.env[1] = self._coeff(1, ms); self._dev = None
    def setSustain(self, level): self.env[2] = np.asarray(level, np.float64); self._dev = None
    def setRelease(self, ms): self.env[3] = self._coeff(2, ms); self._dev = None
    def setHoldtime(self, samples): self._set("holdtime", samples)
    def setPitch(self, v): self._set("pitch", v)
    def setDistortion(self, v): self._set("distortion", v)
    def setCutoff(self, v): self._set("cutoff", v)
    def setResonance(self, v): self._set("resonance", v)
    def setGain(self, v): self._set("gain", v)

    def flags(self):
        return (DRUM_INVERSE if self.inverse else 0) | (DRUM_DISTORTION if self.useDistortion else 0) | \
               (DRUM_FILTER if self.useFilter else 0) | (DRUM_LIMITER if self.useLimiter else 0)

    def _coefs(self):
        c = np.zeros((3, self.V))
        check(lib().mxg_filter_coeffs_host(0, self.V, self.cutoff.ctypes.data, self.resonance.ctypes.data, c.ctypes.data), "mxg_filter_coeffs_host")
        return c

    def _params(self):
        if self._dev is None:
            self.host_coef = self._coefs()
            self._dev = [DeviceBuffer.from_numpy(a) for a in (self.pitch, self.env, self.holdtime, self.distortion, self.host_coef, self.gain)]
        return self._dev

    def render(self, N, trig=None, rand=None, out=None):
        """N x play() per voice.  trig: None (never triggered), or doubles [N] (one trigger signal for the bank) / [N][V], host or
        device -- non-zero: trigger() before that play(); a maxiClockBank's tick block fits.  rand: int32 [N][V], the rand() draws
        (snare and hats)."""
        V, N = self.V, int(N)
        tpv = 0
        if trig is not None:
            if not (isinstance(trig, DeviceBuffer) or hasattr(trig, "data_ptr")):
                trig = DeviceBuffer.from_numpy(np.ascontiguousarray(trig, np.float64))
            n = _fx_dev(trig, np.float64, "trig", (N, N * V))
            tpv = 1 if n == N * V else 0   # (V == 1: the two layouts are one)
        if rand is not None:
            if not (isinstance(rand, DeviceBuffer) or hasattr(rand, "data_ptr")):
                rand = DeviceBuffer.from_numpy(np.ascontiguousarray(rand, np.int32))
            _fx_dev(rand, np.int32, "rand", (N * V,))
        p = self._params()
        out = self._out(N, out)
        check(lib().mxg_drum_render(self.KIND, self.flags(), V, N, _ptr(trig), tpv, _ptr(rand), *[b.ptr for b in p], self.phase.ptr,
                                    self.dstate.ptr, self.istate.ptr, self.fstate.ptr, _ptr(out), self.stream), "mxg_drum_render")
        self._keep = (trig, rand)
        return out


class maxiKickBank(_DrumBank):
    """V x maxiKick: sinewave(pitch*envOut)*envOut -> fastAtanDist -> lores -> limiter."""
    KIND, CTOR = 0, (0, 1, 1.0, 500, 200.0)


class maxiSnareBank(_DrumBank):
    """V x maxiSnare: (triangle(pitch*(0.1+(envOut*0.85))) + noise())*envOut -> fastAtanDist -> lores (on by default) -> limiter."""
    KIND, CTOR, USE_FILTER = 1, (0, 20, 0.05, 300, 800.0), True


class maxiHatsBank(_DrumBank):
    """V x maxiHats: (sinebuf(pitch) + noise())*envOut -> fastAtanDist -> maxiSVF::play(output, 0., 0., 1., 0.) -> limiter.  The SVF's
    coefficients come from setFilterCutoff / setFilterResonance (the reference's filter.setCutoff / setResonance; the constructor:
    8000, 1); cutoff / resonance exist and, as in the reference, are never read."""
    KIND, CTOR = 2, (0, 20, 0.1, 300, 12000.0)

    def __init__(self, voices, stream=None):
        self.svf_cutoff, self.svf_resonance = np.full(int(voices), 8000.0), np.ones(int(voices))
        super().__init__(voices, stream)

    def setFilterCutoff(self, v): self._set("svf_cutoff", v)
    def setFilterResonance(self, v): self._set("svf_resonance", v)

    def _coefs(self):
        c = np.zeros((5, self.V))
        check(lib().mxg_svf_coeffs_host(self.V, self.svf_cutoff.ctypes.data, self.svf_resonance.ctypes.data, c.ctypes.data), "mxg_svf_coeffs_host")
        return c


class maxiClockBank(_Bank):
    """V x maxiClock (src/libs/maxiClock.h; mxg_clock_render): render(N) is N x ticker() per voice and returns the tick block
    [N][V] of 1.0 / 0.0, which a drum bank's render takes as `trig`.  State: clk [V] (timer.phase), playHead int64 [V]; lastCount
    int32 [V] is only read; currentCount int32 [V] is what the last ticker() left."""

    def __init__(self, voices, stream=None):
        super().__init__(voices, stream)
        V = self.V
        self.bpm, self.ticks = np.full(V, 120.0), np.ones(V, np.int32)
        self.clk = DeviceBuffer(V)
        self.playHead = DeviceBuffer(V, np.int64)
        self.lastCount = DeviceBuffer(V, np.int32)
        self.currentCount = DeviceBuffer(V, np.int32)
        self.setTempo(self.bpm)

    def setTempo(self, bpm):
        self.bpm = np.ascontiguousarray(np.broadcast_to(np.asarray(bpm, np.float64), (self.V,))).copy()
        self.bps = (self.bpm / 60.) * self.ticks
        self._dbps = DeviceBuffer.from_numpy(self.bps)

    def setTicksPerBeat(self, ticksPerBeat):
        self.ticks = np.ascontiguousarray(np.broadcast_to(np.asarray(ticksPerBeat, np.int32), (self.V,))).copy()
        self.setTempo(self.bpm)

    def setLastCount(self, n):
        self.lastCount.upload(np.broadcast_to(np.asarray(n, np.int32), (self.V,)))

    def render(self, N, out=None):
        out = self._out(int(N), out)
        check(lib().mxg_clock_render(self.V, int(N), self._dbps.ptr, self.clk.ptr, self.lastCount.ptr, self.playHead.ptr,
                                     self.currentCount.ptr, _ptr(out), self.stream), "mxg_clock_render")
        return out


ATOM_KINDS = {"gabor": 0, "raw": 1}
ATOM_ONSETS = {"block": 0, "sample": 1}


class maxiAtomBank:
    """S x (maxiAccelerator + maxiAtomBook + maxiAtomBookPlayer) (src/libs/maxiAtoms.h; K22, mxg_atoms_*).  Every stream owns a queue
    of at most `capacity` live atoms; `books` gives stream s its book as rows (position, length, amp, frequency, phase) -- what a
    maxiGaborAtom holds -- and `num_samples` the books' numSamples.  `raw` is the pool of floats that raw atoms (addAtom(flArr&)) read.

    fillNextBuffer(N) and play(N) return the float32 block [S][N] on the device, each stream's buffer contiguous; `out` is added to
    when accumulate is true (the reference's buffer[i] += ...).  onset "block" is the reference's: a due atom starts on the first sample
    of the block in which it falls due; "sample" (an extension) starts it on its own sample."""

    def __init__(self, streams, capacity=256, books=None, num_samples=None, raw=None, stream=None):
        check(lib().mxg_init(-1), "mxg_init")
        self.S, self.Q, self.stream = int(streams), int(capacity), stream
        starts = np.zeros(self.S + 1, np.int64)
        rows = [np.zeros((0, 5), np.float32)] * self.S
        if books is not None:
            assert len(books) == self.S, "one book per stream"
            rows = [np.asarray(b, np.float32).reshape(-1, 5) for b in books]
        for s, b in enumerate(rows):
            starts[s + 1] = starts[s] + len(b)
        book = np.ascontiguousarray(np.concatenate(rows, axis=0).T)
        ns = np.ascontiguousarray(np.broadcast_to(np.asarray(1 if num_samples is None else num_samples, np.uint32), (self.S,)))
        pool = np.zeros(0, np.float32) if raw is None else np.ascontiguousarray(raw, np.float32).ravel()
        self._h = lib().mxg_atoms_bank_create(self.S, self.Q, starts.ctypes.data, book.ctypes.data, ns.ctypes.data, pool.ctypes.data, len(pool))
        if not self._h:
            raise ValueError("mxg_atoms_bank_create: %s" % lib().mxg_last_error().decode())

    def appendRaw(self, floats):
        """Adds floats to the raw pool; returns where they start."""
        a = np.ascontiguousarray(floats, np.float32).ravel()
        off = ctypes.c_uint32(0)
        check(lib().mxg_atoms_raw_append(self._h, a.ctypes.data, len(a), ctypes.byref(off)), "mxg_atoms_raw_append")
        return off.value

    def _add(self, stream, kind, length, offset, par, raw_off):
        n = len(stream)
        a = [np.ascontiguousarray(x, t) for x, t in ((stream, np.int32), (kind, np.int32), (length, np.uint32), (offset, np.uint32),
                                                     (par, np.float32), (raw_off, np.uint32))]
        check(lib().mxg_atoms_add(self._h, n, *[x.ctypes.data for x in a]), "mxg_atoms_add")

    def addAtom(self, stream, raw_offset, length, offset=0):
        """addAtom(atom, offset) for raw atoms: arrays (or scalars) over the instances, queued in order."""
        stream = np.atleast_1d(np.asarray(stream, np.int32))
        n = len(stream)
        bc = lambda x, t: np.broadcast_to(np.asarray(x, t), (n,))
        self._add(stream, np.full(n, ATOM_KINDS["raw"]), bc(length, np.uint32), bc(offset, np.uint32), np.zeros((n, 4)), bc(raw_offset, np.uint32))

    def addGabor(self, stream, freq, length, startPhase=0.0, amp=1.0, offset=0, sampleRate=44100.0):
        """addAtom(createGabor(freq, sampleRate, length, startPhase, ., amp), offset): the atom is synthesised on the device."""
        stream = np.atleast_1d(np.asarray(stream, np.int32))
        n = len(stream)
        bc = lambda x, t: np.broadcast_to(np.asarray(x, t), (n,))
        par = np.stack([bc(freq, np.float32), bc(sampleRate, np.float32), bc(startPhase, np.float32), bc(amp, np.float32)], axis=1)
        self._add(stream, np.full(n, ATOM_KINDS["gabor"]), bc(length, np.uint32), bc(offset, np.uint32), par, np.zeros(n))

    def _step(self, fn, what, N, out, onset, accumulate):
        N = int(N)
        if out is None:
            out, accumulate = DeviceBuffer((self.S, N), np.float32, zero=False), False
        check(fn(self._h, N, _ptr(out), ATOM_ONSETS[onset] if isinstance(onset, str) else int(onset), int(bool(accumulate)), self.stream), what)
        return out

    def fillNextBuffer(self, N, out=None, onset="block", accumulate=True):
        return self._step(lib().mxg_atoms_fill, "mxg_atoms_fill", N, out, onset, accumulate)

    def play(self, N, out=None, onset="block", accumulate=True):
        return self._step(lib().mxg_atoms_play, "mxg_atoms_play", N, out, onset, accumulate)

    def state(self):
        """sampleIdx [S], atomIdx [S], and per stream the live entries (startTime, pos, size) in queue order.  Synchronises."""
        S, Q = self.S, self.Q
        idx, ai, nl = np.zeros(S, np.int64), np.zeros(S, np.uint32), np.zeros(S, np.int32)
        start, pos, size = np.zeros((S, Q), np.int64), np.zeros((S, Q), np.uint32), np.zeros((S, Q), np.uint32)
        check(lib().mxg_atoms_state(self._h, *[x.ctypes.data for x in (idx, ai, nl, start, pos, size)]), "mxg_atoms_state")
        return idx, ai, [[(int(start[s, k]), int(pos[s, k]), int(size[s, k])) for k in range(nl[s])] for s in range(S)]

    def free(self):
        if getattr(self, "_h", None):
            lib().mxg_atoms_bank_destroy(self._h)
            self._h = None

    def __del__(self):  # best effort
        try:
            self.free()
        except Exception:
            pass


LOOPER_PLAY = {"none": -1, "play": 0, "playLoop": 2}


class maxiLooperBank(_Bank):
    """R writable maxiSample slots on the device (mxg_sample_pool_alloc, K25): loopRecord (H:706-721) over blocks that other banks
    rendered, with one play head per slot -- play() or playLoop() -- fused behind the record head in the reference's call order,
    and normalise (C:1126-1137).  Bit-exact, and independent of how the samples are split into calls.  The one departure: a record
    index outside [0, len) reads 0, stores nothing and is counted in `dropped`.  slot_pointer(r) with length(r) is an ordinary
    sample pointer for maxiSampleBank, the sampler and the grain banks."""

    def __init__(self, slots, capacity, stream=None):
        super().__init__(slots, stream)
        self.R, self.cap = int(slots), int(capacity)
        st = ctypes.c_size_t(0)
        self.pool = lib().mxg_sample_pool_alloc(self.R, self.cap, ctypes.byref(st))
        if not self.pool:
            raise MemoryError(lib().mxg_last_error().decode())
        self.stride = st.value
        self.lengths = np.full(self.R, self.cap, np.uint64)
        self.len = DeviceBuffer(self.R, np.uint64)
        self._set_lengths()
        self.recpos, self.lagval = DeviceBuffer(self.R), DeviceBuffer(self.R)
        self.position = DeviceBuffer.from_numpy(self.lengths.astype(np.float64) - 1.0)
        self.mix, self.start, self.end = DeviceBuffer.from_numpy(np.full(self.R, 0.5)), DeviceBuffer(self.R), DeviceBuffer.from_numpy(np.ones(self.R))
        self.pstart, self.pend = DeviceBuffer(self.R), DeviceBuffer.from_numpy(np.ones(self.R))
        self.dropped = DeviceBuffer(self.R, np.uint32)

    def _set_lengths(self):
        check(lib().mxg_sample_pool_lengths(self.R, self.cap, self.lengths.ctypes.data, self.len.ptr), "mxg_sample_pool_lengths")

    def _vec(self, buf, x):
        buf.upload(np.broadcast_to(np.asarray(x, np.float64), (self.R,)))

    def length(self, r):
        return int(self.lengths[r])

    def slot_pointer(self, r):
        """Device address of element 0 of slot r."""
        return self.pool + 8 * self.stride * int(r)

    def setSample(self, slot, data):
        """maxiSample::setSample (H:670-678) on one slot: the data, zeros up to the capacity, position = len - 1."""
        a = np.ascontiguousarray(data, np.float64)
        if not 0 < a.size <= self.cap:
            raise ValueError("maxiLooperBank.setSample: %d samples do not fit a slot of %d" % (a.size, self.cap))
        full = np.zeros(self.cap)
        full[:a.size] = a
        check(lib().mxg_sync(), "mxg_sync")
        check(lib().mxg_memcpy_h2d(self.slot_pointer(slot), full.ctypes.data, full.nbytes, None), "mxg_memcpy_h2d")
        self.lengths[slot] = a.size
        self._set_lengths()
        pos = self.position.numpy()
        pos[slot] = a.size - 1.0
        self.position.upload(pos)

    def setLength(self, slot, n):
        """An empty (or kept) slot of n samples, as setSample of that many zeros would leave its length."""
        old = self.lengths.copy()
        self.lengths[slot] = int(n)
        try:
            self._set_lengths()
        except Exception:
            self.lengths = old
            raise

    def trigger(self):
        """maxiSample::trigger (C:597-600) on every slot: position = recordPosition = 0."""
        self._vec(self.position, 0.0)
        self._vec(self.recpos, 0.0)

    def setRecordMix(self, x):
        self._vec(self.mix, x)

    def setLoop(self, start, end):
        self._vec(self.start, start)
        self._vec(self.end, end)

    def setPlayLoop(self, start, end):
        self._vec(self.pstart, start)
        self._vec(self.pend, end)

    def loopRecord(self, x, enable, N=None, play="none", out=None):
        """N calls of loopRecord on every slot.  x: device block [N][R]; enable: a device block [N][R] (a gate block of another
        bank: non-zero = true), or a scalar / array [R] for the whole call.  play = "play" | "playLoop": the fused head's block
        [N][R] is returned."""
        N = int(x.shape[0] if N is None else N)
        _fx_input(x, self.R, N)
        mode = LOOPER_PLAY[play] if isinstance(play, str) else int(play)
        if isinstance(enable, DeviceBuffer) or hasattr(enable, "data_ptr"):
            eps = int(tuple(enable.shape) != (self.R,))
            if eps:
                _fx_dev(enable, np.float64, "enable", (N * self.R,))
        else:
            enable, eps = DeviceBuffer.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(enable, np.float64), (self.R,)))), 0
        if mode != -1:
            out = self._out(N, out)
        check(lib().mxg_looprec_render(self.R, N, self.pool, self.stride, self.cap, self.len.ptr, _ptr(x), _ptr(enable), eps, self.mix.ptr,
                                       self.start.ptr, self.end.ptr, self.recpos.ptr, self.lagval.ptr, mode, self.pstart.ptr, self.pend.ptr,
                                       self.position.ptr, _ptr(out) if mode != -1 else None, self.dropped.ptr, self.stream), "mxg_looprec_render")
        self._keep = (x, enable)   # (alive until the stream has run the launches)
        return out if mode != -1 else None

    def play(self, x, enable, N=None, out=None):
        return self.loopRecord(x, enable, N, "play", out)

    def playLoop(self, x, enable, N=None, out=None):
        return self.loopRecord(x, enable, N, "playLoop", out)

    def normalise(self, maxLevel=0.99):
        lv = DeviceBuffer.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(maxLevel, np.float64), (self.R,))))
        check(lib().mxg_sample_pool_normalise(self.R, self.pool, self.stride, self.cap, self.len.ptr, lv.ptr, self.stream), "mxg_sample_pool_normalise")
        self.sync()

    def download(self, slot):
        out = np.empty(self.length(slot))
        check(lib().mxg_sync(), "mxg_sync")
        check(lib().mxg_memcpy_d2h(out.ctypes.data, self.slot_pointer(slot), out.nbytes, None), "mxg_memcpy_d2h")
        return out

    def free(self):
        if getattr(self, "pool", None):
            lib().mxg_sample_pool_free(self.pool)
            self.pool = None

    def __del__(self):  # best effort
        try:
            self.free()
        except Exception:
            pass


LONG_SCAN_KINDS = {"dc": 0, "svf": 1, "biquad": 2, "lores": 3, "hires": 4, "lag": 5}
_LONG_SCAN_ROWS = {0: (1, 3), 1: (9, 3), 2: (5, 3), 3: (2, 5), 4: (2, 5), 5: (2, 1)}   # kind: (coefficient rows, state rows)


class maxiLongScanBank:
    """V (1 ... 4096) linear filters with block-constant coefficients over LONG signals, parallel in time (mxg_scan_long_render,
    K28): maxiDCBlocker, maxiSVF, maxiBiquad, maxiFilter::lores / hires or maxiLagExp, the signal [N][V] cut into chunks of 2048
    samples that a scan joins.  A tolerance mode (include/maxigpu.h: SCAN_LONG_RTOL per kind), not bit-exact against the
    sequential banks; the state rows are those of the sequential bank of the kind ([3][V], [5][V] or [1][V]), so set_state() /
    state() hand a stream over to one and back.  V = 1 filters a plain contiguous signal: a maxiLooperBank slot_pointer, an uploaded
    maxiSample.  The device is first touched by process(); the setters, state() before it and host() need none.

    A lores, hires or lag bank also takes coefficients that move every sample (mxg_scan_long_render_swept, K31): process_swept(x,
    coef_ps) / host_swept(x, coef_ps) with coef_ps [N][rows][V] from sweep_lores / sweep_hires / sweep_lag (or mxg_filter_render_coefs'
    own [N][3][V] array), chunks of 1024 samples, every lane and chunk carrying its own transition; SWEPT_RTOL per kind in
    include/maxigpu.h.  They share the state with process() / host() and with the sequential per-sample entry points, and need no
    setter; on a dc, svf or biquad bank they raise ValueError."""

    def __init__(self, voices, kind, stream=None):
        self.V = int(voices)
        self.kind = LONG_SCAN_KINDS[kind] if isinstance(kind, str) else int(kind)
        if self.kind not in _LONG_SCAN_ROWS:
            raise ValueError("maxiLongScanBank: kind %r is none of %s" % (kind, sorted(LONG_SCAN_KINDS)))
        self.stream = stream
        self.NC, self.NS = _LONG_SCAN_ROWS[self.kind]
        self.coef = None                      # host [NC][V]
        self._st = np.zeros((self.NS, self.V))
        self._dcoef = self._dst = None

    def _rows(self, *a):
        return [np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), (self.V,))) for x in a]

    def _set(self, kinds, coef):
        if self.kind not in kinds:
            raise ValueError("maxiLongScanBank: this setter is not of kind %d" % self.kind)
        self.coef = np.ascontiguousarray(coef, np.float64).reshape(self.NC, self.V)
        self._dcoef = None

    def setDC(self, R):
        self._set((0,), np.stack(self._rows(R)))

    def setSVF(self, cutoff, res, mixes):
        """maxiSVF::setCutoff / setResonance and the four mixes of play(w, lp, bp, hp, notch)."""
        cu, rs = self._rows(cutoff, res)
        c = np.zeros((5, self.V))
        check(lib().mxg_svf_coeffs_host(self.V, cu.ctypes.data, rs.ctypes.data, c.ctypes.data), "mxg_svf_coeffs_host")
        self._set((1,), np.concatenate([c, np.stack(self._rows(*mixes))]))

    def setBiquad(self, filtType, cutoff, Q, peakGain):
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(filtType, np.int32), (self.V,)))
        cu, q, g = self._rows(cutoff, Q, peakGain)
        c = np.zeros((5, self.V))
        check(lib().mxg_biquad_coeffs_host(self.V, t.ctypes.data, cu.ctypes.data, q.ctypes.data, g.ctypes.data, c.ctypes.data), "mxg_biquad_coeffs_host")
        self._set((2,), c)

    def setLores(self, cutoff, res):
        cu, rs = self._rows(cutoff, res)
        self._set((3,), filter_coeffs(0, cu, rs)[:2])

    def setHires(self, cutoff, res):
        cu, rs = self._rows(cutoff, res)
        self._set((4,), filter_coeffs(0, cu, rs)[:2])   # (lores and hires share c and r, C:456-461 / C:471-476)

    def setLag(self, alpha, alphaReciprocal=None):
        """maxiLagExp::init: alphaReciprocal = 1 - alpha unless given (the reference keeps the two independent)."""
        a, = self._rows(alpha)
        r = 1.0 - a if alphaReciprocal is None else self._rows(alphaReciprocal)[0]
        self._set((5,), np.stack([a, r]))

    def state(self):
        if self._dst is not None:
            self._st = self._dst.numpy()
        return self._st.copy()

    def set_state(self, st):
        self._st = np.ascontiguousarray(np.broadcast_to(np.asarray(st, np.float64), (self.NS, self.V))).copy()
        if self._dst is not None:
            self._dst.upload(self._st)

    def _need_coef(self):
        if self.coef is None:
            raise ValueError("maxiLongScanBank: no coefficients set")

    def process(self, x, N=None, out=None):
        """x: numpy [N][V] (uploaded), a DeviceBuffer / torch tensor [N][V], or a raw device address with N.  out: None (a new
        DeviceBuffer), the same kinds of device object, or x itself for in place.  Returns out."""
        self._need_coef()
        check(lib().mxg_init(-1), "mxg_init")
        if isinstance(x, np.ndarray):
            a = np.ascontiguousarray(x, np.float64).reshape(-1, self.V)
            x = DeviceBuffer.from_numpy(a)
        if N is None:
            if not hasattr(x, "shape"):
                raise ValueError("maxiLongScanBank.process: a raw pointer needs N")
            N = int(x.shape[0]) if len(x.shape) > 1 or self.V > 1 else int(np.prod(x.shape))
        N = int(N)
        if out is None:
            out = DeviceBuffer((N, self.V), np.float64, zero=False)
        if self._dcoef is None:
            self._dcoef = DeviceBuffer.from_numpy(self.coef)
        if self._dst is None:
            self._dst = DeviceBuffer.from_numpy(self._st)
        check(lib().mxg_scan_long_render(self.kind, self.V, N, _ptr(x), self._dcoef.ptr, self._dst.ptr, _ptr(out), self.stream), "mxg_scan_long_render")
        self._keep = (x, out)   # (alive until the stream has run the launches)
        return out

    def host(self, x, advance=False):
        """The host twin (mxg_scan_long_host, the device's bits) on numpy x [N][V] from the bank's state: (out, the state after it).
        advance: the bank's state becomes that state."""
        self._need_coef()
        a = np.ascontiguousarray(x, np.float64).reshape(-1, self.V)
        st, out = self.state(), np.empty_like(a)
        check(lib().mxg_scan_long_host(self.kind, self.V, a.shape[0], a.ctypes.data, self.coef.ctypes.data, st.ctypes.data, out.ctypes.data), "mxg_scan_long_host")
        if advance:
            self.set_state(st)
        return out, st

    def sync(self):
        check(lib().mxg_stream_sync(self.stream), "mxg_stream_sync")

    # ---- per-sample coefficients (mxg_scan_long_render_swept, K31) ---------------------------------------------------------------
    def _need_swept(self, what):
        if self.kind not in (3, 4, 5):
            raise ValueError("maxiLongScanBank.%s: kind %d has no swept form (lores, hires and lag have)" % (what, self.kind))

    def _coef_rows(self, coef_ps, N):
        """coef_ps [N][rows][V] -> rows (a raw pointer cannot say: it is taken as packed, 2 rows)."""
        if not hasattr(coef_ps, "shape"):
            return 2
        shape = tuple(int(s) for s in coef_ps.shape)
        n = int(np.prod(shape))
        if len(shape) == 3:
            return shape[1]
        if N and n % (N * self.V) == 0:
            return n // (N * self.V)
        raise ValueError("maxiLongScanBank: coef_ps is [N][rows][V]")

    def process_swept(self, x, coef_ps, N=None, out=None, coef_rows=None):
        """process() with the coefficients of every sample: coef_ps [N][rows][V] (sweep_lores / sweep_hires / sweep_lag make them on
        the host), rows 2 ... 8, rows 0-1 read -- numpy (uploaded), a DeviceBuffer / torch tensor, or a raw device address with
        coef_rows (default 2).  Shares the bank's state with process(); needs no constant coefficients set."""
        self._need_swept("process_swept")
        check(lib().mxg_init(-1), "mxg_init")
        if isinstance(x, np.ndarray):
            x = DeviceBuffer.from_numpy(np.ascontiguousarray(x, np.float64).reshape(-1, self.V))
        if N is None:
            if not hasattr(x, "shape"):
                raise ValueError("maxiLongScanBank.process_swept: a raw pointer needs N")
            N = int(x.shape[0]) if len(x.shape) > 1 or self.V > 1 else int(np.prod(x.shape))
        N = int(N)
        rows = int(coef_rows) if coef_rows is not None else self._coef_rows(coef_ps, N)
        if isinstance(coef_ps, np.ndarray):
            coef_ps = DeviceBuffer.from_numpy(np.ascontiguousarray(coef_ps, np.float64))
        if out is None:
            out = DeviceBuffer((N, self.V), np.float64, zero=False)
        if self._dst is None:
            self._dst = DeviceBuffer.from_numpy(self._st)
        check(lib().mxg_scan_long_render_swept(self.kind, self.V, N, _ptr(x), _ptr(coef_ps), rows, self._dst.ptr, _ptr(out), self.stream),
              "mxg_scan_long_render_swept")
        self._keep = (x, coef_ps, out)   # (alive until the stream has run the launches)
        return out

    def host_swept(self, x, coef_ps, advance=False):
        """The host twin (mxg_scan_long_swept_host, the device's bits) on numpy x [N][V], coef_ps [N][rows][V] from the bank's state:
        (out, the state after it).  advance: the bank's state becomes that state."""
        self._need_swept("host_swept")
        a = np.ascontiguousarray(x, np.float64).reshape(-1, self.V)
        c = np.ascontiguousarray(coef_ps, np.float64)
        rows = self._coef_rows(c, a.shape[0])
        st, out = self.state(), np.empty_like(a)
        check(lib().mxg_scan_long_swept_host(self.kind, self.V, a.shape[0], a.ctypes.data, c.ctypes.data, rows, st.ctypes.data, out.ctypes.data),
              "mxg_scan_long_swept_host")
        if advance:
            self.set_state(st)
        return out, st


def _sweep_filter(cutoff, res):
    cu, rs = np.broadcast_arrays(np.asarray(cutoff, np.float64), np.asarray(res, np.float64))
    if cu.ndim != 2:
        raise ValueError("sweep_lores / sweep_hires: cutoff and res broadcast to [N][V]")
    N, V = cu.shape
    cu, rs = np.ascontiguousarray(cu).ravel(), np.ascontiguousarray(rs).ravel()
    c = np.zeros((3, N * V))
    check(lib().mxg_filter_coeffs_host(0, N * V, cu.ctypes.data, rs.ctypes.data, c.ctypes.data), "mxg_filter_coeffs_host")
    return np.ascontiguousarray(c.reshape(3, N, V).transpose(1, 0, 2))


def sweep_lores(cutoff, res):
    """Per-sample lores coefficients for maxiLongScanBank.process_swept: cutoff, res [N][V] (or broadcastable to it) through
    mxg_filter_coeffs_host -> host [N][3][V], rows c, r, 0: what mxg_filter_render_coefs takes, unchanged."""
    return _sweep_filter(cutoff, res)


def sweep_hires(cutoff, res):
    """As sweep_lores (lores and hires share c and r, C:456-461 / C:471-476)."""
    return _sweep_filter(cutoff, res)


def sweep_lag(alpha, alphaReciprocal=None):
    """Per-sample maxiLagExp coefficients: alpha [N][V], alphaReciprocal = 1 - alpha unless given -> host [N][2][V]."""
    a = np.asarray(alpha, np.float64)
    r = 1.0 - a if alphaReciprocal is None else np.asarray(alphaReciprocal, np.float64)
    a, r = np.broadcast_arrays(a, r)
    if a.ndim != 2:
        raise ValueError("sweep_lag: alpha is [N][V]")
    return np.ascontiguousarray(np.stack([a, r], axis=1))
