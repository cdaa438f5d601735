"""Host-side mirror of maxiFFT / maxiMFCC (src/libs/maxiFFT.h, maxiMFCC.h) in batch form.

`maxiFFT.setup(fftSize, hopSize, windowSize)` keeps the reference's signature; instead of one
`process(sample)` call per audio sample, `process_signal(signal)` analyses every frame the
reference would have produced for that stream (same hop buffer semantics: the buffer starts
with windowSize-hopSize zeros, L/maxiFFT.cpp:56) in one launch.  `maxiMFCC.mfcc(mags)` takes the
[nframes, bins] magnitudes and returns [nframes, numCoeffs].
"""
import numpy as np

from ._lib import check, lib
from .banks import DeviceBuffer, _ptr


def frames_in_stream(nsamples, hopSize, windowSize):
    """How many times maxiFFT::process() reports a new frame over `nsamples` samples."""
    return 0 if nsamples < hopSize else (nsamples - hopSize) // hopSize + 1


def padded_stream(signal, hopSize, windowSize):
    """The signal as the hop buffer sees it: (windowSize-hopSize) zeros, then the samples."""
    signal = np.ascontiguousarray(signal, np.float32)
    return np.concatenate([np.zeros(windowSize - hopSize, np.float32), signal])


class maxiFFT:
    """maxiFFT (L/maxiFFT.h:45-113) over whole signals / frame batches."""
    NO_POLAR_CONVERSION, WITH_POLAR_CONVERSION = 0, 1

    def __init__(self, stream=None):
        self.plan = None
        self.stream = stream

    def setup(self, fftSize=1024, hopSize=512, windowSize=0):
        """L/maxiFFT.cpp:45-60."""
        self.close()
        check(lib().mxg_init(-1), "mxg_init")
        p = lib().mxg_fft_plan_create(fftSize, hopSize, windowSize)
        if not p:
            raise ValueError(lib().mxg_last_error().decode())
        self.plan = p
        self.fftSize, self.hopSize = fftSize, hopSize
        self.windowSize = max(windowSize, fftSize)  # :48
        self.bins = fftSize // 2

    def getNumBins(self): return self.bins
    def getFFTSize(self): return self.fftSize
    def getHopSize(self): return self.hopSize
    def getWindowSize(self): return self.windowSize

    def process_frames(self, d_signal, frame_stride, nframes, mode=1, want_complex=False):
        """Transform nframes frames starting every frame_stride samples in a device signal."""
        real = imag = mags = phases = None
        if mode == self.WITH_POLAR_CONVERSION:
            mags = DeviceBuffer((nframes, self.bins), np.float32, zero=False)
            phases = DeviceBuffer((nframes, self.bins), np.float32, zero=False)
        if want_complex or mode == self.NO_POLAR_CONVERSION:
            real = DeviceBuffer((nframes, self.bins), np.float32, zero=False)
            imag = DeviceBuffer((nframes, self.bins), np.float32, zero=False)
        check(lib().mxg_fft_batch(self.plan, _ptr(d_signal), frame_stride, nframes, _ptr(real), _ptr(imag),
                                  _ptr(mags), _ptr(phases), self.stream), "mxg_fft_batch")
        self.real, self.imag, self.magnitudes, self.phases = real, imag, mags, phases
        return nframes

    def process_signal(self, signal, mode=1, want_complex=False):
        """Every frame process() would report while consuming `signal` sample by sample."""
        n = frames_in_stream(len(signal), self.hopSize, self.windowSize)
        buf = DeviceBuffer.from_numpy(padded_stream(signal, self.hopSize, self.windowSize))
        self._keep = buf
        if n == 0:
            self.real = self.imag = self.magnitudes = self.phases = None
            return 0
        return self.process_frames(buf, self.hopSize, n, mode, want_complex)

    def getMagnitudes(self): return self.magnitudes
    def getPhases(self): return self.phases
    def getReal(self): return self.real
    def getImag(self): return self.imag

    def _features(self, mags, db=False, flatness=False, centroid=False):
        mags = self.magnitudes if mags is None else mags
        n = mags.shape[0]
        d = DeviceBuffer((n, self.bins), np.float32, zero=False) if db else None
        f = DeviceBuffer(n, np.float32, zero=False) if flatness else None
        c = DeviceBuffer(n, np.float32, zero=False) if centroid else None
        check(lib().mxg_fft_features(self.plan, _ptr(mags), n, _ptr(d), _ptr(f), _ptr(c), self.stream),
              "mxg_fft_features")
        return d, f, c

    def magsToDB(self, mags=None):
        """maxiFFT::magsToDB (L/maxiFFT.cpp:101-111) for every frame: [nframes, bins] fp32."""
        return self._features(mags, db=True)[0]

    def spectralFlatness(self, mags=None):
        """maxiFFT::spectralFlatness (L/maxiFFT.cpp:113-123) per frame."""
        return self._features(mags, flatness=True)[1]

    def spectralCentroid(self, mags=None):
        """maxiFFT::spectralCentroid (L/maxiFFT.cpp:125-132) per frame."""
        return self._features(mags, centroid=True)[2]

    def close(self):
        if self.plan:
            lib().mxg_fft_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class maxiMFCC:
    """maxiMFCCAnalyser<double> (L/maxiMFCC.h:41-211) over batches of spectra."""
    EXACT, MFMA = 0, 1

    def __init__(self, stream=None):
        self.plan = None
        self.stream = stream

    def setup(self, numBins, numFilters, numCoeffs, minFreq, maxFreq):
        """L/maxiMFCC.h:56-75."""
        self.close()
        p = lib().mxg_mfcc_plan_create(numBins, numFilters, numCoeffs, minFreq, maxFreq)
        if not p:
            raise ValueError(lib().mxg_last_error().decode())
        self.plan = p
        self.numBins, self.numFilters, self.numCoeffs = numBins, numFilters, numCoeffs

    def tables(self):
        W = np.zeros(self.numFilters * self.numBins)
        D = np.zeros(self.numCoeffs * self.numFilters)
        used = lib().mxg_mfcc_plan_tables(self.plan, W.ctypes.data, D.ctypes.data)
        return W, D, used

    def mfcc(self, mags, nframes=None, mag_stride=None, method=0, want_bands=False):
        nframes = mags.shape[0] if nframes is None else nframes
        mag_stride = self.numBins if mag_stride is None else mag_stride
        out = DeviceBuffer((nframes, self.numCoeffs), np.float64, zero=False)
        raw = bands = None
        if want_bands:
            raw = DeviceBuffer((nframes, self.numFilters), np.float64, zero=False)
            bands = DeviceBuffer((nframes, self.numFilters), np.float64, zero=False)
        check(lib().mxg_mfcc_batch(self.plan, _ptr(mags), mag_stride, nframes, _ptr(raw), _ptr(bands),
                                   _ptr(out), method, self.stream), "mxg_mfcc_batch")
        self.melraw, self.melBands = raw, bands
        return out

    def mfcc_of_frames(self, fft, signal, nframes, frame_stride=None, want_mags=False, want_bands=False):
        """maxiFFT(1024) magnitudes -> mfcc() for `nframes` frames of `signal` in ONE kernel (mxg_fft_mfcc_batch):
        the per-frame body of mfcctest.cpp:21-32.  `fft` is a maxiFFT set up for 1024 points; returns the [nframes,
        numCoeffs] DeviceBuffer; .mags / .melraw / .melBands hold the optional outputs."""
        frame_stride = fft.fftSize if frame_stride is None else frame_stride
        out = DeviceBuffer((nframes, self.numCoeffs), np.float64, zero=False)
        mags = DeviceBuffer((nframes, self.numBins), np.float32, zero=False) if want_mags else None
        raw = bands = None
        if want_bands:
            raw = DeviceBuffer((nframes, self.numFilters), np.float64, zero=False)
            bands = DeviceBuffer((nframes, self.numFilters), np.float64, zero=False)
        check(lib().mxg_fft_mfcc_batch(fft.plan, self.plan, _ptr(signal), frame_stride, nframes, _ptr(mags), _ptr(raw),
                                       _ptr(bands), _ptr(out), self.stream), "mxg_fft_mfcc_batch")
        self.mags, self.melraw, self.melBands = mags, raw, bands
        return out

    def close(self):
        if self.plan:
            lib().mxg_mfcc_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class maxiBarkBatch:
    """maxiBarkScaleAnalyser<double> (L/maxiBark.h, alias maxiBark) over batches of spectra: specificLoudness /
    relativeLoudness / totalLoudness of every row of [nframes, >= bufferSize / 2] fp32 magnitudes (mxg_bark_batch)."""
    NUM_BARK_BANDS = 24

    def __init__(self, stream=None):
        self.plan = None
        self.stream = stream

    def setup(self, sampleRate, bufferSize):
        """L/maxiBark.h:40-62; the limits are built on the host and need no device."""
        self.close()
        p = lib().mxg_bark_plan_create(int(sampleRate), int(bufferSize))
        if not p:
            raise ValueError(lib().mxg_last_error().decode())
        self.plan = p
        self.sampleRate, self.bufferSize, self.specSize = int(sampleRate), int(bufferSize), int(bufferSize) // 2

    def limits(self):
        lim = np.zeros(25, np.int32)
        check(lib().mxg_bark_plan_limits(self.plan, lim.ctypes.data), "mxg_bark_plan_limits")
        return lim

    def analyse(self, mags, nframes=None, stride=None, bandsum=False, specific=True, relative=False, total=False):
        """-> dict of the DeviceBuffers asked for: bandsum / specific / relative [nframes, 24], total [nframes]."""
        nframes = mags.shape[0] if nframes is None else nframes
        stride = self.specSize if stride is None else stride
        want = {"bandsum": bandsum, "specific": specific, "relative": relative, "total": total}
        out = {k: DeviceBuffer(nframes if k == "total" else (nframes, 24), np.float64, zero=False) for k, w in want.items() if w}
        check(lib().mxg_bark_batch(self.plan, _ptr(mags), stride, nframes, _ptr(out.get("bandsum")), _ptr(out.get("specific")),
                                   _ptr(out.get("relative")), _ptr(out.get("total")), self.stream), "mxg_bark_batch")
        return out

    def specificLoudness(self, mags): return self.analyse(mags)["specific"]
    def relativeLoudness(self, mags): return self.analyse(mags, specific=False, relative=True)["relative"]
    def totalLoudness(self, mags): return self.analyse(mags, specific=False, total=True)["total"]

    def close(self):
        if self.plan:
            lib().mxg_bark_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class maxiOctaveBatch:
    """maxiFFTOctaveAnalyzer (L/maxiFFT.h:162-205) for `streams` analysers: calculate(mags) takes [streams * frames, >= nSpectrum]
    fp32 magnitudes (stream-major) and returns the averages and peaks of every frame; peaks / peakHoldTimes are carried."""

    def __init__(self, streams=1, stream=None):
        self.plan = None
        self.S = int(streams)
        self.stream = stream
        self.peakHoldTime, self.peakDecayRate = 0, 0.9            # L/maxiFFT.cpp:255-258
        self.linearEQIntercept, self.linearEQSlope = 1.0, 0.0

    def setup(self, samplingRate, nSpectrum, nAveragesPerOctave):
        """L/maxiFFT.cpp:207-259; a fresh bank's peaks and hold counters are zeros."""
        self.close()
        p = lib().mxg_octave_plan_create(float(samplingRate), int(nSpectrum), int(nAveragesPerOctave))
        if not p:
            raise ValueError(lib().mxg_last_error().decode())
        self.plan = p
        self.nSpectrum = int(nSpectrum)
        self.nAverages = lib().mxg_octave_plan_averages(p)
        self.spe2avg = np.zeros(self.nSpectrum, np.int32)
        check(lib().mxg_octave_plan_map(p, self.spe2avg.ctypes.data), "mxg_octave_plan_map")
        self.peaks = self.peakHoldTimes = None

    def calculate(self, mags, frames=None, stride=None, peaks=True):
        """-> (averages, peaks or None), DeviceBuffers [streams * frames, nAverages]."""
        frames = mags.shape[0] // self.S if frames is None else frames
        stride = self.nSpectrum if stride is None else stride
        avg = DeviceBuffer((self.S * frames, self.nAverages), np.float32, zero=False)
        pk = None
        if peaks:
            if self.peaks is None:
                self.peaks = DeviceBuffer((self.S, self.nAverages), np.float32)
                self.peakHoldTimes = DeviceBuffer((self.S, self.nAverages), np.int32)
            pk = DeviceBuffer((self.S * frames, self.nAverages), np.float32, zero=False)
        check(lib().mxg_octave_batch(self.plan, _ptr(mags), stride, self.S, frames, self.linearEQIntercept, self.linearEQSlope,
                                     int(self.peakHoldTime), self.peakDecayRate, _ptr(avg), _ptr(pk),
                                     _ptr(self.peaks) if peaks else None, _ptr(self.peakHoldTimes) if peaks else None, self.stream),
              "mxg_octave_batch")
        return avg, pk

    def close(self):
        if self.plan:
            lib().mxg_octave_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class maxiIFFT:
    """maxiIFFT (L/maxiFFT.h:117-156, SPECTRUM mode) over batches of spectra: `process_frames(mags, phases)`
    returns the nframes*hopSize samples `process()` would return when called hopSize times per spectrum;
    the overlap-add buffer is carried between calls."""
    SPECTRUM, COMPLEX = 0, 1

    def __init__(self, stream=None):
        self.plan = None
        self.stream = stream

    def setup(self, fftSize=1024, hopSize=512, windowSize=0):
        self.close()
        p = lib().mxg_ifft_plan_create(int(fftSize), int(hopSize), int(windowSize))
        if not p:
            raise ValueError(lib().mxg_last_error().decode())
        self.plan = p
        self.fftSize, self.hopSize, self.bins = fftSize, hopSize, fftSize // 2
        self.windowSize = windowSize if windowSize else fftSize   # L/maxiFFT.cpp:143
        self.buffer = DeviceBuffer(fftSize, np.float32)           # member `buffer`, zero-filled by setup()
        self.ifftOut = None

    def getNumBins(self): return self.bins

    def process_frames(self, mags, phases, keep_ifft=False):
        dm = mags if isinstance(mags, DeviceBuffer) or hasattr(mags, "data_ptr") else \
            DeviceBuffer.from_numpy(np.ascontiguousarray(mags, np.float32))
        dp = phases if isinstance(phases, DeviceBuffer) or hasattr(phases, "data_ptr") else \
            DeviceBuffer.from_numpy(np.ascontiguousarray(phases, np.float32))
        n = dm.shape[0]
        out = DeviceBuffer(n * self.hopSize, np.float32, zero=False)
        self.ifftOut = DeviceBuffer((n, self.fftSize), np.float32, zero=False) if keep_ifft else None
        check(lib().mxg_ifft_batch(self.plan, _ptr(dm), _ptr(dp), n, self.buffer.ptr, _ptr(out), _ptr(self.ifftOut),
                                   self.stream), "mxg_ifft_batch")
        self._keep = (dm, dp)
        return out

    def close(self):
        if self.plan:
            lib().mxg_ifft_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class maxiConvolve:
    """maxiConvolve (L/maxiConvolve.cpp): partitioned convolution.  `setup(amplitudes, fftsize, hopsize)` takes the
    impulse as the loaded maxiSample holds it (the reference loads it from a file name); `play(x, mode)` renders what
    play(w) returns for every sample of x (a whole number of fftsize blocks), state carried between calls.
    mode 0 = as the reference computes (its COMPLEX-mode maxiIFFT never sees the sums: silence), 1 = as intended."""

    def __init__(self, stream=None):
        self.h = None
        self.stream = stream

    def setup(self, amplitudes, fftsize=1024, hopsize=256, position0=None):
        self.close()
        a = np.ascontiguousarray(amplitudes, np.float64)
        pos = float(a.size if position0 is None else position0)   # load()/read() leave the play head at size (C:681)
        h = lib().mxg_convolve_create(a.ctypes.data, a.size, pos, fftsize, hopsize)
        if not h:
            raise ValueError(lib().mxg_last_error().decode())
        self.h, self.fftsize, self.hopsize, self.bins = h, fftsize, hopsize, fftsize // 2
        self.frames = lib().mxg_convolve_frames(h)

    def impulse(self):
        r = np.zeros((self.frames, self.bins), np.float32)
        i = np.zeros((self.frames, self.bins), np.float32)
        check(lib().mxg_convolve_impulse(self.h, r.ctypes.data, i.ctypes.data), "mxg_convolve_impulse")
        return r, i

    def play(self, x, mode=0, out=None):
        if not (isinstance(x, DeviceBuffer) or hasattr(x, "data_ptr")):
            x = DeviceBuffer.from_numpy(np.ascontiguousarray(x, np.float32))
        n = int(np.prod(x.shape))
        assert n % self.fftsize == 0, "a whole number of fftsize blocks"
        out = out if out is not None else DeviceBuffer(n, np.float32, zero=False)
        check(lib().mxg_convolve_play(self.h, _ptr(x), n // self.fftsize, _ptr(out), mode, self.stream), "mxg_convolve_play")
        self._keep = x
        return out

    def reset(self):
        check(lib().mxg_convolve_reset(self.h), "mxg_convolve_reset")

    def close(self):
        if getattr(self, "h", None):
            lib().mxg_convolve_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class maxiConvolveBank:
    """A bank of V maxiConvolve objects over I shared impulses (mxg_convolve_bank_*, kernel K24).  `impulses` is a list of I
    amplitude arrays (as maxiConvolve.setup takes one), `imp_of[v]` the impulse of stream v; one fftsize / hopsize for the bank.
    Stream v equals, bit for bit, a maxiConvolve set up with impulses[imp_of[v]] and fed stream v's input, state carried between
    calls.  `play(x, mode)` takes float32 [V, nblocks * fftsize]; `play_nv(x, mode)` the layout the other banks speak, float64
    [nblocks * fftsize, V] (narrowed with a plain float cast on the way in).  `frames[i]` is impulse i's frame count."""

    def __init__(self, V, impulses, imp_of, fftsize=1024, hopsize=256, positions0=None, stream=None):
        self.h = None
        self.stream = stream
        amps = [np.ascontiguousarray(a, np.float64) for a in impulses]
        I = len(amps)
        ptrs = np.array([a.ctypes.data for a in amps], np.uintp)
        lens = np.array([a.size for a in amps], np.uintp)
        pos = np.array([float(a.size) for a in amps] if positions0 is None else positions0, np.float64)  # load() leaves the head at size
        of = np.ascontiguousarray(imp_of, np.int32)
        if of.size != V or pos.size != I:
            raise ValueError("maxiConvolveBank: imp_of needs V entries and positions0 one per impulse")
        h = lib().mxg_convolve_bank_create(V, I, ptrs.ctypes.data, lens.ctypes.data, pos.ctypes.data, of.ctypes.data, fftsize, hopsize)
        if not h:
            raise ValueError(lib().mxg_last_error().decode())
        self.h, self.V, self.I, self.fftsize, self.hopsize, self.bins = h, V, I, fftsize, hopsize, fftsize // 2
        self.imp_of = of
        self.frames = [lib().mxg_convolve_bank_frames(h, i) for i in range(I)]

    def impulse(self, i):
        r = np.zeros((self.frames[i], self.bins), np.float32)
        im = np.zeros((self.frames[i], self.bins), np.float32)
        check(lib().mxg_convolve_bank_impulse(self.h, i, r.ctypes.data, im.ctypes.data), "mxg_convolve_bank_impulse")
        return r, im

    def _call(self, fn, name, x, dtype, mode, out):
        if not (isinstance(x, DeviceBuffer) or hasattr(x, "data_ptr")):
            x = DeviceBuffer.from_numpy(np.ascontiguousarray(x, dtype))
        shape = tuple(x.shape)
        n = int(np.prod(shape)) // self.V
        assert n * self.V == int(np.prod(shape)) and n % self.fftsize == 0, "V streams of a whole number of fftsize blocks"
        out = out if out is not None else DeviceBuffer(shape, dtype, zero=False)
        check(fn(self.h, _ptr(x), n // self.fftsize, _ptr(out), mode, self.stream), name)
        self._keep = x
        return out

    def play(self, x, mode=0, out=None):
        return self._call(lib().mxg_convolve_bank_play, "mxg_convolve_bank_play", x, np.float32, mode, out)

    def play_nv(self, x, mode=0, out=None):
        return self._call(lib().mxg_convolve_bank_play_nv, "mxg_convolve_bank_play_nv", x, np.float64, mode, out)

    def reset(self):
        check(lib().mxg_convolve_bank_reset(self.h), "mxg_convolve_bank_reset")

    def close(self):
        if getattr(self, "h", None):
            lib().mxg_convolve_bank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def spectral_bank_plan(fftSize, hopSize, windowSize, fft_fill, ifft_pos, N):
    """mxg_spectral_bank_plan_host: what a call of N samples does to a maxiFFTBank at `fft_fill` and a maxiIFFTBank at `ifft_pos`
    -> (frames, points, first_is_held, new_fill, new_pos).  Integer host code, no device."""
    import ctypes
    F, C = ctypes.c_size_t(0), ctypes.c_size_t(0)
    held, nf, npos = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    st = lib().mxg_spectral_bank_plan_host(int(fftSize), int(hopSize), int(windowSize), int(fft_fill), int(ifft_pos), int(N),
                                           ctypes.addressof(F), ctypes.addressof(C), ctypes.addressof(held), ctypes.addressof(nf),
                                           ctypes.addressof(npos))
    if st < 0:
        raise ValueError(lib().mxg_last_error().decode())
    return F.value, C.value, held.value, nf.value, npos.value


class maxiFFTBank:
    """V maxiFFT objects after setup(fftSize, hopSize, windowSize), fed in lock-step (mxg_fft_bank_*, kernel K29).  `process(x)`
    takes what a bank rendered, float64 [N, V] for any N, and returns the frames(N) frames every stream completes inside the call
    as a dict of float32 [V * F, bins] DeviceBuffers (`want` names them: real / imag / mags / phases), rows frame-major
    (layout 0: row = f * V + v) or stream-major (layout 1: row = v * F + f); state is carried between calls on the device."""
    FRAME_MAJOR, STREAM_MAJOR = 0, 1

    def __init__(self, V, fftSize=1024, hopSize=512, windowSize=0, stream=None):
        self.h = None
        self.stream = stream
        h = lib().mxg_fft_bank_create(int(V), int(fftSize), int(hopSize), int(windowSize))
        if not h:
            raise ValueError(lib().mxg_last_error().decode())
        self.h, self.V, self.fftSize, self.hopSize, self.windowSize, self.bins = h, int(V), fftSize, hopSize, windowSize, fftSize // 2

    @property
    def pos(self):
        return lib().mxg_fft_bank_pos(self.h)

    def frames(self, N):
        return spectral_bank_plan(self.fftSize, self.hopSize, self.windowSize, self.pos, 0, N)[0]

    def process(self, x, N=None, want=("mags", "phases"), layout=0):
        if not (isinstance(x, DeviceBuffer) or hasattr(x, "data_ptr")):
            x = DeviceBuffer.from_numpy(np.ascontiguousarray(x, np.float64))
        N = int(np.prod(tuple(x.shape))) // self.V if N is None else int(N)
        F = self.frames(N)
        out = {k: DeviceBuffer((self.V * F, self.bins), np.float32, zero=False) for k in want}
        check(lib().mxg_fft_bank_process(self.h, _ptr(x), N, int(layout), _ptr(out.get("real")), _ptr(out.get("imag")),
                                         _ptr(out.get("mags")), _ptr(out.get("phases")), self.stream), "mxg_fft_bank_process")
        self._keep = x
        return out

    def reset(self):
        check(lib().mxg_fft_bank_reset(self.h), "mxg_fft_bank_reset")

    def close(self):
        if getattr(self, "h", None):
            lib().mxg_fft_bank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class maxiIFFTBank:
    """V maxiIFFT objects after setup(fftSize, hopSize, windowSize), called once per sample (mxg_ifft_bank_*, kernel K29).
    `process(a, b, N)` returns float64 [N, V], the layout the banks speak.  form SPECTRUM: a = magnitudes, b = phases; CARTESIAN:
    a = real, b = imag.  Rows are float32 [V * nrows, bins] in either layout of maxiFFTBank.  rows DIRECT: one row per consumption
    point, rows(N) of them; AFTER_FFT: the rows a maxiFFTBank of the same hop, created at the same time, returned for the same N
    (the per-sample loop of ffttest.cpp: a point takes the last frame completed before it, held across calls)."""
    SPECTRUM, CARTESIAN = 0, 1
    DIRECT, AFTER_FFT = 0, 1

    def __init__(self, V, fftSize=1024, hopSize=512, windowSize=0, stream=None):
        self.h = None
        self.stream = stream
        h = lib().mxg_ifft_bank_create(int(V), int(fftSize), int(hopSize), int(windowSize))
        if not h:
            raise ValueError(lib().mxg_last_error().decode())
        self.h, self.V, self.fftSize, self.hopSize, self.windowSize, self.bins = h, int(V), fftSize, hopSize, windowSize, fftSize // 2

    @property
    def pos(self):
        return lib().mxg_ifft_bank_pos(self.h)

    def rows(self, N, rows=0):
        """Rows per stream a call of N samples takes."""
        p = self.pos
        F, C = spectral_bank_plan(self.fftSize, self.hopSize, 0, p, p, N)[:2]
        return F if rows == self.AFTER_FFT else C

    def process(self, a, b, N, form=0, rows=0, layout=0, out=None):
        nrows = self.rows(N, rows)
        if nrows:
            a = a if isinstance(a, DeviceBuffer) or hasattr(a, "data_ptr") else DeviceBuffer.from_numpy(np.ascontiguousarray(a, np.float32))
            b = b if isinstance(b, DeviceBuffer) or hasattr(b, "data_ptr") else DeviceBuffer.from_numpy(np.ascontiguousarray(b, np.float32))
            assert int(np.prod(tuple(a.shape))) == self.V * nrows * self.bins, "V * rows(N) rows of bins values"
        out = out if out is not None else DeviceBuffer((int(N), self.V), np.float64, zero=False)
        check(lib().mxg_ifft_bank_process(self.h, int(form), int(rows), int(layout), _ptr(a) if nrows else None,
                                          _ptr(b) if nrows else None, nrows, int(N), _ptr(out), self.stream), "mxg_ifft_bank_process")
        self._keep = (a, b)
        return out

    def buffers(self):
        """The V carried buffers, float32 [V, fftSize], as the reference's objects would hold them."""
        check(lib().mxg_sync(), "mxg_sync")
        out = np.empty((self.V, self.fftSize), np.float32)
        check(lib().mxg_memcpy_d2h(out.ctypes.data, lib().mxg_ifft_bank_buffer(self.h), out.nbytes, None), "mxg_memcpy_d2h")
        return out

    def reset(self):
        check(lib().mxg_ifft_bank_reset(self.h), "mxg_ifft_bank_reset")

    def close(self):
        if getattr(self, "h", None):
            lib().mxg_ifft_bank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
