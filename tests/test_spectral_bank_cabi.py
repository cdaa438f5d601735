"""CPU (-m "not gpu"): the maxiFFTBank / maxiIFFTBank entry points (kernel K29) are declared in include/maxigpu.h, exported by the
library and bound by the Python package; mxg_spectral_bank_plan_host -- the integer arithmetic both _process calls run -- against
a per-sample walk of the reference's `pos` logic (L/maxiFFT.cpp:67-87 and :155-189); the after-FFT row rule against ffttest.cpp's
loop simulated on row indices; creation refuses each bad argument by name before any device call."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ["mxg_fft_bank_create", "mxg_fft_bank_destroy", "mxg_fft_bank_reset", "mxg_fft_bank_pos", "mxg_fft_bank_process",
       "mxg_ifft_bank_create", "mxg_ifft_bank_destroy", "mxg_ifft_bank_reset", "mxg_ifft_bank_pos", "mxg_ifft_bank_buffer",
       "mxg_ifft_bank_process", "mxg_spectral_bank_plan_host"]

SIZES = [(8, 8, 0), (64, 16, 0), (64, 24, 0), (64, 16, 48), (1024, 256, 0), (1024, 1024, 0)]


def splits(hop):
    return [[1, 15, 16, 17, 100, 0, 7, 300], [hop] * 5, [hop - 1, 1, hop + 1], [2000]]


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert len(m._lib.SIGNATURES["mxg_fft_bank_process"][1]) == 9
    assert len(m._lib.SIGNATURES["mxg_ifft_bank_process"][1]) == 10
    assert len(m._lib.SIGNATURES["mxg_spectral_bank_plan_host"][1]) == 11
    for cls, methods in ((m.maxiFFTBank, ("process", "frames", "reset")), (m.maxiIFFTBank, ("process", "rows", "buffers", "reset"))):
        for method in methods:
            assert callable(getattr(cls, method)), (cls, method)
    hpp = open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read()
    assert re.search(r"\bclass maxiFFTBank\b", hpp) and "mxg_fft_bank_process" in hpp
    assert re.search(r"\bclass maxiIFFTBank\b", hpp) and "mxg_ifft_bank_process" in hpp and "mxg_spectral_bank_plan_host" in hpp


class Walk:
    """maxiFFT::process and maxiIFFT::process reduced to their `pos` logic, one sample at a time, the FFT first as in ffttest.cpp's
    loop.  `latest` is the index of the last frame the FFT completed (-1: none yet, the zeros setup leaves in magnitudes / phases)."""

    def __init__(self, fs, hop, win):
        self.W = max(win, fs)                                  # :48
        self.hop = hop
        self.fpos = self.W - hop                               # :55
        self.ipos = 0                                          # :149
        self.nframes = 0
        self.latest = -1

    def call(self, N):
        """-> (global indices of the frames completed, the frame each consumption point saw)"""
        frames, seen = [], []
        for _ in range(N):
            self.fpos += 1                                     # :67
            if self.fpos == self.W:                            # :69
                frames.append(self.nframes)
                self.latest = self.nframes
                self.nframes += 1
                self.fpos = self.W - self.hop                  # :87
            if self.ipos == 0:                                 # :155
                seen.append(self.latest)
            self.ipos += 1                                     # :187
            if self.ipos == self.hop:
                self.ipos = 0
        return frames, seen


@pytest.mark.parametrize("fs,hop,win", SIZES)
def test_plan_host_against_per_sample_walk(fs, hop, win):
    import maximilian_amd as m
    for calls in splits(hop):
        w = Walk(fs, hop, win)
        fill = pos = 0
        for N in calls:
            first_on_point = w.ipos == 0
            frames, seen = w.call(N)
            F, C, held, nfill, npos = m.spectral_bank_plan(fs, hop, win, fill, pos, N)
            assert (F, C) == (len(frames), len(seen)), (calls, N)
            assert held == int(first_on_point and len(seen) > 0), (calls, N)
            assert nfill == w.fpos - (w.W - hop) and 0 <= nfill < hop, (calls, N)
            assert npos == w.ipos, (calls, N)
            fill, pos = nfill, npos


@pytest.mark.parametrize("fs,hop,win", SIZES)
def test_after_fft_rule_names_the_frame_ffttest_sees(fs, hop, win):
    """The caller passes the rows the FFT bank emitted for the same N; point j takes rows[j] when the call is entered between two
    points and rows[j - 1] when it is entered on one, index -1 being the held spectrum = the last row passed before (or the zeros
    of setup, written -1 here).  That must be the frame ffttest's loop has in `magnitudes` at that sample."""
    import maximilian_amd as m
    for calls in splits(hop):
        w = Walk(fs, hop, win)
        pos, held_row = 0, -1
        for N in calls:
            rows, seen = w.call(N)
            F, C, first_is_held, _, npos = m.spectral_bank_plan(fs, hop, win, pos, pos, N)
            assert F == len(rows) and C == len(seen)
            for j in range(C):
                r = j - first_is_held
                assert -1 <= r < F, (calls, N, j)
                assert (held_row if r < 0 else rows[r]) == seen[j], (calls, N, j)
            if rows:
                held_row = rows[-1]
            pos = npos


def test_plan_host_refuses_bad_arguments():
    import maximilian_amd as m
    for args, word in (((1000, 16, 0, 0, 0, 5), "fftSize"), ((64, 0, 0, 0, 0, 5), "hopSize"), ((64, 65, 0, 0, 0, 5), "hopSize"),
                       ((64, 16, 65, 0, 0, 5), "windowSize"), ((64, 16, 0, 16, 0, 5), "fft_fill"), ((64, 16, 0, 0, -1, 5), "ifft_pos")):
        with pytest.raises(ValueError, match=word):
            m.spectral_bank_plan(*args)
    assert m.lib().mxg_spectral_bank_plan_host(64, 16, 0, 3, 5, 100, None, None, None, None, None) == 0


@pytest.mark.parametrize("kind", ["fft", "ifft"])
def test_create_refuses_bad_arguments_by_name(kind):
    """Every refusal happens before the device is touched: the message names the argument, with or without a device."""
    import maximilian_amd as m
    lib = m.lib()
    create = getattr(lib, "mxg_%s_bank_create" % kind)

    def refused(V, fs, hop, win, word):
        assert not create(V, fs, hop, win)
        msg = lib.mxg_last_error().decode()
        assert ("mxg_%s_bank_create" % kind) in msg and word in msg, msg

    refused(0, 1024, 256, 0, "V = 0")
    refused(3, 1000, 256, 0, "fftSize")
    refused(3, 4, 2, 0, "fftSize")
    refused(3, 16384, 256, 0, "fftSize")
    refused(3, 1024, 256, 2048, "windowSize")
    refused(3, 1024, 0, 0, "hopSize")
    refused(3, 1024, 1025, 0, "hopSize")
    with pytest.raises(ValueError, match="hopSize"):
        (m.maxiFFTBank if kind == "fft" else m.maxiIFFTBank)(3, 1024, 2048)


def test_process_refuses_null_pointers_by_name():
    import maximilian_amd as m
    lib = m.lib()
    assert lib.mxg_fft_bank_process(None, None, 0, 0, None, None, None, None, None) < 0
    assert b"mxg_fft_bank_process" in lib.mxg_last_error() and b"null object" in lib.mxg_last_error()
    assert lib.mxg_ifft_bank_process(None, 0, 0, 0, None, None, 0, 0, None, None) < 0
    assert b"mxg_ifft_bank_process" in lib.mxg_last_error() and b"null object" in lib.mxg_last_error()
    assert lib.mxg_fft_bank_reset(None) < 0 and lib.mxg_ifft_bank_reset(None) < 0
    assert lib.mxg_fft_bank_destroy(None) == 0 and lib.mxg_ifft_bank_destroy(None) == 0
    assert lib.mxg_ifft_bank_buffer(None) is None
