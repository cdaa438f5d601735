"""CPU (-m "not gpu"): the maxiConvolveBank entry points (kernel K24) are declared in include/maxigpu.h, exported by the library and
bound by the Python package; mxg_convolve_bank_mac_host -- the text of the kernel's lanes and its ring indexing, run on host arrays --
against a naive numpy float32 evaluation of L/maxiConvolve.cpp:86-97, bit for bit (numpy's element-wise float32 multiply, subtract
and add are correctly rounded and never fused); mxg_convolve_bank_create refuses bad arguments by name before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import convolve_host as ch
from conftest import ROOT

NEW = ["mxg_convolve_bank_create", "mxg_convolve_bank_destroy", "mxg_convolve_bank_reset", "mxg_convolve_bank_frames",
       "mxg_convolve_bank_impulse", "mxg_convolve_bank_play", "mxg_convolve_bank_play_nv", "mxg_convolve_bank_mac_host"]
TILE = 4  # output frames per lane (kConvM, csrc/mxg_convolve.h)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert len(m._lib.SIGNATURES["mxg_convolve_bank_create"][1]) == 8
    assert len(m._lib.SIGNATURES["mxg_convolve_bank_mac_host"][1]) == 17
    assert hasattr(m, "maxiConvolveBank")
    for method in ("play", "play_nv", "reset", "impulse"):
        assert callable(getattr(m.maxiConvolveBank, method))
    hpp = open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read()
    assert re.search(r"\bclass maxiConvolveBank\b", hpp) and "mxg_convolve_bank_play_nv" in hpp
    assert re.search(r"kConvM = %d\b" % TILE, open(os.path.join(ROOT, "maximilian_amd", "csrc", "mxg_convolve.h")).read())
    assert re.search(r"kChunk = %d\b" % ch.KCHUNK, open(os.path.join(ROOT, "maximilian_amd", "csrc", "convolve_bank.hip")).read())


class Naive:
    """One maxiConvolve::play per frame, as the reference writes it: push_front / pop_back on a deque of K frames, the sums refilled
    with 0 and accumulated over k in order, bin 0 without the cross terms."""

    def __init__(self, impR, impI, bins):
        self.iR, self.iI, self.K = impR, impI, impR.shape[0]
        self.fR = [np.zeros(bins, np.float32) for _ in range(self.K)]
        self.fI = [np.zeros(bins, np.float32) for _ in range(self.K)]
        self.sR, self.sI = np.zeros(bins, np.float32), np.zeros(bins, np.float32)

    def frame(self, xR, xI):
        """-> the sums the inverse transform consumes for THIS block (formed by the previous frame)"""
        outR, outI = self.sR, self.sI
        if self.K:
            self.fR = [xR] + self.fR[:-1]
            self.fI = [xI] + self.fI[:-1]
        sR, sI = np.zeros_like(outR), np.zeros_like(outI)
        with np.errstate(all="ignore"):
            for k in range(self.K):
                a, b, c, d = self.iR[k], self.iI[k], self.fR[k], self.fI[k]
                tR = (a * c) - (b * d)   # :96
                tI = (a * d) + (b * c)   # :97
                tR[0] = a[0] * c[0]      # :93
                tI[0] = b[0] * d[0]      # :94
                sR = sR + tR
                sI = sI + tI
        self.sR, self.sI = sR, sI
        return outR, outI


@pytest.mark.parametrize("bins", [32, 512])
@pytest.mark.parametrize("R", [5, 9])
@pytest.mark.parametrize("Ks", [(5, 1), (0, 5), (1, 0)])
@pytest.mark.parametrize("calls", [[1, 1, 1], [5], [2, 7, 1]])
def test_mac_host_against_numpy(bins, R, Ks, calls):
    """V = 3 streams on I = 2 impulses (imp_of = [0, 1, 0]) of K in {0, 1, 5} frames; a ring of capacity 5 = max K (one frame per launch:
    every call wraps it, and the calls of 5 and 7 exceed it) and one of 9 (launches of up to 5 frames: a full tile and a ragged one, the
    call of 7 in two launches); no call is a multiple of the tile of 4.  Bin 0 carries imaginary parts; one input value is +Inf."""
    assert all(n % TILE for n in calls)
    mac_host_against_numpy(bins, R, Ks, calls)


DEVICE_CALLS = ([45], [19, 1, 2, 23], [3, 16, 1, 20, 5])


@pytest.mark.parametrize("bins", [4, 32, 512, 4096])
@pytest.mark.parametrize("Ks", [(5, 1), (0, 5)])
@pytest.mark.parametrize("calls", DEVICE_CALLS)
def test_mac_host_against_numpy_device_ring(bins, Ks, calls):
    """The same at the ring the DEVICE gives these impulses, R = max K + 15 = 20 rows in chunks of 16 frames, and the calls of
    tests/test_gpu_convolve_bank.py's wrap cases: 45 frames wrap the ring twice, the calls together straddle its end, land on slot 0,
    read history across the end and span chunks (tests/convolve_host.py).  bins 4 is two lanes a row, the fewest the entry point takes;
    4096 is fftsize 8192.  The lane text is thereby pinned to numpy at the geometry the GPU tests run: what remains device-only is
    the head word, the advance kernel, the chunk loop's launch arguments and the block decode of convolve_bank.hip."""
    R = ch.ring_rows(Ks)
    assert R == max(Ks) + 15 == 20
    assert set().union(*(ch.ring_events(R, max(Ks), c) for c in DEVICE_CALLS)) == ch.EVENTS
    assert ch.ring_events(R, max(Ks), DEVICE_CALLS[1]) == ch.EVENTS
    mac_host_against_numpy(bins, R, Ks, calls)


def test_ring_model_and_the_gpu_cases_inputs():
    """tests/convolve_host.py's model of the head at splits worked through by hand, and the condition the GPU tests put on their own
    inputs, checked here as well so that it is seen without a GPU: every case feeds more blocks than R + max K, the splits of a wrap case
    produce all four events together, the split of a geometry case alone."""
    ev = ch.ring_events
    assert ev(20, 5, [11]) == set() and ev(20, 5, [2, 7, 1, 1]) == set()           # what the suite ran before: no event at all
    assert ev(20, 5, [17]) == {"later_chunk"}
    assert ev(20, 5, [16, 4]) == {"lands_on_0"} and ev(20, 5, [16, 5]) == {"store_wrap"}
    assert ev(20, 5, [16, 4, 1]) == {"lands_on_0", "read_wrap"}                     # head 0 on a ring that holds frames
    assert ev(20, 5, [3, 1]) == set()                                               # head 3 < K - 1 on a fresh ring: the rows read are reset()'s
    assert ev(20, 5, [16, 7, 1]) == {"store_wrap", "read_wrap"} and ev(20, 5, [16, 8, 1]) == {"store_wrap"}   # heads 3 and 4 = K - 1
    assert ev(20, 1, [16, 4, 1]) == {"lands_on_0"}                                  # K = 1 reads no history
    assert ev(20, 5, [45]) == {"later_chunk", "store_wrap"} and ev(20, 5, [19, 1, 2, 23]) == ch.EVENTS
    assert ev(54, 39, [54, 33, 25]) == ch.EVENTS and ev(54, 39, [38, 16, 58]) == ch.EVENTS and ev(17, 2, [1, 16, 20]) == ch.EVENTS
    assert ch.ring_head(20, [45]) == 5 and ch.ring_head(20, [19, 1, 2, 23]) == 5 and ch.ring_head(17, [17, 17, 3]) == 3
    assert ch.frames_of(300, 64) == 5 and ch.frames_of(20, 64) == 0 and ch.frames_of(40000, 1024) == 39 and ch.frames_of(30, 8) == 4
    assert sorted(c[0] for c in ch.GEOMETRY_CASES.values()) == [8, 16, 256, 512, 1024, 2048, 4096, 8192]
    for name, (F, H, lens, splits) in ch.ALL_CASES.items():
        frames = ch.case_frames(name)
        R, Kmax = ch.ring_rows(frames), max(frames)
        assert Kmax >= 2 and min(frames) <= 1 and 0 < H <= F, name
        assert ch.case_blocks(name) > R + Kmax, name
        each = [ev(R, Kmax, s) for s in splits]
        assert set().union(*each) == ch.EVENTS, name
        assert name in ch.WRAP_CASES or each == [ch.EVENTS], name


def mac_host_against_numpy(bins, R, Ks, calls):
    import maximilian_amd as m
    lib = m.lib()
    V, imp_of = 3, [0, 1, 0]
    rng = np.random.default_rng(bins + 7 * R + 31 * Ks[0] + len(calls))
    rows = sum(Ks)
    impR = rng.uniform(-1, 1, (max(rows, 1), bins)).astype(np.float32)
    impI = rng.uniform(-1, 1, (max(rows, 1), bins)).astype(np.float32)
    row0 = [0, Ks[0]]
    hK = np.array([Ks[i] for i in imp_of], np.int32)
    hRow = np.array([row0[i] for i in imp_of], np.int32)
    if Ks[0]:
        assert impI[0, 0] != 0
    ringR, ringI = np.zeros((V, R, bins), np.float32), np.zeros((V, R, bins), np.float32)
    pendR, pendI = np.zeros((V, bins), np.float32), np.zeros((V, bins), np.float32)
    head = np.zeros(1, np.int32)
    ref = [Naive(impR[row0[i]:row0[i] + Ks[i]], impI[row0[i]:row0[i] + Ks[i]], bins) for i in imp_of]
    nonfinite = 0
    for ci, nb in enumerate(calls):
        XR = rng.uniform(-1, 1, (V, nb, bins)).astype(np.float32)
        XI = rng.uniform(-1, 1, (V, nb, bins)).astype(np.float32)
        assert XI[0, 0, 0] != 0
        if ci == 0:
            XR[0, 0, 3] = np.inf
        SR, SI = np.full((V, nb, bins), 7.0, np.float32), np.full((V, nb, bins), 7.0, np.float32)
        st = lib.mxg_convolve_bank_mac_host(V, bins, R, hK.ctypes.data, hRow.ctypes.data, impR.ctypes.data, impI.ctypes.data,
                                            ringR.ctypes.data, ringI.ctypes.data, head.ctypes.data, pendR.ctypes.data, pendI.ctypes.data,
                                            XR.ctypes.data, XI.ctypes.data, nb, SR.ctypes.data, SI.ctypes.data)
        assert st == 0, lib.mxg_last_error()
        for v in range(V):
            for b in range(nb):
                eR, eI = ref[v].frame(XR[v, b], XI[v, b])
                assert np.array_equal(bits(SR[v, b]), bits(eR)), (ci, v, b)
                assert np.array_equal(bits(SI[v, b]), bits(eI)), (ci, v, b)
            assert np.array_equal(bits(pendR[v]), bits(ref[v].sR)) and np.array_equal(bits(pendI[v]), bits(ref[v].sI)), (ci, v)
            nonfinite += int((~np.isfinite(SR[v])).sum())
    assert head[0] == sum(calls) % R
    if Ks[0] and sum(calls) > 1:
        assert nonfinite > 0  # the Inf reached the sums of stream 0
    if Ks == (1, 0):
        assert not pendR[1].any() and not pendI[1].any()  # K = 0: the sums stay 0


def test_mac_host_refuses_bad_arguments():
    import maximilian_amd as m
    lib = m.lib()
    z = np.zeros(64, np.float32)
    k = np.array([5], np.int32)
    r0 = np.zeros(1, np.int32)
    head = np.zeros(1, np.int32)
    p = z.ctypes.data
    assert lib.mxg_convolve_bank_mac_host(1, 4, 4, k.ctypes.data, r0.ctypes.data, p, p, p, p, head.ctypes.data, p, p, p, p, 1, p, p) < 0
    assert b"ring" in lib.mxg_last_error()          # R < max K
    assert lib.mxg_convolve_bank_mac_host(1, 6, 5, k.ctypes.data, r0.ctypes.data, p, p, p, p, head.ctypes.data, p, p, p, p, 1, p, p) < 0
    assert b"bins" in lib.mxg_last_error()
    assert lib.mxg_convolve_bank_mac_host(1, 4, 5, k.ctypes.data, r0.ctypes.data, p, p, None, p, head.ctypes.data, p, p, p, p, 1, p, p) < 0
    assert b"null" in lib.mxg_last_error()


def test_create_refuses_bad_arguments_by_name():
    """Every refusal happens before the device is touched: the message names the argument, with or without a device."""
    import maximilian_amd as m
    lib = m.lib()
    a = np.zeros(100)
    ptrs = np.array([a.ctypes.data, a.ctypes.data], np.uintp)
    lens = np.array([100, 100], np.uintp)
    pos = np.array([100.0, 100.0])
    of = np.array([0, 1, 0], np.int32)

    def refused(V, I, amps, ln, ps, io, F, H, word):
        assert not lib.mxg_convolve_bank_create(V, I, amps, ln, ps, io, F, H)
        msg = lib.mxg_last_error().decode()
        assert "mxg_convolve_bank_create" in msg and word in msg, msg

    ok = (ptrs.ctypes.data, lens.ctypes.data, pos.ctypes.data, of.ctypes.data)
    refused(3, 0, *ok, 1024, 256, "I = 0")
    refused(1, 2, *ok, 1024, 256, "I = 2")                                   # I > V
    bad = np.array([0, 2, 0], np.int32)
    refused(3, 2, ok[0], ok[1], ok[2], bad.ctypes.data, 1024, 256, "h_imp_of[1]")
    neg = np.array([0, -1, 0], np.int32)
    refused(3, 2, ok[0], ok[1], ok[2], neg.ctypes.data, 1024, 256, "h_imp_of[1]")
    refused(3, 2, *ok, 1000, 256, "fftsize")
    refused(3, 2, *ok, 4, 2, "fftsize")
    refused(3, 2, *ok, 1024, 2048, "hopsize")
    refused(3, 2, *ok, 1024, 0, "hopsize")
    refused(3, 2, None, ok[1], ok[2], ok[3], 1024, 256, "h_amps")
    refused(3, 2, ok[0], None, ok[2], ok[3], 1024, 256, "h_lens")
    refused(3, 2, ok[0], ok[1], None, ok[3], 1024, 256, "h_pos0")
    refused(3, 2, ok[0], ok[1], ok[2], None, 1024, 256, "h_imp_of")
    nul = np.array([a.ctypes.data, 0], np.uintp)
    refused(3, 2, nul.ctypes.data, ok[1], ok[2], ok[3], 1024, 256, "h_amps[1]")
    zer = np.array([100, 0], np.uintp)
    refused(3, 2, ok[0], zer.ctypes.data, ok[2], ok[3], 1024, 256, "h_lens[1]")
    with pytest.raises(ValueError, match="h_imp_of"):
        m.maxiConvolveBank(3, [a, a], [0, 5, 0], 1024, 256)
