"""CPU (-m "not gpu"): the K19 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package; the plan tables equal the model's without a device; every refusal returns the error and a message naming the argument --
the checks run before the device is touched -- and compute otherwise fails loudly here (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

import bands_host as bh
from conftest import ROOT

NEW = ["mxg_bark_plan_create", "mxg_bark_plan_destroy", "mxg_bark_plan_limits", "mxg_bark_batch", "mxg_octave_plan_create",
       "mxg_octave_plan_destroy", "mxg_octave_plan_averages", "mxg_octave_plan_map", "mxg_octave_batch"]


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert re.search(r"#define MXG_BARK_BANDS 24\b", hdr)
    assert hasattr(m, "maxiBarkBatch") and hasattr(m, "maxiOctaveBatch")


def test_plan_tables_without_a_device(golden):
    import maximilian_amd as m
    model = bh.ModelBackend()
    g = golden("bands.npz")
    for i, (sR, bS) in enumerate(bh.BARK_CONFIGS):   # the reference's own tables
        b = m.maxiBarkBatch()
        b.setup(sR, bS)
        assert b.limits().tolist() == g["bark/%d/limits" % i].tolist(), (sR, bS)
    for i, (sr, n, per) in enumerate(bh.OCTAVE_CONFIGS):
        o = m.maxiOctaveBatch()
        o.setup(sr, n, per)
        assert o.nAverages == int(g["oct/%d/nAverages" % i]) and o.spe2avg.tolist() == g["oct/%d/map" % i].tolist(), (sr, n, per)
    for sR, bS in bh.BARK_CONFIGS:
        b = m.maxiBarkBatch()
        b.setup(sR, bS)
        assert b.limits().tolist() == model.bark_limits(sR, bS).tolist(), (sR, bS)
        b.close()
    for sr, n, per in bh.OCTAVE_CONFIGS:
        o = m.maxiOctaveBatch()
        o.setup(sr, n, per)
        mp, nA = model.octave_map(sr, n, per)
        assert o.nAverages == nA and o.spe2avg.tolist() == mp.tolist(), (sr, n, per)
        o.close()


def test_refusals_name_the_argument():
    import maximilian_amd as m
    lib = m.lib()
    for args, word in (((44100, 1), b"bufferSize"), ((44100, 0), b"bufferSize"), ((44100, 4097), b"bufferSize"),
                       ((4000000, 4096), b"sampleRate")):
        assert not lib.mxg_bark_plan_create(*args) and word in lib.mxg_last_error(), args
    for args, word in (((44100.0, 0, 12), b"nSpectrum"), ((44100.0, 4097, 12), b"nSpectrum"), ((0.0, 512, 12), b"samplingRate"),
                       ((-1.0, 512, 12), b"samplingRate"), ((float("inf"), 512, 12), b"samplingRate"),
                       ((float("nan"), 512, 12), b"samplingRate"), ((44100.0, 512, -1), b"nAveragesPerOctave"),
                       ((100.0, 8, 1), b"nAverages")):
        assert not lib.mxg_octave_plan_create(*args) and word in lib.mxg_last_error(), args
    bp = lib.mxg_bark_plan_create(44100, 1024)
    op = lib.mxg_octave_plan_create(44100.0, 512, 12)
    assert bp and op
    buf = np.zeros(64)
    p = buf.ctypes.data   # host addresses stand in for device pointers: every call below is refused before anything is read
    cases = [(lib.mxg_bark_batch, (None, p, 512, 1, p, None, None, None, None), b"plan"),
             (lib.mxg_bark_batch, (bp, None, 512, 1, p, None, None, None, None), b"d_spectrum"),
             (lib.mxg_bark_batch, (bp, p, 511, 1, p, None, None, None, None), b"stride"),
             (lib.mxg_bark_plan_limits, (bp, None), b"h_limits"),
             (lib.mxg_octave_plan_map, (op, None), b"h_spe2avg"),
             (lib.mxg_octave_batch, (None, p, 512, 1, 1, 1.0, 0.0, 0, 0.9, p, None, None, None, None), b"plan"),
             (lib.mxg_octave_batch, (op, None, 512, 1, 1, 1.0, 0.0, 0, 0.9, p, None, None, None, None), b"d_mags"),
             (lib.mxg_octave_batch, (op, p, 512, 1, 1, 1.0, 0.0, 0, 0.9, None, None, None, None, None), b"d_averages"),
             (lib.mxg_octave_batch, (op, p, 511, 1, 1, 1.0, 0.0, 0, 0.9, p, None, None, None, None), b"stride"),
             (lib.mxg_octave_batch, (op, p, 512, 1, 1, 1.0, 0.0, 0, 0.9, p, None, p, None, None), b"d_hold_state"),
             (lib.mxg_octave_batch, (op, p, 512, 1, 1, 1.0, 0.0, 0, 0.9, p, p, None, None, None), b"d_peaks_out")]
    for fn, args, word in cases:
        assert fn(*args) < 0, word
        assert word in lib.mxg_last_error(), (word, lib.mxg_last_error())
    if lib.mxg_init(-1) < 0:   # no device: compute fails loudly
        assert lib.mxg_bark_batch(bp, p, 512, 1, p, None, None, None, None) < 0 and lib.mxg_last_error()
        assert lib.mxg_octave_batch(op, p, 512, 1, 1, 1.0, 0.0, 0, 0.9, p, None, None, None, None) < 0 and lib.mxg_last_error()
    lib.mxg_bark_plan_destroy(bp)
    lib.mxg_octave_plan_destroy(op)
