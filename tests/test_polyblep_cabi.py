"""CPU (-m "not gpu"): the K20 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package, the waveform numbers are the recorded reference's enum values in all three places, the bank classes are present in the
package and in the C++ facade; mxg_polyblep_render and mxg_polyblep_host refuse bad arguments with MXG_ERR_INVALID and a message
that names the argument -- the checks run before the device is touched -- and the render otherwise fails loudly here (no CPU
fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

import polyblep_host as ph
from conftest import ROOT

NEW = ["mxg_polyblep_render", "mxg_polyblep_host", "mxg_envgen_set_level_host", "mxg_envgen_set_curve_host"]
MXG_ERR_INVALID = -1


def test_symbols_declared_exported_and_bound(golden):
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    arith = open(os.path.join(ROOT, "maximilian_amd", "csrc", "mxg_polyblep.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    values = golden("polyblep.npz")["enum/values"].tolist()
    assert len(values) == len(ph.WAVEFORMS) == 14
    for name, val in zip(ph.WAVEFORMS, values):
        assert re.search(r"\bMXG_PBLEP_%s = %d\b" % (name, val), hdr), name
        assert re.search(r"#define MXG_PBLEP_%s %d\b" % (name, val), arith), name
        assert m.POLYBLEP_WAVEFORMS[name] == val and ph.WF[name] == val
    assert re.search(r"#define MXG_PBLEP_WAVEFORMS 14\b", hdr)
    assert hasattr(m, "maxiPolyBLEPBank")
    assert re.search(r"\bclass maxiPolyBLEPBank\b", open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read())
    m_err = re.search(r"MXG_ERR_INVALID\s*=\s*(-?\d+)", hdr)
    assert m_err and int(m_err.group(1)) == MXG_ERR_INVALID


def test_calls_refuse_bad_arguments_before_touching_anything():
    """Host addresses stand in for device pointers: every render call below is refused before anything is dereferenced."""
    import maximilian_amd as m
    lib = m.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    base = dict(waveform=5, V=4, N=4, freq=p, fps=0, pw=None, sr=44100.0, t=p, out=p)
    cases = [(dict(V=0), b"V and N"), (dict(N=0), b"V and N"), (dict(waveform=14), b"waveform"), (dict(waveform=-1), b"waveform"),
             (dict(sr=0.0), b"sample_rate"), (dict(sr=-44100.0), b"sample_rate"), (dict(sr=float("nan")), b"sample_rate"),
             (dict(freq=None), b"_freq"), (dict(t=None), b"_t"), (dict(out=None), b"_out")]
    for kw, word in cases:
        args = list({**base, **kw}.values())
        assert lib.mxg_polyblep_render(*args, None) == MXG_ERR_INVALID, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
        assert lib.mxg_polyblep_host(*args) == MXG_ERR_INVALID, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    assert (buf == 0).all()
    # a null pulse width is 0.5
    f, t, o1, o2 = np.full(4, 61.7), np.zeros(4), np.zeros((9, 4)), np.zeros((9, 4))
    half = np.full(4, 0.5)
    for wf in range(14):
        t[:] = 0
        assert lib.mxg_polyblep_host(wf, 4, 9, f.ctypes.data, 0, None, 1000.0, t.ctypes.data, o1.ctypes.data) == 0
        t[:] = 0
        assert lib.mxg_polyblep_host(wf, 4, 9, f.ctypes.data, 0, half.ctypes.data, 1000.0, t.ctypes.data, o2.ctypes.data) == 0
        assert o1.view(np.uint64).tolist() == o2.view(np.uint64).tolist() and len(np.unique(o1)) > 2


def test_render_fails_loudly_without_a_device():
    import maximilian_amd as m
    lib = m.lib()
    if lib.mxg_init(-1) >= 0:
        return  # a device is present: the GPU suite covers the calls
    buf = np.zeros(64)
    p = buf.ctypes.data
    assert lib.mxg_polyblep_render(5, 4, 4, p, 0, None, 44100.0, p, p, None) < 0 and lib.mxg_last_error()
    with pytest.raises(m.MaxiGpuError):
        m.maxiPolyBLEPBank(4)
