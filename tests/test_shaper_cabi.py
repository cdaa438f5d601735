"""CPU (-m "not gpu"): the K18 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package, and the classes are present in the three headers and the package; mxg_line_prepare_host and mxg_atan_norm_host give
the reference's bits without a device; the render entry points refuse bad arguments with a message that names the argument --
their checks run before the device is touched -- and otherwise fail loudly here (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

import shaper_host as sh
from conftest import ROOT

NEW = ["mxg_atan_norm_host", "mxg_shape_render", "mxg_xfade_render", "mxg_select_render", "mxg_line_prepare_host", "mxg_line_render"]
BANKS = ["maxiShaperBank", "maxiXFadeBank", "maxiSelectBank", "maxiLineBank"]
DROPIN = ["maxiNonlinearity", "maxiXFade", "maxiSelect", "maxiSelectX", "maxiLine", "maxiBits"]


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    for name, val in sh.MODES.items():
        assert re.search(r"#define MXG_SHAPE_%s %d\b" % (name.upper(), val), hdr), name
        assert m.SHAPE_MODES[name] == val
    assert re.search(r"#define MXG_SELECT_MAX_K 64\b", hdr) and re.search(r"#define MXG_XFADE_MAX_C 8\b", hdr)
    bank_hpp = open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read()
    dropin = open(os.path.join(ROOT, "include", "maximilian.h")).read()
    for cls in BANKS:
        assert hasattr(m, cls), cls
        assert re.search(r"\bclass %s\b" % cls, bank_hpp), cls
    for cls in DROPIN:
        assert re.search(r"\bclass %s\b" % cls, dropin), cls
    assert "using maxiDistortion = maxiNonlinearity;" in dropin


def test_atan_norm_is_the_reference_factor(golden):
    import maximilian_amd as m
    g = golden("shaper.npz")
    got = m.atan_norm(g["shape/pv/shape"])
    assert got.view(np.uint64).tolist() == g["shape/pv/norm"].view(np.uint64).tolist()
    assert len(np.unique(got)) == 3 and ((got > 0.6) & (got < 2.2)).all()


def test_line_prepare_host_gives_the_reference_bits(golden):
    """The line case's events replayed through mxg_line_prepare_host on host arrays, the samples in between through the numpy
    model: parameters and state at every cut are the reference's, prepare()'s previous-lineStart quirk included."""
    import maximilian_amd as m
    g = golden("shaper.npz")
    lib = m.lib()

    def prepare(par, st, v, start, end, ms, oneshot, sr):
        V = par.shape[1]
        mask = np.zeros(V, np.int32)
        mask[v] = 1
        a, b, c = (np.full(V, t, np.float64) for t in (start, end, ms))
        one = np.full(V, oneshot, np.int32)
        assert lib.mxg_line_prepare_host(V, a.ctypes.data, b.ctypes.data, c.ctypes.data, one.ctypes.data, mask.ctypes.data, float(sr),
                                         par.ctypes.data, st.ctypes.data) == 0

    sh.play_line_case(sh.ModelBackend(), g, prepare)
    # no mask: every voice; a duration of 0 is not refused (inc = +-Inf / NaN)
    par, st = sh.line_fresh(3)
    par[0] = [0.25, 0.5, 0.75]
    s, e, ms, one = np.array([0.0, 1.0, 2.0]), np.array([1.0, -1.0, 2.0]), np.array([10.0, 0.0, 0.0]), np.array([1, 0, 1], np.int32)
    assert lib.mxg_line_prepare_host(3, s.ctypes.data, e.ctypes.data, ms.ctypes.data, one.ctypes.data, None, 1000.0, par.ctypes.data,
                                     st.ctypes.data) == 0
    assert st[0].tolist() == [0.25, 0.5, 0.75] and par[0].tolist() == [0.0, 1.0, 2.0] and par[2, 0] == 1.0 / 10.0
    assert par[2, 1] == -np.inf and np.isnan(par[2, 2]) and par[3].tolist() == [1.0, 0.0, 1.0] and st[1].tolist() == [-1.0] * 3
    for i, name in enumerate(["h_start", "h_end", "h_ms", "h_oneshot", None, None, "h_par", "h_st"]):
        if name is None:
            continue
        args = [s.ctypes.data, e.ctypes.data, ms.ctypes.data, one.ctypes.data, None, 1000.0, par.ctypes.data, st.ctypes.data]
        args[i] = None
        assert lib.mxg_line_prepare_host(3, *args) < 0 and name.encode() in lib.mxg_last_error(), name


def test_renders_refuse_bad_arguments_before_touching_the_device():
    """Host addresses stand in for device pointers: every call below is refused before anything is dereferenced."""
    import maximilian_amd as m
    lib = m.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data

    def caller(fn, **defaults):
        return lambda **kw: fn(*{**defaults, **kw}.values())

    shape = caller(lib.mxg_shape_render, mode=0, V=4, N=4, d_in=p, d_a=p, d_b=p, per_sample=0, d_out=p, stream=None)
    xfade = caller(lib.mxg_xfade_render, C=2, V=4, N=4, d_ch1=p, d_ch2=p, d_xfader=p, ps=0, d_out=p, stream=None)
    select = caller(lib.mxg_select_render, x=1, K=4, V=2, N=2, d_index=p, d_values=p, sig=0, norm=0, cnt=None, d_out=p, stream=None)
    line = caller(lib.mxg_line_render, V=4, N=4, d_trig=None, c=1.0, d_par=p, d_st=p, d_out=p, stream=None)
    cases = [(shape, dict(mode=6), b"mode"), (shape, dict(mode=-1), b"mode"), (shape, dict(d_in=None), b"d_in"), (shape, dict(d_out=None), b"d_out"),
             (shape, dict(mode=3, d_a=None), b"d_a"), (shape, dict(mode=4, d_a=None), b"d_a"), (shape, dict(mode=4, d_b=None), b"d_b"),
             (shape, dict(mode=5, d_a=None), b"d_a"), (shape, dict(mode=5, d_b=None, per_sample=1), b"d_b"),
             (xfade, dict(C=0), b"C "), (xfade, dict(C=9), b"C "), (xfade, dict(d_ch1=None), b"d_ch1"), (xfade, dict(d_ch2=None), b"d_ch2"),
             (xfade, dict(d_xfader=None), b"d_xfader"), (xfade, dict(d_out=None), b"d_out"),
             (select, dict(K=0), b"K "), (select, dict(K=65), b"K "), (select, dict(d_index=None), b"d_index"),
             (select, dict(d_values=None), b"d_values"), (select, dict(d_out=None), b"d_out"),
             (line, dict(d_par=None), b"d_par"), (line, dict(d_st=None), b"d_st"), (line, dict(d_out=None), b"d_out")]
    for fn, kw, word in cases:
        assert fn(**kw) < 0, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    # parameters a mode does not read may be null: the refusal, if any, is then not about them
    for mode in (0, 1, 2):
        assert shape(mode=mode, d_a=None, d_b=None, d_out=None) < 0 and b"d_out" in lib.mxg_last_error()
    assert shape(mode=3, d_b=None, d_out=None) < 0 and b"d_out" in lib.mxg_last_error()
    assert shape(mode=4, d_b=None, per_sample=1, d_out=None) < 0 and b"d_out" in lib.mxg_last_error()


def test_compute_fails_loudly_without_a_device():
    import maximilian_amd as m
    lib = m.lib()
    if lib.mxg_init(-1) >= 0:
        return  # a device is present: the GPU suite covers the calls
    buf = np.zeros(64)
    p = buf.ctypes.data
    assert lib.mxg_shape_render(0, 4, 4, p, None, None, 0, p, None) < 0 and lib.mxg_last_error()
    assert lib.mxg_xfade_render(1, 4, 4, p, p, p, 0, p, None) < 0 and lib.mxg_last_error()
    assert lib.mxg_select_render(0, 2, 4, 4, p, p, 0, 0, None, p, None) < 0 and lib.mxg_last_error()
    assert lib.mxg_line_render(4, 4, None, 1.0, p, p, p, None) < 0 and lib.mxg_last_error()
    for cls in (m.maxiShaperBank, m.maxiXFadeBank, m.maxiSelectBank, m.maxiLineBank):
        with pytest.raises(m.MaxiGpuError):
            cls(4)
