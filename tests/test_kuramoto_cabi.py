"""CPU (-m "not gpu"): the K17 entry point is declared in include/maxigpu.h, exported by the library and bound by the Python
package, and the classes are present in the three headers and the package; mxg_kuramoto_render refuses bad arguments with a
message that names the argument -- its checks run before the device is touched, so N == 0 and N == 65 never launch -- and
otherwise fails loudly here (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

DROPIN = ["maxiKuramotoOscillator", "maxiKuramotoOscillatorSet", "maxiAsyncKuramotoOscillator"]
ARGS = ["mode", "S", "N", "B", "d_freq", "freq_per_sample", "d_K", "K_per_sample", "d_phase", "d_gathered", "d_update", "want", "d_mix",
        "d_phases_out"]


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    assert re.search(r"\bmxg_kuramoto_render\s*\(", hdr)
    assert hasattr(L, "mxg_kuramoto_render") and "mxg_kuramoto_render" in m._lib.SIGNATURES
    assert len(m._lib.SIGNATURES["mxg_kuramoto_render"][1]) == len(ARGS) + 1
    for name, val in (("MEANFIELD", 1), ("ASYNC", 2), ("WANT_MIX", 1), ("WANT_PHASES", 2)):
        assert re.search(r"#define MXG_KURA_%s %d\b" % (name, val), hdr), name
    kh = open(os.path.join(ROOT, "maximilian_amd", "csrc", "mxg_kuramoto.h")).read()
    for name, val in (("MEANFIELD", 1), ("ASYNC", 2), ("WANT_MIX", 1), ("WANT_PHASES", 2)):
        assert re.search(r"#define MXG_KURA_%s %d\b" % (name, val), kh), name
    assert hasattr(m, "maxiKuramotoBank")
    for meth in ("play", "phases", "set_phase", "set_phases", "render_phases"):
        assert callable(getattr(m.maxiKuramotoBank, meth)), meth
    bank_hpp = open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read()
    dropin = open(os.path.join(ROOT, "include", "maximilian.h")).read()
    assert re.search(r"\bclass maxiKuramotoBank\b", bank_hpp)
    for cls in DROPIN:
        assert re.search(r"\bclass %s\b" % cls, dropin), cls
    assert "double play(double freq, double K, std::vector<double> phases)" in dropin   # by value, as the reference has it


def _call(lib, p, **kw):
    a = {k: p for k in ARGS}
    a.update(mode=0, S=4, N=3, B=4, freq_per_sample=0, K_per_sample=0, want=3)
    a.update(kw)
    return lib.mxg_kuramoto_render(*[a[k] for k in ARGS], None)


def test_render_refuses_bad_arguments_before_touching_the_device():
    """Host addresses stand in for device pointers: every call below is refused before anything is dereferenced or launched."""
    import maximilian_amd as m
    lib = m.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    cases = [(dict(N=0), b"0 oscillators"), (dict(N=65), b"more than 64"), (dict(N=1 << 40), b"more than 64"),
             (dict(mode=4), b"mode"), (dict(mode=-1), b"mode"), (dict(want=4), b"want"), (dict(want=-1), b"want"),
             (dict(d_phase=None), b"d_phase"), (dict(d_freq=None), b"d_freq"), (dict(d_K=None), b"d_K"),
             (dict(want=1, d_mix=None), b"d_mix"), (dict(want=3, d_mix=None), b"d_mix"),
             (dict(want=2, d_phases_out=None), b"d_phases_out"), (dict(want=3, d_phases_out=None), b"d_phases_out"),
             (dict(mode=2, d_gathered=None), b"d_gathered"), (dict(mode=3, d_update=None), b"d_update"),
             (dict(S=1 << 31), b"sets")]
    for kw, word in cases:
        st = _call(lib, p, **kw)
        assert st < 0, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    # what is not wanted, and the async arrays of a sync set, may be null: the refusal, if any, is then not about them
    for kw in (dict(want=1, d_phases_out=None), dict(want=2, d_mix=None), dict(want=0, d_mix=None, d_phases_out=None),
               dict(mode=1, d_gathered=None, d_update=None)):
        st = _call(lib, p, N=0, **kw)
        assert st < 0 and b"0 oscillators" in lib.mxg_last_error(), (kw, lib.mxg_last_error())


def test_compute_fails_loudly_without_a_device():
    import maximilian_amd as m
    lib = m.lib()
    for N in (0, 65):
        with pytest.raises(ValueError, match="1 .. 64"):
            m.maxiKuramotoBank(4, N)
    if lib.mxg_init(-1) >= 0:
        return  # a device is present: the GPU suite covers the call
    buf = np.zeros(64)
    st = _call(lib, buf.ctypes.data)
    assert st < 0 and lib.mxg_last_error()
    with pytest.raises(m.MaxiGpuError):
        m.maxiKuramotoBank(4, 3)
