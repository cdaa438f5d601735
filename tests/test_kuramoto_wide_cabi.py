"""CPU (-m "not gpu"): the K26 entry point is declared in include/maxigpu.h, exported by the library and bound by the Python
package, and maxiKuramotoWideBank is present in the bank header and the package; mxg_kuramoto_wide_render refuses bad arguments
with a message that names the argument -- its checks run before the device is touched, so N == 0 and N == 1025 never launch --
and otherwise fails loudly here (no CPU fallback).  mxg_kuramoto_render and maxiKuramotoBank keep refusing 65."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_kuramoto_cabi import ARGS


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    decl = re.search(r"\bint mxg_kuramoto_wide_render\s*\(([^)]*)\)", hdr)
    narrow = re.search(r"\bint mxg_kuramoto_render\s*\(([^)]*)\)", hdr)
    assert decl and narrow and " ".join(decl.group(1).split()) == " ".join(narrow.group(1).split())   # the same arguments
    assert hasattr(L, "mxg_kuramoto_wide_render") and "mxg_kuramoto_wide_render" in m._lib.SIGNATURES
    assert m._lib.SIGNATURES["mxg_kuramoto_wide_render"] == m._lib.SIGNATURES["mxg_kuramoto_render"]
    assert len(m._lib.SIGNATURES["mxg_kuramoto_wide_render"][1]) == len(ARGS) + 1
    kh = open(os.path.join(ROOT, "maximilian_amd", "csrc", "mxg_kuramoto.h")).read()
    for txt in (hdr, kh):
        assert re.search(r"#define MXG_KURA_WIDE_MAX_N 1024\b", txt) and re.search(r"#define MXG_KURA_MAX_N 64\b", kh)
    for fn in ("kura_meanfield_sums", "kura_meanfield_adj", "kura_adj_meanfield"):
        assert re.search(r"\b%s\s*\(" % fn, kh), fn
    assert hasattr(m, "maxiKuramotoWideBank") and "maxiKuramotoWideBank" in dir(m.banks)
    for meth in ("play", "phases", "set_phase", "set_phases", "render_phases", "render", "reset"):
        assert callable(getattr(m.maxiKuramotoWideBank, meth)), meth
    bank_hpp = open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read()
    assert re.search(r"\bclass maxiKuramotoWideBank\b", bank_hpp) and re.search(r"\bclass maxiKuramotoBank\b", bank_hpp)
    wide = bank_hpp[bank_hpp.index("class maxiKuramotoWideBank"):]
    wide = wide[:wide.index("\n};")]
    for meth in ("reset", "sets", "size", "setFreq", "setK", "setPhases", "setPhase", "phases", "play", "phase", "gathered", "update"):
        assert re.search(r"\b%s\(" % meth, wide), meth
    assert "mxg_kuramoto_wide_render(" in wide and "mxg_kuramoto_render(" not in wide
    dropin = open(os.path.join(ROOT, "include", "maximilian.h")).read()
    assert re.search(r"\bclass maxiKuramotoOscillatorSet\b", dropin) and "maxiKuramotoWideBank" not in dropin   # still a host value type


def _call(fn, p, **kw):
    a = {k: p for k in ARGS}
    a.update(mode=0, S=4, N=200, B=4, freq_per_sample=0, K_per_sample=0, want=3)
    a.update(kw)
    return fn(*[a[k] for k in ARGS], None)


def test_render_refuses_bad_arguments_before_touching_the_device():
    """Host addresses stand in for device pointers: every call below is refused before anything is dereferenced or launched."""
    import maximilian_amd as m
    lib = m.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    cases = [(dict(N=0), b"N: a set of 0 oscillators"), (dict(N=1025), b"N: a set of more than 1024"),
             (dict(N=1 << 40), b"N: a set of more than 1024"),
             (dict(mode=4), b"mode"), (dict(mode=-1), b"mode"), (dict(want=4), b"want"), (dict(want=-1), b"want"),
             (dict(d_phase=None), b"d_phase"), (dict(d_freq=None), b"d_freq"), (dict(d_K=None), b"d_K"),
             (dict(want=1, d_mix=None), b"d_mix"), (dict(want=3, d_mix=None), b"d_mix"),
             (dict(want=2, d_phases_out=None), b"d_phases_out"), (dict(want=3, d_phases_out=None), b"d_phases_out"),
             (dict(mode=2, d_gathered=None), b"d_gathered"), (dict(mode=3, d_update=None), b"d_update"),
             (dict(S=1 << 31), b"sets")]
    for kw, word in cases:
        st = _call(lib.mxg_kuramoto_wide_render, p, **kw)
        assert st < 0, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    # what is not wanted, and the async arrays of a sync set, may be null: the refusal, if any, is then not about them
    for kw in (dict(want=1, d_phases_out=None), dict(want=2, d_mix=None), dict(want=0, d_mix=None, d_phases_out=None),
               dict(mode=1, d_gathered=None, d_update=None)):
        st = _call(lib.mxg_kuramoto_wide_render, p, N=0, **kw)
        assert st < 0 and b"0 oscillators" in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    # the narrow entry point keeps its scope
    st = _call(lib.mxg_kuramoto_render, p, N=65)
    assert st < 0 and b"more than 64" in lib.mxg_last_error()
    assert buf.tobytes() == bytes(64 * 8)


def test_compute_fails_loudly_without_a_device():
    import maximilian_amd as m
    lib = m.lib()
    for N in (0, 1025):
        with pytest.raises(ValueError, match="1 .. 1024"):
            m.maxiKuramotoWideBank(4, N)
    with pytest.raises(ValueError, match="1 .. 64"):
        m.maxiKuramotoBank(4, 65)
    if lib.mxg_init(-1) >= 0:
        return  # a device is present: the GPU suite covers the call
    buf = np.zeros(64)
    st = _call(lib.mxg_kuramoto_wide_render, buf.ctypes.data)
    assert st < 0 and lib.mxg_last_error()
    with pytest.raises(m.MaxiGpuError):
        m.maxiKuramotoWideBank(4, 200)
