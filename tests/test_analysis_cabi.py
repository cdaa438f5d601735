"""CPU (-m "not gpu"): the K16 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package, and the classes are present in the three headers and the package; the host-only ones work without a device;
mxg_analysis_render refuses bad arguments with a message that names the argument -- its checks run before the device is
touched -- and otherwise fails loudly here (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ["mxg_envfollow_coeff_host", "mxg_analysis_window_host", "mxg_analysis_render"]
DROPIN = ["maxiZeroCrossingDetector", "maxiZeroCrossingRate", "maxiEnvelopeFollowerType", "maxiSampleAndHold", "maxiPoll"]


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert len(m._lib.SIGNATURES["mxg_analysis_render"][1]) == 23
    for name, val in (("ZX", 1), ("ZCR", 2), ("ENV", 4), ("SAH", 8), ("ALL", 15)):
        assert re.search(r"#define MXG_ANA_WANT_%s %d\b" % (name, val), hdr), name
    assert hasattr(m, "maxiAnalysisBank") and m.analysis_want(("zx", "sah")) == 9 and m.analysis_want("zcr") == 2
    with pytest.raises(ValueError, match="want"):
        m.analysis_want(("zx", "rms"))
    bank_hpp = open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read()
    dropin = open(os.path.join(ROOT, "include", "maximilian.h")).read()
    assert re.search(r"\bclass maxiAnalysisBank\b", bank_hpp)
    for cls in DROPIN:
        assert re.search(r"\bclass %s\b" % cls, dropin), cls
    assert "typedef maxiEnvelopeFollowerType<double> maxiEnvelopeFollower;" in dropin
    assert "typedef maxiEnvelopeFollowerType<float> maxiEnvelopeFollowerF;" in dropin


def test_follower_coefficients_are_the_reference_bits(golden):
    import maximilian_amd as m
    g = golden("analysis.npz")
    for case in ("a", "b"):
        sr = float(g[case + "/sr"])
        for ms, ref in ((g[case + "/attack_ms"], g[case + "/attack"]), (g[case + "/release_ms"], g[case + "/release"])):
            got = m.envfollow_coeff(ms, sr)
            assert got.view(np.uint64).tolist() == ref.view(np.uint64).tolist()
            assert ((ref > 0) & (ref < 1)).all() and len(np.unique(ref)) >= 4
    assert m.lib().mxg_envfollow_coeff_host(100.0, 44100.0) == 0.01 ** (1.0 / (100.0 * 44100.0 * 0.001))


def test_window_check_needs_no_device_and_refuses():
    import maximilian_amd as m
    lib = m.lib()
    ok = np.array([1, 1000, 5000], np.uint32)   # above cap passes: the kernel holds it there and counts it
    assert lib.mxg_analysis_window_host(3, ok.ctypes.data, 1000) == 0
    bad = np.array([5, 0, 7], np.uint32)
    assert lib.mxg_analysis_window_host(3, bad.ctypes.data, 1000) < 0
    assert b"window" in lib.mxg_last_error() and b"0" in lib.mxg_last_error()
    assert lib.mxg_analysis_window_host(3, ok.ctypes.data, 0) < 0
    assert b"cap" in lib.mxg_last_error()
    assert lib.mxg_analysis_window_host(3, None, 10) < 0
    assert b"h_window" in lib.mxg_last_error()


ARGS = ["d_in", "want", "d_prev_x", "d_window", "d_zring", "cap", "d_zpos", "d_zcount", "d_overflow", "d_attack", "d_release", "d_env",
        "d_hold_ms", "hold_per_sample", "d_sah_phase", "d_sah_value", "d_zx", "d_zcr", "d_env_out", "d_sah"]


def _call(lib, p, **kw):
    a = {k: p for k in ARGS}
    a.update(want=15, cap=100, hold_per_sample=0)
    a.update(kw)
    return lib.mxg_analysis_render(4, 4, *[a[k] for k in ARGS], None)


def test_render_refuses_bad_arguments_before_touching_the_device():
    """Host addresses stand in for device pointers: every call below is refused before anything is dereferenced."""
    import maximilian_amd as m
    lib = m.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    cases = [(dict(cap=0), b"cap"), (dict(cap=1 << 31), b"cap"), (dict(want=16), b"unknown bit"), (dict(want=-1), b"unknown bit"),
             (dict(want=0), b"no output"), (dict(d_in=None), b"d_in")]
    # a wanted stage with a null array names that array
    for want, names in ((1, ["d_prev_x", "d_zx"]), (2, ["d_prev_x", "d_window", "d_zring", "d_zpos", "d_zcount", "d_zcr"]),
                        (4, ["d_attack", "d_release", "d_env", "d_env_out"]), (8, ["d_hold_ms", "d_sah_phase", "d_sah_value", "d_sah"])):
        for n in names:
            cases.append(({"want": want, n: None}, n.encode()))
            cases.append(({"want": 15, n: None}, n.encode()))
    for kw, word in cases:
        st = _call(lib, p, **kw)
        assert st < 0, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    # the arrays of a stage that is not wanted may be null: the refusal, if any, is then not about them
    for want, free in ((1, ["d_window", "d_zring", "d_zpos", "d_zcount", "d_zcr", "d_attack", "d_env", "d_hold_ms", "d_sah"]),
                       (4, ["d_prev_x", "d_window", "d_zring", "d_zx", "d_sah_phase"]), (8, ["d_prev_x", "d_attack", "d_env_out"])):
        st = _call(lib, p, d_in=None, want=want, cap=0, **{n: None for n in free})
        assert st < 0 and b"d_in" in lib.mxg_last_error(), (want, lib.mxg_last_error())


def test_compute_fails_loudly_without_a_device():
    import maximilian_amd as m
    lib = m.lib()
    if lib.mxg_init(-1) >= 0:
        return  # a device is present: the GPU suite covers the call
    buf = np.zeros(64)
    st = _call(lib, buf.ctypes.data)
    assert st < 0 and lib.mxg_last_error()
    with pytest.raises(m.MaxiGpuError):
        m.maxiAnalysisBank(4, 100)
