"""CPU (-m "not gpu"): the K14 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package; the layout helper works without a device, equals the reference constructor's lengths (tests/golden/dattaro.npz) at the
five rates and at both ends of the accepted range, rejects the rates just outside it, and accepts exactly the rates a brute-force
evaluation of the rule in numpy accepts among 1 .. 400 000; the compute entry point refuses bad arguments or fails loudly (no CPU
fallback); the drop-in header compiles in every failure mode and a patch on a dead engine plays silence."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dattaro_cases as dc
import dattaro_host as dh
from conftest import ROOT

NEW = ["mxg_dattaro_layout_host", "mxg_dattaro_render"]


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert len(m._lib.SIGNATURES["mxg_dattaro_render"][1]) == 9
    assert len(m._lib.SIGNATURES["mxg_dattaro_layout_host"][1]) == 6
    assert hasattr(m, "maxiDattaroReverbBank") and hasattr(m, "dattaro_layout")
    for name, val in (("RINGS", 10), ("TAPS", 14), ("STATE", 5)):
        assert re.search(r"#define MXG_DATTARO_%s %d\b" % (name, val), hdr), name


def test_layout_helper_needs_no_device_and_matches_the_reference():
    import maximilian_amd as m
    lib = m.lib()
    g = dh.load_golden()
    rates = g["rates"].tolist()
    lo, hi = dc.accepted_ends()
    assert rates == dc.RATES + [lo, hi]
    for k, rate in enumerate(rates):
        lens, offs, S, taps, rings = m.dattaro_layout(rate)
        assert lens == g["lengths"][k].tolist(), rate
        assert taps == g["taps"][k].tolist(), rate
        assert (lens, offs, S) == dc.layout(rate) and rings == dc.TAP_RING
        assert lib.mxg_dattaro_layout_host(rate, None, None, None, None, None) == 0  # every output is optional
    assert m.dattaro_layout(44100)[0][6:] == dc.CHECK_44100["D"] and m.dattaro_layout(48000)[0][6:] == dc.CHECK_48000["D"]
    assert m.dattaro_layout()[2] == 32312
    for rate in (lo - 1, hi + 1, 0, 1, 2 ** 32 - 1):
        assert lib.mxg_dattaro_layout_host(rate, None, None, None, None, None) < 0, rate
        msg = lib.mxg_last_error().decode()
        assert str(lo) in msg and str(hi) in msg, msg
        with pytest.raises(m.MaxiGpuError):
            m.dattaro_layout(rate)


def test_accepted_rates_against_brute_force():
    import maximilian_amd as m
    fn = m.lib().mxg_dattaro_layout_host
    rates = np.arange(1, 400001)
    exp = dc.accepted(rates)
    got = np.array([fn(int(r), None, None, None, None, None) == 0 for r in rates])
    assert np.array_equal(got, exp)
    assert (int(rates[exp].min()), int(rates[exp].max())) == dc.accepted_ends() == (3345, 295129)
    # where the input rings are shorter than two tiles the kernel stages both in 320 LDS slots
    L0, L1 = dc.scale(dc.ORIG_LEN[0], rates), dc.scale(dc.ORIG_LEN[1], rates)
    assert (L0 + L1)[exp & (np.minimum(L0, L1) < 2 * dc.TILE)].max() <= 320


def test_render_without_valid_arguments_fails_loudly():
    """No device here, or a refused argument on a GPU box: either way a negative status and a message, never a quiet success."""
    import maximilian_amd as m
    lib = m.lib()
    z = np.zeros(64)
    p = z.ctypes.data
    lo, hi = dc.accepted_ends()

    def refused(*args):
        return lib.mxg_dattaro_render(*args) < 0 and len(lib.mxg_last_error()) > 0

    assert refused(44100, 4, 4, None, None, None, None, None, None)
    for k in range(5):  # each pointer by itself
        args = [p] * 5
        args[k] = None
        assert refused(44100, 1, 1, *args, None), k
        assert b"null" in lib.mxg_last_error()
    for rate in (0, 1000, lo - 1, hi + 1, 400000):
        assert refused(rate, 1, 1, p, p, p, p, p, None), rate
        assert b"sample rate" in lib.mxg_last_error()
    if lib.mxg_init(-1) != 0:
        assert refused(44100, 1, 1, p, p, p, p, p, None)  # no device: an error, not a CPU rendering
        with pytest.raises(m.MaxiGpuError):
            m.maxiDattaroReverbBank(8)
    with pytest.raises(m.MaxiGpuError):
        m.maxiDattaroReverbBank(8, 1000)


@pytest.mark.parametrize("flags", [[], ["-DMAXIGPU_THROW"], ["-fno-exceptions", "-DMAXIGPU_NO_EXCEPTIONS"]])
def test_dropin_header_builds_in_every_failure_mode(flags):
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-I" + os.path.join(ROOT, "include")] + flags +
                       [os.path.join(ROOT, "tests", "patches", "dattaro_patch.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    # the reference keeps the header under libs/: that spelling works too
    src = '#include "libs/maxiReverb.h"\nmaxiDattaroReverb a;\nint main() { maxiDattaroReverb b = a; b = a; return a.playStereo(0.0)[1] + b.playStereo(1.0)[0]; }\n'
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", "-I" + os.path.join(ROOT, "include")] + flags + ["-"],
                       input=src, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_dattaro_patch_on_a_dead_engine_is_silent(tmp_path):
    """No device (or none made visible): one printed line, exit status 0, silence -- nothing is computed on the CPU instead."""
    exe = os.path.join(ROOT, "host", "dropin_dt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "dropin_dt"])
    out = str(tmp_path / "o.f64")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, "300", out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("ERROR: maxigpu") == 1 and "no CPU fallback" in r.stderr
    got = np.fromfile(out, np.float64)
    assert got.size == 600 and not got.any(), "silence, not a CPU rendering"
