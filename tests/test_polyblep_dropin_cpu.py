"""CPU (-m "not gpu"): the drop-in maxiPolyBLEP (include/maxiPolyBLEP.h, include/libs/maxiPolyBLEP.h) and the two maxiEnvGen setters
the reference's 9.Envelopes3 needs.  tests/patches/polyblep_patch.cpp and, where the reference is present, the examples
9.Envelopes1 / 2 / 3 VERBATIM pass g++ -fsyntax-only against include/; the patch also compiles against the reference.
maxiEnvGen::setLevel / setCurve are host edits of the [nstages][6] stage table (mxg_envgen_set_level_host /
mxg_envgen_set_curve_host): replayed over the recorded edits they give the reference's stage values and return values after
every call (tests/golden/polyblep.npz "envgen/...").  (The drop-in maxiPolyBLEP renders on the device and has no host path, so
the patch's stream is compared on the GPU: tests/test_gpu_polyblep_dropin.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import polyblep_host as ph
from conftest import ROOT, assert_bits_equal

INC = os.path.join(ROOT, "include")
PATCH = os.path.join(ROOT, "tests", "patches", "polyblep_patch.cpp")


def ref_root():
    ref = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    ref = os.environ.get("MAXI_REF") or ref
    return ref if os.path.exists(os.path.join(ref, "src", "maximilian.cpp")) else None


def test_patch_compiles_both_ways():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + INC, PATCH])
    ref = ref_root()
    if ref:   # the reference is not in this tree
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I" + os.path.join(ref, "src"), PATCH])


@pytest.mark.parametrize("example", sorted(ph.EXAMPLES.values()))
def test_reference_examples_compile_verbatim(example):
    ref = ref_root()
    if not ref:
        return   # the reference is not in this tree
    main = os.path.join(ref, "cpp", "commandline", "maximilian_examples", example, "main.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-I" + INC, main])


def test_headers_compile_alone_and_hold_the_class(tmp_path):
    for inc in ("maxiPolyBLEP.h", "libs/maxiPolyBLEP.h"):
        src = tmp_path / "alone.cpp"
        src.write_text('#include "%s"\nint main() { return (int)maxiPolyBLEP::Waveform::SAWTOOTH - (int)maxiPolyBLEP::SAWTOOTH; }\n' % inc)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + INC, str(src)])
    hdr = open(os.path.join(INC, "maxiPolyBLEP.h")).read()
    body = re.search(r"enum Waveform \{(.*?)\}", hdr, re.S).group(1)
    assert [n.strip() for n in body.split(",")] == ph.WAVEFORMS   # the reference's names and order: values 0 .. 13 as recorded
    for member in ("play", "setWaveform", "setPulseWidth", "setSampleRate", "sync"):
        assert re.search(r"\b%s\(" % member, hdr), member
    assert "maxiSettings::sampleRate" in hdr
    dropin = open(os.path.join(INC, "maximilian.h")).read()
    assert re.search(r"\bstruct PolyBLEPPool\b", dropin) and re.search(r"bool setLevel\(size_t index, double value\)", dropin)
    assert re.search(r"bool setCurve\(size_t index, double value\)", dropin)


def test_envgen_setters_edit_the_table_like_the_reference(golden):
    import maximilian_amd as m
    lib = m.lib()
    g = golden("polyblep.npz")
    lv, tm, cv = (np.array(a, np.float64) for a in (ph.ENV_LEVELS, ph.ENV_TIMES, ph.ENV_CURVES))
    ns = len(tm)
    tab = np.zeros((ns, 6))
    prev = m.maxiSettings.sampleRate
    assert lib.mxg_settings(44100, 2, 1024) == 0
    try:
        assert lib.mxg_envgen_stages_host(len(lv), lv.ctypes.data, tm.ctypes.data, cv.ctypes.data, tab.ctypes.data) == ns
    finally:
        lib.mxg_settings(int(prev), 2, 1024)
    exp, ret = g["envgen/tables"], g["envgen/ret"]
    assert len(ph.ENV_OPS) == exp.shape[0] and len(np.unique(exp[:, :, [0, 1, 3]])) > 8
    for i, (kind, index, value) in enumerate(ph.ENV_OPS):
        fn = lib.mxg_envgen_set_level_host if kind == 0 else lib.mxg_envgen_set_curve_host
        assert fn(tab.ctypes.data, ns, index, float(value)) == ret[i], (i, kind, index)
        assert_bits_equal(tab, exp[i], "after edit %d" % i)
    # setCurve(nstages) writes nothing (the reference writes outside its vector there); bad tables are refused
    before = tab.copy()
    assert lib.mxg_envgen_set_curve_host(tab.ctypes.data, ns, ns, 5.0) == 0
    assert_bits_equal(tab, before, "setCurve(nstages)")
    assert lib.mxg_envgen_set_level_host(None, ns, 0, 1.0) < 0 and lib.mxg_envgen_set_level_host(tab.ctypes.data, 0, 0, 1.0) < 0
    assert lib.mxg_envgen_set_curve_host(None, ns, 0, 1.0) < 0 and lib.mxg_envgen_set_curve_host(tab.ctypes.data, 33, 0, 1.0) < 0
