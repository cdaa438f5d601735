"""CPU (-m "not gpu"): the K13 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package; the size / offset helper works without a device and agrees with the topology of the three classes; the compute entry
point refuses bad arguments or fails loudly (no CPU fallback); the drop-in header compiles in every failure mode and a patch on a
dead engine plays silence."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import reverb_cases as rc
from conftest import ROOT

NEW = ["mxg_reverb_layout_host", "mxg_reverb_render"]


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert len(m._lib.SIGNATURES["mxg_reverb_render"][1]) == 14
    assert len(m._lib.SIGNATURES["mxg_reverb_layout_host"][1]) == 6
    for cls in ("maxiSatReverbBank", "maxiFreeVerbBank", "maxiFreeVerbStereoBank"):
        assert hasattr(m, cls)
    for name, val in (("SAT", 0), ("FREEVERB", 1), ("FREEVERB_STEREO", 2), ("PLAY", 0), ("PLAY_PARAMS", 1), ("PS_ROOMSIZE", 1),
                      ("PS_ABSORBTION", 2), ("PS_ALL", 3), ("MAX_FILTERS", 39)):
        assert re.search(r"#define MXG_REVERB_%s %d\b" % (name, val), hdr), name
    assert m.banks.REVERB_KINDS == {"sat": 0, "freeverb": 1, "freeverb_stereo": 2}
    assert sorted(m.banks.REVERB_PS.values()) == [1, 2]


def test_layout_helper_needs_no_device_and_matches_the_classes():
    import maximilian_amd as m
    lib = m.lib()
    for kind in (rc.SAT, rc.FREEVERB, rc.STEREO):
        lens, offs, S = rc.layout(kind)
        nc, na, got_S, got_lens, got_offs = m.reverb_layout(kind)
        assert (nc, nc + na, got_S) == (rc.NCOMB[kind], len(lens), S)
        assert got_lens == lens and got_offs == offs
        assert len(lens) <= 39
        # every output is optional
        assert lib.mxg_reverb_layout_host(kind, None, None, None, None, None) == 0
    assert [rc.RING_DOUBLES[k] for k in (0, 1, 2)] == [3992, 18905, 12587]
    assert lib.mxg_reverb_layout_host(3, None, None, None, None, None) < 0
    assert b"kind" in lib.mxg_last_error()


def test_render_without_valid_arguments_fails_loudly():
    """No device here, or a refused argument on a GPU box: either way a negative status and a message, never a quiet success."""
    import maximilian_amd as m
    lib = m.lib()
    z = np.zeros(64)
    p = z.ctypes.data
    assert lib.mxg_reverb_render(0, 0, 4, 4, None, None, None, 0, None, None, None, None, None, None) < 0 and lib.mxg_last_error()
    assert lib.mxg_reverb_render(7, 0, 1, 1, p, None, None, 0, p, p, None, None, p, None) < 0       # unknown kind
    assert lib.mxg_reverb_render(0, 1, 1, 1, p, p, p, 0, p, p, None, None, p, None) < 0             # the overload is maxiFreeVerb's
    assert lib.mxg_reverb_render(1, 0, 1, 1, p, None, None, 0, p, p, None, None, p, None) < 0       # maxiFreeVerb without lp / wc
    assert lib.mxg_reverb_render(1, 1, 1, 1, p, None, None, 0, p, p, p, p, p, None) < 0             # play(x, r, a) without r, a
    assert lib.mxg_reverb_render(1, 1, 1, 1, p, p, p, 4, p, p, p, p, p, None) < 0                   # unknown ps bit
    if lib.mxg_init(-1) != 0:
        with pytest.raises(m.MaxiGpuError):
            m.maxiSatReverbBank(8)


@pytest.mark.parametrize("flags", [[], ["-DMAXIGPU_THROW"], ["-fno-exceptions", "-DMAXIGPU_NO_EXCEPTIONS"]])
def test_dropin_header_builds_in_every_failure_mode(flags):
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-I" + os.path.join(ROOT, "include")] + flags +
                       [os.path.join(ROOT, "tests", "patches", "reverb_patch.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    # the reference keeps the header under libs/: that spelling works too
    src = '#include "libs/maxiReverb.h"\nmaxiFreeVerb a; maxiSatReverb b; maxiFreeVerbStereo c;\nint main() { return a.play(0.0, 0.0, 0.0) + b.playStereo(0.0)[1] + c.playStereo(0.0, 0.0, 0.0)[0]; }\n'
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", "-I" + os.path.join(ROOT, "include")] + flags + ["-"],
                       input=src, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_reverb_patch_on_a_dead_engine_is_silent(tmp_path):
    """No device (or none made visible): one printed line, exit status 0, silence -- nothing is computed on the CPU instead."""
    exe = os.path.join(ROOT, "host", "dropin_rv")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "dropin_rv"])
    out = str(tmp_path / "o.f64")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, "300", out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("ERROR: maxigpu") == 1 and "no CPU fallback" in r.stderr
    got = np.fromfile(out, np.float64)
    assert got.size == 600 and not got.any(), "silence, not a CPU rendering"
