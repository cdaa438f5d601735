"""CPU (-m "not gpu"): the drop-in maxiKick / maxiSnare / maxiHats (include/maxiSynths.h) and maxiClock (include/maxiClock.h,
include/libs/maxiClock.h).  tests/patches/drums_patch.cpp and, where the reference is present, the example 7.Counting1 VERBATIM pass
g++ -fsyntax-only -Wall against include/; the patch also compiles against the reference; the two clock headers compile alone;
the classes carry the reference's public surface and are value types.  (The drop-in drums render on the device and have no host
path, so the streams are compared on the GPU: tests/test_gpu_drums_dropin.py.)"""
import os
import re
import subprocess

import pytest

import drums_host as dh
from conftest import ROOT

INC = os.path.join(ROOT, "include")
PATCH = os.path.join(ROOT, "tests", "patches", "drums_patch.cpp")


def ref_root():
    ref = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    ref = os.environ.get("MAXI_REF") or ref
    return ref if os.path.exists(os.path.join(ref, "src", "maximilian.cpp")) else None


def test_patch_compiles_against_the_dropin_headers():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + INC, PATCH])


def test_patch_compiles_against_the_reference():
    ref = ref_root()
    if not ref:
        pytest.skip("the reference sources are not on this machine: the patch was not compiled against them")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I" + os.path.join(ref, "src"), "-I" + os.path.join(ref, "src", "libs"), PATCH])


def test_counting1_compiles_verbatim():
    ref = ref_root()
    if not ref:
        pytest.skip("the reference sources are not on this machine: 7.Counting1 was not compiled")
    main = os.path.join(ref, "cpp", "commandline", "maximilian_examples", dh.EXAMPLES["07"], "main.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + INC, main])


def test_headers_compile_alone_and_hold_the_classes(tmp_path):
    for inc in ("maxiClock.h", "libs/maxiClock.h"):
        src = tmp_path / "alone.cpp"
        src.write_text('#include "%s"\nint main() { maxiClock c; c.setTicksPerBeat(4); c.setTempo(90); c.setLastCount(1); return c.getPlayHead() + c.isTick(); }\n' % inc)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + INC, str(src)])
    src = tmp_path / "values.cpp"
    src.write_text('''#include "maxiSynths.h"
#include <type_traits>
#include <vector>
static_assert(std::is_copy_constructible<maxiKick>::value && std::is_copy_assignable<maxiSnare>::value && std::is_copy_constructible<maxiHats>::value, "value types");
int main() {
    std::vector<maxiKick> kicks(3);
    std::vector<maxiHats> hats(2);
    maxiSnare s, t(s);
    maxiClock c;
    kicks[0].setPitch(100); kicks[0].setRelease(10); kicks[0].setDistortion(2); kicks[0].setCutoff(500); kicks[0].setResonance(2);
    kicks[0].setUseDistortion(true); kicks[0].setUseLimiter(true); kicks[0].setUseFilter(true);
    double g = kicks[0].getPitch() + kicks[0].getDistortion() + kicks[0].getCutoff() + kicks[0].getResonance() + kicks[0].getUseDistortion() +
               kicks[0].getUseLimiter() + kicks[0].getUseFilter();
    s.pitch = 1; s.output = 0; s.outputD = 0; s.envOut = 0; s.useDistortion = s.useLimiter = s.useFilter = s.inverse = false;
    s.distortion = s.cutoff = s.resonance = s.gain = 1;
    s.envelope.setAttack(1); s.envelope.setDecay(1); s.envelope.setSustain(1); s.envelope.setRelease(1); s.envelope.holdtime = 2; s.envelope.trigger = 1;
    s.tone.phaseReset(0); (void)s.noise; (void)s.distort; (void)s.filter;
    hats[0].filter.setCutoff(100); hats[0].filter.setResonance(2); hats[0].setPitch(1); hats[0].setRelease(1); hats[0].trigger();
    t = s;
    return (int)g + (int)hats[1].pitch + c.ticks;
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + INC, str(src)])
    hdr = open(os.path.join(INC, "maxiSynths.h")).read()
    assert '#include "maxiClock.h"' in hdr
    for cls in ("maxiKick", "maxiSnare", "maxiHats"):
        assert re.search(r"\bclass %s\b" % cls, hdr), cls
    assert "mxg_drum_render" in hdr and "throw" not in hdr.split("maxiKick / maxiSnare / maxiHats")[1] and "abort" not in hdr.split("maxiKick / maxiSnare / maxiHats")[1]
