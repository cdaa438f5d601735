"""CPU (-m "not gpu"): tests/patches/bands_patch.cpp -- maxiFFT -> maxiBark and maxiFFTOctaveAnalyzer, every public member of the
analyser and maxiBark::NUM_BARK_BANDS touched -- compiles against the drop-in headers (include/maximilian.h, include/maxiBark.h
through include/libs/maxim.h) and, where the reference is present, against the reference; the classes are present in the three
headers."""
import os
import re
import subprocess

from conftest import ROOT

PATCH = os.path.join(ROOT, "tests", "patches", "bands_patch.cpp")
MEMBERS = ["samplingRate", "nSpectrum", "nAverages", "nAveragesPerOctave", "spectrumFrequencySpan", "firstOctaveFrequency",
           "averageFrequencyIncrement", "averages", "peaks", "peakHoldTimes", "peakHoldTime", "peakDecayRate", "spe2avg", "linearEQSlope",
           "linearEQIntercept"]


def test_patch_compiles_both_ways():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), PATCH])
    ref = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    src = os.path.join(os.environ.get("MAXI_REF") or ref, "src")
    if os.path.exists(os.path.join(src, "maximilian.cpp")):   # the reference is not in this tree
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I" + src, PATCH])


def test_classes_present_in_the_three_headers():
    inc = os.path.join(ROOT, "include")
    dropin, bark, bank = (open(os.path.join(inc, f)).read() for f in ("maximilian.h", "maxiBark.h", "maximilian_bank.hpp"))
    assert re.search(r"\bclass maxiFFTOctaveAnalyzer\b", dropin) and dropin.index("class maxiFFTOctaveAnalyzer") > dropin.index("class maxiIFFT")
    assert re.search(r"\bclass maxiBarkScaleAnalyser\b", bark) and "typedef maxiBarkScaleAnalyser<double> maxiBark;" in bark
    assert re.search(r"\bint NUM_BARK_BANDS\b", bark)
    for cls in ("maxiBarkBatch", "maxiOctaveBatch"):
        assert re.search(r"\bclass %s\b" % cls, bank), cls
    assert '#include "../maxiBark.h"' in open(os.path.join(inc, "libs", "maxim.h")).read()
    assert '#include "../maxiBark.h"' in open(os.path.join(inc, "libs", "maxiBark.h")).read()
    patch = open(PATCH).read()
    for m in MEMBERS:
        assert re.search(r"\boctv\.%s\b" % m, patch), m
    # the facade header compiles with the new classes
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + inc, "-x", "c++", os.path.join(inc, "maximilian_bank.hpp")])
