"""CPU (-m "not gpu"): the drop-in atoms classes (include/maxiAtoms.h, include/libs/maxiAtoms.h, and include/libs/maxim.h, which now
includes them as the reference's does).  tests/patches/atoms_patch.cpp VERBATIM compiles against include/ with -Wall and LINKS against
the library; where the reference is present it also compiles against the reference; the headers compile alone; the classes carry the
reference's public surface.  (fillNextBuffer renders on the device: the stream is compared in tests/test_gpu_atoms_dropin.py.)"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
PATCH = os.path.join(ROOT, "tests", "patches", "atoms_patch.cpp")


def ref_root():
    ref = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    ref = os.environ.get("MAXI_REF") or ref
    return ref if os.path.exists(os.path.join(ref, "src", "maximilian.cpp")) else None


def test_patch_compiles_and_links_against_the_dropin_headers(tmp_path):
    import maximilian_amd as m
    libdir = os.path.dirname(m.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + INC, "-o", str(tmp_path / "dropin_at"), PATCH, "-L" + libdir, "-lmaxigpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])


def test_patch_compiles_against_the_reference():
    ref = ref_root()
    if not ref:
        pytest.skip("the reference sources are not on this machine: the patch was not compiled against them")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I" + os.path.join(ref, "src"), "-I" + os.path.join(ref, "src", "libs"), PATCH])


def test_headers_compile_alone_and_hold_the_classes(tmp_path):
    body = '''
#include <type_traits>
int main() {
    maxiAccelerator acc;
    maxiAtomBook book;
    maxiAtomBookPlayer player;
    maxiGaborAtom *g = new maxiGaborAtom();
    g->atomType = GABOR; g->length = 64; g->position = 0; g->amp = 1; g->frequency = 0.5f; g->phase = 0;
    book.atoms.push_back(g);
    book.numSamples = 1024; book.sampleRate = 44100;
    maxiAtomBook::maxiAtomBookData &d = book.atoms;
    maxiAtom *base = d[0];
    flArr atom;
    maxiCollider::createGabor(atom, 440.0f, 44100.0f, 64u, 0.0f, 0.3f, 1.0f);
    float buffer[64] = {0};
    acc.addAtom(atom);
    acc.addAtom(atom, 10u);
    player.play(book, acc, buffer, 64);
    acc.fillNextBuffer(buffer, 64u);
    long idx = acc.getSampleIdx();
    maxiAtomTypes t = base->atomType;
    return (int)idx + (int)t + (maxiAtom::atomSortPositionAsc(base, g) ? 1 : 0);
}
'''
    for inc in ("maxiAtoms.h", "libs/maxiAtoms.h", "libs/maxim.h"):
        src = tmp_path / "alone.cpp"
        src.write_text('#include "%s"\n%s' % (inc, body))
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + INC, str(src)])
    hdr = open(os.path.join(INC, "maxiAtoms.h")).read()
    for cls in ("maxiCollider", "maxiAccelerator", "maxiAtomBook", "maxiAtomBookPlayer"):
        assert re.search(r"\bclass %s\b" % cls, hdr), cls
    assert re.search(r"\benum maxiAtomTypes\b", hdr) and re.search(r"\bstruct maxiGaborAtom : maxiAtom\b", hdr)
    assert "mxg_atoms_fill" in hdr and "mxg_atoms_gabor_host" in hdr
    assert '#include "../maxiAtoms.h"' in open(os.path.join(INC, "libs", "maxim.h")).read()
