"""CPU (-m "not gpu"): the shared step headers (maximilian_amd/csrc/mxg_*.h) say where a function runs with the one vocabulary of
mxg_hd.h.  Every step header that has a host build -- the mxg_*.h files that g++ really reads when it compiles tests/host_*.cpp and
csrc/*_host.cpp -- compiles alone, and all of them compile together in alphabetical and in reverse order: no header's meaning depends
on which other header came first.  A text check keeps the old dialects out: no redefined __device__ / __host__ / __forceinline__, no
qualifier macro defined outside mxg_hd.h, no per-file MXG_STEP_HOST_CALLABLE switch."""
import glob
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "maximilian_amd", "csrc")
# unknown pragmas: the kernels' `#pragma unroll` / `#pragma clang fp contract`, which g++ reports under -Wall and skips
GXX = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I" + CSRC]


def host_built_sources():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "host_*.cpp")) + glob.glob(os.path.join(CSRC, "*_host.cpp")))


@pytest.fixture(scope="module")
def step_headers():
    """The mxg_*.h files in the dependency lists g++ writes for the host-built sources (so a header behind `#if defined(__HIPCC__)`
    is not one of them, and a header reached through another one is)."""
    def deps(src):
        out = subprocess.run(["g++", "-std=c++17", "-MM", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src],
                             check=True, capture_output=True, text=True).stdout
        return {os.path.basename(p) for p in out.replace("\\\n", " ").split() if re.fullmatch(r"mxg_\w+\.h", os.path.basename(p))}
    with ThreadPoolExecutor(4) as pool:
        found = sorted(set().union(*pool.map(deps, host_built_sources())))
    assert "mxg_hd.h" in found and len(found) >= 25, found
    return found


def compile_including(tmp_path, name, headers):
    src = tmp_path / name
    src.write_text("".join('#include "%s"\n' % h for h in headers) + "int main() { return 0; }\n")
    r = subprocess.run(GXX + [str(src)], capture_output=True, text=True)
    return r.returncode, r.stderr


def test_each_step_header_compiles_alone(step_headers, tmp_path):
    with ThreadPoolExecutor(4) as pool:
        results = list(pool.map(lambda h: compile_including(tmp_path, "alone_" + h[:-2] + ".cpp", [h]), step_headers))
    failed = {h: err for h, (rc, err) in zip(step_headers, results) if rc != 0}
    assert not failed, "\n".join("%s:\n%s" % kv for kv in failed.items())


@pytest.mark.parametrize("reverse", [False, True], ids=["alphabetical", "reverse"])
def test_all_step_headers_compile_in_either_order(step_headers, tmp_path, reverse):
    rc, err = compile_including(tmp_path, "all.cpp", sorted(step_headers, reverse=reverse))
    assert rc == 0, err


def test_one_vocabulary_in_the_sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*"))) + sorted(glob.glob(os.path.join(ROOT, "tests", "host_*.cpp")))
    files = [f for f in files if os.path.isfile(f) and os.path.splitext(f)[1] in (".h", ".hip", ".cpp", "")]  # ("": the Makefile)
    assert len(files) > 60
    reserved = re.compile(r"#\s*define\s+__(device|host|forceinline)__")
    qualifier = re.compile(r"#\s*(define|undef)\s+(MXG_\w*HD\w*|MXG_DEV)\b")
    bad, vocabulary = [], set()
    for f in files:
        rel = os.path.relpath(f, ROOT)
        for n, line in enumerate(open(f, errors="replace"), 1):
            if reserved.search(line) or "MXG_STEP_HOST_CALLABLE" in line:
                bad.append("%s:%d: %s" % (rel, n, line.strip()))
            m = qualifier.search(line)
            if m and os.path.basename(f) != "mxg_hd.h":
                bad.append("%s:%d: %s" % (rel, n, line.strip()))
            elif m:
                assert m.group(1) == "define", line
                vocabulary.add(m.group(2))
    assert not bad, "\n".join(bad)
    assert {"MXG_HD", "MXG_DEV"} <= vocabulary and len(vocabulary) <= 4, vocabulary
