#!/usr/bin/env python3
"""tools/gen/gen_golden_atoms.py -- TEST INFRASTRUCTURE.  Writes tests/golden/atoms.npz: what the UNMODIFIED reference's
maxiCollider::createGabor, maxiAccelerator and maxiAtomBookPlayer give for the cases described in tests/atoms_host.py, and the stream
of tests/patches/atoms_patch.cpp.

It compiles tools/gen/atoms_ref_dump.cpp -- which includes the reference's src/libs/maxiAtoms.cpp, the only way to createGabor --
with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling checkout the oracle uses, see oracle/Makefile REF) under
oracle/Makefile's FPFLAGS into a temporary directory outside the tree, and records the compiler, flags, libc and the sha256 of the
reference sources inside the file.  Nothing else in the tree changes.

What is stored:
  gabor/<i>      float32 [length]: createGabor(atoms_host.GABOR_CASES[i]);
  out/<case>     float32 [S][T]: the buffers after the fills (they start from the case's `init`);
  rows/<case>    int64 [S][blocks][3]: sampleIdx, atomIdx, queue length after every block;
  queue/<case>   int64 [S][blocks][maxq][3]: startTime, pos, size of every queue entry in order (-1 beyond the queue);
  patch          float32: the stream of tests/patches/atoms_patch.cpp.

The generator ASSERTS on the reference's own output: the Python restatement of the queue's rules (atoms_host.Model) gives the same
rows and queues; in "accel" an entry stalls (it is in the queue, begun, and not due); in "order" the output CHANGES when the three
atoms are queued in reverse; the buffer of the sorted book in which (idx + 64) % 512 is 0 schedules nothing; the late atoms of the
unsorted book sound; sinf differs from the rounded double sine on fewer than 2 % of the recorded non-zero Gabor samples and never by
more than the contract's bound.

    python tools/gen/gen_golden_atoms.py [--ref DIR]
"""
import argparse
import ctypes
import hashlib
import os
import platform
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import atoms_host as ah  # noqa: E402  (the case: one place for this script and the tests)

OUT = os.path.join(ROOT, "tests", "golden", "atoms.npz")
P, S, U, F = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_float


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def run_stream(R, case, s, maxq, reverse=False):
    st = case.streams[s]
    ops = np.ascontiguousarray(case.ops(s, reverse))
    starts = np.zeros(len(st.raws) + 1, np.int64)
    for k, r in enumerate(st.raws):
        starts[k + 1] = starts[k] + len(r)
    raw = np.concatenate(st.raws).astype(np.float32) if st.raws else np.zeros(1, np.float32)
    out = np.ascontiguousarray(case.init[s].copy())
    nb = len(case.blocks)
    rows, queue = np.zeros((nb, 3), np.int64), np.zeros((nb, maxq, 3), np.int64)
    book = np.ascontiguousarray(st.book)
    rc = R.at_run(len(ops), ops.ctypes.data, raw.ctypes.data, starts.ctypes.data, book.shape[1], book.ctypes.data, st.num_samples,
                  out.ctypes.data, rows.ctypes.data, queue.ctypes.data, maxq)
    assert rc == 0, (case.name, s, "queue longer than maxq")
    return out, rows, queue


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "libs", "maxiAtoms.cpp"), os.path.join(src, "libs", "maxiAtoms.h"),
                   os.path.join(src, "libs", "maxiGrains.h"), os.path.join(src, "maximilian.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    g = {}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libatref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-I" + os.path.join(src, "libs"), "-o", so, os.path.join(HERE, "atoms_ref_dump.cpp"),
                               ref_sources[0], "-lm"])
        R = ctypes.CDLL(so)
        R.at_gabor.argtypes = [F, F, U, F, F, P]
        R.at_run.argtypes = [S, P, P, P, S, P, U, P, P, P, S]
        # ---- createGabor
        differ = total = 0
        for i, (freq, sr, length, phase, amp) in enumerate(ah.GABOR_CASES):
            a = np.zeros(length, np.float32)
            R.at_gabor(freq, sr, length, phase, amp, a.ctypes.data)
            assert np.isfinite(a).all()
            m = ah.gabor_numpy(freq, sr, length, phase, amp)
            nz = a != 0
            differ += int((ah.bits(a)[nz] != ah.bits(m)[nz]).sum())
            total += int(nz.sum())
            assert (np.abs(a.astype(np.float64) - m) <= ah.gabor_bound(length, amp)).all(), (i, "sinf further than 1 ULP from the rounded double sine")
            g[ah.gabor_key(i)] = a
        print("createGabor: sinf differs from the rounded double sine on %d of %d non-zero samples (%.2f %%)" % (differ, total, 100.0 * differ / total))
        assert differ < 0.02 * total
        # ---- the queue and the player
        for name, case in ah.cases().items():
            model = ah.run_model(case)
            maxq = max(1, max(len(q) for (_, _, queues) in model for q in queues))
            outs, rows, queues = zip(*[run_stream(R, case, s, maxq) for s in range(case.S)])
            out, rows, queues = np.stack(outs), np.stack(rows), np.stack(queues)
            assert np.isfinite(out).all(), name
            for s, (_, mrows, mq) in enumerate(model):
                assert np.array_equal(rows[s], np.array(mrows, np.int64)), (name, s, "the Python model of the queue disagrees with the reference")
                for j, q in enumerate(mq):
                    assert [tuple(int(x) for x in e) for e in queues[s, j] if e[2] >= 0] == [tuple(e) for e in q], (name, s, j)
            if name == "accel":
                stalled = 0
                for j in range(rows.shape[1]):
                    for e in queues[0, j]:
                        stalled += int(e[2] >= 0 and e[1] > 0 and e[0] + e[1] != rows[0, j, 0])
                assert stalled >= 2, "no entry stalls"
                assert (out[2] == case.init[2]).all(), "the stream without atoms keeps its buffers"
                assert (out[0] != case.init[0]).mean() > 0.5
            if name == "order":
                rev, _, _ = run_stream(R, case, 0, maxq, reverse=True)
                changed = int((ah.bits(rev) != ah.bits(out[0])).sum())
                print("order: %d of 33 samples change when the queue is reversed" % changed)
                assert changed >= 4
            if name == "piece":
                assert rows[0, 0, 2] > 0 and len(model[0][0][0]) == ah.PIECE + 1
            if name == "player":
                assert (out[0, 448:512] == 0).all() and (out[0, 960:1024] == 0).all(), "(idx + 64) % 512 == 0: nothing is scheduled"
                assert (out[0, 0:64] != 0).sum() > 40 and np.array_equal(ah.bits(out[0, :512]), ah.bits(out[0, 512:1024])), "two equal loops"
                assert rows[1, 0, 1] == 1 and rows[1, 1, 1] == 1 and rows[1, 2, 1] == 4, "the unsorted book: the walk stops at the first atom that fails"
                assert (out[1, 192:256] != 0).any() and (out[1, 256:320] != 0).any(), "the late atoms of the unsorted book sound"
                assert (out[2] == 0).all()
            if name == "player65":
                assert len({out[s].tobytes() for s in range(case.S)}) == case.S, "every stream differs"
            g["out/" + name], g["rows/" + name], g["queue/" + name] = out, rows, queues
            print("%-9s S %2d T %4d  max queue %2d  peak %.3g" % (name, case.S, case.T, maxq, np.abs(out).max()))
        # ---- the patch, compiled verbatim against the reference
        patch = os.path.join(ROOT, "tests", "patches", "atoms_patch.cpp")
        if os.path.exists(patch):
            exe = os.path.join(td, "atoms_patch")
            subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-I" + os.path.join(src, "libs"), "-o", exe, patch,
                                   ref_sources[0], ref_sources[1], "-lm", "-lpthread"])
            rawf = os.path.join(td, "patch.f32")
            subprocess.run([exe, rawf], check=True, cwd=td, stdout=subprocess.DEVNULL)
            st = np.fromfile(rawf, np.float32)
            assert np.isfinite(st).all() and (st != 0).mean() > 0.2
            g["patch"] = st
    sha = hashlib.sha256()
    for fn in ref_sources:
        sha.update(open(fn, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    g["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp, libs/maxiAtoms.cpp, libs/maxiAtoms.h, libs/maxiGrains.h, "
        "maximilian.h) sha256: %s; harness: tools/gen/atoms_ref_dump.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 200 * 1000


if __name__ == "__main__":
    main()
