#!/usr/bin/env python3
"""tools/gen/gen_golden_grainpool.py -- TEST INFRASTRUCTURE.  Writes tests/golden/grainpool.npz: what the UNMODIFIED reference's
maxiTimeStretch / maxiPitchShift / maxiStretch (src/libs/maxiGrains.h) compute for the streams of tests/grainpool_host.py (the table
STREAMS there: one object with its own maxiSample per row; every input is derived there from the stored integers, for this script
and the tests alike).

It compiles tools/gen/grainpool_ref_dump.cpp with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling checkout
the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS and -fno-access-control into a temporary directory
outside the tree, routes the grain code's rand() to the table's draws, and records the compiler, flags, libc and the sha256 of the
reference sources inside the file.  Nothing else in the tree changes.  The archive is written with fixed member dates.

What is stored: cuts; pool (the slots' content, concatenated) and lens; window/<name> (the reference's own window tables of 441
values); out [2000][streams]; at every cut snap<i>/st [3][streams] = position, looper (maxiPitchShift: cycles), randomOffset and
snap<i>/gst [4][8][streams] = the live grains in creation order: pos, inc, sampleIdx, sampleDur; loops [3][streams] at the end
(loopStart, loopEnd, loopLength; zeros for the classes without); patch_sl [10500][2]: tests/patches/stretch_loop_patch.cpp compiled
with the unmodified reference and run through oracle/example_host.cpp (what tests/test_gpu_dropin_stretch.py compares the drop-in
build of the same file with).

The generator ASSERTS on the reference's own output: no stream ever holds more than 8 live grains; every read index lies in
[0, len); every loop stream's position is inside its loop once it has walked in and is seen wrapping at least twice; the grains of
the short slots wrap; no stream's output is constant; every stream has at least 6 births and 4 grain deaths; no draw queue ran dry.

    python tools/gen/gen_golden_grainpool.py [--ref DIR]
"""
import argparse
import ctypes
import hashlib
import io
import os
import platform
import re
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grainpool_host as gh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "grainpool.npz")
P, Z, I, D = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates and order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "maximilian.h"), os.path.join(src, "libs", "maxiGrains.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    T, CUTS, NS = gh.T, gh.CUTS, gh.NS
    content = gh.pool_content()
    g = {"cuts": np.array(CUTS, np.int64), "pool": np.concatenate(content), "lens": np.array(gh.LENS, np.int64)}
    n = np.arange(T)
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libgrainpoolref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "grainpool_ref_dump.cpp"), ref_sources[0], "-lm"])
        Rf = ctypes.CDLL(so)
        Rf.gp_sample_new.restype = P
        Rf.gp_sample_new.argtypes = [P, Z]
        Rf.gp_sample_free.argtypes = [P]
        Rf.gp_new.restype = P
        Rf.gp_new.argtypes = [I, I, P, P, Z]
        Rf.gp_free.argtypes = [P]
        Rf.gp_set_sample.argtypes = [P, P]
        Rf.gp_set_position_raw.argtypes = [P, D]
        Rf.gp_set_loop_start.argtypes = [P, D]
        Rf.gp_set_loop_end.argtypes = [P, D]
        Rf.gp_run.argtypes = [P, I, Z, P, P, P, D, I, P, P]
        Rf.gp_state.restype = Z
        Rf.gp_state.argtypes = [P, P, P, P, P]
        Rf.gp_window.argtypes = [I, I, P]
        for name, kind in gh.WINDOWS.items():
            w = np.zeros(gh.SAMPLE_DUR)
            Rf.gp_window(kind, gh.SAMPLE_DUR, w.ctypes.data)
            g["window/" + name] = w
        out = np.zeros((T, NS))
        pos = np.zeros((T, NS))
        snaps = [(np.zeros((3, NS)), np.zeros((4, 8, NS))) for _ in CUTS[1:]]
        loops = np.zeros((3, NS), np.uint64)
        for i, s in enumerate(gh.STREAMS):
            mode, ov, win, has_rnd, ps, slot, fa, fb, fpm, pos0, loop = s
            # one maxiSample per object, as in a patch (a second one for the setSlot event)
            smp = Rf.gp_sample_new(np.ascontiguousarray(content[slot]).ctypes.data, content[slot].size)
            extra = []
            rnd = gh.rnd_draws(i) if has_rnd else None
            h = Rf.gp_new(mode, gh.WINDOWS[win], smp, None if rnd is None else rnd.ctypes.data, 0 if rnd is None else rnd.size)
            Rf.gp_set_position_raw(h, pos0)
            if loop is not None:
                Rf.gp_set_loop_start(h, loop[0])
                Rf.gp_set_loop_end(h, loop[1])
            a = np.ascontiguousarray(fa(n), np.float64)
            b = None if fb is None else np.ascontiguousarray(fb(n), np.float64)
            pm = None if fpm is None else np.ascontiguousarray(fpm(n), np.float64)
            if not (mode == 2 or ps & gh.PS_A):
                assert (a == a[0]).all()
            if b is not None and not ps & gh.PS_B:
                assert (b == b[0]).all()
            if pm is not None and not ps & gh.PS_POSMOD:
                assert (pm == pm[0]).all()
            cur_len = gh.LENS[slot]
            for ci, (n0, n1) in enumerate(zip(CUTS[:-1], CUTS[1:])):
                ev = gh.EVENTS.get(n0)
                if ev and ev[1] == i:
                    if ev[0] == "loopStart":
                        Rf.gp_set_loop_start(h, ev[2])
                    else:
                        s2 = Rf.gp_sample_new(np.ascontiguousarray(content[ev[2]]).ctypes.data, content[ev[2]].size)
                        extra.append(s2)
                        Rf.gp_set_sample(h, s2)
                        cur_len = gh.LENS[ev[2]]
                k = n1 - n0
                o, p = np.zeros(k), np.zeros(k)
                Rf.gp_run(h, mode, k, a[n0:n1].ctypes.data, None if b is None else b[n0:n1].ctypes.data,
                          None if pm is None else pm[n0:n1].ctypes.data, gh.GRAIN_LENGTH, ov, o.ctypes.data, p.ctypes.data)
                out[n0:n1, i], pos[n0:n1, i] = o, p
                st, gst, l3, stats = np.zeros(3), np.zeros((4, 8)), np.zeros(3, np.uint64), np.zeros(8, np.int64)
                live = Rf.gp_state(h, st.ctypes.data, gst.ctypes.data, l3.ctypes.data, stats.ctypes.data)
                assert live <= 8, "stream %d: %d live grains at a cut" % (i, live)
                snaps[ci][0][:, i], snaps[ci][1][:, :, i] = st, gst
                # ---- the stream does what its row claims (the indices: against the length of the slot it was on in this piece)
                assert stats[1] < cur_len and (stats[1] < 0 or stats[0] >= 0), "stream %d: a read index outside [0, %d)" % (i, cur_len)
            loops[:, i] = l3
            assert stats[2] <= 8, "stream %d: %d live grains" % (i, stats[2])
            assert stats[3] >= 6 and stats[4] >= 4, "stream %d: %d births, %d deaths" % (i, stats[3], stats[4])
            assert stats[6] == 0, "stream %d: the draws ran out" % i
            assert has_rnd == (stats[7] > 0)
            assert len(np.unique(out[:, i])) > 50, "stream %d: constant output" % i
            if gh.LENS[slot] < gh.SAMPLE_DUR:
                assert stats[5] >= 4, "stream %d: the grains of a short slot wrap (%d wraps, %d births)" % (i, stats[5], stats[3])
            if i in gh.LOOP_STREAMS:
                ls, le = gh.loop_samples(gh.LENS[slot], *loop)
                assert (int(l3[0]), int(l3[1]), int(l3[2])) == (ls, le, le - ls), (i, l3)
                inside = (pos[:, i] >= ls) & (pos[:, i] < le)
                first = int(np.argmax(inside))
                assert inside[first:].all(), "stream %d leaves its loop after walking in" % i
                d = np.diff(pos[first:, i])
                rate = b[0]
                wraps = int((d < 0).sum()) if rate > 0 else int((d > 0).sum())
                assert wraps >= 2, "stream %d wraps %d times" % (i, wraps)
            Rf.gp_free(h)
            for x in [smp] + extra:
                Rf.gp_sample_free(x)
        # the walk-ins: stream 6 by 1 a sample, stream 8 by 16 a sample, stream 7 from above
        assert not (pos[:100, 6] >= 1000).any() and (pos[-1, 6] >= 1000), "stream 6 walks in slowly"
        assert (np.diff(pos[:40, 8]) == 17.0).all(), "stream 8 walks in by loopLength + rate a sample"
        assert pos[0, 7] == 3900.0 - 1.0 - 1024.0
        assert loops[0, 9] == int(0.25 * 777) and loops[1, 9] == 777 and loops[2, 9] == 777 - int(0.25 * 777), "stream 9: setLoopStart at the cut"
        assert (pos[601:, 9] >= loops[0, 9]).all() and (pos[:601, 9] < loops[0, 9]).any()
        assert loops[1, 10] == 777 and pos[1429, 10] == 1.0 and pos[1428, 10] > 1.0, "stream 10: setSample at the cut"
        # ---- tests/patches/stretch_loop_patch.cpp linked against the unmodified reference, run through oracle/example_host.cpp
        patch = os.path.join(ROOT, "tests", "patches", "stretch_loop_patch.cpp")
        exe = os.path.join(td, "example_sl")
        subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-I" + os.path.join(src, "libs"), "-o", exe,
                               os.path.join(ROOT, "oracle", "example_host.cpp"), patch, ref_sources[0], "-lm", "-lpthread"])
        raw = os.path.join(td, "sl.f64")
        subprocess.run([exe, str(gh.PATCH_SL_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        sl = np.fromfile(raw, np.float64).reshape(gh.PATCH_SL_FRAMES, 2)
        assert np.abs(sl[:9000, 0]).max() > 0.2 and np.abs(sl[9000:, 0]).max() > 0.2, "both halves of the patch sound"
        assert (sl[:, 1] == 0.5 * sl[:, 0]).all() and sl[:, 1].any(), "the loop members are what the setters made them"
        g["patch_sl"] = sl
        ref_sources.append(patch)
    g["out"], g["loops"] = out, loops
    for ci in range(len(CUTS) - 1):
        g["snap%d/st" % (ci + 1)], g["snap%d/gst" % (ci + 1)] = snaps[ci]
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    g["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h + libs/maxiGrains.h) and tests/patches/stretch_loop_patch.cpp sha256: %s; harness: "
        "tools/gen/grainpool_ref_dump.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    save_npz(OUT, g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 1000 * 1000


if __name__ == "__main__":
    main()
