#!/usr/bin/env python3
"""tools/gen/gen_golden_bands.py -- TEST INFRASTRUCTURE.  Writes tests/golden/bands.npz: what the UNMODIFIED reference's maxiBark
(src/libs/maxiBark.h) and maxiFFTOctaveAnalyzer (src/libs/maxiFFT.cpp) compute for the cases below.

It compiles tools/gen/bands_ref_dump.cpp with the reference's src/libs/maxiFFT.cpp, fft.cpp and src/maximilian.cpp (path:
$MAXI_REF, default the checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary directory outside the tree,
and records the compiler, flags, libc and the sha256 of the reference sources inside the file.  Nothing else in the tree changes.

What is stored (tests/bands_host.py derives every input from a seed, for this script and the tests alike):
  bark/<i>/...: for each of bands_host.BARK_CONFIGS the 25 limits and specific / relative / total of bands_host.bark_spectra(9,
  bins, BARK_SEED): magnitudes with a dynamic range of 2^60 inside every band, frame 1 silent, frame 2 with a NaN bin, frame 3 with
  negative band sums, frame 4 with an Inf;
  oct/<i>/...: for each of bands_host.OCTAVE_CONFIGS the map, nAverages and, for each of bands_host.OCTAVE_RUNS (hold time, decay,
  EQ slope), averages / peaks / peakHoldTimes after every one of the 44 frames of bands_host.octave_spectra(44, n, OCTAVE_SEED)
  (one NaN frame), the analyser's arrays zeroed after setup();
  patch: the stream of tests/patches/bands_patch.cpp built against the reference (bands_host.PATCH_FRAMES samples, 2 channels).

The generator ASSERTS on the reference's own output: limit 24 reads back as specSize - 1; every Bark band is non-empty in some
configuration and 19 of the 24 are empty in another (band 0 never can be); the dynamic range of at least 2^30 inside one band
is asserted on band 23 of frame 0 wherever that band has 16 bins or more (all but (44100, 16), whose widest band has 6);
relative is exactly 1.0 at each frame's maximum; the silent frame is 24 NaNs; every octave band is seen rising, holding,
counting down and decaying.

    python tools/gen/gen_golden_bands.py [--ref DIR]
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
import bands_host as bh  # noqa: E402  (the derived inputs: one place for this script and the tests)

OUT = os.path.join(ROOT, "tests", "golden", "bands.npz")
P, S, I, F, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_uint


def oracle_var(name, op):
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^%s\s*%s\s*(.*)$" % (name, op), txt, re.M).group(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MAXI_REF") or oracle_var("REF", r"\?=").split()[0])
    args = ap.parse_args()
    libs = os.path.join(args.ref, "src", "libs")
    ref_sources = [os.path.join(libs, f) for f in ("maxiFFT.cpp", "fft.cpp", "maxiBark.h", "maxiFFT.h")] + [os.path.join(args.ref, "src", "maximilian.cpp")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + oracle_var("FPFLAGS", "=").split() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    g = {}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libbandsref.so")
        subprocess.check_call([cxx] + flags + ["-I" + os.path.join(args.ref, "src"), "-I" + libs, "-o", so,
                               os.path.join(HERE, "bands_ref_dump.cpp"), ref_sources[0], ref_sources[1], ref_sources[4], "-lm"])
        R = ctypes.CDLL(so)
        R.bnd_ref_bark.argtypes = [U, U, P, S, S, P, P, P, P]
        R.bnd_ref_octave_new.restype = P
        R.bnd_ref_octave_new.argtypes = [F, I, I]
        R.bnd_ref_octave_info.argtypes = [P, P]
        R.bnd_ref_octave_calc.argtypes = [P, P, S, S, I, F, F, F, P, P, P]
        R.bnd_ref_octave_free.argtypes = [P]

        # ---- maxiBark ------------------------------------------------------------------------------------------------------
        empty, full = np.zeros(24, bool), np.zeros(24, bool)
        for i, (sR, bS) in enumerate(bh.BARK_CONFIGS):
            bins = bS // 2
            x = bh.bark_spectra(bh.BARK_FRAMES, bins, bh.BARK_SEED)
            lim = np.zeros(25, np.int32)
            sp, rl, tt = np.zeros((bh.BARK_FRAMES, 24)), np.zeros((bh.BARK_FRAMES, 24)), np.zeros(bh.BARK_FRAMES)
            R.bnd_ref_bark(sR, bS, x.ctypes.data, bins, bh.BARK_FRAMES, lim.ctypes.data, sp.ctypes.data, rl.ctypes.data, tt.ctypes.data)
            assert lim[24] == bins - 1, "the reference's bbLimits[24] does not read back as specSize - 1: %r" % (lim,)
            assert lim[0] == 0 and (np.diff(lim) >= 0).all(), lim
            empty |= np.diff(lim) == 0
            full |= np.diff(lim) > 0
            assert np.isnan(rl[1]).all() and (sp[1] == 0).all() and tt[1] == 0, "the silent frame is not 24 NaNs"
            assert np.isnan(sp[2]).sum() == 1 and np.isnan(sp[3]).any() and np.isinf(sp[4]).sum() == 1
            ok = np.isfinite(sp).all(axis=1) & (sp.max(axis=1) > 0)
            assert ok.sum() >= 5 and (rl[ok].max(axis=1) == 1.0).all(), "relative is not exactly 1.0 at a frame's maximum"
            lo, hi = int(lim[23]), int(lim[24])
            if hi - lo >= 16:   # a dynamic range of at least 2^30 inside the widest band
                assert x[0, lo:hi].max() / x[0, lo:hi].min() >= 2.0 ** 30
            g["bark/%d/limits" % i], g["bark/%d/specific" % i], g["bark/%d/relative" % i], g["bark/%d/total" % i] = lim, sp, rl, tt
        # every band is summed somewhere; 19 of the 24 are also empty somewhere.  Band 0 can never be empty (barkScale[0] = 0 passes no
        # edge, so limit 1 is at least 1), and bands 15, 19, 22 and 23 are non-empty in all five configurations.
        assert full.all() and empty.sum() >= 19 and not empty[0], ("Bark bands: empty / non-empty coverage", empty, full)

        # ---- maxiFFTOctaveAnalyzer --------------------------------------------------------------------------------------------
        for i, (sr, n, per) in enumerate(bh.OCTAVE_CONFIGS):
            x = bh.octave_spectra(bh.OCTAVE_FRAMES, n, bh.OCTAVE_SEED)
            for r, (hold, decay, slope) in enumerate(bh.OCTAVE_RUNS):
                h = R.bnd_ref_octave_new(sr, n, per)
                m = np.zeros(n, np.int32)
                nA = R.bnd_ref_octave_info(h, m.ctypes.data)
                av, pk = np.zeros((bh.OCTAVE_FRAMES, nA), np.float32), np.zeros((bh.OCTAVE_FRAMES, nA), np.float32)
                hd = np.zeros((bh.OCTAVE_FRAMES, nA), np.int32)
                R.bnd_ref_octave_calc(h, x.ctypes.data, n, bh.OCTAVE_FRAMES, hold, decay, 1.0, slope, av.ctypes.data, pk.ctypes.data, hd.ctypes.data)
                R.bnd_ref_octave_free(h)
                g["oct/%d/map" % i], g["oct/%d/nAverages" % i] = m, np.int32(nA)
                g["oct/%d/%d/averages" % (i, r)], g["oct/%d/%d/peaks" % (i, r)], g["oct/%d/%d/holds" % (i, r)] = av, pk, hd
                assert np.isnan(av[9]).any() and np.isfinite(av[:9]).all()
                if hold > 0 and 0 < decay < 1:   # every band rising, holding, counting down and decaying
                    fin = np.isfinite(pk).all(axis=0)
                    d = np.diff(pk, axis=0)
                    assert fin.any()
                    assert (d > 0).any(axis=0)[fin].all() and (d < 0).any(axis=0)[fin].all(), "a band never rises or never decays"
                    assert (hd == hold).any(axis=0)[fin].all() and (np.diff(hd, axis=0) == -1).any(axis=0)[fin].all(), "a band never holds"
                    assert ((d == 0) & (hd[1:] < hd[:-1])).any(axis=0)[fin].all(), "a band never counts down on a held peak"
        # ---- the patch's stream: tests/patches/bands_patch.cpp + oracle/example_host.cpp (read only) + the reference --------------
        exe = os.path.join(td, "patch")
        subprocess.check_call([cxx, "-std=c++17"] + oracle_var("FPFLAGS", "=").split() + ["-w", "-I" + os.path.join(args.ref, "src"), "-o", exe,
                               os.path.join(ROOT, "oracle", "example_host.cpp"), os.path.join(ROOT, "tests", "patches", "bands_patch.cpp"),
                               ref_sources[4], ref_sources[0], ref_sources[1], "-lm", "-lpthread"])
        raw = os.path.join(td, "patch.f64")
        subprocess.run([exe, str(bh.PATCH_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        st = np.fromfile(raw, np.float64).reshape(bh.PATCH_FRAMES, 2)
        assert np.isfinite(st).all() and (st[600:, 0] != 0).mean() > 0.5 and (st[600:, 1] != 0).mean() > 0.5 and len(np.unique(st)) > 500
        g["patch"] = st
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    g["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/libs/maxiFFT.cpp, fft.cpp, maxiBark.h, maxiFFT.h, src/maximilian.cpp) sha256: %s; "
        "harness: tools/gen/bands_ref_dump.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 500 * 1000


if __name__ == "__main__":
    main()
