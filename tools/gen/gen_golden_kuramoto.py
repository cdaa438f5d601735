#!/usr/bin/env python3
"""tools/gen/gen_golden_kuramoto.py -- TEST INFRASTRUCTURE.  Writes tests/golden/kuramoto.npz: mixes, phases and states of the
UNMODIFIED reference's maxiKuramotoOscillatorSet / maxiAsyncKuramotoOscillator for the cases below, and the stream of
tests/patches/kuramoto_patch.cpp.

It compiles tools/gen/kuramoto_ref_dump.cpp with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling
checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary directory outside the tree,
and records the compiler, flags, libc and the sha256 of the reference sources inside the file.  Nothing else in the tree changes.

Cases ("<case>/..."): one set of N oscillators, 3000 samples at a sample rate of 1000 (one case: 44 100), played in blocks cut at
uneven positions (lengths 1 and 7 among them).  Initial phases are seeded uniform in [0, 2 pi).  Stored per case: the parameters,
the mix whole, phase / gathered / update at every cut ("snap_*", row i = after the block that ends at cuts[i + 1]), the whole
phase streams of the cases in WHOLE, the events (setPhase calls made at cuts: cut, index, value), and "tol".

The file is held under 500 KB, and a stream of 3000 doubles is 24 KB that does not compress: the 14 mixes are 336 KB, so whole
phase streams are kept for n2 and n3 only (n1's phase IS its mix: N = 1 divides by 1.0).  Every other case is checked on its
mix at every sample and on its phases at every cut.

"<case>/tol": the generator runs a long double restatement of the recurrence (kuramoto_ref_dump.cpp, kld_*) beside the
reference and stores the reference's largest distance from it over all samples, phases (on the circle) and mix: the measured
size of the reference's own accumulated rounding, which is what a second implementation of the same recurrence may differ by.

The generator ASSERTS on the reference's own output: every case with freq != 0 wraps at least 3 times; a negative-freq case wraps
through 0; at least one case ends desynchronised (final phase spread > 1) and one synchronised; no phase of any case comes
within 1000 x that case's tol of 0 or of TWOPI (the phase after the wrap is within that distance of 0 or TWOPI exactly when the
phase before the wrap is, so the wrap decision of a model within tol cannot differ).  A case that fails the last is re-seeded.

    python tools/gen/gen_golden_kuramoto.py [--ref DIR]
"""
import argparse
import ctypes
import hashlib
import os
import platform
import re
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(ROOT, "tests", "golden", "kuramoto.npz")
NS = 3000
TWOPI = 6.283185307179586476925286766559
CUTS = [0, 1, 8, 143, 999, 1000, 1429, 2500, 2999, NS]
PATCH_FRAMES = 4100
WHOLE = ("n2", "n3")
P = ctypes.c_void_p

# name, N, async, sample rate, freq, K; "ps": per sample (int16 q, value = q / 256)
CASES = [
    ("n1", 1, 0, 1000, 3.0, 5.0),
    ("n2", 2, 0, 1000, -2.0, 4.0),
    ("n3", 3, 0, 1000, 1.5, -5.0),
    ("n5", 5, 0, 1000, 2.5, 0.0),
    ("n31", 31, 0, 1000, 4.0, 20.0),
    ("n32", 32, 0, 1000, -3.0, -5.0),
    ("n33", 33, 0, 1000, 2.0, 8.0),
    ("n63", 63, 0, 1000, 5.0, 3.0),
    ("n64", 64, 0, 1000, 3.0, 50.0),
    ("ps", 5, 0, 1000, "ps", "ps"),
    ("setp", 7, 0, 1000, 2.0, 6.0),
    ("async_raise", 3, 1, 1000, 2.0, 30.0),
    ("async_never", 5, 1, 1000, -1.5, 30.0),
    ("kt", 2, 0, 44100, 60.0, 1900.0),
]


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def per_sample():
    n = np.arange(NS)
    fq = np.round(256 * (3.0 + 2.5 * np.sin(2 * np.pi * n / 700.0))).astype(np.int16)          # 0.5 .. 5.5
    kq = np.round(256 * 3.0 * np.sin(2 * np.pi * n / 1100.0 + 0.5)).astype(np.int16)         # both signs, through 0
    return fq, kq


def events(name, N, rng):
    """setPhase calls made at cuts: (cut, index, value)."""
    if name == "setp":
        return [(143, 0, float(rng.uniform(0, TWOPI))), (1000, 6, float(rng.uniform(0, TWOPI))), (1000, 3, 0.5), (2500, 2, 6.0)]
    if name == "async_raise":
        return [(999, 1, float(rng.uniform(0, TWOPI))), (1429, 2, float(rng.uniform(0, TWOPI))), (2999, 0, 1.25)]
    return []


def circ(d):
    d = np.abs(d) % TWOPI
    return np.minimum(d, TWOPI - d)


def spread(p):
    s = np.sort(np.asarray(p) % TWOPI)
    if len(s) < 2:
        return 0.0
    gaps = np.diff(np.concatenate([s, [s[0] + TWOPI]]))
    return float(TWOPI - gaps.max())


def run_case(R, name, N, asyn, sr, freq, K, seed):
    rng = np.random.default_rng(seed)
    phase0 = rng.uniform(0, TWOPI, N)
    ev = events(name, N, rng)
    raise0 = 1 if name == "async_raise" else 0
    R.kura_set_rate(sr)
    h = R.kura_new(N, asyn)
    dt = R.kura_dt(h)
    assert dt == TWOPI / sr
    l = R.kld_new(N, asyn, dt)
    R.kura_set_phases(h, phase0.ctypes.data, raise0)
    R.kld_set_phases(l, phase0.ctypes.data, raise0)
    fq, kq = per_sample()
    f_arr = fq / 256.0 if freq == "ps" else np.array([freq])
    k_arr = kq / 256.0 if K == "ps" else np.array([K])
    mix, lmix = np.zeros(NS), np.zeros(NS)
    ph, lph = np.zeros((NS, N)), np.zeros((NS, N))
    snaps = {"phase": [], "gathered": [], "update": []}
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        for cut, idx, val in ev:
            if cut == a:
                R.kura_set_phase(h, val, idx)
                R.kld_set_phase(l, val, idx)
        fb = np.ascontiguousarray(f_arr[a:b]) if freq == "ps" else f_arr
        kb = np.ascontiguousarray(k_arr[a:b]) if K == "ps" else k_arr
        for play, hh, m, p in ((R.kura_play, h, mix, ph), (R.kld_play, l, lmix, lph)):
            mo, po = np.zeros(b - a), np.zeros((b - a, N))
            play(hh, b - a, fb.ctypes.data, int(freq == "ps"), kb.ctypes.data, int(K == "ps"), mo.ctypes.data, po.ctypes.data)
            m[a:b], p[a:b] = mo, po
        sp, sg, su = np.zeros(N), np.zeros(N), np.zeros(1, np.int32)
        R.kura_state(h, sp.ctypes.data, sg.ctypes.data, su.ctypes.data)
        assert np.array_equal(sp, ph[b - 1])
        snaps["phase"].append(sp)
        snaps["gathered"].append(sg)
        snaps["update"].append(su[0])
    R.kura_free(h)
    R.kld_free(l)
    tol = float(max(circ(ph - lph).max(), np.abs(mix - lmix).max()))
    # a mix can differ by TWOPI / N where the two wrapped on different samples; the margin below rules that out, so check it first
    margin = float(min(ph.min(), (TWOPI - ph).min()))
    rec = {"N": np.int64(N), "async": np.int64(asyn), "sr": np.int64(sr), "seed": np.int64(seed), "phase0": phase0, "raise0": np.int64(raise0),
           "cuts": np.array(CUTS, np.int64), "events": np.array(ev, np.float64).reshape(-1, 3), "mix": mix, "tol": np.float64(tol),
           "margin": np.float64(margin), "snap_phase": np.array(snaps["phase"]), "snap_update": np.array(snaps["update"], np.int32)}
    if asyn:
        rec["snap_gathered"] = np.array(snaps["gathered"])
    if freq == "ps":
        rec["freq_q"], rec["K_q"] = fq, kq
    else:
        rec["freq"], rec["K"] = np.float64(freq), np.float64(K)
    if name in WHOLE:
        rec["phases"] = ph
    wraps = int((np.abs(np.diff(ph, axis=0)) > np.pi).sum(axis=0).min()) if NS > 1 else 0
    down = bool(((np.diff(ph, axis=0) > np.pi).sum(axis=0) >= 1).all())   # a rise by almost TWOPI: the phase went below 0
    rec["wraps"] = np.int64(wraps)
    return rec, ph, tol, margin, wraps, down


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "maximilian.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    out = {}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libkuraref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "kuramoto_ref_dump.cpp"), ref_sources[0], "-lm"])
        R = ctypes.CDLL(so)
        for fn in (R.kura_new, R.kld_new):
            fn.restype = P
        R.kura_new.argtypes = [ctypes.c_size_t, ctypes.c_int]
        R.kld_new.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_double]
        R.kura_dt.restype = ctypes.c_double
        R.kura_dt.argtypes = [P]
        R.kura_set_rate.argtypes = [ctypes.c_int]
        for fn in (R.kura_free, R.kld_free):
            fn.argtypes = [P]
        for fn in (R.kura_set_phases, R.kld_set_phases):
            fn.argtypes = [P, P, ctypes.c_int]
        for fn in (R.kura_set_phase, R.kld_set_phase):
            fn.argtypes = [P, ctypes.c_double, ctypes.c_size_t]
        for fn in (R.kura_play, R.kld_play):
            fn.argtypes = [P, ctypes.c_size_t, P, ctypes.c_int, P, ctypes.c_int, P, P]
        R.kura_state.argtypes = [P, P, P, P]
        spreads, through_zero = {}, False
        for ci, (name, N, asyn, sr, freq, K) in enumerate(CASES):
            seed = 1700 + 10 * ci
            while True:
                rec, ph, tol, margin, wraps, down = run_case(R, name, N, asyn, sr, freq, K, seed)
                if margin > 1000 * tol:
                    break
                print("  re-seeding %s: tol %.3e margin %.3e" % (name, tol, margin))
                seed += 1
                assert seed < 1700 + 10 * ci + 10, name
            assert margin > 1000 * tol, (name, margin, tol)
            assert wraps >= 3, (name, wraps)
            if not isinstance(freq, str) and freq < 0:
                assert down, name
                through_zero = True
            if asyn:
                if name == "async_never":
                    assert not rec["snap_update"].any() and not rec["snap_gathered"].any()
                else:
                    assert rec["events"].shape[0] >= 2 and (rec["snap_gathered"][0] == rec["phase0"]).all()
            spreads[name] = spread(ph[-1])
            print("%-12s N %2d  tol %.3e  margin %.3e  wraps %3d  final spread %.4f  seed %d" % (name, N, tol, margin, wraps, spreads[name], seed))
            for k, arr in rec.items():
                out[name + "/" + k] = arr
        R.kura_set_rate(44100)
        assert through_zero
        assert any(s > 1 for n, s in spreads.items() if out[n + "/N"] > 1), spreads
        assert any(s < 1e-6 for n, s in spreads.items() if out[n + "/N"] > 1), spreads

        # ---- the patch's stream: tests/patches/kuramoto_patch.cpp + oracle/example_host.cpp (read only) + the reference ---------
        exe = os.path.join(td, "patch")
        subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-o", exe, os.path.join(ROOT, "oracle", "example_host.cpp"),
                               os.path.join(ROOT, "tests", "patches", "kuramoto_patch.cpp"), ref_sources[0], "-lm", "-lpthread"])
        raw = os.path.join(td, "patch.f64")
        subprocess.run([exe, str(PATCH_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        s = np.fromfile(raw, np.float64).reshape(PATCH_FRAMES, 2)
        assert np.isfinite(s).all() and len(np.unique(s[:, 0])) > 0.9 * PATCH_FRAMES and len(np.unique(s[:, 1])) > 0.9 * PATCH_FRAMES
        out["patch"] = s
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    out["libc"] = np.array(" ".join(platform.libc_ver()))
    out["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; "
        "harness: tools/gen/kuramoto_ref_dump.cpp; patch: tests/patches/kuramoto_patch.cpp via oracle/example_host.cpp"
        % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    out["cases"] = np.array([c[0] for c in CASES])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 500000


if __name__ == "__main__":
    main()
