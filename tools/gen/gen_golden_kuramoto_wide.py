#!/usr/bin/env python3
"""tools/gen/gen_golden_kuramoto_wide.py -- TEST INFRASTRUCTURE.  Writes tests/golden/kuramoto_wide.npz: mixes, phases and
states of the UNMODIFIED reference's maxiKuramotoOscillatorSet / maxiAsyncKuramotoOscillator for sets of 65 .. 1024 oscillators,
the sizes of kernel K26 (mxg_kuramoto_wide_render).

It is tools/gen/gen_golden_kuramoto.py for wider sets: the same harness (tools/gen/kuramoto_ref_dump.cpp, unchanged, compiled
with the reference's src/maximilian.cpp under oracle/Makefile's FPFLAGS into a temporary directory outside the tree), the same
record per case ("<case>/...": parameters, the mix at every sample, phase / gathered / update at every cut, the events, "tol" =
the reference's largest distance from the harness's long double restatement, "margin", "wraps") and the same assertions on the
reference's own output: every case wraps at least 3 times; one case ends synchronised and one does not; no phase of any case
lies within 1000 x that case's tol of 0 or of TWOPI (a failing case is re-seeded); and a case whose tol exceeds 1e-10 is refused
-- that is the chaotic regime, where two correct implementations part by 1e-4 .. 1 and the file could hold nobody to anything.

Cases, at a sample rate of 1000, in blocks cut at uneven positions (lengths 1 and 7 among them):
    n65, n128, n129         300 samples, on both sides of a second and a third wavefront; whole phase streams for n65 only
    ps1000                  N = 1000, freq and K per sample (int16 q, value = q / 256), 96 samples
    desync1024, sync1024    N = 1024 with K < 0 (ends spread over the circle) and K > 0 (ends in one point), 96 samples
    async_raise, async_never  async sets of 200: one told something at two cuts, one never told anything, 300 samples
96 samples at freq 40 are 3.84 turns: every oscillator wraps 3 or 4 times.  The exact form is N * N sines per sample in double
and in long double: the whole run takes a minute or two.

    python tools/gen/gen_golden_kuramoto_wide.py [--ref DIR]
"""
import argparse
import ctypes
import hashlib
import os
import platform
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_kuramoto import ROOT, TWOPI, circ, default_ref, fpflags, spread  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kuramoto_wide.npz")
MAX_BYTES = 416 * 1024      # the size of tests/golden/kuramoto.npz
MAX_TOL = 1e-10
P = ctypes.c_void_p
CUTS_300 = [0, 1, 8, 143, 250, 299, 300]
CUTS_96 = [0, 1, 8, 61, 96]
WHOLE = ("n65",)

# name, N, async, samples, cuts, freq, K; "ps": per sample
CASES = [
    ("n65", 65, 0, 300, CUTS_300, 15.0, 8.0),
    ("n128", 128, 0, 300, CUTS_300, -14.0, 3.0),
    ("n129", 129, 0, 300, CUTS_300, 17.0, -4.0),
    ("ps1000", 1000, 0, 96, CUTS_96, "ps", "ps"),
    ("desync1024", 1024, 0, 96, CUTS_96, 40.0, -5.0),
    ("sync1024", 1024, 0, 96, CUTS_96, 40.0, 150.0),
    ("async_raise", 200, 1, 300, CUTS_300, 16.0, 30.0),
    ("async_never", 200, 1, 300, CUTS_300, -15.0, 30.0),
]


def per_sample(ns):
    n = np.arange(ns)
    fq = np.round(256 * (40.0 + 6.0 * np.sin(2 * np.pi * n / 37.0))).astype(np.int16)      # 34 .. 46
    kq = np.round(256 * 6.0 * np.sin(2 * np.pi * n / 53.0 + 0.5)).astype(np.int16)         # both signs, through 0
    return fq, kq


def events(name, N, rng):
    """setPhase calls made at cuts: (cut, index, value)."""
    if name == "async_raise":
        return [(143, 1, float(rng.uniform(0, TWOPI))), (143, N - 1, 0.75), (250, 130, float(rng.uniform(0, TWOPI)))]
    return []


def run_case(R, name, N, asyn, ns, cuts, freq, K, seed):
    rng = np.random.default_rng(seed)
    phase0 = rng.uniform(0, TWOPI, N)
    ev = events(name, N, rng)
    raise0 = 1 if name == "async_raise" else 0
    sr = 1000
    R.kura_set_rate(sr)
    h = R.kura_new(N, asyn)
    dt = R.kura_dt(h)
    assert dt == TWOPI / sr
    l = R.kld_new(N, asyn, dt)
    R.kura_set_phases(h, phase0.ctypes.data, raise0)
    R.kld_set_phases(l, phase0.ctypes.data, raise0)
    fq, kq = per_sample(ns)
    f_arr = fq / 256.0 if freq == "ps" else np.array([freq])
    k_arr = kq / 256.0 if K == "ps" else np.array([K])
    mix, lmix = np.zeros(ns), np.zeros(ns)
    ph, lph = np.zeros((ns, N)), np.zeros((ns, N))
    snaps = {"phase": [], "gathered": [], "update": []}
    for a, b in zip(cuts[:-1], cuts[1:]):
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
    margin = float(min(ph.min(), (TWOPI - ph).min()))
    rec = {"N": np.int64(N), "async": np.int64(asyn), "sr": np.int64(sr), "seed": np.int64(seed), "phase0": phase0, "raise0": np.int64(raise0),
           "cuts": np.array(cuts, np.int64), "events": np.array(ev, np.float64).reshape(-1, 3), "mix": mix, "tol": np.float64(tol),
           "margin": np.float64(margin), "snap_phase": np.array(snaps["phase"]), "snap_update": np.array(snaps["update"], np.int32)}
    if asyn:
        rec["snap_gathered"] = np.array(snaps["gathered"])
    if freq == "ps":
        rec["freq_q"], rec["K_q"] = fq, kq
    else:
        rec["freq"], rec["K"] = np.float64(freq), np.float64(K)
    if name in WHOLE:
        rec["phases"] = ph
    wraps = int((np.abs(np.diff(ph, axis=0)) > np.pi).sum(axis=0).min())
    rec["wraps"] = np.int64(wraps)
    return rec, ph, tol, margin, wraps


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
        spreads = {}
        for ci, (name, N, asyn, ns, cuts, freq, K) in enumerate(CASES):
            assert cuts[0] == 0 and cuts[-1] == ns and 1 in np.diff(cuts) and 7 in np.diff(cuts)
            seed = 2600 + 10 * ci
            while True:
                rec, ph, tol, margin, wraps = run_case(R, name, N, asyn, ns, cuts, freq, K, seed)
                assert tol <= MAX_TOL, "%s: tol %.3e is the chaotic regime, not a reference" % (name, tol)
                if margin > 1000 * tol:
                    break
                print("  re-seeding %s: tol %.3e margin %.3e" % (name, tol, margin))
                seed += 1
                assert seed < 2600 + 10 * ci + 10, name
            assert wraps >= 3, (name, wraps)
            if asyn:
                if name == "async_never":
                    assert not rec["snap_update"].any() and not rec["snap_gathered"].any()
                else:
                    assert len(set(rec["events"][:, 0])) >= 2 and (rec["snap_gathered"][0] == rec["phase0"]).all()
            spreads[name] = spread(ph[-1])
            print("%-12s N %4d  tol %.3e  margin %.3e  wraps %3d  final spread %.3e  seed %d" % (name, N, tol, margin, wraps, spreads[name],
                                                                                                 seed), flush=True)
            for k, arr in rec.items():
                out[name + "/" + k] = arr
        R.kura_set_rate(44100)
        assert spreads["desync1024"] > 1 and spreads["sync1024"] < 1e-6, spreads
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    out["libc"] = np.array(" ".join(platform.libc_ver()))
    out["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; "
        "harness: tools/gen/kuramoto_ref_dump.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    out["cases"] = np.array([c[0] for c in CASES])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < MAX_BYTES


if __name__ == "__main__":
    main()
