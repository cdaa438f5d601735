#!/usr/bin/env python3
"""tools/gen/gen_golden_shaper.py -- TEST INFRASTRUCTURE.  Writes tests/golden/shaper.npz: outputs and states of the UNMODIFIED
reference's maxiNonlinearity, maxiXFade, maxiSelect, maxiSelectX and maxiLine for the cases below, and the stream of
tests/patches/shaper_patch.cpp.

It compiles tools/gen/shaper_ref_dump.cpp with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling checkout
the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary directory outside the tree, and
records the compiler, flags, libc and the sha256 of the reference sources inside the file.  Nothing else in the tree changes.

What is stored (tests/shaper_host.py derives every input from the stored integers, for this script and the tests alike):
  q int16 [2000][3] (the signal is q / 16384.0, in [-1.5, 1.5]) + patches (n, v, value): exact +-1, 0.0, -0.0, one NaN;
  shape/pv/<mode>: every maxiNonlinearity call with per-voice parameters over the whole signal (asymclip: voices 0 and 1, the
  patched -0.0 samples are in voice 2); shape/ps/<mode>: the three parameterised calls with a parameter per sample (pq int16)
  over the first 400 samples; asym_zero: asymclip of -0.0 under three exponents; softclip_u: softclip of 3000 uniform draws with
  full mantissas (the quantised signal's cubes are exact in a double);
  xfade/ps, xfade/pv: two channels cross-faded by an xfader per sample (it passes both clamps) / per voice;
  sel/const, sel/sig: maxiSelect and maxiSelectX over 5 constants (index in [-0.5, 5.5]) and over 4 signals (normalised index in
  [-0.1, 1.1]);
  line/...: 5 maxiLine objects (one-shot, looping, descending, disabled then enabled, prepared again at two cuts) on trigger
  blocks cut at uneven positions (lengths 1 and 7 among them), parameters and state at every cut; line_const: line.play(1).

The generator ASSERTS on the reference's own output that every shaping mode takes every branch in every voice, that every
select voice reads every element and SelectX wraps a2, that every line voice is seen starting, running, completing and
re-arming, and that the xfader passes both clamps: a test can then not pass on rows of zeros.

    python tools/gen/gen_golden_shaper.py [--ref DIR]
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
import shaper_host as sh  # noqa: E402  (the derived inputs: one place for this script and the tests)

OUT = os.path.join(ROOT, "tests", "golden", "shaper.npz")
N, V, SR = 2000, 3, 1000
CUTS = [0, 1, 8, 143, 600, 601, 1429, 1993, N]
PATCH_FRAMES = 4000
P, S, I, D = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
NAN = float("nan")
PATCHES = [(10, 0, 1.0), (11, 0, -1.0), (50, 1, 1.0), (51, 1, -1.0), (60, 2, 1.0), (61, 2, -1.0),   # exact +-1: the clipped branches' edge
           (142, 0, 1.0), (143, 0, -1.0),                                                            # ... on the last / first sample of a block
           (20, 0, 0.0), (21, 1, 0.0), (22, 2, 0.0), (30, 2, -0.0), (900, 2, -0.0), (1700, 1, NAN)]
SHAPE_PV = [0.5, 3.7, 50.0]
ASYM_A, ASYM_B = [0.25, 8.0], [3.0, 0.6]
XFADE_PV = [-1.2, 0.3, 1.0]
SEL_CONST = [[0.5, -1.0, 2.0], [1.5, 0.25, -3.0], [-0.75, 4.0, 0.125], [2.5, -2.0, 1.0], [-4.0, 0.0625, 8.0]]
LINE_V = 5
# (sample, kind, voice, start / on, end, ms, oneshot): kind 0 = prepare, 1 = triggerEnable
LINE_EVENTS = [(0, 0, 0, 0.0, 1.0, 100.0, 1), (0, 0, 1, 0.0, 1.0, 70.0, 0), (0, 0, 2, 1.0, -1.0, 90.0, 0), (0, 0, 3, 0.25, 1.0, 30.0, 0),
               (0, 0, 4, 0.5, 2.0, 33.3, 1), (0, 1, 0, 1.0, 0, 0, 0), (0, 1, 1, 1.0, 0, 0, 0), (0, 1, 2, 0.5, 0, 0, 0), (0, 1, 3, -1.0, 0, 0, 0),
               (0, 1, 4, 1.0, 0, 0, 0),
               (143, 0, 3, 0.75, 1.5, 30.0, 0),     # prepared while disabled: lineValue shows the PREVIOUS start until it is enabled
               (601, 0, 0, 0.0, 1.0, 100.0, 1), (601, 1, 3, 0.5, 0, 0, 0), (601, 0, 4, 2.0, 0.5, 45.0, 1),
               (1429, 0, 4, -1.0, 1.0, 20.0, 0)]
LINE_PERIOD = [160, 110, 130, 90, 75]


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def signals():
    """Sines of a few periods under a tremolo that carries them past +-1, a little noise; int16 of x * 16384."""
    rng = np.random.default_rng(1800)
    n = np.arange(N)[:, None]
    v = np.arange(V)[None, :]
    x = 1.45 * np.sin(2 * np.pi * n * (7.0 + 3.0 * v) / N + v) * (0.6 + 0.4 * np.sin(2 * np.pi * n * (31.0 + 5 * v) / N)) + 0.05 * rng.standard_normal((N, V))
    return np.round(np.clip(x, -1.5, 1.5) * 16384).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "maximilian.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    rng = np.random.default_rng(1801)
    g = {"q": signals(), "patches": np.array(PATCHES, np.float64), "cuts": np.array(CUTS, np.int64), "sr": np.int64(SR),
         "pq": rng.integers(-32768, 32768, (sh.NPS, V)).astype(np.int16)}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libshpref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "shaper_ref_dump.cpp"), ref_sources[0], "-lm"])
        R = ctypes.CDLL(so)
        R.shp_set_rate.argtypes = [I]
        R.shp_shape.argtypes = [I, S, P, P, P, P]
        R.shp_xfade.argtypes = [S, S, P, P, P, P]
        R.shp_select.argtypes = [I, S, S, P, P, I, P]
        R.shp_line_new.restype = P
        R.shp_line_new.argtypes = [S]
        R.shp_line_free.argtypes = [P]
        R.shp_line_prepare.argtypes = [P, S, D, D, D, I]
        R.shp_line_enable.argtypes = [P, S, D]
        R.shp_line_play.argtypes = [P, S, P, D, P, P, P]
        R.shp_line_state.argtypes = [P, P, P]
        R.shp_set_rate(SR)
        libm = ctypes.CDLL("libm.so.6")
        libm.atan.restype = D
        libm.atan.argtypes = [D]
        x = sh.signal(g)
        assert 20000 < np.abs(g["q"]).max() <= 24576 and np.isnan(x).sum() == 1

        # ---- maxiNonlinearity ----------------------------------------------------------------------------------------------
        def shape(mode, xs, a, b):
            xs = np.ascontiguousarray(xs)
            a, b = (np.ascontiguousarray(np.broadcast_to(np.zeros(1) if t is None else t, xs.shape)) for t in (a, b))
            o = np.zeros(xs.shape)
            R.shp_shape(sh.MODES[mode], xs.size, xs.ctypes.data, a.ctypes.data, b.ctypes.data, o.ctypes.data)
            return o

        g["shape/pv/shape"], g["shape/pv/asym_a"], g["shape/pv/asym_b"] = np.array(SHAPE_PV), np.array(ASYM_A), np.array(ASYM_B)
        g["shape/pv/norm"] = np.array([1.0 / libm.atan(s) for s in SHAPE_PV])
        shape_ps, a_ps, b_ps = sh.per_sample_params(g)
        assert shape_ps.min() >= 0.5 and shape_ps.max() <= 50 and a_ps.min() >= 0.25 and b_ps.max() <= 8
        for mode in sh.MODES:
            xs = x[:, :sh.ASYM_V] if mode == "asymclip" else x
            o = shape(mode, xs, g["shape/pv/asym_a"] if mode == "asymclip" else g["shape/pv/shape"], g["shape/pv/asym_b"] if mode == "asymclip" else None)
            fin = ~np.isnan(xs)
            assert np.array_equal(np.isnan(o), ~fin), mode
            hi, lo, mid = xs >= 1, xs <= -1, (np.abs(xs) < 1)
            if mode in ("hardclip", "softclip", "asymclip"):   # every branch in every voice, the exact +-1 among them
                assert (o[hi] == 1).all() and (o[lo] == -1).all() and (np.abs(o[mid]) < 1).all(), mode
                assert hi.any(axis=0).all() and lo.any(axis=0).all() and mid.any(axis=0).all() and (xs == 1).any(axis=0).all() and (xs == -1).any(axis=0).all()
            if mode == "asymclip":
                assert (mid & (xs < 0)).any(axis=0).all() and (mid & (xs > 0)).any(axis=0).all() and not (np.signbit(xs) & (xs == 0)).any()
                assert len(np.unique(o[mid])) > 1000
            elif mode == "softclip":   # x - cube / 3.0 of -0.0 is -0.0 - -0.0 = +0.0
                assert (np.signbit(xs) & (xs == 0)).any() and not np.signbit(o[xs == 0]).any()
            else:
                assert (np.signbit(xs) & (xs == 0)).any() and np.array_equal(np.signbit(o[xs == 0]), np.signbit(xs[xs == 0])), mode
            if mode == "hardclip":
                assert np.array_equal(o.astype(np.float32).astype(np.float64)[fin], o[fin])
                o = o.astype(np.float32)
            g["shape/pv/" + mode] = o
            if mode in sh.PARAM_MODES:
                a, b = (a_ps, b_ps) if mode == "asymclip" else (shape_ps, None)
                g["shape/ps/" + mode] = shape(mode, xs[:sh.NPS], a, b)
                assert np.isfinite(g["shape/ps/" + mode]).all() and len(np.unique(g["shape/ps/" + mode])) > sh.NPS
        # full-mantissa inputs: the quantised signal's cubes are exact, these are where (x * x) * x and pow(x, 3) can differ
        g["softclip_u/x"] = rng.uniform(-1.0, 1.0, (1500, 2))
        g["softclip_u/out"] = shape("softclip", g["softclip_u/x"], None, None)
        g["asym_zero/x"] = np.full((3, 1), -0.0)
        g["asym_zero/a"] = np.full((3, 1), 2.0)
        g["asym_zero/b"] = np.array([[3.0], [2.0], [0.5]])
        g["asym_zero/out"] = shape("asymclip", g["asym_zero/x"], g["asym_zero/a"], g["asym_zero/b"])
        assert np.signbit(g["asym_zero/out"]).ravel().tolist() == [True, False, False]   # pow(-0.0, odd integer) keeps the sign

        # ---- maxiXFade -------------------------------------------------------------------------------------------------------
        def xfade(ch1, ch2, xf):
            ch1, ch2 = np.ascontiguousarray(ch1), np.ascontiguousarray(ch2)
            xf = np.ascontiguousarray(np.broadcast_to(xf, ch1.shape[-2:]))
            o = np.zeros(ch1.shape)
            R.shp_xfade(1 if ch1.ndim == 2 else ch1.shape[0], xf.size, ch1.ctypes.data, ch2.ctypes.data, xf.ctypes.data, o.ctypes.data)
            return o

        ch1, ch2, xf = sh.xfade_inputs(g)
        assert (xf > 1).any(axis=0).all() and (xf < -1).any(axis=0).all() and (np.abs(xf) < 1).any(axis=0).all(), "the xfader misses a clamp"
        g["xfade/ps"] = xfade(ch1, ch2, xf)
        mono = xfade(ch1[0], ch2[0], xf)   # the mono overload gives the vector one's bits
        assert np.array_equal(mono.view(np.uint64), g["xfade/ps"][0].view(np.uint64))
        assert np.array_equal(g["xfade/ps"][0][xf >= 1], ch2[0][xf >= 1], equal_nan=True) and np.array_equal(g["xfade/ps"][0][xf <= -1], ch1[0][xf <= -1], equal_nan=True)
        g["xfade/pv_xf"] = np.array(XFADE_PV)
        g["xfade/pv"] = xfade(ch1[:, :sh.NXV], ch2[:, :sh.NXV], g["xfade/pv_xf"])

        # ---- maxiSelect / maxiSelectX ------------------------------------------------------------------------------------------
        g["sel/const/values"] = np.array(SEL_CONST)
        g["sel/sig/vq"] = np.round(np.clip(rng.standard_normal((4, sh.NX, V)) * 0.5, -1.5, 1.5) * 16384).astype(np.int16)
        for name, (index, values, normalised) in sh.select_inputs(g).items():
            K = values.shape[0]
            vals = np.ascontiguousarray(np.broadcast_to(values[:, None, :], (K, sh.NX, V)) if values.ndim == 2 else values)
            index = np.ascontiguousarray(index)
            scaled = index * (K - 1e-9) if normalised else index
            assert (scaled < 0).any(axis=0).all() and (scaled >= K).any(axis=0).all(), "the index misses a clamp"
            a1 = np.floor(np.clip(scaled, 0, K - 1)).astype(int)
            for k in range(K):
                assert (a1 == k).any(axis=0).all(), "a select voice never reads element %d" % k
            assert ((a1 == K - 1) & (scaled > K - 1) & (scaled < K)).any(axis=0).all(), "SelectX never wraps a2 with a non-zero mix"
            for interp, key in ((0, "select"), (1, "selectx")):
                o = np.zeros((sh.NX, V))
                R.shp_select(interp, K, index.size, index.ctypes.data, vals.ctypes.data, int(normalised), o.ctypes.data)
                g["sel/%s/%s" % (name, key)] = o
            assert len(np.unique(g["sel/%s/selectx" % name])) > sh.NX

        # ---- maxiLine ----------------------------------------------------------------------------------------------------------
        n = np.arange(N)[:, None]
        per = np.array(LINE_PERIOD)[None, :]
        low = np.where(np.arange(LINE_V) % 2 == 1, 0, -1)[None, :]          # odd voices fall to exactly 0.0, even ones to -0.25
        g["line/tq"] = np.where((n % per) < 0.4 * per, np.where(n % 3 == 0, 4, 2), low).astype(np.int8)
        g["line/events"] = np.array(LINE_EVENTS, np.float64)
        trig = sh.line_trigger(g)
        ev = sh.line_events(g)

        def apply(h, at):
            for kind, v, p0, p1, ms, one in ev.get(at, []):
                if kind == 0:
                    R.shp_line_prepare(h, v, p0, p1, ms, one)
                else:
                    R.shp_line_enable(h, v, p0)

        h = R.shp_line_new(LINE_V)
        out, trg, done = (np.zeros((N, LINE_V)) for _ in range(3))
        for i, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
            apply(h, a)
            o, t, d = (np.zeros((b - a, LINE_V)) for _ in range(3))
            tb = np.ascontiguousarray(trig[a:b])
            R.shp_line_play(h, b - a, tb.ctypes.data, 0.0, o.ctypes.data, t.ctypes.data, d.ctypes.data)
            out[a:b], trg[a:b], done[a:b] = o, t, d
            par, st = np.zeros((5, LINE_V)), np.zeros((4, LINE_V))
            R.shp_line_state(h, par.ctypes.data, st.ctypes.data)
            g["line/snap%d/par" % i], g["line/snap%d/st" % i] = par, st
        R.shp_line_free(h)
        assert set(ev) <= set(CUTS)
        g["line/out"] = out
        kinds = {"oneshot": 0, "looping": 0, "descending": 0, "disabled": 0, "again": 0}
        for v in range(LINE_V):
            t = np.concatenate([[0.0], trg[:, v]])
            starts = np.flatnonzero((t[1:] == 1) & (t[:-1] == 0))
            stops = np.flatnonzero((t[1:] == 0) & (t[:-1] == 1))
            finished = np.flatnonzero(done[:, v] == 1)
            ends = np.concatenate([stops, finished[:1]])
            assert len(starts) >= 2 and (trg[:, v] == 1).sum() >= 20 and len(ends) >= 1, "line voice %d: start / run / complete" % v
            assert (starts > ends.min()).any(), "line voice %d never re-arms" % v
            prepares = [e for at in ev for e in ev[at] if e[0] == 0 and e[1] == v]
            kinds["oneshot"] += any(e[5] for e in prepares) and len(finished) > 0
            kinds["looping"] += any(not e[5] for e in prepares) and len(stops) > 0
            kinds["descending"] += any(e[3] < e[2] for e in prepares) and (np.diff(out[:, v]) < 0).sum() > 20
            kinds["disabled"] += any(e[0] == 1 and e[1] == v and e[2] <= 0 for e in ev[0])
            kinds["again"] += len(prepares) >= 2
        assert all(kinds.values()), kinds
        assert out[150, 3] == 0.25 and out[100, 3] == 0.0, "the disabled voice does not show prepare()'s previous lineStart"
        assert len(np.unique(out)) > 300
        h = R.shp_line_new(LINE_V)
        apply(h, 0)
        nc = 300
        o, t, d = (np.zeros((nc, LINE_V)) for _ in range(3))
        R.shp_line_play(h, nc, None, 1.0, o.ctypes.data, t.ctypes.data, d.ctypes.data)
        par, st = np.zeros((5, LINE_V)), np.zeros((4, LINE_V))
        R.shp_line_state(h, par.ctypes.data, st.ctypes.data)
        R.shp_line_free(h)
        assert t[0, :3].all() and t[-1, 0] == 1 and (t[-1, 1:4] == 0).all() and d[-1, 0] == 1 and d[-1, 1] == 0   # a looping line under a constant trigger never re-arms
        g["line_const/out"], g["line_const/st"] = o, st
        R.shp_set_rate(44100)

        # ---- the patch's stream: tests/patches/shaper_patch.cpp + oracle/example_host.cpp (read only) + the reference ---------
        patch = os.path.join(ROOT, "tests", "patches", "shaper_patch.cpp")
        if os.path.exists(patch):
            exe = os.path.join(td, "patch")
            subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-o", exe, os.path.join(ROOT, "oracle", "example_host.cpp"),
                                   patch, ref_sources[0], "-lm", "-lpthread"])
            raw = os.path.join(td, "patch.f64")
            subprocess.run([exe, str(PATCH_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            s = np.fromfile(raw, np.float64).reshape(PATCH_FRAMES, 2)
            assert np.isfinite(s).all() and (s[:, 0] != 0).mean() > 0.5 and (s[:, 1] != 0).mean() > 0.3 and len(np.unique(s)) > 1000
            g["patch"] = s
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    g["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; harness: tools/gen/shaper_ref_dump.cpp; "
        "patch: tests/patches/shaper_patch.cpp via oracle/example_host.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 500 * 1000


if __name__ == "__main__":
    main()
