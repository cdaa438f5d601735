#!/usr/bin/env python3
"""tools/gen/gen_golden_seq.py -- TEST INFRASTRUCTURE.  Writes tests/golden/seq.npz: outputs and states of the UNMODIFIED
reference's maxiRatioSeq / maxiStep / maxiCounter / maxiIndex / maxiZXToPulse / maxiTrigger for the cases below, and the streams
of tests/patches/seq_patch.cpp and tests/patches/seq_host_patch.cpp.

It compiles tools/gen/seq_ref_dump.cpp with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling checkout
the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary directory outside the tree, and
records the compiler, flags, libc and the sha256 of the reference sources inside the file.  Nothing else in the tree changes.

Fused cases ("<case>/..."): V voices x 4000 samples at the sample rate the case names (1000 Hz: clocks of 0.7 .. 40 Hz then
wrap a few times inside the run), played in blocks cut at uneven positions, the state arrays of include/maxigpu.h stored at
every cut ("<case>/snap<i>/dst|ist|clk").  Triggers and gates are stored as uint8, values as uint8 indices into the voice's
list (the lists hold distinct numbers), an external phase as float64.  Tables that change at a cut are stored per block
("<case>/values<i>", "<case>/vlen<i>").  Signal cases ("sig/<kind>/..."): the same classes driven by stored signals (int16 q,
the signal is q / 32768.0).

The generator ASSERTS on the reference's own output that every voice of every case fires at least 3 triggers, that every
clocked voice wraps at least twice, and that at least one wrap and at least one trigger fall on the first or last sample of a
block: a test can then not pass on rows of zeros.

    python tools/gen/gen_golden_seq.py [--ref DIR]
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
OUT = os.path.join(ROOT, "tests", "golden", "seq.npz")
N = 4000
SR = 1000
PATCH_FRAMES = 8000
P = ctypes.c_void_p

PATTERNS = [[3, 3, 2], [1], [4, 4, 4, 1, 1, 1, 1], [33, 991, 13, 153], [12, 1, 12]]  # the last: two boundaries one sample apart at 37 Hz
L = 7
VALUES = [[440.0], [40.0, 80.0, 170.0], [40.0, 80.0, 170.0, 350.0, 900.0, 3888.0], [float(60 + 2 * i) for i in range(10)]]
VALUES_LATER = [[440.0], [40.0, 80.0, 170.0, 350.0, 900.0], VALUES[2], VALUES[3]]  # list 1 grows from 3 to 5 entries at a cut
LV = 10
HOLDS = [0.0, 1.0, 2.5, 300.0]


def table(rows, width):
    t = np.zeros((len(rows), width))
    for i, r in enumerate(rows):
        t[i, :len(r)] = r
    return t, np.array([len(r) for r in rows], np.int32)


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def steps_for(vlen_of_voice):
    """1, 2, -1, 0.5, len + 3, -len, voice after voice."""
    out = []
    for v, n in enumerate(vlen_of_voice):
        out.append([1.0, 2.0, -1.0, 0.5, n + 3.0, -float(n)][v % 6])
    return np.array(out)


def to_index(val, rows, vpat):
    """values -> uint8 indices into each voice's list (exact matches only)."""
    idx = np.zeros(val.shape, np.uint8)
    for v in range(val.shape[1]):
        r = np.asarray(rows[vpat[v]])
        m = val[:, v][:, None] == r[None, :]
        assert (m.sum(axis=1) == 1).all(), "a value that is not in its list"
        idx[:, v] = m.argmax(axis=1)
    return idx


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
        so = os.path.join(td, "libseqref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "seq_ref_dump.cpp"), ref_sources[0], "-lm"])
        R = ctypes.CDLL(so)
        R.seq_new.restype = P
        R.seq_new.argtypes = [ctypes.c_size_t]
        R.seq_free.argtypes = [P]
        R.seq_set_rate.argtypes = [ctypes.c_int]
        R.seq_play.argtypes = [P, ctypes.c_size_t, P, ctypes.c_int, P, P, P, ctypes.c_size_t, P, ctypes.c_int, P, P, ctypes.c_size_t,
                               P, P, P, ctypes.c_int, P, P, P, P]
        R.seq_state.argtypes = [P] * 4
        R.sig_new.restype = P
        R.sig_new.argtypes = [ctypes.c_size_t]
        R.sig_free.argtypes = [P]
        R.sig_play.argtypes = [P, ctypes.c_int, ctypes.c_size_t, P, P, P, P, ctypes.c_size_t, P, P, P]
        R.sig_state.argtypes = [P, ctypes.c_int, P, P]
        R.seq_set_rate(SR)
        times, tlen = table(PATTERNS, L)
        edge_trig = edge_wrap = False
        consecutive = False
        n = np.arange(N)

        # name, V, clock ('int' / 'ext'), mode (0 playValues, 1 maxiStep::pull), cuts
        cases = [("values", 12, "int", 0, [0, 143, 1001, 1429, 2500, N]),
                 ("step", 12, "int", 1, [0, 27, 1429, 2222, N]),
                 ("extphase", 8, "ext", 1, [0, 501, 1777, N])]
        for name, V, clock, mode, cuts in cases:
            pat = (np.arange(V) % len(PATTERNS)).astype(np.int32)
            vpat = ((np.arange(V) // 2) % len(VALUES)).astype(np.int32)
            # 0.7 .. 40 Hz; the slow end goes to voices whose pattern fires often enough, {12, 1, 12} runs at 37 Hz
            freq = np.array([0.7 * (40.0 / 0.7) ** (v / (V - 1.0)) for v in range(V)])
            freq[pat == 4] = 37.0
            freq[pat == 1] = np.maximum(freq[pat == 1], 0.8)
            hold = np.array([HOLDS[(v // 3) % 4] for v in range(V)])
            rec = {"sr": np.int64(SR), "times": times, "len": tlen, "pat": pat, "vpat": vpat, "mode": np.int32(mode), "hold": hold,
                   "cuts": np.array(cuts, np.int64)}
            phase_in = None
            h = R.seq_new(V)
            if clock == "ext":
                # the modulated clock of 9.Envelopes3: phasor(3 - 2 * controller) scaled to this run, from the reference's maxiOsc
                ctl = 0.1 + 0.9 * n / N
                fmod = np.ascontiguousarray((30.0 - 20.0 * ctl)[:, None] * (0.5 + 0.25 * np.arange(V))[None, :])
                hp = R.seq_new(V)
                phase_in, dummy = np.zeros((N, V)), np.zeros((N, V))
                R.seq_play(hp, N, fmod.ctypes.data, 1, None, times.ctypes.data, tlen.ctypes.data, L, pat.ctypes.data, -1, None, None, LV,
                           None, None, None, 0, dummy.ctypes.data, None, None, phase_in.ctypes.data)
                R.seq_free(hp)
                rec["phase"] = phase_in
            else:
                rec["freq"] = freq
            trig, val, gate, phase = np.zeros((N, V)), np.zeros((N, V)), np.zeros((N, V)), np.zeros((N, V))
            vidx = np.zeros((N, V), np.uint8)
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                rows = VALUES if i < 2 else VALUES_LATER  # the length change between two blocks
                vals, vlen = table(rows, LV)
                rec["values%d" % i], rec["vlen%d" % i] = vals, vlen
                step = steps_for(vlen[vpat])
                rec["step%d" % i] = step
                tb, xb, gb, pb = (np.zeros((b - a, V)) for _ in range(4))
                pin = None if phase_in is None else np.ascontiguousarray(phase_in[a:b])
                R.seq_play(h, b - a, freq.ctypes.data if pin is None else None, 0, None if pin is None else pin.ctypes.data,
                           times.ctypes.data, tlen.ctypes.data, L, pat.ctypes.data, mode, vals.ctypes.data, vlen.ctypes.data, LV,
                           vpat.ctypes.data, step.ctypes.data, hold.ctypes.data, 1, tb.ctypes.data, xb.ctypes.data, gb.ctypes.data,
                           pb.ctypes.data)
                trig[a:b], val[a:b], gate[a:b], phase[a:b] = tb, xb, gb, pb
                vidx[a:b] = to_index(xb, rows, vpat)
                dst, ist, clk = np.zeros((5, V)), np.zeros((6, V), np.int64), np.zeros(V)
                R.seq_state(h, dst.ctypes.data, ist.ctypes.data, clk.ctypes.data)
                rec["snap%d/dst" % i], rec["snap%d/ist" % i] = dst, ist
                if clock == "int":
                    rec["snap%d/clk" % i] = clk
            R.seq_free(h)
            assert set(np.unique(trig)) <= {0.0, 1.0} and set(np.unique(gate)) <= {0.0, 1.0}
            wraps = (np.diff(phase, axis=0) < 0)
            assert (trig.sum(axis=0) >= 3).all(), (name, trig.sum(axis=0))
            assert (wraps.sum(axis=0) >= 2).all(), (name, wraps.sum(axis=0))
            inner = cuts[1:-1]
            edges = sorted(set(inner) | {c - 1 for c in inner})
            edge_trig |= bool(trig[edges].any())
            edge_wrap |= bool(np.concatenate([wraps[[e - 1 for e in edges]]]).any())
            consecutive |= bool((trig[1:] * trig[:-1]).any())
            rec.update(trig=trig.astype(np.uint8), val_idx=vidx, gate=gate.astype(np.uint8))
            print("%-9s triggers per voice %s  wraps %s" % (name, trig.sum(axis=0).astype(int), wraps.sum(axis=0)))
            for k, a in rec.items():
                out[name + "/" + k] = a
        assert edge_trig, "no trigger on the first or last sample of a block"
        assert edge_wrap, "no wrap on the first or last sample of a block"
        assert consecutive, "no two boundaries in consecutive samples"

        # ---- the classes driven by signals -------------------------------------------------------------------------------
        V = 8
        rng = np.random.default_rng(1500)
        trig_u8 = np.ascontiguousarray(out["values/trig"][:, 4:4 + V])  # triggers of the fused case's faster voices, two consecutive 1s included
        trig_in = trig_u8.astype(np.float64)
        saw_q = np.round((((n[:, None] * (1.3 + 0.4 * np.arange(V))[None, :] / SR) % 1.0) - 0.5) * 32767).astype(np.int16)   # slow reset saws
        sine_q = np.round(np.sin(2 * np.pi * n[:, None] * (2.0 + np.arange(V))[None, :] / SR) * 32767).astype(np.int16)
        noise_q = rng.integers(-32767, 32768, (N, V)).astype(np.int16)
        saw, sine, noise = saw_q / 32768.0, sine_q / 32768.0, noise_q / 32768.0
        index_sig = np.ascontiguousarray(sine * 0.7 + 0.5)            # leaves [0, 1] on both sides
        vals, vlen = table(VALUES, LV)
        vpat = (np.arange(V) % len(VALUES)).astype(np.int32)
        step = steps_for(vlen[vpat])
        hold = np.array([HOLDS[v % 4] for v in range(V)])
        out.update({"sig/trig": trig_u8, "sig/saw_q": saw_q, "sig/sine_q": sine_q, "sig/noise_q": noise_q,
                    "sig/values": vals, "sig/vlen": vlen, "sig/vpat": vpat, "sig/step": step, "sig/hold": hold})
        cuts = [0, 333, 1501, 1502, N]
        out["sig/cuts"] = np.array(cuts, np.int64)
        # kind -> (name, first input, second input, per-voice parameter)
        kinds = {0: ("onzx", np.ascontiguousarray(sine + 0.3 * noise), None, None), 1: ("counter", trig_in, saw, None),
                 2: ("step", trig_in, None, step), 3: ("index", trig_in, index_sig, None), 4: ("zxtopulse", trig_in, None, hold)}
        h = R.sig_new(V)
        for kind, (kname, a, b2, par) in kinds.items():
            y = np.zeros((N, V))
            for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
                ab = np.ascontiguousarray(a[c0:c1])
                bb = None if b2 is None else np.ascontiguousarray(b2[c0:c1])
                yb = np.zeros((c1 - c0, V))
                R.sig_play(h, kind, c1 - c0, ab.ctypes.data, None if bb is None else bb.ctypes.data, vals.ctypes.data, vlen.ctypes.data, LV,
                           vpat.ctypes.data, None if par is None else par.ctypes.data, yb.ctypes.data)
                y[c0:c1] = yb
                dst, ist = np.zeros((3, V)), np.zeros((2, V), np.int64)
                R.sig_state(h, kind, dst.ctypes.data, ist.ctypes.data)
                out["sig/%s/snap%d/dst" % (kname, i)], out["sig/%s/snap%d/ist" % (kname, i)] = dst, ist
            if kind in (0, 4):
                assert (y.sum(axis=0)[hold > 0 if kind == 4 else slice(None)] >= 3).all(), kname  # (a hold of 0 never opens the gate)
                out["sig/%s/out" % kname] = y.astype(np.uint8)
            elif kind == 1:
                assert (y.max(axis=0) >= 3).all() and ((np.diff(y, axis=0) < 0).sum(axis=0) >= 2).all(), kname  # counted and reset
                assert (y == np.round(y)).all() and y.max() < 65535
                out["sig/counter/out"] = y.astype(np.uint16)
            elif kind == 2:
                out["sig/step/out_idx"] = to_index(y, VALUES, vpat)
                moves = (np.abs(np.diff(y, axis=0)) > 0).sum(axis=0)  # (a step of len + 3 or -len comes back to the same entry)
                assert (moves[(vlen[vpat] > 1) & (np.abs(step) < vlen[vpat])] >= 3).all() and (moves >= 3).sum() >= 3, kname
            else:
                # maxiIndex returns its initial 0.0 until the first trigger: stored as index 255
                first = (trig_in.cumsum(axis=0) == 0)
                assert (y[first] == 0.0).all()
                idx = to_index(np.where(first, np.array([VALUES[r][0] for r in vpat])[None, :], y), VALUES, vpat)  # (placeholder value where `first`)
                idx[first] = 255
                out["sig/index/out_idx"] = idx
                assert all(len(np.unique(idx[:, v])) >= min(3, vlen[vpat[v]]) for v in range(V)), kname
        R.sig_free(h)
        R.seq_set_rate(44100)

        # ---- the patches' streams: tests/patches/*.cpp + oracle/example_host.cpp (read only) + the reference ---------------------
        for key, patch, frames in (("patch", "seq_patch.cpp", PATCH_FRAMES), ("host_patch", "seq_host_patch.cpp", PATCH_FRAMES)):
            exe = os.path.join(td, key)
            subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-o", exe,
                                   os.path.join(ROOT, "oracle", "example_host.cpp"),
                                   os.path.join(ROOT, "tests", "patches", patch), ref_sources[0], "-lm", "-lpthread"])
            raw = os.path.join(td, key + ".f64")
            subprocess.run([exe, str(frames), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            s = np.fromfile(raw, np.float64).reshape(frames, 2)
            assert np.isfinite(s).all() and (s[:, 0] != 0).mean() > 0.5 and (s[:, 1] != 0).mean() > 0.3, key
            out[key] = s
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    out["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; "
        "harness: tools/gen/seq_ref_dump.cpp; patches: tests/patches/seq_patch.cpp, seq_host_patch.cpp via oracle/example_host.cpp"
        % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    out["cases"] = np.array(["values", "step", "extphase"])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
