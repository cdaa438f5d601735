#!/usr/bin/env python3
"""tools/gen/gen_golden_polyblep.py -- TEST INFRASTRUCTURE.  Writes tests/golden/polyblep.npz: outputs and phases of the UNMODIFIED
reference's maxiPolyBLEP for the case described in tests/polyblep_host.py.

It compiles tools/gen/polyblep_ref_dump.cpp with the reference's src/maximilian.cpp and src/libs/PolyBLEP/PolyBLEP.cpp (path:
$MAXI_REF, default the sibling checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary
directory outside the tree, and records the compiler, flags, libc and the sha256 of the reference sources inside the file.
Nothing else in the tree changes.

What is stored (tests/polyblep_host.py derives every input from the stored integers, for this script and the tests alike):
  fq int16 [N][6]: the frequencies are fq / 8.0 Hz at SR = 1000; pw_q: the pulse widths are pw_q / 100000.0, rotated by one voice
  at every cut; cuts; out/<WAVEFORM>: the [N][6] output, as bytes of equal weight side by side (polyblep_host.unshuffle);
  t/<WAVEFORM> [cuts][6]: the phase at every cut (before the sync at sample 601); enum/values: the reference's Waveform values;
  envgen/tables, envgen/ret: a maxiEnvGen's stage table and the return value after each setLevel / setCurve of ENV_OPS.
tests/golden/polyblep_streams.npz: the streams of tests/patches/polyblep_patch.cpp ("patch") and of the reference's examples
9.Envelopes1 / 2 / 3 ("09a", "09b", "09c") over STREAM_FRAMES frames with oracle/example_host.cpp, and what 9.Envelopes3 prints
through maxiPoll ("09c/poll").

The generator ASSERTS on the reference's own output, for every waveform: each blep / blamp branch is taken (t < dt,
t > 1 - dt, neither), the fallback is taken and not taken, each piecewise arm of tri, tri2, trip, trap and trap2 is taken, and no
output row or column is constant: a test can then not pass on rows of zeros.

    python tools/gen/gen_golden_polyblep.py [--ref DIR]
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
import polyblep_host as ph  # noqa: E402  (the derived inputs: one place for this script and the tests)

OUT = os.path.join(ROOT, "tests", "golden", "polyblep.npz")
OUT_STREAMS = os.path.join(ROOT, "tests", "golden", "polyblep_streams.npz")   # (a file of its own: each stays well below the size limit)
P, S, I, D = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
# frequency of voice 2 in eighths of a Hz, block by block up to PS_FROM: below, above, below, above, just at SR / 4 (taken), below
V2_BLOCKS = [1210, 2400, 1990, 2001, 2000, 433]


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def frequencies():
    """int16 [N][6], eighths of a Hz: constant inside every stored block before PS_FROM, per sample after it."""
    rng = np.random.default_rng(2000)
    N, C = ph.N, ph.CUTS
    fq = np.zeros((N, ph.V), np.int64)
    n = np.arange(N)
    for b, (a, e) in enumerate(zip(C[:-1], C[1:])):
        if a >= ph.PS_FROM:
            break
        fq[a:e, 0] = [931, 1733, 77, 405, 0, 0][b]                     # voice 0: moves first, then rests at 0 Hz
        fq[a:e, 1] = [-301, -1999, -45, -813, -2600, -167][b]          # voice 1: backwards
        fq[a:e, 2] = V2_BLOCKS[b]                                      # voice 2: crosses SR / 4 between blocks
        fq[a:e, 3] = 1999                                              # voice 3: 249.875 Hz, just below SR / 4
        fq[a:e, 4] = [58, 21, 333, 97, 61, 113][b]                     # voice 4: slow
        fq[a:e, 5] = [1444, 1021, 777, 1603, 1187, 1499][b]            # voice 5: mid
    m = n[ph.PS_FROM:] - ph.PS_FROM
    fq[ph.PS_FROM:, 0] = 0
    fq[ph.PS_FROM:, 1] = np.round(-900 + 700 * np.sin(2 * np.pi * m / 211.0))
    fq[ph.PS_FROM:, 2] = np.round(2000 + 480 * np.sin(2 * np.pi * m / 97.0))        # crosses SR / 4 inside the blocks, both ways
    fq[ph.PS_FROM:, 3] = 1999
    fq[ph.PS_FROM:, 4] = np.round(90 + 60 * np.sin(2 * np.pi * m / 53.0))
    fq[ph.PS_FROM:, 5] = rng.integers(300, 1990, N - ph.PS_FROM)
    return fq.astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "libs", "PolyBLEP", "PolyBLEP.cpp"),
                   os.path.join(src, "maximilian.h"), os.path.join(src, "libs", "maxiPolyBLEP.h"), os.path.join(src, "libs", "PolyBLEP", "PolyBLEP.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    g = {"fq": frequencies(), "pw_q": np.array(ph.PW_Q, np.int32), "cuts": np.array(ph.CUTS, np.int64), "sr": np.int64(ph.SR)}
    N, V, C = ph.N, ph.V, ph.CUTS
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libpbref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "polyblep_ref_dump.cpp")] + ref_sources[:2] + ["-lm"])
        R = ctypes.CDLL(so)
        R.pb_set_rate.argtypes = [I]
        R.pb_new.restype = P
        R.pb_new.argtypes = [S]
        R.pb_free.argtypes = [P]
        R.pb_waveform.argtypes = [P, I]
        R.pb_pulse_width.argtypes = [P, S, D]
        R.pb_sync.argtypes = [P, S, D]
        R.pb_play.argtypes = [P, S, P, P]
        R.pb_phase.argtypes = [P, P]
        R.pb_enum.argtypes = [P]
        ev = np.zeros(14, np.int32)
        R.pb_enum(ev.ctypes.data)
        assert ev.tolist() == list(range(14))
        g["enum/values"] = ev
        R.pb_set_rate(ph.SR)
        f = ph.freqs(g)
        dt = f / ph.SR
        fb = ph.fallback(f)
        assert fb[:, 2].any() and (~fb[:, 2]).any() and not fb[:, [0, 1, 3, 4, 5]].any(), "the fallback: voice 2 only, on and off"
        assert fb[C[4]:C[5], 2].all() and f[C[4], 2] == ph.SR / 4.0, "the block just AT SR / 4 takes the fallback"
        d = np.diff(fb[ph.PS_FROM:, 2].astype(int))
        assert (d == 1).sum() >= 3 and (d == -1).sum() >= 3, "voice 2 crosses SR / 4 inside a block in both directions"
        assert (f[:, 1] < 0).all() and (f[C[4]:, 0] == 0).all() and (f[:, 3] == 249.875).all()
        for wf in ph.WAVEFORMS:
            h = R.pb_new(V)
            R.pb_waveform(h, ph.WF[wf])
            out, phases = np.zeros((N, V)), np.zeros((len(C), V))
            tt = np.zeros((N, V))   # the phase every sample is evaluated on
            for b, (a, e) in enumerate(zip(C[:-1], C[1:])):
                pw = ph.pulse_widths(g, b)
                for v in range(V):
                    R.pb_pulse_width(h, v, pw[v])
                if a == ph.SYNC_AT:
                    for v, phase in ph.SYNC:
                        R.pb_sync(h, v, phase)
                for n in range(a, e):   # sample by sample, to record the phase in front of each
                    t = np.zeros(V)
                    R.pb_phase(h, t.ctypes.data)
                    tt[n] = t
                    fr, o = np.ascontiguousarray(f[n]), np.zeros(V)
                    R.pb_play(h, 1, fr.ctypes.data, o.ctypes.data)
                    out[n] = o
                t = np.zeros(V)
                R.pb_phase(h, t.ctypes.data)
                phases[b + 1] = t
            R.pb_free(h)
            # the same blocks in one call each give the same bits (the harness adds nothing per call)
            h = R.pb_new(V)
            R.pb_waveform(h, ph.WF[wf])
            again = np.zeros((N, V))
            for b, (a, e) in enumerate(zip(C[:-1], C[1:])):
                pw = ph.pulse_widths(g, b)
                for v in range(V):
                    R.pb_pulse_width(h, v, pw[v])
                if a == ph.SYNC_AT:
                    for v, phase in ph.SYNC:
                        R.pb_sync(h, v, phase)
                fr, o = np.ascontiguousarray(f[a:e]), np.zeros((e - a, V))
                R.pb_play(h, e - a, fr.ctypes.data, o.ctypes.data)
                again[a:e] = o
            R.pb_free(h)
            assert np.array_equal(again.view(np.uint64), out.view(np.uint64)), wf

            pwn = np.concatenate([np.broadcast_to(ph.pulse_widths(g, b), (e - a, V)) for b, (a, e) in enumerate(zip(C[:-1], C[1:]))])
            live = ~fb
            assert np.isfinite(out[:, [0, 2, 3, 4, 5]]).all(), wf     # (voice 1 runs backwards: TRIANGULAR_PULSE divides by pw = 0 there)
            assert tt[ph.SYNC_AT, 5] == 1.0 and tt[ph.SYNC_AT, 4] == 0.75 and tt[ph.SYNC_AT, 2] == 0.75, "sync"
            assert (tt[:, 1] <= 0).all() and (tt[:, 1] < 0).sum() > 1000 and (tt[:, [0, 2, 3, 4]] >= 0).all()
            for v in range(V):
                assert len(np.unique(out[:, v])) > 3, (wf, v, "a constant column")
            for n in range(1, N):   # (row 0: every phase is 0)
                assert len(np.unique(out[n])) > 1, (wf, n, "a constant row")
            # blep / blamp on the phase itself: every branch, among the samples that are not the fallback's
            t_, d_ = tt[live], dt[live]
            lo, hi = t_ < d_, ~(t_ < d_) & (t_ > 1 - d_)
            assert lo.sum() > 30 and hi.sum() > 30 and (~lo & ~hi).sum() > 30, (wf, lo.sum(), hi.sum())
            code, count = ph.arms(wf, tt, dt, pwn)
            if wf in ("TRIANGLE", "MODIFIED_TRIANGLE"):
                for k in range(count):
                    assert (code[live] == k).sum() > 20, (wf, k)
            elif wf in ("TRAPEZOID_FIXED", "TRAPEZOID_VARIABLE"):
                for k in range(3):
                    assert (code[live] // 3 == k).sum() > 20 and (code[live] % 3 == k).sum() > 20, (wf, k)
            elif wf == "TRIANGULAR_PULSE":
                for k in range(3):
                    assert (code[live] == 2 * k + 1).sum() > 20, (wf, k)
                assert (code[live] % 2 == 0).sum() > 20
            if wf in ("MODIFIED_TRIANGLE", "TRAPEZOID_VARIABLE"):   # both sides of the clamps of the pulse width
                assert (pwn < 0.0001).any() and (pwn > 0.9999).any() and ((pwn > 0.0001) & (pwn < 0.9999)).any()
            g["out/" + wf] = ph.shuffle(out)
            g["t/" + wf] = phases
        for wf in ph.WAVEFORMS[1:]:   # the phase does not depend on the waveform
            assert np.array_equal(g["t/" + wf].view(np.uint64), g["t/SINE"].view(np.uint64))
        # where the fallback is taken every waveform is the same sine
        for wf in ph.WAVEFORMS[1:]:
            assert np.array_equal(ph.ref_out(g, wf)[fb].view(np.uint64), ph.ref_out(g, "SINE")[fb].view(np.uint64))
        R.pb_set_rate(44100)

        # ---- maxiEnvGen::setLevel / setCurve: the stage table after every edit ---------------------------------------------------
        R.pb_envgen_edits.argtypes = [S, P, P, P, S, P, P, P]
        lv, tm, cv = (np.array(a, np.float64) for a in (ph.ENV_LEVELS, ph.ENV_TIMES, ph.ENV_CURVES))
        ops = np.array(ph.ENV_OPS, np.float64)
        ns = len(tm)
        tabs, ret = np.zeros((len(ops), ns, 6)), np.zeros(len(ops), np.int32)
        R.pb_envgen_edits(len(lv), lv.ctypes.data, tm.ctypes.data, cv.ctypes.data, len(ops), ops.ctypes.data, tabs.ctypes.data, ret.ctypes.data)
        assert ret.tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0] and tabs[3, 2, 1] == 0.0625 and tabs[1, 0, 1] == 0.75 and tabs[-1, 1, 3] == 3.0
        g["envgen/tables"], g["envgen/ret"] = tabs, ret

        # ---- the streams: tests/patches/polyblep_patch.cpp and the three examples, oracle/example_host.cpp (read only) + the reference
        streams = {}
        ex = os.path.join(args.ref, "cpp", "commandline", "maximilian_examples")
        progs = {"patch": os.path.join(ROOT, "tests", "patches", "polyblep_patch.cpp")}
        progs.update({k: os.path.join(ex, d, "main.cpp") for k, d in ph.EXAMPLES.items()})
        for key, main in progs.items():
            exe = os.path.join(td, "prog_" + key)
            subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-I" + os.path.join(src, "libs"), "-o", exe,
                                   os.path.join(ROOT, "oracle", "example_host.cpp"), main] + ref_sources[:2] + ["-lm", "-lpthread"])
            raw = os.path.join(td, key + ".f64")
            r = subprocess.run([exe, str(ph.STREAM_FRAMES), raw], check=True, cwd=td, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
            st = np.fromfile(raw, np.float64).reshape(ph.STREAM_FRAMES, 2)
            assert np.isfinite(st).all() and (st[:, 0] != 0).mean() > 0.3 and len(np.unique(st[:, 0])) > 1000, key
            if np.array_equal(st[:, 0].view(np.uint64), st[:, 1].view(np.uint64)):
                st = st[:, :1]   # both channels carry the same samples: one is stored
            streams[key] = ph.shuffle(st)
            streams[key + "/channels"] = np.int64(st.shape[1])
            if key == "09c":
                streams["09c/poll"] = np.array(r.stdout.decode())
                assert len(r.stdout) > 10, "9.Envelopes3 prints through maxiPoll"
        np.savez_compressed(OUT_STREAMS, **streams)
        print("wrote %s (%d bytes)" % (OUT_STREAMS, os.path.getsize(OUT_STREAMS)))
        assert os.path.getsize(OUT_STREAMS) <= 1000 * 1000
    sha = hashlib.sha256()
    for fn in ref_sources:
        sha.update(open(fn, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    g["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp, libs/PolyBLEP/PolyBLEP.cpp, maximilian.h, "
        "libs/maxiPolyBLEP.h, libs/PolyBLEP/PolyBLEP.h) sha256: %s; harness: tools/gen/polyblep_ref_dump.cpp"
        % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 1000 * 1000


if __name__ == "__main__":
    main()
