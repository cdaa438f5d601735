#!/usr/bin/env python3
"""tools/gen/gen_golden_drums.py -- TEST INFRASTRUCTURE.  Writes tests/golden/drums.npz: outputs, state rows and rand() draws of the
UNMODIFIED reference's maxiKick, maxiSnare, maxiHats and maxiClock for the case described in tests/drums_host.py.

It compiles tools/gen/drums_ref_dump.cpp with the reference's src/maximilian.cpp, src/libs/maxiSynths.cpp and src/libs/maxiClock.cpp
(path: $MAXI_REF, default the sibling checkout the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a
temporary directory outside the tree, and records the compiler, flags, libc and the sha256 of the reference sources inside the
file.  Nothing else in the tree changes.

What is stored, per drum, variant and sample rate (key = "<drum>/<variant>/<rate>"):
  out/<key>     [N] the return values of play(), as bytes of equal weight side by side (drums_host.unshuffle);
  rows/<key>    [len(CUTS)][12] the state in front of every CUTS position (drums_host.ROWS);
  envpar/<key>  attack, decay, sustain, release, holdtime as the reference's setters left them;
  envout/<key>  (kick) [N] envelope.output after every play(): the factor of the kick's error bound;
  draws         int32 [N] what rand() returns after srand(1): one draw per play() of snare and hats;
  clock/...     tick, playHead, currentCount and the phasor's phase per sample at both rates, lastCount 0 and 1; clock/bps.
tests/golden/drums_streams.npz: the streams of tests/patches/drums_patch.cpp ("patch") and of the reference's example 7.Counting1
("07") over drums_host.STREAM_FRAMES frames with oracle/example_host.cpp.

The generator ASSERTS on the reference's own output: every envelope phase (attack, decay, hold, release, and rest before the first
trigger) is entered, a trigger is refused in decay or hold and accepted in release, the limiter returns +-1 on at least 30 samples
of each full variant and on none of the plain ones' (there is no limiter), no value is NaN, the clock ticks 16 times with the first
tick at sample 74 (44 100 Hz).

    python tools/gen/gen_golden_drums.py [--ref DIR]
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
import drums_host as dh  # noqa: E402  (the case: one place for this script and the tests)

OUT = os.path.join(ROOT, "tests", "golden", "drums.npz")
OUT_STREAMS = os.path.join(ROOT, "tests", "golden", "drums_streams.npz")
P, S, I, D = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "libs", "maxiSynths.cpp"), os.path.join(src, "libs", "maxiClock.cpp"),
                   os.path.join(src, "maximilian.h"), os.path.join(src, "libs", "maxiSynths.h"), os.path.join(src, "libs", "maxiClock.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    N, C = dh.N, dh.CUTS
    g = {"cuts": np.array(C, np.int64), "trig_at": np.array(dh.TRIG_AT, np.int64)}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libdrref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "drums_ref_dump.cpp")] + ref_sources[:3] + ["-lm"])
        R = ctypes.CDLL(so)
        R.dr_set_rate.argtypes = [I]
        R.dr_run.argtypes = [I, P, S, P, P, P, P]
        R.dr_draws.argtypes = [S, P]
        R.dr_clock.restype = D
        R.dr_clock.argtypes = [I, D, I, S, P, P, P, P]
        draws = np.zeros(N, np.int32)
        R.dr_draws(N, draws.ctypes.data)
        g["draws"] = draws
        trig = dh.triggers().astype(np.uint8)
        col = {n: i for i, n in enumerate(dh.ROWS)}
        for sr in dh.RATES:
            R.dr_set_rate(sr)
            for kind in dh.KINDS:
                for variant in dh.VARIANTS:
                    k = dh.key(kind, variant, sr)
                    cfg = dh.cfg_array(kind, variant)
                    out, rows, envpar = np.zeros(N), np.zeros((N + 1, 12)), np.zeros(5)
                    R.dr_run(dh.KIND[kind], cfg.ctypes.data, N, trig.ctypes.data, out.ctypes.data, rows.ctypes.data, envpar.ctypes.data)
                    again, rows2 = np.zeros(N), np.zeros((N + 1, 12))
                    R.dr_run(dh.KIND[kind], cfg.ctypes.data, N, trig.ctypes.data, again.ctypes.data, rows2.ctypes.data, envpar.ctypes.data)
                    assert np.array_equal(out.view(np.uint64), again.view(np.uint64)) and np.array_equal(rows.view(np.uint64), rows2.view(np.uint64)), k
                    assert np.isfinite(out).all() and np.isfinite(rows).all(), k + ": NaN"
                    assert envpar[0] == 1.0 and envpar[4] == 1, k + ": setAttack(0) gives 1, holdtime 1"
                    after = rows[1:]
                    # rest before the first trigger: the output is 0 (the kick's phase stands still: 1 / (sr / 0) = 0)
                    if not dh.flags_of(kind, variant) & dh.INVERSE:
                        assert (out[:dh.TRIG_AT[0]] == 0).all(), k + ": silence before the first trigger"
                    if kind == "kick":
                        assert (after[:dh.TRIG_AT[0], col["phase"]] == 0).all(), "the kick's phase stands still before the first trigger"
                    # every phase is entered: attack -> decay within the triggering call (attack 1), then decay / hold / release
                    seen_decay = (after[:, col["decayphase"]] == 1).any() or kind == "kick"   # (the kick's decay ends in its first call: sustain 1)
                    # (hold lasts one call -- holdtime 1 -- and hands over to release inside it unless that call was triggered: its trace is holdcount)
                    held = (after[:, col["holdphase"]] == 1) | (np.diff(rows[:, col["holdcount"]]) == 1)
                    assert seen_decay and held.any() and (after[:, col["releasephase"]] == 1).any(), k
                    assert (after[:, col["attackphase"]] == 0).all(), "attack 1 reaches 1 in the triggering call"
                    amp = after[:, col["amplitude"]]
                    # a trigger either restarts the envelope (the amplitude rises) or is refused by the state machine
                    accepted = [t for t in dh.TRIG_AT if amp[t] > (amp[t - 1] if t else 0)]
                    refused = [t for t in dh.TRIG_AT if t not in accepted]
                    assert len(accepted) >= 3 and (len(refused) >= 1 or kind == "kick"), (k, accepted, refused)
                    assert amp[-1] < amp[dh.TRIG_AT[-1]] * 0.02, k + ": a long tail (the slowest release, 6 ms, falls to 1 % in 265 samples)"
                    clipped = int((np.abs(out) == 1.0).sum())
                    if variant == "full":
                        assert clipped >= 30, (k, clipped)
                    assert len(np.unique(out)) > 200, k
                    print("%-22s clipped %4d  peak %.3f  accepted %s refused %s" % (k, clipped, np.abs(out).max(), accepted, refused))
                    g["out/" + k] = dh.shuffle(out)
                    g["rows/" + k] = rows[list(C)]
                    g["envpar/" + k] = envpar
                    if kind == "kick":
                        g["envout/" + k] = dh.shuffle(after[:, col["output"]])
            for last in (0, 1):
                tick, ph, cnt, phase = np.zeros(N, np.uint8), np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N)
                bps = R.dr_clock(dh.CLOCK_TICKS, dh.CLOCK_TEMPO, last, N, tick.ctypes.data, ph.ctypes.data, cnt.ctypes.data, phase.ctypes.data)
                assert bps == 600.0
                if last == 0:
                    assert tick.sum() == (16 if sr == 44100 else tick.sum()) and (sr != 44100 or int(np.argmax(tick)) == 74), (tick.sum(), np.argmax(tick))
                    assert ph[-1] == tick.sum()
                else:
                    assert (tick == (cnt != 1)).all() and tick.sum() > N - 40
                ck = "clock/%d/%d/" % (sr, last)
                g[ck + "tick"], g[ck + "playhead"], g[ck + "count"], g[ck + "phase"] = tick, ph, cnt, phase
        g["clock/bps"] = np.float64(600.0)
        R.dr_set_rate(44100)

        # ---- the streams: tests/patches/drums_patch.cpp and 7.Counting1, oracle/example_host.cpp (read only) + the reference.  The
        # example includes maxiSynths.h for maxiClock, which the reference declares in libs/maxiClock.h: it compiles only with that
        # header included first.
        streams = {}
        ex = os.path.join(args.ref, "cpp", "commandline", "maximilian_examples")
        progs = {"patch": (os.path.join(ROOT, "tests", "patches", "drums_patch.cpp"), [])}
        progs.update({k: (os.path.join(ex, d, "main.cpp"), ["-include", "libs/maxiClock.h"]) for k, d in dh.EXAMPLES.items()})
        for key, (main_cpp, extra) in progs.items():
            exe, frames = os.path.join(td, "prog_" + key), dh.STREAM_FRAMES[key]
            base = [cxx, "-std=c++17"] + fpflags() + ["-w", "-I" + src, "-I" + os.path.join(src, "libs")]
            obj = os.path.join(td, "main_" + key + ".o")   # (the forced include is for the example alone: libs/maxiClock.h has no include guard)
            subprocess.check_call(base + extra + ["-c", "-o", obj, main_cpp])
            subprocess.check_call(base + ["-o", exe, os.path.join(ROOT, "oracle", "example_host.cpp"), obj] + ref_sources[:3] + ["-lm", "-lpthread"])
            raw = os.path.join(td, key + ".f64")
            subprocess.run([exe, str(frames), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            st = np.fromfile(raw, np.float64).reshape(frames, 2)
            assert np.isfinite(st).all() and (st[:, 0] != 0).mean() > 0.3 and len(np.unique(st[:, 0])) > 1000, key
            if np.array_equal(st[:, 0].view(np.uint64), st[:, 1].view(np.uint64)):
                st = st[:, :1]   # both channels carry the same samples: one is stored
            streams[key] = dh.shuffle(st)
            streams[key + "/channels"] = np.int64(st.shape[1])
        pst = dh.unshuffle(streams["patch"], (dh.STREAM_FRAMES["patch"], 2))
        assert (np.abs(pst[7000:, 0]) > 0).all() and np.abs(pst[:, 1]).max() > 0.5 and (pst[:400] == 0).all(), "the patch: silence, then every voice"
        np.savez_compressed(OUT_STREAMS, **streams)
        print("wrote %s (%d bytes)" % (OUT_STREAMS, os.path.getsize(OUT_STREAMS)))
        assert os.path.getsize(OUT_STREAMS) <= 440 * 1000
    sha = hashlib.sha256()
    for fn in ref_sources:
        sha.update(open(fn, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    g["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp, libs/maxiSynths.cpp, libs/maxiClock.cpp, maximilian.h, "
        "libs/maxiSynths.h, libs/maxiClock.h) sha256: %s; harness: tools/gen/drums_ref_dump.cpp"
        % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 440 * 1000


if __name__ == "__main__":
    main()
