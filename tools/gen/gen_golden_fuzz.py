#!/usr/bin/env python3
"""tools/gen/gen_golden_fuzz.py -- TEST INFRASTRUCTURE.  Writes tests/golden/dropin_fuzz.npz: what the UNMODIFIED reference computes
for tests/patches/fuzz_patch.cpp (oracle/_ref/example_fz, built by oracle/Makefile where the reference sources are present), for

  * a CORE list of (profile, seed) pairs: the full stereo stream, float64 (`core_<profile>_<seed>`), and
  * a longer DIGEST list: one 64-bit digest per 256-frame block (the first 8 bytes of the sha256 of the block's bytes, every NaN
    written as the one quiet NaN first -- IEEE 754 leaves an arithmetic NaN's sign open, tests/conftest.py assert_bits_equal), the
    frame count, and the patch's own counts of events and calls.

The seed lists are chosen HERE, from the reference alone: seeds are taken in order from CORE_FIRST / DIGEST_FIRST per profile, and a
seed is SKIPPED (and listed in the file) when its stream is not finite on 99 % of the frames or has a peak outside [0.05, 1e6] on
either channel -- such a graph compares nothing.  The file is refused when more than one drawn seed in four is skipped, when an
event kind occurred fewer than 20 times over the digest list, or when a class / method / operator the patch counts was used in
fewer than three seeds.  tests/test_dropin_fuzz_cpu.py recomputes these conditions from the stored file.

    python tools/gen/gen_golden_fuzz.py [--check]      (--check: run everything, write nothing)
"""
import argparse
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
OUT = os.path.join(ROOT, "tests", "golden", "dropin_fuzz.npz")
EXE = os.path.join(ROOT, "oracle", "_ref", "example_fz")

BLOCK = 256
FRAMES = {0: 6000, 1: 6000, 2: 6100, 3: 6000}   # core list.  Profile 2 runs bufferSize 1024: a frame count that is no multiple of it
# digest list: shorter runs (the GPU file's wall time is mostly its children's start-up); profile 3 keeps a steady state of 1500 frames
DIGEST_FRAMES = {0: 2048, 1: 2048, 2: 2148, 3: 3072}
CORE_PER_PROFILE = {0: 3, 1: 2, 2: 3, 3: 2}     # ten full streams
DIGEST_PER_PROFILE = {0: 16, 1: 16, 2: 16, 3: 16}
CORE_FIRST, DIGEST_FIRST = 1, 101
MIN_FINITE, PEAK_LO, PEAK_HI = 0.99, 0.05, 1e6
MAX_SKIPPED = 0.25
MIN_EVENTS, MIN_SEEDS = 20, 3
EVENT_NAMES = ["ev%d" % k for k in range(1, 10)]


def run_reference(profile, seed, frames, exe=EXE, extra_env=None):
    """-> (stream [frames, 2] float64, counts dict) of one run of the reference build of the patch."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "o.f64")
        env = dict(os.environ, MXG_FUZZ_SEED=str(seed), MXG_FUZZ_PROFILE=str(profile), MXG_FUZZ_FRAMES=str(frames))
        env.pop("MXG_FUZZ_LOG", None)
        env.pop("MXG_FUZZ_MAXOBJ", None)
        env.update(extra_env or {})
        r = subprocess.run([exe, str(frames), out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
        if r.returncode != 0:
            raise RuntimeError("example_fz profile %d seed %d: exit %d\n%s" % (profile, seed, r.returncode, r.stderr))
        return np.fromfile(out, np.float64).reshape(frames, 2), parse_counts(r.stderr)


def parse_counts(stderr):
    """The patch's "FUZZ profile=.. ev1=.. phasor=.." line -> {name: int}."""
    line = [ln for ln in stderr.splitlines() if ln.startswith("FUZZ ")]
    if not line:
        raise RuntimeError("no FUZZ line on stderr:\n" + stderr)
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line[-1])}


def block_digests(stream):
    """One uint64 per 256-frame block (the last may be short) of the stream's bytes, NaNs canonical."""
    a = np.ascontiguousarray(stream, np.float64).copy()
    a[np.isnan(a)] = np.float64("nan")
    n = a.shape[0]
    out = []
    for b in range(0, n, BLOCK):
        out.append(int.from_bytes(hashlib.sha256(a[b:b + BLOCK].tobytes()).digest()[:8], "little"))
    return np.array(out, np.uint64)


def stream_ok(stream):
    """The condition a chosen stream meets; -> (ok, why)."""
    fin = np.isfinite(stream).all(axis=1).mean()
    if fin < MIN_FINITE:
        return False, "finite on %.1f %% of the frames" % (100 * fin)
    for ch in (0, 1):
        x = stream[:, ch]
        peak = np.abs(x[np.isfinite(x)]).max()
        if not (PEAK_LO <= peak <= PEAK_HI):
            return False, "channel %d peak %.3g" % (ch, peak)
    return True, ""


def coverage_problems(count_names, counts):
    """counts [pairs, names] of the digest list -> list of unmet conditions (empty: fine)."""
    bad = []
    names = list(count_names)
    for k, name in enumerate(names):
        col = counts[:, k]
        if name in EVENT_NAMES:
            if col.sum() < MIN_EVENTS:
                bad.append("event %s occurred %d times (< %d)" % (name, col.sum(), MIN_EVENTS))
        elif name not in ("profile", "frames", "objects"):
            if (col > 0).sum() < MIN_SEEDS:
                bad.append("%s used in %d seeds (< %d)" % (name, (col > 0).sum(), MIN_SEEDS))
    return bad


def choose(per_profile, first, frames):
    chosen, skipped = [], []
    for p in sorted(per_profile):
        seed, have = first, 0
        while have < per_profile[p]:
            s, c = run_reference(p, seed, frames[p])
            ok, why = stream_ok(s)
            if ok:
                chosen.append((p, seed, s, c))
                have += 1
            else:
                skipped.append((p, seed, why))
            seed += 1
            if len(skipped) > 50:
                raise SystemExit("too many seeds skipped: %r" % skipped[:10])
    return chosen, skipped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "_ref/example_fz"])
    core, skipped_c = choose(CORE_PER_PROFILE, CORE_FIRST, FRAMES)
    dig, skipped_d = choose(DIGEST_PER_PROFILE, DIGEST_FIRST, DIGEST_FRAMES)
    drawn = len(core) + len(dig) + len(skipped_c) + len(skipped_d)
    skipped = skipped_c + skipped_d
    print("drawn %d seeds, skipped %d: %r" % (drawn, len(skipped), skipped))
    if len(skipped) > MAX_SKIPPED * drawn:
        raise SystemExit("more than one drawn seed in four skipped: the patch's clamps are wrong, not the list")
    names = sorted(dig[0][3])
    counts = np.array([[c.get(n, 0) for n in names] for _, _, _, c in dig], np.int64)
    bad = coverage_problems(names, counts)
    for n in names:
        k = names.index(n)
        print("  %-26s total %9d   seeds %3d" % (n, counts[:, k].sum(), (counts[:, k] > 0).sum()))
    if bad:
        raise SystemExit("coverage conditions not met:\n  " + "\n  ".join(bad))
    out = {}
    out["core_pairs"] = np.array([(p, s) for p, s, _, _ in core], np.int64)
    for p, s, stream, _ in core:
        out["core_%d_%d" % (p, s)] = stream
    out["digest_pairs"] = np.array([(p, s) for p, s, _, _ in dig], np.int64)
    out["digest_frames"] = np.array([st.shape[0] for _, _, st, _ in dig], np.int64)
    nb = max((st.shape[0] + BLOCK - 1) // BLOCK for _, _, st, _ in dig)
    table = np.zeros((len(dig), nb), np.uint64)
    for i, (_, _, st, _) in enumerate(dig):
        d = block_digests(st)
        table[i, :len(d)] = d
    out["digests"] = table
    out["digest_peak"] = np.array([[np.nanmax(np.abs(st[:, 0])), np.nanmax(np.abs(st[:, 1]))] for _, _, st, _ in dig])
    out["digest_finite"] = np.array([np.isfinite(st).all(axis=1).mean() for _, _, st, _ in dig])
    out["count_names"] = np.array(names)
    out["counts"] = counts
    out["skipped"] = np.array([(p, s) for p, s, _ in skipped], np.int64).reshape(-1, 2)
    out["drawn"] = np.array(drawn, np.int64)
    ver = subprocess.check_output(["g++", "--version"], text=True).splitlines()[0]
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    flags = re.search(r"^FPFLAGS\s*=\s*(.*)$", mk, re.M).group(1)
    ref = os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1)
    sha = hashlib.sha256()
    for f in ("src/maximilian.cpp", "src/maximilian.h"):
        sha.update(open(os.path.join(ref, f), "rb").read())
    psha = hashlib.sha256(open(os.path.join(ROOT, "tests", "patches", "fuzz_patch.cpp"), "rb").read()).hexdigest()
    out["provenance"] = np.array(
        "compiler: %s; flags: -std=c++17 %s -w; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; "
        "patch: tests/patches/fuzz_patch.cpp sha256 %s via oracle/example_host.cpp (oracle/_ref/example_fz); "
        "seeds drawn in order from %d (core) / %d (digest) per profile; drawn %d, skipped %d: %s" % (
            ver, flags, " ".join(platform.libc_ver()), sha.hexdigest(), psha, CORE_FIRST, DIGEST_FIRST, drawn, len(skipped),
            "; ".join("profile %d seed %d (%s)" % x for x in skipped) or "none"))
    if args.check:
        print("--check: nothing written")
        return
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d bytes, %d core pairs, %d digest pairs" % (OUT, os.path.getsize(OUT), len(core), len(dig)))
    if os.path.getsize(OUT) > 958 * 1024:
        raise SystemExit("the file is larger than the largest drop-in golden (958 KB): fewer core pairs")


if __name__ == "__main__":
    sys.exit(main())
