#!/usr/bin/env python3
"""tools/gen/gen_golden_classic.py -- TEST INFRASTRUCTURE.  Writes tests/golden/classic.npz: outputs and states of the UNMODIFIED
reference's maxiDyn (gate, compressor, compress with the setters), maxiEnvelope (line, trigger), maxiLagExp<double>, maxiMap and
maxiConvert::ampToDbs / dbsToAmp for the cases below, and the streams of tests/patches/classic_patch.cpp.

It compiles tools/gen/classic_ref_dump.cpp with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling checkout
the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS into a temporary directory outside the tree, and
records the compiler, flags, libc and the sha256 of the reference sources inside the file.  Nothing else in the tree changes.

What is stored (tests/classic_host.py derives every input from the stored integers, for this script and the tests alike):
  gate/...: 5 maxiDyn objects through gate() on bursts (q int16, the signal is q / 16384.0): holdtime 0, 1, 200, 30, and one voice
  whose threshold the input never passes; comp/...: three objects through compressor() (ratio 4, 0.75, and 8 that becomes 2.5
  at a cut), one through compress() after the four setters; env/...: 7 maxiEnvelope objects (ascending and descending segments,
  a table of two entries, a zero segment time, a trigger in the middle of a segment, a trigger at a non-zero index, a voice
  never triggered, a short table that sits in the end-of-table oscillation), triggers inside blocks (tq int8) and between
  launches (events), at 44.1 kHz and (env48) at 48 kHz; lag/...: alpha 0, 1, 0.5, a setter-desynchronised pair, a NaN sample;
  map/...: every mode over 7 ranges (a reversed one and one whose explin denominator is -Inf among them) on a signal that passes both clips, with values exactly on both
  edges, -0.0 and NaN.  Blocks are cut at uneven positions (lengths 1 and 7 among them) and every state array is stored at every
  cut.

The generator ASSERTS on the reference's own output that every gate voice is seen idle, in attack, in hold (holdtime > 0), in
release and re-triggered during release, that the attack of the compressor really runs where ratio > 2 and never where ratio <=
1, that every envelope voice does what its row above says (valindex n -> n - 2 -> n among it), that no envelope output depends
on what lies behind the table, and that explin meets a val / inMin of 0 and a negative one: a test can then not pass on rows of
zeros.

    python tools/gen/gen_golden_classic.py [--ref DIR]
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
import classic_host as ch  # noqa: E402  (the derived inputs: one place for this script and the tests)

OUT = os.path.join(ROOT, "tests", "golden", "classic.npz")
N, SR = 2000, 44100
CUTS = [0, 1, 8, 143, 600, 601, 1429, 1993, N]
PATCH_FRAMES = 4000
P, S, I, D = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
NAN = float("nan")
GATE_THR = [0.5, 0.5, 0.5, 0.5, 1.9]
GATE_HOLD = [0, 1, 200, 30, 1]
GATE_ATT = [0.5, 1.0, 0.01, 0.2, 1.0]
GATE_REL = [0.99, 0.9995, 0.9, 0.995, 0.9]
GATE_PERIOD = [400, 330, 610, 450, 380]
COMP_RATIO, COMP_RATIO_LATE = [4.0, 0.75, 8.0], [4.0, 0.75, 2.5]
COMP_THR, COMP_ATT, COMP_REL = [0.5, 0.4, 0.6], [0.3, 0.5, 0.05], [0.99, 0.995, 0.97]
COMP_CHANGE_AT = 601
COMP_SETTERS = (3.0, 0.45, 2.0, 1.5)   # setRatio, setThreshold, setAttack (ms), setRelease (ms)
ENV_S = 8
# (value, samples at 44.1 kHz) pairs; the stored time is samples / (44100 * 0.0011).  The reference's line() only leaves a segment
# when it lands within 1e-7 of the target, so the durations are whole numbers of samples at 44.1 kHz; where it does not land
# (voice 4 after its second trigger, and most voices of the 48 kHz run) the reference walks on past the target, and so must the bank.
ENV_TABLES = [[1.0, 190, 0.25, 290, 0.75, 150, 0.0, 240],     # 0: ascending and descending
              [0.8, 240],                                       # 1: two entries
              [0.5, 150, 1.0, 0, 0.2, 200],                     # 2: a zero segment time
              [0.9, 390, 0.1, 390, 0.6, 100],                   # 3: triggered again in the middle of a segment
              [0.3, 100, 1.0, 290, 0.4, 150, 0.9, 100],         # 4: triggered at index 2; later at index 0, where it misses the target
              [0.7, 150, 0.2, 150],                             # 5: never triggered
              [0.6, 50, 0.1, 50]]                               # 6: short: the end-of-table oscillation
ENV_TINDEX = [0, 0, 0, 0, 2, 0, 0]
ENV_TAMP = [0.0, 0.1, 0.0, 0.0, 0.3, 0.5, 0.0]
ENV_BLOCK_TRIGGERS = [(0, 0), (0, 1), (0, 2), (3, 4), (5, 6), (250, 3), (1300, 0), (1300, 6), (1992, 1)]   # (sample, voice)
ENV_EVENTS = [(0, 3, 0, 0.0), (601, 4, 0, 0.8), (1429, 2, 2, 0.6)]   # (cut, voice, index, amp): trigger() between launches
LAG_ALPHA, LAG_VAL0 = [0.0, 1.0, 0.5, 0.25, 0.5], [0.3, -0.2, 0.0, 1.0, 0.0]
LAG_DESYNC = (3, 0.9)   # setAlpha on voice 3 after init: alphaReciprocal stays 0.75
MAP_N = 400
MAP_RANGE = [[-1.0, 0.1, 1.0, 0.25, 0.01, 0.5, -1.0],       # inMin
             [1.0, 1.2, -1.0, 0.75, 1.0, 1.25, 0.0],        # inMax (voice 2: reversed; voice 6: den = log(-0.0) = -Inf)
             [0.0, 20.0, 5.0, -3.0, 100.0, 1.0, 2.0],       # outMin
             [10.0, 2000.0, 50.0, 3.0, 200.0, 2.0, 8.0]]    # outMax


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


def default_ref():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", txt, re.M).group(1)


def bursts(periods, seed, loud=1.4):
    """A carrier under an envelope that is near silence for a fifth of its period, loud for 30 % and quiet for the rest."""
    rng = np.random.default_rng(seed)
    n = np.arange(N)[:, None]
    per = np.array(periods)[None, :]
    ph = (n % per) / per
    env = np.where(ph < 0.2, 0.1, np.where(ph < 0.5, loud, 0.3))
    x = env * np.sin(2 * np.pi * n * (0.031 + 0.007 * np.arange(len(periods))[None, :])) + 0.02 * rng.standard_normal((N, len(periods)))
    return np.round(np.clip(x, -1.9, 1.9) * 16384).astype(np.int16)


def blk(p, n, V):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(p, np.float64), (n, V)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "maximilian.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    g = {"cuts": np.array(CUTS, np.int64), "sr": np.int64(SR)}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libclsref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "classic_ref_dump.cpp"), ref_sources[0], "-lm"])
        R = ctypes.CDLL(so)
        R.cls_set_rate.argtypes = [I]
        R.cls_dyn_new.restype = P
        R.cls_dyn_new.argtypes = [S]
        R.cls_dyn_free.argtypes = [P]
        R.cls_dyn_gate.argtypes = [P, S] + [P] * 8
        R.cls_dyn_compressor.argtypes = [P, S] + [P] * 7
        R.cls_dyn_set.argtypes = [P, S, D, D, D, D]
        R.cls_dyn_members.argtypes = [P, S, P]
        R.cls_dyn_compress.argtypes = [P, S, P, P, P]
        R.cls_dyn_state.argtypes = [P, P, P]
        R.cls_env_new.restype = P
        R.cls_env_new.argtypes = [S, S, P, P, D]
        R.cls_env_free.argtypes = [P]
        R.cls_env_trigger.argtypes = [P, S, I, D]
        R.cls_env_line.argtypes = [P, S, P, P, P, P, P]
        R.cls_env_state.argtypes = [P, P, P]
        R.cls_lag_new.restype = P
        R.cls_lag_new.argtypes = [S, P, P]
        R.cls_lag_free.argtypes = [P]
        R.cls_lag_set_alpha.argtypes = [P, S, D]
        R.cls_lag_add.argtypes = [P, S, P, P]
        R.cls_lag_state.argtypes = [P, P, P]
        R.cls_map.argtypes = [I, S, P, P, P]
        R.cls_set_rate(SR)
        libm = ctypes.CDLL("libm.so.6")
        libm.log.restype = D
        libm.log.argtypes = [D]

        # ---- maxiDyn::gate -----------------------------------------------------------------------------------------------------
        V = 5
        g["gate/q"] = bursts(GATE_PERIOD, 2300)
        g["gate/thr"], g["gate/att"], g["gate/rel"] = np.array(GATE_THR), np.array(GATE_ATT), np.array(GATE_REL)
        g["gate/hold"] = np.array(GATE_HOLD, np.int64)
        x = ch.signal(g["gate/q"])
        assert np.abs(x[:, 4]).max() < GATE_THR[4] and (np.abs(x[:, :4]) > 0.5).any(axis=0).all()
        h = R.cls_dyn_new(V)
        out, lvl, tr = np.zeros((N, V)), np.zeros((N, V)), np.zeros((N, V), np.int32)
        for i, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
            xb, o, l, t = np.ascontiguousarray(x[a:b]), np.zeros((b - a, V)), np.zeros((b - a, V)), np.zeros((b - a, V), np.int32)
            bt, ba, br = blk(GATE_THR, b - a, V), blk(GATE_ATT, b - a, V), blk(GATE_REL, b - a, V)   # (kept alive over the call)
            R.cls_dyn_gate(h, b - a, xb.ctypes.data, bt.ctypes.data, g["gate/hold"].ctypes.data, ba.ctypes.data, br.ctypes.data, o.ctypes.data, t.ctypes.data,
                           l.ctypes.data)
            out[a:b], lvl[a:b], tr[a:b] = o, l, t
            dst, ist = ch.dyn_fresh(V)
            R.cls_dyn_state(h, dst.ctypes.data, ist.ctypes.data)
            g["gate/snap%d/dst" % i], g["gate/snap%d/ist" % i] = dst, ist
        R.cls_dyn_free(h)
        g["gate/out"] = out
        for v in range(4):
            att, hold, rel = (tr[:, v] & 1) != 0, (tr[:, v] & 2) != 0, (tr[:, v] & 4) != 0
            assert (out[:20, v] == 0).all() and (lvl[:20, v] == 0).all(), "gate voice %d is not idle at first" % v
            assert att.sum() >= 3 and rel.sum() >= 100, "gate voice %d: attack / release" % v
            passed = (out[:, v] == x[:, v]) & (x[:, v] != 0)
            if GATE_HOLD[v] > 1:    # (the last held sample enters release in the same call, which overwrites its output)
                assert passed.sum() >= GATE_HOLD[v] - 1 and hold.sum() >= GATE_HOLD[v] - 1, "gate voice %d never holds" % v
            elif GATE_HOLD[v] == 1:
                assert g["gate/snap7/ist"][0, v] == 1, "gate voice %d never counts its one held sample" % v
            assert ((np.diff(lvl[:, v]) > 0) & rel[:-1]).any(), "gate voice %d is never re-triggered during release" % v   # the amplitude rises again
            assert len(np.unique(out[:, v])) > 300
        assert (out[:, 4] == 0).all() and (tr[:, 4] & 1).sum() == 0 and (g["gate/snap7/ist"][:, 4] == 0).all(), "the voice below its threshold"
        assert (g["gate/snap7/ist"][3, 0] == 1) and (tr[0, 0] == 4), "holdtime 0: a fresh object enters release on its first sample"

        # ---- maxiDyn::compressor / compress --------------------------------------------------------------------------------------
        g["comp/q"] = bursts([400, 330, 610, 450], 2301)
        x = ch.signal(g["comp/q"])
        g["comp/ratio"], g["comp/ratio_late"] = np.array(COMP_RATIO), np.array(COMP_RATIO_LATE)
        g["comp/makeup"] = np.array([1 + libm.log(r) for r in COMP_RATIO])
        g["comp/makeup_late"] = np.array([1 + libm.log(r) for r in COMP_RATIO_LATE])
        g["comp/thr"], g["comp/att"], g["comp/rel"] = np.array(COMP_THR), np.array(COMP_ATT), np.array(COMP_REL)
        g["comp/change_at"] = np.int64(COMP_CHANGE_AT)
        V = 3
        h = R.cls_dyn_new(V)
        out, lvl = np.zeros((N, V)), np.zeros((N, V))
        for i, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
            xb, o, l = np.ascontiguousarray(x[a:b, :3]), np.zeros((b - a, V)), np.zeros((b - a, V))
            bq = blk(COMP_RATIO_LATE if a >= COMP_CHANGE_AT else COMP_RATIO, b - a, V)
            bt, ba, br = blk(COMP_THR, b - a, V), blk(COMP_ATT, b - a, V), blk(COMP_REL, b - a, V)
            R.cls_dyn_compressor(h, b - a, xb.ctypes.data, bq.ctypes.data, bt.ctypes.data, ba.ctypes.data, br.ctypes.data, o.ctypes.data, l.ctypes.data)
            out[a:b], lvl[a:b] = o, l
            dst, ist = ch.dyn_fresh(V)
            R.cls_dyn_state(h, dst.ctypes.data, ist.ctypes.data)
            g["comp/snap%d/dst" % i], g["comp/snap%d/ist" % i] = dst, ist
        R.cls_dyn_free(h)
        g["comp/out"] = out
        rises = np.diff(lvl, axis=0) > 0
        assert rises[:, 0].sum() >= 3 and rises[:, 2].sum() >= 3, "the attack of a ratio > 2 never runs"
        assert rises[:COMP_CHANGE_AT, 2].any() and rises[COMP_CHANGE_AT:, 2].any(), "voice 2 must attack under both ratios"
        # (the one rise of voice 1 is its first trigger, from 0 to ratio * release: set and released in the same call)
        assert rises[:, 1].sum() == 1 and lvl[:, 1].max() == 0.75 * 0.995, "ratio <= 1 goes straight to release"
        assert not rises[np.flatnonzero(lvl[:-1, 1] > 0), 1].any() and (np.diff(lvl[:, 1]) < 0).sum() > 100
        assert np.isfinite(out).all() and len(np.unique(out)) > 3000
        h = R.cls_dyn_new(1)
        R.cls_dyn_set(h, 0, *COMP_SETTERS)
        mem = np.zeros(4)
        R.cls_dyn_members(h, 0, mem.ctypes.data)
        assert mem[0] == COMP_SETTERS[0] and mem[1] == COMP_SETTERS[1] and 0 < mem[2] < 1 and 0 < mem[3] < 1
        xb, o, l = np.ascontiguousarray(x[:, 3:4]), np.zeros((N, 1)), np.zeros((N, 1))
        R.cls_dyn_compress(h, N, xb.ctypes.data, o.ctypes.data, l.ctypes.data)
        dst, ist = ch.dyn_fresh(1)
        R.cls_dyn_state(h, dst.ctypes.data, ist.ctypes.data)
        R.cls_dyn_free(h)
        g["comp/members"], g["comp/members_makeup"] = mem, np.array([1 + libm.log(mem[0])])
        g["comp/setters"] = np.array(COMP_SETTERS)
        g["comp/out_members"], g["comp/members_dst"], g["comp/members_ist"] = o, dst, ist
        assert (np.diff(l[:, 0]) > 0).sum() >= 2 and len(np.unique(o)) > 1000, "compress(): the attack (1 + the setter's pow) never runs"

        # ---- maxiEnvelope --------------------------------------------------------------------------------------------------------
        V = len(ENV_TABLES)
        seg = np.zeros((ENV_S, V))
        for v, t in enumerate(ENV_TABLES):
            seg[:len(t), v] = t
            seg[1:len(t):2, v] /= (44100 * 0.0011)
        count = np.array([len(t) for t in ENV_TABLES], np.int32)
        tq = np.zeros((N, V), np.int8)
        for n_, v in ENV_BLOCK_TRIGGERS:
            tq[n_, v] = 2 if (n_ + v) % 2 == 0 else -3     # any non-zero value triggers
        g["env/seg"], g["env/count"], g["env/tq"] = seg, count, tq
        g["env/tindex"], g["env/tamp"] = np.array(ENV_TINDEX, np.int32), np.array(ENV_TAMP)
        g["env/events"] = np.array(ENV_EVENTS, np.float64)
        trig = ch.env_trigger_block(g)
        ev = ch.env_events(g)
        assert set(ev) <= set(CUTS) and all(0 <= i <= count[v] - 2 for es in ev.values() for v, i, _ in es)

        def run_env(sr, pad, key):
            R.cls_set_rate(sr)
            h = R.cls_env_new(V, ENV_S, seg.ctypes.data, count.ctypes.data, pad)
            out, vi = np.zeros((N, V)), np.zeros((N, V), np.int32)
            snaps = {}
            for i, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
                for v, index, amp in ev.get(a, []):
                    R.cls_env_trigger(h, v, index, amp)
                tb, o, w = np.ascontiguousarray(trig[a:b]), np.zeros((b - a, V)), np.zeros((b - a, V), np.int32)
                R.cls_env_line(h, b - a, tb.ctypes.data, g["env/tindex"].ctypes.data, g["env/tamp"].ctypes.data, o.ctypes.data, w.ctypes.data)
                out[a:b], vi[a:b] = o, w
                dst, ist = ch.env_fresh(V)
                R.cls_env_state(h, dst.ctypes.data, ist.ctypes.data)
                snaps["%s/snap%d/dst" % (key, i)], snaps["%s/snap%d/ist" % (key, i)] = dst, ist
            R.cls_env_free(h)
            R.cls_set_rate(SR)
            return out, vi, snaps

        out, vi, snaps = run_env(SR, 12345.0, "env")
        out2, vi2, snaps2 = run_env(SR, -777.25, "env")
        assert np.array_equal(out.view(np.uint64), out2.view(np.uint64)) and np.array_equal(vi, vi2), "an output depends on what lies behind the table"
        assert all(np.array_equal(snaps[k].view(np.uint8), snaps2[k].view(np.uint8)) for k in snaps)
        g.update(snaps)
        g["env/out"] = out
        d0 = np.diff(out[:1300, 0])
        assert (d0 > 0).sum() > 100 and (d0 < 0).sum() > 100, "voice 0: ascending and descending segments"
        assert count[1] == 2 and out[1, 1] > 0.1 and len(np.unique(out[:, 1])) > 100
        assert not np.isfinite(out[:, 2]).all() and np.isfinite(out[:100, 2]).all(), "voice 2: the zero segment time gives no Inf / NaN"
        assert vi[249, 3] == 0 and 0.3 < out[249, 3] < 0.9 and out[250, 3] < 0.01, "voice 3: the trigger in the middle of a segment"
        assert vi[3, 4] == 2 and (out[:3, 4] == 0).all() and out[3, 4] != 0, "voice 4: a trigger at index 2"
        assert (out[:, 5] == 0).all() and (vi[:, 5] == 0).all(), "voice 5 is never triggered"
        n6 = int(count[6])
        w = vi[200:1200, 6]
        assert set(w.tolist()) == {n6, n6 - 2} and (np.diff(w) != 0).all(), "voice 6: the end-of-table oscillation n -> n - 2 -> n"
        assert (vi.max(axis=0)[[0, 1, 3, 4, 6]] == count[[0, 1, 3, 4, 6]]).all(), "a voice never reaches the end of its table"
        assert out[1990, 4] < -1.0, "voice 4 does not walk past the target it misses"
        out48, _, snaps48 = run_env(48000, 12345.0, "env48")
        g.update(snaps48)
        g["env48/out"] = out48
        both = np.isfinite(out) & np.isfinite(out48)
        assert (out48[both] != out[both]).mean() > 0.3, "the 48 kHz run repeats the 44.1 kHz one"

        # ---- maxiLagExp<double> ----------------------------------------------------------------------------------------------------
        V = 5
        g["lag/q"] = bursts([400, 330, 610, 450, 380], 2302, loud=1.0)
        g["lag/patches"] = np.array([(50, 4, NAN), (10, 2, -0.0)], np.float64)
        x = ch.patched(g["lag/q"], g["lag/patches"])
        a0, v0 = np.array(LAG_ALPHA), np.array(LAG_VAL0)
        h = R.cls_lag_new(V, a0.ctypes.data, v0.ctypes.data)
        R.cls_lag_set_alpha(h, LAG_DESYNC[0], LAG_DESYNC[1])
        par, val = np.zeros((2, V)), np.zeros(V)
        R.cls_lag_state(h, par.ctypes.data, val.ctypes.data)
        g["lag/alpha"], g["lag/recip"], g["lag/val0"] = par[0].copy(), par[1].copy(), val.copy()
        assert par[0, 3] == 0.9 and par[1, 3] == 0.75 and (par[1, [0, 1, 2]] == [1.0, 0.0, 0.5]).all()
        out = np.zeros((N, V))
        for i, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
            xb, o = np.ascontiguousarray(x[a:b]), np.zeros((b - a, V))
            R.cls_lag_add(h, b - a, xb.ctypes.data, o.ctypes.data)
            out[a:b] = o
            R.cls_lag_state(h, par.ctypes.data, val.ctypes.data)
            g["lag/snap%d/val" % i] = val.copy()
        R.cls_lag_free(h)
        g["lag/out"] = out
        assert (out[:, 0] == 0.3).all() and np.array_equal(out[:, 1], x[:, 1]) and np.isnan(out[50:, 4]).all() and np.isfinite(out[:50, 4]).all()
        assert len(np.unique(out[:, 2])) > 1000 and len(np.unique(out[:, 3])) > 1000

        # ---- maxiMap / maxiConvert -------------------------------------------------------------------------------------------------
        V = len(MAP_RANGE[0])
        rng_ = np.random.default_rng(2303)
        n = np.arange(MAP_N)[:, None]
        xs = 1.45 * np.sin(2 * np.pi * n * (3.0 + np.arange(V)[None, :]) / MAP_N + np.arange(V)[None, :]) + 0.03 * rng_.standard_normal((MAP_N, V))
        g["map/q"] = np.round(np.clip(xs, -1.6, 1.6) * 16384).astype(np.int16)
        rng = np.array(MAP_RANGE)
        patches = []
        for v in range(V):
            patches += [(7 + v, v, rng[0, v]), (70 + v, v, rng[1, v]), (142, v, rng[0, v]), (143, v, rng[1, v])]   # exactly on both edges
        patches += [(20, 0, -0.0), (21, 3, -0.0), (22, 4, 0.0), (30, 1, NAN), (31, 0, NAN), (399, 5, NAN), (33, 0, 0.0)]
        g["map/patches"] = np.array(patches, np.float64)
        g["map/range"] = rng
        g["map/aux"] = np.array([libm.log(rng[1, v] / rng[0, v]) for v in range(V)])   # (voices 0 and 2: the log of -1, a NaN; voice 6: -Inf)
        for mode, code in ch.MAP_MODES.items():
            x = ch.map_input(g, mode)
            r4 = np.ascontiguousarray(np.broadcast_to(rng[:, None, :], (4, MAP_N, V)))
            o = np.zeros((MAP_N, V))
            R.cls_map(code, x.size, x.ctypes.data, r4.ctypes.data, o.ctypes.data)
            g["map/" + mode] = o
            if mode in ("linlin", "linexp", "explin", "clamp"):
                lo, hi = np.minimum(rng[0], rng[1]), np.maximum(rng[0], rng[1])
                assert (x < lo).any(axis=0).all() and (x > hi).any(axis=0).all() and ((x > lo) & (x < hi)).any(axis=0).all(), "the signal misses a clip"
            if mode in ("linlin", "clamp"):
                assert np.array_equal(np.isnan(o), np.isnan(x)), "a NaN val passes the compares"
        xe = ch.map_input(g, "explin")[:, 0]
        with np.errstate(all="ignore"):
            q = np.where(xe < rng[0, 0], rng[0, 0], np.where(rng[1, 0] < xe, rng[1, 0], xe)) / rng[0, 0]   # voice 0: inMin = -1
        e = g["map/explin"]
        # A val / inMin of 0 needs a range that holds 0, a negative one an inMin and a val of different signs: inMin <= 0 <= inMax either
        # way, so den = log(inMax / inMin) is never a finite number there.  Voice 0 (den = log(-1) = NaN) answers NaN to both.  Voice 6
        # (inMax = 0: den = log(-0.0) = -Inf) tells the -Inf of log(0) apart from any finite value: -Inf / -Inf is NaN where val
        # reaches 0, and a finite logarithm over -Inf is a zero, i.e. outMin, everywhere else.
        assert (q == 0).sum() >= 2 and (q < 0).sum() > 50 and np.isnan(e[:, 0]).all(), "explin: val / inMin of 0 and a negative one"
        x6 = ch.map_input(g, "explin")[:, 6]
        assert g["map/aux"][6] == -np.inf and (x6 >= 0).sum() > 50 and np.isnan(e[x6 >= 0, 6]).all() and (x6 < 0).sum() > 50 and (e[x6 < 0, 6] == 2.0).all(), \
            "explin: log(0) over a den of -Inf"
        assert np.isfinite(e[:, [1, 3, 4, 5]][~np.isnan(ch.map_input(g, "explin")[:, [1, 3, 4, 5]])]).all()
        assert len(np.unique(g["map/linexp"][:, 1])) > 100 and np.isfinite(g["map/linexp"][:, 1][~np.isnan(ch.map_input(g, "linexp")[:, 1])]).all()
        a2d = g["map/ampToDbs"]
        assert (a2d == -np.inf).any() and np.isnan(a2d).any() and np.isfinite(a2d).sum() > MAP_N
        assert np.isfinite(g["map/dbsToAmp"][~np.isnan(ch.map_input(g, "dbsToAmp"))]).all()

        # ---- the patch's streams: tests/patches/classic_patch.cpp + oracle/example_host.cpp (read only) + the reference ----------
        patch = os.path.join(ROOT, "tests", "patches", "classic_patch.cpp")
        for key, defs in (("patch", []), ("patch_arith", ["-DCLASSIC_PATCH_ARITH"])):
            exe = os.path.join(td, key)
            subprocess.check_call([cxx, "-std=c++17"] + fpflags() + ["-w"] + defs + ["-I" + src, "-o", exe, os.path.join(ROOT, "oracle", "example_host.cpp"),
                                   patch, ref_sources[0], "-lm", "-lpthread"])
            raw = os.path.join(td, key + ".f64")
            subprocess.run([exe, str(PATCH_FRAMES), raw], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            s = np.fromfile(raw, np.float64).reshape(PATCH_FRAMES, 2)
            assert np.isfinite(s).all() and (s[:, 0] != 0).mean() > 0.5 and (s[:, 1] != 0).mean() > 0.5 and len(np.unique(s)) > 2000, key
            g[key] = s
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    g["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; harness: tools/gen/classic_ref_dump.cpp; "
        "patch: tests/patches/classic_patch.cpp via oracle/example_host.cpp" % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 1000 * 1000


if __name__ == "__main__":
    main()
