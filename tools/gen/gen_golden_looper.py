#!/usr/bin/env python3
"""tools/gen/gen_golden_looper.py -- TEST INFRASTRUCTURE.  Writes tests/golden/looper.npz: what the UNMODIFIED reference's
maxiSample::loopRecord, followed in every sample by playLoop or play() on the same object, and maxiSample::normalise compute for
the cases of tests/looper_host.py (the table ROWS there: one maxiSample per row; every input is derived there from the stored
integers, for this script and the tests alike).

It compiles tools/gen/looper_ref_dump.cpp with the reference's src/maximilian.cpp (path: $MAXI_REF, default the sibling checkout
the oracle uses, see oracle/Makefile REF) under oracle/Makefile's FPFLAGS and -fno-access-control into a temporary directory
outside the tree, and records the compiler, flags, libc and the sha256 of the reference sources inside the file.  Nothing else in
the tree changes.  The archive is written with fixed member dates: the same inputs give the same bytes.

What is stored: cuts; inq int16 [2000][R] (the input is inq / 16384.0, with the special values of SPECIAL_IN put in); en uint8
[2000][R]; for the run "loop" (every row, playLoop) and the run "play" (PLAY_SLOTS, play()): out [2000][rows], and at every cut
recordPosition, the lag's val and position of every row and the elements of every slot whose bits changed since the cut before
(idx = row * CAP + element, val); norm/after<i>: the slots of NORM_ROWS after normalise.

The generator ASSERTS on the reference's own output that each row does what its comment says: the one-index rows stay on one
index, every other span is seen wrapping as often as its length implies, the lag reaches exactly 1.0 in the rows that are always
on and stays below it under the bursts of period 7, the play head on the record head returns the value stored in the same
sample, the one ahead returns old content, the one behind the sample before, no row's output is constant, and every index
either head uses lies inside [0, len).

    python tools/gen/gen_golden_looper.py [--ref DIR]
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
import looper_host as lh  # noqa: E402  (the cases and the derived inputs: one place for this script and the tests)

OUT = os.path.join(ROOT, "tests", "golden", "looper.npz")
P, S, I, D = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double


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


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref())
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    ref_sources = [os.path.join(src, "maximilian.cpp"), os.path.join(src, "maximilian.h")]
    cxx = os.environ.get("CXX", "g++")
    flags = ["-std=c++17"] + fpflags() + ["-fPIC", "-shared", "-w", "-fno-access-control"]
    N, CUTS, CAP = lh.N, lh.CUTS, lh.CAP
    g = {"cuts": np.array(CUTS, np.int64), "inq": lh.input_q(), "en": lh.enable_u8()}
    x_all, en_all = lh.signal(g["inq"]), lh.enable_block(g["en"])
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "liblooperref.so")
        subprocess.check_call([cxx] + flags + ["-I" + src, "-o", so, os.path.join(HERE, "looper_ref_dump.cpp"), ref_sources[0], "-lm"])
        Rf = ctypes.CDLL(so)
        Rf.lp_new.restype = P
        Rf.lp_new.argtypes = [S]
        Rf.lp_free.argtypes = [P]
        Rf.lp_set_sample.argtypes = [P, S, P, S]
        Rf.lp_set_heads.argtypes = [P, S, D, D]
        Rf.lp_trigger.argtypes = [P, S]
        Rf.lp_run.argtypes = [P, S] + [P] * 5 + [I] + [P] * 5
        Rf.lp_state.argtypes = [P, P, P, P]
        Rf.lp_content.restype = S
        Rf.lp_content.argtypes = [P, S, P]
        Rf.lp_normalise.argtypes = [P, S, D]

        contents = {}
        for key, mode, rows in (("loop", lh.PLAYLOOP, list(range(lh.R))), ("play", lh.PLAY, lh.PLAY_SLOTS)):
            b = lh.golden_bank(mode, rows)
            nr = len(rows)
            h = Rf.lp_new(nr)
            for i in range(nr):
                a = np.ascontiguousarray(b.slot(i))
                Rf.lp_set_sample(h, i, a.ctypes.data, a.size)
                Rf.lp_set_heads(h, i, b.recpos[i], b.position[i])
            x, en = np.ascontiguousarray(x_all[:, rows]), np.ascontiguousarray(en_all[:, rows])
            out, ridx, pidx = np.zeros((N, nr)), np.zeros((N, nr), np.int64), np.zeros((N, nr), np.int64)
            prev = [b.slot(i).copy() for i in range(nr)]
            for ci, (a0, a1) in enumerate(zip(CUTS[:-1], CUTS[1:])):
                if a0 in lh.EVENTS:
                    ev = lh.EVENTS[a0]
                    lh.apply_event(b, ev, rows)
                    if ev[1] in rows and ev[0] == "trigger":
                        Rf.lp_trigger(h, rows.index(ev[1]))
                n = a1 - a0
                xb, eb = np.ascontiguousarray(x[a0:a1]), np.ascontiguousarray(en[a0:a1])
                o, ri, pi = np.zeros((n, nr)), np.zeros((n, nr), np.int64), np.zeros((n, nr), np.int64)
                Rf.lp_run(h, n, xb.ctypes.data, eb.ctypes.data, b.mix.ctypes.data, b.start.ctypes.data, b.end.ctypes.data, mode,
                          b.pstart.ctypes.data, b.pend.ctypes.data, o.ctypes.data, ri.ctypes.data, pi.ctypes.data)
                out[a0:a1], ridx[a0:a1], pidx[a0:a1] = o, ri, pi
                rp, lg, ps = np.zeros(nr), np.zeros(nr), np.zeros(nr)
                Rf.lp_state(h, rp.ctypes.data, lg.ctypes.data, ps.ctypes.data)
                snap = "%s/snap%d/" % (key, ci + 1)
                g[snap + "recpos"], g[snap + "lag"], g[snap + "position"] = rp, lg, ps
                fi, fv = [], []
                for i in range(nr):
                    cur = np.zeros(int(b.len[i]))
                    assert Rf.lp_content(h, i, cur.ctypes.data) == cur.size
                    ch = np.nonzero(bits(cur) != bits(prev[i]))[0]
                    fi.append(i * CAP + ch)
                    fv.append(cur[ch])
                    prev[i] = cur
                g[snap + "idx"], g[snap + "val"] = np.concatenate(fi).astype(np.int32), np.concatenate(fv)
            Rf.lp_free(h)
            g[key + "/out"] = out
            contents[key] = prev
            # ---- the rows do what they claim ---------------------------------------------------------------------------------
            lens = np.array([lh.ROWS[r][0] for r in rows])
            assert (ridx >= 0).all() and (ridx < lens[None, :]).all() and (pidx >= 0).all() and (pidx < lens[None, :]).all(), "an index outside [0, len)"
            for i, r in enumerate(rows):
                col = out[:, i]
                assert len(np.unique(col[~np.isnan(col)])) > 3, "row %d: constant output" % r
            if key == "loop":
                e = g["en"]
                wraps = (np.diff(ridx, axis=0) < 0).sum(axis=0)
                for r in (0, 1, 2):
                    assert len(np.unique(ridx[:, r])) == 1, "row %d is not on one index" % r
                span = {3: 39, 4: 200, 5: 500, 6: 50, 8: 250, 10: 2, 11: 101, 12: 50}
                for r, w in span.items():
                    assert wraps[r] == (N - 1) // w or wraps[r] == N // w, "row %d wraps %d times" % (r, wraps[r])
                    assert len(np.unique(ridx[:, r])) == w, "row %d touches %d indices" % (r, len(np.unique(ridx[:, r])))
                assert wraps[7] == 0 and wraps[13] >= 2 and wraps[14] >= 6
                assert ridx[601, 13] == int(0.9003 * 777) and ridx[600, 13] == 600, "row 13: the clamp at the cut"
                assert ridx[1429, 14] == 0 and ridx[1428, 14] != 299, "row 14: trigger() at the cut"
                assert ridx[0, 18] == 3072 and pidx[:, 18].max() < 1024
                lag_end = g["loop/snap8/lag"]
                assert lag_end[0] == 1.0 and lag_end[4] == 1.0 and g["loop/snap3/lag"][7] == 1.0, "the lag reaches exactly 1.0"
                assert all(0 < g["loop/snap%d/lag" % c][1] < 1.0 for c in range(1, 9)), "the lag under the bursts of period 7 stays below 1.0"
                assert 0 < g["loop/snap4/lag"][6] < 1.0 and e[:, 6].min() == 0 and e[:, 6].max() == 1
                assert e[:, 9].max() == 0 and (bits(contents["loop"][9]) == bits(lh.ramp(101))).all(), "row 9 records"
                assert np.isnan(out[:, 12]).any() and np.isnan(contents["loop"][12]).any()
                assert (e[143:600, 11].min(), e[143:600, 11].max(), e[601:1429, 11].min(), e[601:1429, 11].max()) == (0, 1, 0, 1)
                assert (out[:, 8] != np.round(out[:, 8]))[50:].any(), "row 8: / 32767 and * 32767 round visibly"
            on, ahead, behind = rows.index(15), rows.index(16), rows.index(17)
            assert (pidx[:, on] == ridx[:, on]).all() and (pidx[:, ahead] == (ridx[:, ahead] + 1) % 300).all() and \
                (pidx[:, behind] == (ridx[:, behind] - 1) % 300).all(), "the play head placements"
            # on the head: the value stored in the same sample = the content of that index right after the sample; from the third pass
            # on every visit changes it, so the output differs from the old content at every sample
            first = lh.ramp(300)
            assert (out[:295, on] != first[ridx[:295, on]]).mean() > 0.9, "on the head: the output is not old content"
            assert (bits(out[:294, ahead]) == bits(first[pidx[:294, ahead]])).all(), "one ahead: old content"
            assert (bits(out[1:, behind]) == bits(out[:-1, on])).all(), "one behind: the sample before (rows 15 and 17 record alike)"
        for a, c in zip(contents["loop"][15:19], contents["play"][1:5]):
            assert (bits(a) == bits(c)).all(), "the recording depends on the play mode"

        # ---- normalise --------------------------------------------------------------------------------------------------------
        b, level = lh.norm_bank()
        h = Rf.lp_new(b.R)
        for i in range(b.R):
            a = np.ascontiguousarray(b.slot(i))
            Rf.lp_set_sample(h, i, a.ctypes.data, a.size)
            Rf.lp_normalise(h, i, level[i])
            cur = np.zeros(a.size)
            Rf.lp_content(h, i, cur.ctypes.data)
            g["norm/after%d" % i] = cur
        Rf.lp_free(h)
        assert np.abs(g["norm/after0"]).max() == 1.0 and (g["norm/after0"] != 0).sum() == 1, "unique peak, maxLevel 1: everything else rounds to 0"
        assert g["norm/after1"].min() == -1.0 or g["norm/after1"].min() == -0.0 or g["norm/after1"].min() == 0.0
        assert np.abs(g["norm/after2"]).max() == 200.0 and len(np.unique(g["norm/after2"])) > 100
        assert np.isnan(g["norm/after3"]).all(), "an all-zero slot becomes NaN"
    sha = hashlib.sha256()
    for f in ref_sources:
        sha.update(open(f, "rb").read())
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    g["provenance"] = np.array(
        "compiler: %s; flags: %s; libc: %s; reference sources (src/maximilian.cpp + .h) sha256: %s; harness: tools/gen/looper_ref_dump.cpp"
        % (ver, " ".join(flags), " ".join(platform.libc_ver()), sha.hexdigest()))
    save_npz(OUT, g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 1000 * 1000


if __name__ == "__main__":
    main()
