#!/usr/bin/env python3
"""tools/measure_longscan_tolerance.py -- where SCAN_LONG_RTOL (tests/scan_long_host.py) comes from: the WHOLE full-domain sweep
of the long scan's host twin (mxg_scan_long_host, the device's bits) at a given number of chunks per call, three carried calls
from random states, against the sequential recurrence -- every setting of tests/scan_host.py's sweep and of the lag's alpha sweep,
in batches of voices over a pool of processes (at 4097 chunks a voice is 25 M samples; the biquad's 440 settings at once would be
83 GB).  CPU only.  Per kind: the worst |twin - sequential| / peak after one call and after three, the setting it comes from, the
sequential recurrence's own distance from the long-double recurrence for that setting, the worst carried state, and the settings
above --list x the worst.  One JSON line, also written to --out.

    python tools/measure_longscan_tolerance.py [--chunks 4097] [--jobs 8] [--batch 2] [--kinds dc svf ...] [--out profiles/longscan_tolerance.json]
"""
import argparse
import json
import os
import pathlib
import sys
import tempfile
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_host as sh  # noqa: E402
import scan_long_host as sl  # noqa: E402

_ctx = {}


def _init(tmp):
    from oracle import pyoracle
    port = pyoracle.port()
    port.settings(44100, 2, 1024)
    t = pathlib.Path(tmp) / str(os.getpid())   # (every worker builds its own copy of the two small host libraries)
    t.mkdir()
    _ctx["port"], _ctx["hosts"] = port, (sh.build(t), sl.build(t))


def _task(job):
    kind, N, lo, hi = job
    port, hosts = _ctx["port"], _ctx["hosts"]
    par = np.ascontiguousarray(sl.sweep_params(kind)[:, lo:hi])
    _, x, st0 = sl.sweep_case(kind, N, par=par, seed=2024 + lo)
    coef = sl.coef_rows(port, kind, par)
    exp, est = sl.oracle_seq(port, kind, x, par, st0)
    got, gst = sl.host_long(kind, x, coef, sl.full_state(kind, st0), 3)
    truth, _ = sl.seq_long_double(hosts, kind, x, coef, st0)
    ok = np.isfinite(exp).all(axis=0)
    err3, own = sh.scaled_err(got, exp), sh.scaled_err(exp, truth)
    err1 = sh.scaled_err(got[:N], exp[:N], peak_of=exp)
    serr = sl.state_err(port, kind, par, gst[:sl.NSTATE[kind]], est, exp)
    return [{"kind": kind, "setting": par[:, i].tolist(), "stable": bool(ok[i]), "err_1_call": float(err1[i]), "err_3_calls": float(err3[i]),
             "sequential_vs_long_double": float(own[i]), "state": float(serr[i])} for i in range(hi - lo)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=64 * 64 + 1)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--kinds", nargs="*", default=sl.KINDS)
    ap.add_argument("--list", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longscan_tolerance.json"))
    a = ap.parse_args()
    N = a.chunks * sl.T
    jobs = []
    for kind in a.kinds:
        V = sl.sweep_params(kind).shape[1]
        jobs += [(kind, N, lo, min(lo + a.batch, V)) for lo in range(0, V, a.batch)]
    with tempfile.TemporaryDirectory() as tmp:
        with Pool(a.jobs, _init, (tmp,)) as pool:
            rows = [r for rs in pool.imap_unordered(_task, jobs) for r in rs]
    res = {"chunks_per_call": a.chunks, "calls": 3, "kinds": {}}
    for kind in a.kinds:
        rs = [r for r in rows if r["kind"] == kind]
        assert all(r["stable"] for r in rs), kind
        w = max(rs, key=lambda r: r["err_3_calls"])
        res["kinds"][kind] = {"settings": len(rs), "worst_3_calls": w["err_3_calls"], "worst_1_call": max(r["err_1_call"] for r in rs),
                              "worst_setting": w["setting"], "its_sequential_vs_long_double": w["sequential_vs_long_double"],
                              "worst_state": max(r["state"] for r in rs),
                              "near_worst": sorted(([r["setting"], r["err_1_call"], r["err_3_calls"]] for r in rs if r["err_3_calls"] >= a.list * w["err_3_calls"]),
                                                   key=lambda t: -t[2])[:12]}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
