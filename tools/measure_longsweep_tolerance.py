#!/usr/bin/env python3
"""tools/measure_longsweep_tolerance.py -- where SWEPT_RTOL (tests/scan_long_swept_host.py) comes from: the sweep set of the swept
long scan's host twin (mxg_scan_long_swept_host, the device's bits; K31) at 2 and 66 chunks a call and the ragged N -- every
setting -- and at 4097 chunks a call (every setting with --long-all, else the barely-damped ones), three carried calls from random
states, against the sequential per-sample recurrence: the oracle's filter(..., cps=True, rps=True) for lores / hires, mxg_lag_host
with alpha_per_sample = 1 for the lag; beside it the long-double recurrence.  CPU only: the twin gives the device's bits.  Two
noise seeds per length.  Per kind and per length: the worst |twin - sequential| / peak after one call and after three, the setting
it comes from (a "const" setting is one of tests/scan_long_host.py's full-domain settings held still, run at 66 and 4097 chunks), the sequential recurrence's own distance from the long-double one, the worst carried state; per kind the bound: the
worst x 2, rounded up to one significant digit.  One JSON line, also written to --out.

    python tools/measure_longsweep_tolerance.py [--jobs 8] [--long-all] [--out profiles/longsweep_tolerance.json]
"""
import argparse
import json
import math
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
import scan_long_swept_host as sw  # noqa: E402

_ctx = {}


def _init(tmp):
    from oracle import pyoracle
    port = pyoracle.port()
    port.settings(44100, 2, 1024)
    t = pathlib.Path(tmp) / str(os.getpid())
    t.mkdir()
    _ctx["port"], _ctx["ld"] = port, sw.build(t)


def _task(job):
    kind, case, seed, only = job
    port, N = _ctx["port"], sw.SWEEP_N[case]
    const = only in ("const", "const-long")   # coefficients that stand still: the constant long scan's domain through the swept twin
    names, par, x, st0 = sw.const_case(kind, N, seed=seed, long=only == "const-long") if const else sw.sweep_case(kind, N, seed=seed, only=only)
    coef = sw.coef_ps(kind, par, 2)
    exp, est = sw.oracle_seq(port, kind, x, par, st0)
    stable = bool(np.isfinite(exp).all() and np.abs(exp).max() <= 1e6)
    if const or not (case == "4097" and only[0] not in sw.barely_damped(kind)):   # (the sweep set's condition; --long-all goes past what the tests run)
        sw.assert_stable(exp, names, "%s %s" % (kind, case))
    if not stable:  # a setting of --long-all whose sequential output leaves the condition at this length: listed, not measured
        return [{"kind": kind, "case": case, "seed": seed, "setting": names[0], "stable": False, "peak": float(np.abs(exp).max())}]
    got, gst = sw.host_swept(kind, x, coef, sw.full_state(kind, st0), 3)
    truth, _ = sw.seq_long_double(_ctx["ld"], kind, x, coef, st0)
    err3, own = sh.scaled_err(got, exp), sh.scaled_err(exp, truth)
    err1 = sh.scaled_err(got[:N], exp[:N], peak_of=exp)
    serr = sw.state_err(port, kind, par, gst[:sw.NSTATE[kind]], est, exp)
    return [{"kind": kind, "case": case, "seed": seed, "setting": names[i], "stable": True, "err_1_call": float(err1[i]), "err_3_calls": float(err3[i]),
             "sequential_vs_long_double": float(own[i]), "state": float(serr[i]), "peak": float(np.abs(exp[:, i]).max())} for i in range(len(names))]


def bound(worst):
    """worst x 2, rounded up to one significant digit."""
    b = 2.0 * worst
    e = math.floor(math.log10(b))
    return float("%de%d" % (math.ceil(b / 10.0 ** e - 1e-9), e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--long-all", action="store_true", help="every setting at 4097 chunks (one job per setting), not only the barely-damped ones")
    ap.add_argument("--seeds", type=int, nargs="*", default=[2031, 77])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longsweep_tolerance.json"))
    a = ap.parse_args()
    jobs = []
    for kind in sw.KINDS:
        for seed in a.seeds:
            jobs += [(kind, case, seed, None) for case in ("2", "66", "ragged")]
            jobs += [(kind, "4097", seed, [s]) for s in (sw.settings(kind) if a.long_all else sw.barely_damped(kind))]
            jobs += [(kind, "66", seed, "const"), (kind, "4097", seed, "const-long")]
    with tempfile.TemporaryDirectory() as tmp:
        with Pool(a.jobs, _init, (tmp,)) as pool:
            rows = [r for rs in pool.imap_unordered(_task, jobs) for r in rs]
    res = {"chunk": sw.TS, "calls": 3, "seeds": a.seeds, "long_all": a.long_all, "kinds": {}}
    for kind in sw.KINDS:
        per = {}
        for case in sw.SWEEP_N:
            rs = [r for r in rows if r["kind"] == kind and r["case"] == case and r["stable"]]
            out = sorted({r["setting"] for r in rows if r["kind"] == kind and r["case"] == case and not r["stable"]})
            w = max(rs, key=lambda r: r["err_3_calls"])
            per[case] = {"settings": len({r["setting"] for r in rs}), "samples_per_call": sw.SWEEP_N[case], "worst_3_calls": w["err_3_calls"],
                         "worst_1_call": max(r["err_1_call"] for r in rs), "worst_setting": w["setting"],
                         "its_sequential_vs_long_double": w["sequential_vs_long_double"],
                         "worst_sequential_vs_long_double": max(r["sequential_vs_long_double"] for r in rs),
                         "worst_state": max(r["state"] for r in rs), "largest_peak": max(r["peak"] for r in rs),
                         "outside_the_condition_at_this_length": out}
        worst = max(max(p["worst_3_calls"], p["worst_state"]) for p in per.values())
        res["kinds"][kind] = {"lengths": per, "worst": worst, "bound": bound(worst)}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
