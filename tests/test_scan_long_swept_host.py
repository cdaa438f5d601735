"""CPU (-m "not gpu"): mxg_scan_long_swept.h -- the arithmetic of the long time-parallel scan with per-sample coefficients
(scan_long_swept.hip, K31) -- through the library's host twin mxg_scan_long_swept_host.  Its arithmetic is reordered (a state reaches
a lane and a chunk through products of per-lane and per-chunk transitions); the anchor is the bound |error| <= SWEPT_RTOL[kind] x
the voice's peak of the sequential output over the carried calls, against the sequential per-sample recurrence: the oracle's
filter(..., cps=True, rps=True) for lores / hires, the library's bit-exact mxg_lag_host with alpha_per_sample = 1 for the lag.  The
device is held to the twin bit for bit (tests/test_gpu_scan_long_swept.py).

The sweep set (tests/scan_long_swept_host.py), one voice per setting, cutoffs inside 10 Hz ... 8 kHz: a 2 Hz LFO over 200 Hz ... 8 kHz,
a 200 Hz LFO over 100 Hz ... 8 kHz, a ramp 10 Hz -> 8 kHz over every call, a 2 Hz LFO over 10 ... 60 Hz and a cutoff stepping to a random
value every 37 samples, each at resonance 1, 30, 1000 and under a 3 Hz resonance LFO 1 ... 100; for the lag alpha log-swept
1e-6 ... 1, on a random walk in [0, 1] and stepping between 1e-6 and 1, alphaReciprocal 1 - alpha and independent.  The condition on
the set -- the float64 sequential output of every setting finite, peak <= 1e6 -- is asserted for every case.  Two combinations do NOT
meet it and are not in the set: the stepped cutoff at resonance 1000 and under the resonance LFO diverges in the reference's own
recurrence (peaks 5e9 ... 3e33 after 6 chunks, NaN after 198; test_the_two_settings_left_out_do_diverge).  (A low LFO at 5 Hz instead
of 2 Hz pumps res 1000 the same way, 4e46 after 1.26e7 samples; the set's is at 2 Hz.)

The bound was not fixed in advance: the measured worst x 2, rounded up to one significant digit.  Measured (three carried calls
from random states, two noise seeds, worst of |twin - sequential| / peak and the carried state continued; in brackets the worst
distance of the float64 sequential recurrence itself from the long-double one; the 4097-chunk columns are EVERY setting --
tools/measure_longsweep_tolerance.py --long-all, profiles/longsweep_tolerance.json).  First the sweep set:
                2 chunks            ragged (3399)       66 chunks           4097 chunks         worst setting
    lores       1.0e-14 (6.6e-15)   2.2e-14 (4.7e-15)   2.8e-14 (3.0e-14)   3.8e-14 (3.2e-14)   low LFO, res 1000
    hires       1.1e-14 (5.9e-15)   8.0e-15 (1.1e-14)   1.5e-14 (2.5e-14)   4.1e-14 (3.0e-14)   low LFO, res 1000
    maxiLagExp  2.9e-15 (3.1e-15)   2.9e-15 (2.7e-15)   1.3e-14 (1.1e-14)   2.9e-14 (2.7e-14)   alpha log-swept, 1 - alpha
(At 4097 chunks the stepped cutoff at resonance 30 leaves the condition as well -- its random pumping has a heavy tail -- and is listed
in the JSON, not measured; at the lengths this file runs it its peak stays below 2e5.)  On the sweep set the twin is as near the
sequential recurrence as that is to the long-double one.  That set alone would give bounds of 6e-14 ... 9e-14, and they would be
wrong: a sweep may stand still, and the worst input is a barely-damped setting that does.  The constant long scan's full-domain
settings (tests/scan_long_host.py: 10 Hz ... 8 kHz x res 1 ... 1000, alpha 1e-6 ... 1) HELD for the whole stream, through the swept twin
(const_case; at 4097 chunks its long_params):
                66 chunks, after 1 call / 3 calls    4097 chunks, after 1 call / 3 calls    worst setting       worst     bound
    lores       3.6e-13 / 9.6e-13                    2.8e-12 / 2.8e-12                      10 Hz, res 1000     2.8e-12   6e-12
    hires       3.4e-13 / 9.3e-13                    2.8e-12 / 2.8e-12                      10 Hz, res 1000     2.8e-12   6e-12
    maxiLagExp  4.6e-13 / 1.2e-12                    2.1e-12 / 2.1e-12                      alpha 1.2e-6        2.1e-12   5e-12
The error of such a setting grows with the stream until the stream is as long as the setting's memory (1e6 samples at alpha 1e-6)
and stops there: one call of 4097 chunks and three give the same figure.  So the bound does not depend on the length; it is stated
for the 1.26e7 samples per voice that were measured.  (K28's constant scan has 7.6e-13 at the same settings: one M and its powers
err together, where 1024-sample pairs each round on their own.)  THIS file runs the barely-damped settings at 4097 chunks (res 1000
at the low LFO; alpha near 1e-6; the held long_params) and the whole sets at the other lengths.
"""
import os
import subprocess

import numpy as np
import pytest

import scan_host as sh
import scan_long_host as sl
import scan_long_swept_host as sw
from conftest import ROOT, assert_bits_equal
from scan_long_swept_host import RAGGED, SWEPT_RTOL, TS

MXG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ld(tmp_path_factory):
    return sw.build(tmp_path_factory.mktemp("scan_long_swept"))


@pytest.mark.parametrize("case", list(sw.SWEEP_N))
@pytest.mark.parametrize("kind", sw.KINDS)
def test_sweep_set(ld, port, kind, case):
    """The twin against the sequential yardstick (and that against long double): prints the figures, asserts the bound."""
    rtol, N = SWEPT_RTOL[kind], sw.SWEEP_N[case]
    names, par, x, st0 = sw.sweep_case(kind, N, only=sw.barely_damped(kind) if case == "4097" else None)
    coef = sw.coef_ps(kind, par, 2 if case in ("66", "4097") else 3)
    what = "%s, %s chunks x 3 calls (%d settings)" % (kind, case, len(names))
    exp, est = sw.oracle_seq(port, kind, x, par, st0)
    sw.assert_stable(exp, names, what)
    got, gst = sw.host_swept(kind, x, coef, sw.full_state(kind, st0, 7.25), 3)
    truth, _ = sw.seq_long_double(ld, kind, x, coef, st0)
    err, own = sh.scaled_err(got, exp), sh.scaled_err(exp, truth)
    serr = sw.state_err(port, kind, par, gst[:sw.NSTATE[kind]], est, exp)
    w = int(err.argmax())
    print("%s: max |twin - sequential| / peak = %.3e at %s; |sequential - long double| / peak = %.3e; carried state continued: %.3e "
          "(bound %.0e)" % (what, err.max(), names[w], own.max(), serr.max(), rtol))
    assert err.max() <= rtol, what
    assert serr.max() <= rtol, what + ": carried state"
    assert np.all(gst[sw.NSTATE[kind]:] == 7.25), what + ": state rows the kind does not own"


@pytest.mark.parametrize("case", ["66", "4097"])
@pytest.mark.parametrize("kind", sw.KINDS)
def test_coefficients_that_stand_still(ld, port, kind, case):
    """The constant long scan's full-domain settings held for the whole stream: where the bound's worst figures are."""
    rtol, N = SWEPT_RTOL[kind], sw.SWEEP_N[case]
    names, par, x, st0 = sw.const_case(kind, N, long=case == "4097")
    coef = sw.coef_ps(kind, par, 2)
    what = "%s held, %s chunks x 3 calls (%d settings)" % (kind, case, len(names))
    exp, est = sw.oracle_seq(port, kind, x, par, st0)
    sw.assert_stable(exp, names, what)
    got, gst = sw.host_swept(kind, x, coef, sw.full_state(kind, st0), 3)
    err = sh.scaled_err(got, exp)
    serr = sw.state_err(port, kind, par, gst[:sw.NSTATE[kind]], est, exp)
    print("%s: max |twin - sequential| / peak = %.3e at %s; carried state continued: %.3e (bound %.0e)" % (what, err.max(), names[int(err.argmax())], serr.max(), rtol))
    assert err.max() <= rtol and serr.max() <= rtol, what


@pytest.mark.parametrize("kind", ["lores", "hires"])
def test_the_two_settings_left_out_do_diverge(port, kind):
    names, par, x, st0 = sw.sweep_case(kind, 66 * TS, only=sw.DIVERGING)
    exp, _ = sw.oracle_seq(port, kind, x, par, st0)
    for v, name in enumerate(names):
        assert not np.isfinite(exp[:, v]).all() or np.abs(exp[:, v]).max() > 1e6, name + ": would belong in the sweep set"


@pytest.mark.parametrize("kind", sw.KINDS)
def test_plain_steps_are_the_sequential_bits(port, kind):
    """N = 1 ... 63: no block, the step itself sample after sample."""
    names, par, x, st0 = sw.sweep_case(kind, 63, calls=1)
    coef = sw.coef_ps(kind, par)
    for N in range(1, 64):
        exp, est = sw.oracle_seq(port, kind, x[:N], tuple(p[:N] for p in par), st0)
        got, gst = sw.host_swept(kind, x[:N], coef[:N], sw.full_state(kind, st0))
        assert_bits_equal(got, exp, "%s N=%d" % (kind, N))
        assert_bits_equal(gst[:sw.NSTATE[kind]], est, "%s N=%d: state" % (kind, N))


@pytest.mark.parametrize("kind", sw.KINDS)
def test_constant_rows_against_the_constant_long_scan(port, kind):
    """Block-constant coefficients through the swept twin: within SWEPT_RTOL + SCAN_LONG_RTOL of mxg_scan_long_host."""
    N = 5 * sl.T + 300
    par, x, st0 = sl.sweep_case(kind, N, calls=1)
    coef = sl.coef_rows(port, kind, par)                                       # [2][V]
    cps = np.ascontiguousarray(np.broadcast_to(coef[None], (N,) + coef.shape))  # [N][2][V]
    exp, est = sl.host_long(kind, x, coef, sl.full_state(kind, st0))
    got, gst = sw.host_swept(kind, x, cps, sw.full_state(kind, st0))
    seq, _ = sl.oracle_seq(port, kind, x, par, st0)
    assert np.isfinite(seq).all()
    tol = SWEPT_RTOL[kind] + sl.SCAN_LONG_RTOL[kind]
    assert sh.scaled_err(got, exp, peak_of=seq).max() <= tol
    assert sl.state_err(port, kind, par, gst[:sw.NSTATE[kind]], est[:sw.NSTATE[kind]], seq).max() <= tol
    assert sh.scaled_err(got, seq).max() <= SWEPT_RTOL[kind], "and within its own bound of the sequential recurrence"


@pytest.mark.parametrize("kind", sw.KINDS)
def test_one_call_equals_two_halves(port, kind):
    N = 2 * (3 * TS + 2 * 64 + 5)
    names, par, x, st0 = sw.sweep_case(kind, N, calls=1)
    coef = sw.coef_ps(kind, par)
    st = sw.full_state(kind, st0, -3.5)
    one, s1 = sw.host_swept(kind, x, coef, st, 1)
    two, s2 = sw.host_swept(kind, x, coef, st, 2)
    exp, _ = sw.oracle_seq(port, kind, x, par, st0)
    assert sh.scaled_err(one, two, peak_of=exp).max() <= SWEPT_RTOL[kind]
    assert sw.state_err(port, kind, par, s1[:sw.NSTATE[kind]], s2[:sw.NSTATE[kind]], exp).max() <= SWEPT_RTOL[kind]
    for s in (s1, s2):
        assert_bits_equal(s[sw.NSTATE[kind]:], st[sw.NSTATE[kind]:], kind + ": rows the kind does not own")


def test_in_place_on_the_host():
    names, par, x, st0 = sw.sweep_case("lores", RAGGED, calls=1)
    coef = sw.coef_ps("lores", par)
    a, sa = sw.host_swept("lores", x, coef, sw.full_state("lores", st0))
    b, sb = sw.host_swept("lores", x, coef, sw.full_state("lores", st0), inplace=True)
    assert_bits_equal(b, a, "in place")
    assert_bits_equal(sb, sa, "in place: state")


def test_argument_validation():
    L = sw.lib()
    buf = np.zeros(4 * TS)
    coef, st = np.zeros(8 * TS), np.zeros(5)
    p, k = buf.ctypes.data, coef.ctypes.data

    def call(fn, kind=3, V=1, N=TS, i=p, c=k, rows=2, s=st.ctypes.data, o=p + 8 * 2 * TS, extra=()):
        return fn(kind, V, N, i, c, rows, s, o, *extra)

    for fn, extra in ((L.mxg_scan_long_swept_host, ()), (L.mxg_scan_long_render_swept, (None,))):
        for what, args in (("kind 0", dict(kind=0)), ("kind 1", dict(kind=1)), ("kind 2", dict(kind=2)), ("kind 6", dict(kind=6)), ("kind -1", dict(kind=-1)),
                           ("coef_rows 1", dict(rows=1)), ("coef_rows 9", dict(rows=9)), ("V = 0", dict(V=0)), ("V = 4097", dict(V=4097)), ("N = 0", dict(N=0)),
                           ("N past 2^28", dict(N=2**28 + 1)), ("null in", dict(i=None)), ("null coef", dict(c=None)), ("null st", dict(s=None)), ("null out", dict(o=None)),
                           ("out overlaps in from above", dict(o=p + 8)), ("out overlaps in from below", dict(i=p + 8 * (TS - 1), o=p)),
                           ("out overlaps coef", dict(o=k + 8 * TS)), ("out is coef", dict(o=k)), ("out ends inside coef", dict(c=p + 8 * (3 * TS - 1)))):
            assert call(fn, extra=extra, **args) == MXG_ERR_INVALID, what
            assert L.mxg_last_error(), what
        for kind in (0, 1, 2):
            assert call(fn, kind=kind, extra=extra) == MXG_ERR_INVALID and b"no swept form" in L.mxg_last_error()
    assert call(L.mxg_scan_long_swept_host) == 0                                   # disjoint
    assert call(L.mxg_scan_long_swept_host, o=p) == 0                              # in place
    assert call(L.mxg_scan_long_swept_host, c=p + 8 * 3 * TS, o=p + 8 * 2 * TS, N=TS // 2) == 0   # coef behind out in one buffer, disjoint
    assert call(L.mxg_scan_long_swept_host, rows=8, N=TS // 2) == 0
    assert call(L.mxg_scan_long_swept_host, kind=5, rows=2) == 0


BAD_AT = [TS - 1, TS, 2 * TS + 100, 3 * TS + 5 * 64 + 3]  # a chunk's last sample, the next one's first, inside a chunk, the plain steps


@pytest.mark.parametrize("kind", sw.KINDS)
def test_nan_sample(port, kind):
    """One NaN in the middle voice of three: the voices beside it keep their bits; from it onward that voice is non-finite wherever
    the sequential recurrence is, and before it the bound holds."""
    only = ["slow-lfo/res30", "audio-lfo/res30", "ramp/res30"] if kind != "lag" else ["walk/one-minus", "log-sweep/independent", "walk/independent"]
    names, par, clean, st0 = sw.sweep_case(kind, RAGGED, calls=2, only=only)
    coef = sw.coef_ps(kind, par)
    V, mid = 3, 1
    good, good_st = sw.host_swept(kind, clean, coef, sw.full_state(kind, st0), 2)
    for at in BAD_AT:
        x = clean.copy()
        x[at, mid] = np.nan
        exp, est = sw.oracle_seq(port, kind, x, par, st0)
        got, gst = sw.host_swept(kind, x, coef, sw.full_state(kind, st0), 2)
        gst = gst[:sw.NSTATE[kind]]
        what = "%s NaN at %d" % (kind, at)
        assert not np.isfinite(exp[at:, mid]).any(), what + ": the setting is meant to stay non-finite"
        bad = ~np.isfinite(exp)
        assert not np.isfinite(got[bad]).any(), what + ": non-finite wherever the sequential recurrence is"
        assert not np.isfinite(gst[~np.isfinite(est)]).any(), what + ": state"
        assert sh.scaled_err(got[:at], exp[:at]).max() <= SWEPT_RTOL[kind], what + ": before the bad sample"
        keep = np.arange(V) != mid
        assert_bits_equal(got[:, keep], good[:, keep], what + ": the voices beside it")
        assert_bits_equal(gst[:, keep], good_st[:sw.NSTATE[kind]][:, keep], what + ": their states")


def test_bank_swept_and_helpers(port):
    """maxiLongScanBank.host_swept is the twin on the bank's state, shared with host(); sweep_lores / sweep_hires give
    mxg_filter_coeffs_host's rows per sample ([N][3][V]), sweep_lag [N][2][V]; kinds 0-2 raise ValueError."""
    import maximilian_amd as mx
    for kind in sw.KINDS:
        names, par, x, st0 = sw.sweep_case(kind, RAGGED, calls=2)
        V = len(names)
        coef = sw.coef_ps(kind, par)
        assert coef.shape == (2 * RAGGED, 2 if kind == "lag" else 3, V)
        if kind != "lag":
            n = 5
            assert_bits_equal(coef[n], port.filter_coeffs(0, par[0][n], par[1][n]), kind + ": the oracle's coefficients of sample 5")
            assert_bits_equal(mx.sweep_lores(par[0][:, :1], 30.0)[:, 0, 0], mx.sweep_lores(par[0][:, :1], np.full((2 * RAGGED, 1), 30.0))[:, 0, 0], "broadcast")
        else:
            assert_bits_equal(coef[:, 1], par[1], "alphaReciprocal")
            assert_bits_equal(mx.sweep_lag(par[0])[:, 1], 1.0 - par[0], "alphaReciprocal = 1 - alpha")
        b = mx.maxiLongScanBank(V, kind)
        b.set_state(sw.full_state(kind, st0))
        got1, _ = b.host_swept(x[:RAGGED], coef[:RAGGED], advance=True)
        got2, st = b.host_swept(x[RAGGED:], coef[RAGGED:], advance=True)
        exp, est = sw.host_swept(kind, x, coef, sw.full_state(kind, st0), 2)
        assert_bits_equal(np.concatenate([got1, got2]), exp, kind)
        assert_bits_equal(b.state(), est, kind + ": state")
    for kind in ("dc", "svf", "biquad"):
        b = mx.maxiLongScanBank(1, kind)
        with pytest.raises(ValueError):
            b.host_swept(np.zeros((8, 1)), np.zeros((8, 2, 1)))
        with pytest.raises(ValueError):
            b.process_swept(np.zeros((8, 1)), np.zeros((8, 2, 1)))


def test_standalone_program_under_sanitizers(tmp_path):
    """tests/host_scan_long_swept_main.cpp -- mxg_scan_long_swept.h in a program of its own, built with AddressSanitizer and
    UndefinedBehaviorSanitizer: a small ragged case of every kind against the plain sequential step."""
    exe = str(tmp_path / "host_scan_long_swept_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_scan_long_swept_main.cpp")])
    r = subprocess.run([exe] + ["%.17g" % SWEPT_RTOL[k] for k in sw.KINDS], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
