"""CPU (-m "not gpu"): mxg_scan_long.h -- the arithmetic of the long time-parallel scan (scan_long.hip, K28) -- through the library's
host twin mxg_scan_long_host.  As K10's, its arithmetic is reordered and has no bit-exact anchor in the reference; the anchor is
the bound |error| <= SCAN_LONG_RTOL[kind] x the voice's peak of the sequential output over the carried calls, against the oracle's
sequential recurrence (the lag: the library's bit-exact mxg_lag_host), over the whole parameter domain (tests/scan_host.py's
sweep; alpha 1e-6 ... 1 for the lag), stable settings and finite input.  The device is held to the twin bit for bit
(tests/test_gpu_scan_long.py).

The bound was not fixed in advance: it is the measured worst x 2, rounded up to one significant digit (the twin's bits are the
device's, so the slack is for settings between the sweep's points and for other noise).  It is stated for a stream of up to
3 x 4097 chunks (2.5e7 samples per voice) carried from a state: see the undamped SVF below.

Measured (three carried calls from random start states; worst |twin - sequential| / peak per N on this file's streams, in
brackets the float64 sequential recurrence's own distance from the long-double recurrence at that N; then the WHOLE sweep at 4097
chunks on other noise, every setting, in batches -- tools/measure_longscan_tolerance.py, profiles/longscan_tolerance.json):
                   2 chunks            ragged (6471)       65 chunks           4097 chunks, here    whole sweep, 4097   worst     bound
    maxiDCBlocker  4.4e-14 (7.8e-15)   2.6e-14 (1.1e-14)   9.0e-13 (6.6e-14)   1.3e-12 (1.2e-13)    2.3e-12             2.3e-12   5e-12   R = 1 - 1.1e-7, 0.999999
    maxiSVF        1.2e-13 (1.2e-14)   1.9e-13 (1.8e-14)   5.3e-12 (7.1e-14)   3.5e-10 (5.3e-13)    3.3e-10             3.5e-10   8e-10   res 0 (undamped), 15 kHz
    maxiBiquad     5.1e-11 (4.1e-11)   3.3e-11 (2.5e-11)   9.0e-11 (4.9e-11)   1.4e-10 (1.3e-10)    1.6e-10             1.6e-10   4e-10   low-pass 10 Hz, Q 50
    lores          9.3e-14 (8.6e-15)   1.3e-13 (1.1e-14)   4.4e-13 (3.1e-14)   7.6e-13 (2.9e-14)    7.2e-13             7.6e-13   2e-12   10 Hz, res 1000
    hires          1.0e-13 (7.5e-15)   1.4e-13 (9.1e-15)   4.4e-13 (2.6e-14)   7.3e-13 (3.3e-14)    7.4e-13             7.4e-13   2e-12   10 Hz, res 1000
    maxiLagExp     1.3e-13 (1.8e-14)   1.9e-13 (1.9e-14)   3.0e-12 (3.3e-14)   4.1e-12 (5.4e-14)    4.1e-12             4.1e-12   9e-12   alpha 1e-6
The carried state, continued by the sequential recurrence, is never worse than the stream.  The 4097-chunk calls of THIS file
(8.4 M samples per voice and call; the biquad's 440 settings at once would be 83 GB of input and the six sweeps 45 minutes of CPU)
run tests/scan_long_host.py's long_params: every setting of the sweep that barely decays or does not decay -- R >= 0.999999, ALL
six undamped SVFs (res 0 has |pole| = 1 at every cutoff), the 10 Hz biquads at Q 50 and the -18 dB high shelves at 10 Hz, res 1000
at 10 and 100 Hz, alpha < 2e-6 -- which is where the whole sweep has every one of its worst figures, and three spread over it.

The error grows with the length of the stream only for those settings.  The undamped SVF is the worst by far and the one kind
whose bound is NOT independent of the length: at 15 kHz, res 0 the whole sweep gave 5.1e-11 after one call of 4097 chunks and
3.3e-10 after three.  M_T comes out of six squarings of K10's M and carries a rounding of its own, a fixed small error of the rotation
it stands for; with |pole| = 1 nothing damps it, every chunk adds the same error again, and after c chunks it is c times as
large -- while the sequential recurrence rounds afresh at every sample (it is 5e-13 from the long-double one there).  Beyond 2.5e7
samples of an undamped setting the bound does not hold; every other setting's error has stopped growing by then (the whole sweep after one call and
after three: DC blocker 2.3e-12 and 2.3e-12, lores, hires and the lag unchanged, the biquad 1.2e-10 and 1.6e-10).

Non-finite input: from a NaN / Inf sample onward the outputs and the state are non-finite exactly where the sequential
recurrence's are, but NaN and Inf may trade places: a chunk's start state is reached through products with M_T, whose entries
underflow to 0 for fast-decaying settings, and 0 * Inf is NaN where the sequential recurrence still holds Inf.
"""
import os
import subprocess

import numpy as np
import pytest

import scan_host as sh
import scan_long_host as sl
from conftest import ROOT, assert_bits_equal
from scan_long_host import RAGGED, SCAN_LONG_RTOL, T

MXG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scan_long")
    return sh.build(tmp), sl.build(tmp)


def _check(hosts, port, kind, par, x, st0, calls, what):
    """The twin against the sequential recurrence (and that against long double): prints the figures, asserts the bound."""
    rtol = SCAN_LONG_RTOL[kind]
    coef = sl.coef_rows(port, kind, par)
    exp, est = sl.oracle_seq(port, kind, x, par, st0)
    assert np.isfinite(exp).all(), what + ": the sweep holds stable settings only"
    got, gst = sl.host_long(kind, x, coef, sl.full_state(kind, st0, 7.25), calls)
    truth, _ = sl.seq_long_double(hosts, kind, x, coef, st0)
    err, own = sh.scaled_err(got, exp), sh.scaled_err(exp, truth)
    serr = sl.state_err(port, kind, par, gst[:sl.NSTATE[kind]], est, exp)
    w, ws = int(err.argmax()), int(serr.argmax())
    print("%s: max |twin - sequential| / peak = %.3e at voice %d %s; |sequential - long double| / peak = %.3e; carried state "
          "continued: %.3e at voice %d (bound %.0e)" % (what, err.max(), w, par[:, w].tolist(), own.max(), serr.max(), ws, rtol))
    assert err.max() <= rtol, what
    assert serr.max() <= rtol, what + ": carried state"
    assert np.all(gst[sl.NSTATE[kind]:] == 7.25), what + ": state rows the kind does not own"


@pytest.mark.parametrize("case", list(sl.SWEEP_N))
@pytest.mark.parametrize("kind", sl.KINDS)
def test_full_domain_sweep(hosts, port, kind, case):
    par, x, st0 = sl.sweep_case(kind, sl.SWEEP_N[case], par=sl.long_params(kind) if case == "4097" else None)
    _check(hosts, port, kind, par, x, st0, 3, "%s, %s chunks x 3 calls (%d settings)" % (kind, case, par.shape[1]))


@pytest.mark.parametrize("typ,cut,q", [(0, 20.0, 50.0), (2, 20.0, 50.0), (0, 30.0, 8.0)])
def test_low_biquads(hosts, port, typ, cut, q):
    """tests/test_scan_host.py's low biquads (both poles near z = 1) at 16 chunks a call."""
    N = 16 * T
    rng = np.random.default_rng(N + typ)
    par = np.array([[float(typ)], [cut], [q], [0.0]])
    x = rng.uniform(-1, 1, (3 * N, 1))
    for st0 in (np.zeros((3, 1)), rng.uniform(-1, 1, (3, 1))):
        _check(hosts, port, "biquad", par, x, st0, 3, "biquad type %d %g Hz Q %g, 16 chunks" % (typ, cut, q))


@pytest.mark.parametrize("L", sh.ALL_L)
@pytest.mark.parametrize("kind", sh.KINDS)
def test_one_k10_block_is_k10(hosts, port, kind, L):
    """N = 64 * 2^j <= 2048: the long form of a single K10-shaped block is K10 -- scan_host_render's bits, output and state."""
    N = 64 * L
    par, x, st0 = sh.sweep_case(kind, N, blocks=1)
    coef = sh.coef_rows(port, kind, par)
    exp, est = sh.host_scan(hosts[0], kind, x, coef, st0)
    got, gst = sl.host_long(kind, x, coef, sl.full_state(kind, st0))
    assert_bits_equal(got, exp, "%s N=%d" % (kind, N))
    assert_bits_equal(gst[:sl.NSTATE[kind]], est, "%s N=%d: state" % (kind, N))


NONFINITE = sh.NONFINITE_SETTINGS + [("lag", [0.01])]
BAD_AT = [T - 1, T, 3 * T + 100, 3 * T + 5 * 64 + 3]  # a chunk's last sample, the next one's first, a K10 block of the tail, its plain steps


@pytest.mark.parametrize("bad", [b for b, _ in sh.BAD_SAMPLES])
@pytest.mark.parametrize("setting", range(len(NONFINITE)), ids=["%s%d" % (k, i) for i, (k, _) in enumerate(NONFINITE)])
def test_nonfinite_sample(port, setting, bad):
    """One NaN / +Inf / -Inf in the middle voice of three: before it the bound holds; from it onward isfinite of output and state
    is the sequential recurrence's (NaN and Inf may trade places, see above); the voices beside it keep their bits."""
    kind, p = NONFINITE[setting]
    V, mid = 3, 1
    par = np.repeat(np.array(p, np.float64)[:, None], V, axis=1)
    coef = sl.coef_rows(port, kind, par)
    rng = np.random.default_rng(setting)
    clean = rng.uniform(-1, 1, (2 * RAGGED, V))
    st0 = rng.uniform(-1, 1, (sl.NSTATE[kind], V))
    good, good_st = sl.host_long(kind, clean, coef, sl.full_state(kind, st0), 2)
    for at in BAD_AT:
        x = clean.copy()
        x[at, mid] = dict(sh.BAD_SAMPLES)[bad]
        exp, est = sl.oracle_seq(port, kind, x, par, st0)
        got, gst = sl.host_long(kind, x, coef, sl.full_state(kind, st0), 2)
        gst = gst[:sl.NSTATE[kind]]
        what = "%s %s at %d" % (kind, bad, at)
        assert not np.isfinite(exp[at:, mid]).any(), what + ": the setting is meant to stay non-finite"
        assert np.array_equal(np.isfinite(got), np.isfinite(exp)), what + ": isfinite mask, first differing %s" % np.argwhere(np.isfinite(got) != np.isfinite(exp))[:1]
        assert np.array_equal(np.isfinite(gst), np.isfinite(est)), what + ": state"
        assert sh.scaled_err(got[:at], exp[:at]).max() <= SCAN_LONG_RTOL[kind], what + ": before the bad sample"
        keep = np.arange(V) != mid
        assert_bits_equal(got[:, keep], good[:, keep], what + ": the voices beside it")
        assert_bits_equal(gst[:, keep], good_st[:sl.NSTATE[kind]][:, keep], what + ": their states")


def test_unstable_voice_leaves_the_others_alone(port):
    """lores / hires at 10 kHz, res 1 diverge in the reference too: such a voice changes no other voice's bits."""
    rng = np.random.default_rng(5)
    V, bad = 7, 3
    x = rng.uniform(-1, 1, (2 * RAGGED, V))
    st0 = rng.uniform(-1, 1, (2, V))
    par = np.stack([np.full(V, 800.0) + 100.0 * np.arange(V), np.full(V, 3.0)])
    par_bad = par.copy()
    par_bad[:, bad] = [10000.0, 1.0]
    for kind in ("lores", "hires"):
        exp, _ = sl.oracle_seq(port, kind, x, par_bad, st0)
        assert not np.isfinite(exp[:, bad]).all() or np.abs(exp[:, bad]).max() > 1e100, "the setting is meant to diverge"
        good, gst = sl.host_long(kind, x, sl.coef_rows(port, kind, par), sl.full_state(kind, st0), 2)
        got, st = sl.host_long(kind, x, sl.coef_rows(port, kind, par_bad), sl.full_state(kind, st0), 2)
        keep = np.arange(V) != bad
        assert_bits_equal(got[:, keep], good[:, keep], kind + ": voices beside the unstable one")
        assert_bits_equal(st[:, keep], gst[:, keep], kind + ": their states")
        assert sh.scaled_err(got[:, keep], exp[:, keep]).max() <= SCAN_LONG_RTOL[kind]


def test_in_place_on_the_host(port):
    kind, p = sh.NONFINITE_SETTINGS[2]
    par = np.repeat(np.array(p, np.float64)[:, None], 2, axis=1)
    x = np.random.default_rng(3).uniform(-1, 1, (RAGGED, 2))
    coef = sl.coef_rows(port, kind, par)
    a, sa = sl.host_long(kind, x, coef, sl.full_state(kind, np.zeros((3, 2))))
    b, sb = sl.host_long(kind, x, coef, sl.full_state(kind, np.zeros((3, 2))), inplace=True)
    assert_bits_equal(b, a, "in place")
    assert_bits_equal(sb, sa, "in place: state")


def test_argument_validation():
    L = sl.lib()
    buf = np.zeros(4 * T)
    coef, st = np.zeros(9), np.zeros(5)
    p = buf.ctypes.data

    def call(fn, kind, V, N, i=p, o=p + 8 * 2 * T, extra=()):
        return fn(kind, V, N, i, coef.ctypes.data, st.ctypes.data, o, *extra)

    for fn, extra in ((L.mxg_scan_long_host, ()), (L.mxg_scan_long_render, (None,))):
        for what, args in (("V = 0", dict(kind=0, V=0, N=T)), ("V = 4097", dict(kind=0, V=4097, N=T)), ("N = 0", dict(kind=0, V=1, N=0)),
                           ("N past 2^28", dict(kind=0, V=1, N=2**28 + 1)), ("kind 6", dict(kind=6, V=1, N=T)), ("kind -1", dict(kind=-1, V=1, N=T)),
                           ("out overlaps in from above", dict(kind=0, V=1, N=T, o=p + 8)), ("out overlaps in from below", dict(kind=0, V=1, N=T, i=p + 8 * (T - 1), o=p))):
            assert call(fn, extra=extra, **args) == MXG_ERR_INVALID, what
            assert L.mxg_last_error(), what
    assert call(L.mxg_scan_long_host, 0, 1, T) == 0              # disjoint
    assert call(L.mxg_scan_long_host, 0, 1, T, o=p) == 0         # in place
    assert call(L.mxg_scan_long_host, 0, 1, T, o=p + 8 * T) == 0  # adjacent


def test_bank_setters_and_host(port):
    """maxiLongScanBank's setters give the coefficient rows of the sequential entry points, and host() is the twin."""
    import maximilian_amd as mx
    V = 3
    x = np.random.default_rng(8).uniform(-1, 1, (RAGGED, V))
    par = {"dc": [[0.995] * V], "svf": [[700.0, 900.0, 1100.0], [2.0] * V] + [[m] * V for m in sh.SVF_MIX],
           "biquad": [[0.0, 2.0, 6.0], [1200.0] * V, [0.7] * V, [0.0, 0.0, 6.0]], "lores": [[800.0] * V, [3.0] * V],
           "hires": [[800.0] * V, [3.0] * V], "lag": [[0.01, 0.1, 0.5]]}
    for kind in sl.KINDS:
        p = np.array(par[kind], np.float64)
        b = mx.maxiLongScanBank(V, kind)
        {"dc": lambda: b.setDC(p[0]), "svf": lambda: b.setSVF(p[0], p[1], p[2:6]), "biquad": lambda: b.setBiquad(p[0], p[1], p[2], p[3]),
         "lores": lambda: b.setLores(p[0], p[1]), "hires": lambda: b.setHires(p[0], p[1]), "lag": lambda: b.setLag(p[0])}[kind]()
        assert_bits_equal(b.coef, sl.coef_rows(port, kind, p), kind + ": coefficient rows")
        st0 = np.random.default_rng(9).uniform(-1, 1, (sl.NSTATE[kind], V))
        b.set_state(sl.full_state(kind, st0))
        got, st = b.host(x, advance=True)
        exp, est = sl.host_long(kind, x, b.coef, sl.full_state(kind, st0))
        assert_bits_equal(got, exp, kind)
        assert_bits_equal(b.state(), est, kind + ": state")
        seq, _ = sl.oracle_seq(port, kind, x, p, st0)
        assert sh.scaled_err(got, seq).max() <= SCAN_LONG_RTOL[kind], kind


def test_standalone_program_under_sanitizers(tmp_path):
    """tests/host_scan_long_main.cpp -- mxg_scan_long.h in a program of its own, built with AddressSanitizer and
    UndefinedBehaviorSanitizer: the ragged and the 65-chunk shapes of every kind against the plain sequential step."""
    exe = str(tmp_path / "host_scan_long_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_scan_long_main.cpp")])
    r = subprocess.run([exe] + ["%.17g" % SCAN_LONG_RTOL[k] for k in sl.KINDS], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
