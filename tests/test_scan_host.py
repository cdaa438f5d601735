"""CPU (-m "not gpu"): mxg_scan.h -- the arithmetic of the time-parallel scan (scan.hip, knob "time_parallel") -- compiled for the
host as a 64-lane model (tests/host_scan.cpp).  The scan's arithmetic is reordered, so it has no bit-exact anchor in the reference;
its anchor is the stated bound |error| <= SCAN_RTOL (1e-10) x the voice's peak of the sequential output over the carried blocks,
against the oracle's sequential recurrence -- over the WHOLE parameter domain the classes accept, for stable settings and finite
input.  The device is then held to this host model bit for bit (tests/test_gpu_scan.py).

Measured (host model = device bits; worst over the sweep, the six L, three carried blocks from random start states; in brackets the
float64 sequential recurrence's own distance from the long-double recurrence on the same scale, then the final state continued):
    maxiDCBlocker  3.6e-14  (1.2e-14)  3.6e-14
    maxiSVF        7.5e-14  (8.8e-15)  7.6e-14
    maxiBiquad     6.3e-11  (3.8e-11)  5.1e-11     type 6 at 10 Hz, Q 0.1, -18 dB, N = 2048; 1.4e-11 up to N = 512
    lores          5.0e-14  (9.5e-15)  4.7e-14
    hires          5.7e-14  (1.2e-14)  5.7e-14
The biquad's figure is mostly the sequential recurrence's own rounding at 10 Hz: the reference it is measured against is itself
3.8e-11 from the truth there.  On the arithmetic before the (v2, v1, v1 - v2) basis the same sweep reached 5.2e-8.
"""
import numpy as np
import pytest

import scan_host as sh
from conftest import assert_bits_equal
from scan_host import SCAN_RTOL


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("scan"))


def _check(host, port, kind, par, x, st0, blocks, what):
    """Host model against the oracle's sequential recurrence (and that against long double); returns the two worst figures."""
    coef = sh.coef_rows(port, kind, par)
    exp, est = sh.oracle_seq(port, kind, x, par, st0)
    assert np.isfinite(exp).all(), what + ": the sweep holds stable settings only"
    got, gst = sh.host_scan(host, kind, x, coef, st0, blocks)
    truth, _ = sh.seq_long_double(host, kind, x, coef, st0)
    err, own = sh.scaled_err(got, exp), sh.scaled_err(exp, truth)
    w = int(err.argmax())
    print("%s: max |scan - sequential| / peak = %.3e at voice %d %s; |sequential - long double| / peak = %.3e (tolerance %.0e)"
          % (what, err.max(), w, par[:, w].tolist(), own.max(), SCAN_RTOL))
    assert err.max() <= SCAN_RTOL, what
    serr = sh.state_err(port, kind, par, gst, est, exp)   # the carried state, by what the stream does from it
    ws = int(serr.argmax())
    print("    carried state: max |continued from it - sequential| / peak = %.3e at voice %d %s" % (serr.max(), ws, par[:, ws].tolist()))
    assert serr.max() <= SCAN_RTOL, what + ": carried state"
    return float(err.max()), float(own.max())


@pytest.mark.parametrize("L", sh.ALL_L)
@pytest.mark.parametrize("kind", sh.KINDS)
def test_full_domain_sweep(host, port, kind, L):
    par, x, st0 = sh.sweep_case(kind, 64 * L)
    _check(host, port, kind, par, x, st0, 3, "%s L=%d (%d settings)" % (kind, L, par.shape[1]))


@pytest.mark.parametrize("N", [512, 2048])
@pytest.mark.parametrize("typ,cut,q", [(0, 20.0, 50.0), (2, 20.0, 50.0), (0, 30.0, 8.0)])
def test_low_biquads_regression(host, port, typ, cut, q, N):
    """Both poles near z = 1: in the plain direct-form-II basis the entries of A^n grow like n and the scan subtracts terms near
    1e9 to get 1e5 (measured on that arithmetic: 2.0e-10 ... 1.1e-8 x peak for these six cases); carried in (v2, v1, v1 - v2) it does not."""
    rng = np.random.default_rng(N + typ)
    par = np.array([[float(typ)], [cut], [q], [0.0]])
    x = rng.uniform(-1, 1, (3 * N, 1))
    for st0 in (np.zeros((3, 1)), rng.uniform(-1, 1, (3, 1))):
        _check(host, port, "biquad", par, x, st0, 3, "biquad type %d %g Hz Q %g N=%d" % (typ, cut, q, N))


def test_unstable_voice_leaves_the_others_alone(host, port):
    """The reference's lores diverges at high cutoff with low resonance (10 kHz, res 1): the bound cannot cover such a voice.  What
    holds: it changes no other voice's bits."""
    rng = np.random.default_rng(5)
    V, N, bad = 7, 512, 3
    x = rng.uniform(-1, 1, (2 * N, V))
    st0 = rng.uniform(-1, 1, (2, V))
    par = np.stack([np.full(V, 800.0) + 100.0 * np.arange(V), np.full(V, 3.0)])
    par_bad = par.copy()
    par_bad[:, bad] = [10000.0, 1.0]
    for kind in ("lores", "hires"):
        exp, _ = sh.oracle_seq(port, kind, x, par_bad, st0)
        assert not np.isfinite(exp[:, bad]).all() or np.abs(exp[:, bad]).max() > 1e100, "the setting is meant to diverge"
        good, gst = sh.host_scan(host, kind, x, sh.coef_rows(port, kind, par), st0, 2)
        got, st = sh.host_scan(host, kind, x, sh.coef_rows(port, kind, par_bad), st0, 2)
        keep = np.arange(V) != bad
        assert_bits_equal(got[:, keep], good[:, keep], kind + ": voices beside the unstable one")
        assert_bits_equal(st[:, keep], gst[:, keep], kind + ": their states")
        assert sh.scaled_err(got[:, keep], exp[:, keep]).max() <= SCAN_RTOL


@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("bad", [b for b, _ in sh.BAD_SAMPLES])
@pytest.mark.parametrize("setting", range(len(sh.NONFINITE_SETTINGS)), ids=["%s%d" % (k, i) for i, (k, _) in enumerate(sh.NONFINITE_SETTINGS)])
def test_nonfinite_sample(host, port, setting, bad, L):
    """One NaN / +Inf / -Inf sample inside a segment in mid-block, as the last sample of that segment and as the block's last: the output's isnan and isfinite masks are the sequential recurrence's; before the
    bad sample the tolerance applies.  (A finite sample near 1e308 is not part of the contract: the two orders overflow at
    different samples.)"""
    kind, p = sh.NONFINITE_SETTINGS[setting]
    N = 64 * L
    par = np.array(p, np.float64)[:, None]
    coef = sh.coef_rows(port, kind, par)
    for at in sorted({N // 2 + 3 * L // 8, N // 2 + L - 1, N - 1}):  # inside lane 32's segment, its last sample, the block's last
        rng = np.random.default_rng(setting * 10 + L)
        x = rng.uniform(-1, 1, (2 * N, 1))
        x[at, 0] = dict(sh.BAD_SAMPLES)[bad]
        st0 = rng.uniform(-1, 1, (sh.NSTATE[kind], 1))
        exp, est = sh.oracle_seq(port, kind, x, par, st0)
        got, gst = sh.host_scan(host, kind, x, coef, st0, 2)
        what = "%s %s at %d, L=%d" % (kind, bad, at, L)
        assert np.array_equal(np.isnan(got), np.isnan(exp)), what + ": isnan mask, first differing sample %s" % np.argwhere(np.isnan(got) != np.isnan(exp))[:1]
        assert np.array_equal(np.isfinite(got), np.isfinite(exp)), what + ": isfinite mask"
        assert np.array_equal(np.isnan(gst), np.isnan(est)) and np.array_equal(np.isfinite(gst), np.isfinite(est)), what + ": state"
        assert sh.scaled_err(got[:at], exp[:at]).max() <= SCAN_RTOL, what + ": before the bad sample"
