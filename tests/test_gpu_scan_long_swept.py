"""GPU (-m gpu): K31, the long time-parallel scan with per-sample coefficients (csrc/scan_long_swept.hip,
mxg_scan_long_render_swept, maxiLongScanBank.process_swept): three launches -- chunk pairs, the scan over the chunks, the render --
over signals of any length.  Its arithmetic (csrc/mxg_scan_long_swept.h) is + - * in a fixed order with contraction off, so the
device is held to the library's host twin mxg_scan_long_swept_host BIT FOR BIT; the twin is held to the sequential per-sample
recurrence within SWEPT_RTOL per kind in tests/test_scan_long_swept_host.py, and the device once more here on the sweep set."""
import os
import subprocess

import numpy as np
import pytest

import scan_host as sh
import scan_long_host as sl
import scan_long_swept_host as sw
from conftest import ROOT, assert_bits_equal
from scan_long_swept_host import RAGGED, SWEPT_RTOL, TS

pytestmark = pytest.mark.gpu

# (V, N, coef_rows): a chunk boundary; phase B with runs of two chunks per lane and its Kogge-Stone; the ragged tail; plain steps
# only; one block of 64; a call one sample short of a chunk (blocks of 512 ... 64 and 63 steps); more than one workgroup of voices
# with an odd voice left over; the V limit
SHAPES = [(1, 2 * TS, 2), (3, 66 * TS, 3), (5, RAGGED, 2), (1, 63, 3), (1, 64, 2), (2, TS - 1, 3), (65, 2 * TS + 64, 2), (4096, TS + 1, 3)]
GUARD = 777.5


def _case(kind, V, N, rows, seed=0):
    """V voices over 2 N samples: the sweep set's settings dealt round the voices, noise and start states of their own."""
    names = sw.settings(kind)
    rng = np.random.default_rng(V * 7 + N + seed)
    only = [names[i] for i in rng.permutation(len(names))[:min(V, len(names))]]
    _, par, _, _ = sw.sweep_case(kind, N, calls=2, only=only)
    idx = np.arange(V) % len(only)
    par = tuple(np.ascontiguousarray(p[:, idx]) for p in par)
    x = rng.uniform(-1, 1, (2 * N, V))
    st0 = rng.uniform(-1, 1, (sw.NROWS[kind], V))
    return par, sw.coef_ps(kind, par, rows), x, st0


class _Dev:
    """A state array on the device; render() is one mxg_scan_long_render_swept between guard bands."""

    def __init__(self, mx, kind, st):
        self.mx, self.kind, self.L = mx, kind, mx.lib()
        self.st = mx.DeviceBuffer.from_numpy(np.ascontiguousarray(st))

    def render(self, x, coef, inplace=False, stream=None, pad=64):
        N, V = x.shape
        D = self.mx.DeviceBuffer
        buf = np.full(N * V + 2 * pad, GUARD)
        if inplace:
            buf[pad:pad + N * V] = x.ravel()
        dout = D.from_numpy(buf)
        din = dout if inplace else D.from_numpy(np.ascontiguousarray(x))
        dcoef = D.from_numpy(np.ascontiguousarray(coef))
        po = dout.ptr + 8 * pad
        self.mx._lib.check(self.L.mxg_scan_long_render_swept(sw.KIND_ID[self.kind], V, N, po if inplace else din.ptr, dcoef.ptr, coef.shape[1], self.st.ptr, po, stream),
                           "mxg_scan_long_render_swept")
        got = dout.numpy()
        assert np.all(got[:pad] == GUARD) and np.all(got[-pad:] == GUARD), "guard bands round d_out"
        return got[pad:-pad].reshape(N, V)

    def state(self):
        return self.st.numpy()


@pytest.mark.parametrize("V,N,rows", SHAPES)
@pytest.mark.parametrize("kind", sw.KINDS)
def test_device_equals_host_twin_bit_for_bit(mx, kind, V, N, rows):
    par, coef, x, st0 = _case(kind, V, N, rows)
    dev = _Dev(mx, kind, st0)
    got = np.concatenate([dev.render(x[:N], coef[:N]), dev.render(x[N:], coef[N:])])    # two calls, the state carried
    exp, est = sw.host_swept(kind, x, coef, st0, 2)
    what = "%s V=%d N=%d rows=%d" % (kind, V, N, rows)
    assert_bits_equal(got, exp, what + ": output")
    assert_bits_equal(dev.state(), est, what + ": state (the rows the kind does not own among them)")
    assert_bits_equal(est[sw.NSTATE[kind]:], st0[sw.NSTATE[kind]:], what + ": rows the kind does not own")


@pytest.mark.parametrize("kind", sw.KINDS)
def test_sweep_set_on_device_within_the_bound(mx, port, kind):
    """The sweep set of tests/test_scan_long_swept_host.py at 66 chunks, one voice per setting, from random states."""
    names, par, x, st0 = sw.sweep_case(kind, 66 * TS, calls=1)
    exp, est = sw.oracle_seq(port, kind, x, par, st0)
    sw.assert_stable(exp, names, kind)
    dev = _Dev(mx, kind, sw.full_state(kind, st0))
    got = dev.render(x, sw.coef_ps(kind, par))
    gst = dev.state()[:sw.NSTATE[kind]]
    err, serr = sh.scaled_err(got, exp), sw.state_err(port, kind, par, gst, est, exp)
    print("%s, 66 chunks, %d settings: max |err| / peak = %.3e at %s; continued from the final state %.3e (bound %.0e)"
          % (kind, len(names), err.max(), names[int(err.argmax())], serr.max(), SWEPT_RTOL[kind]))
    assert err.max() <= SWEPT_RTOL[kind] and serr.max() <= SWEPT_RTOL[kind]


@pytest.mark.parametrize("V,N", [(1, 3 * TS + 64 + 5), (6, RAGGED)])
@pytest.mark.parametrize("kind", sw.KINDS)
def test_in_place_equals_out_of_place(mx, kind, V, N):
    par, coef, x, st0 = _case(kind, V, N, 3, seed=5)
    x, coef = x[:N], coef[:N]
    a, b = _Dev(mx, kind, st0), _Dev(mx, kind, st0)
    out = a.render(x, coef)
    assert_bits_equal(b.render(x, coef, inplace=True), out, kind + ": in place")
    assert_bits_equal(b.state(), a.state(), kind + ": in place, state")
    assert_bits_equal(a.state()[sw.NSTATE[kind]:], st0[sw.NSTATE[kind]:], kind + ": rows the kind does not own")


def _sequential_swept(mx, kind, V, N, dx, dcoef, dst, dout):
    """The sequential per-sample entry point of the kind on the same state array; dcoef [N][3][V] (lores / hires) or [N][2][V] (the
    lag: mxg_lag_render takes alpha and alphaReciprocal as [N][V] each, so they are split here)."""
    L = mx.lib()
    if kind == "lag":
        c = dcoef.numpy().reshape(N, 2, V)
        da, dr = mx.DeviceBuffer.from_numpy(np.ascontiguousarray(c[:, 0])), mx.DeviceBuffer.from_numpy(np.ascontiguousarray(c[:, 1]))
        rc = L.mxg_lag_render(V, N, dx.ptr, da.ptr, dr.ptr, 1, dst.ptr, dout.ptr, None)
    else:
        rc = L.mxg_filter_render_coefs(0 if kind == "lores" else 1, V, N, dx.ptr, dcoef.ptr, dst.ptr, dout.ptr, None)
    mx._lib.check(rc, "sequential per-sample entry point")
    mx._lib.check(L.mxg_sync(), "mxg_sync")


@pytest.mark.parametrize("kind", sw.KINDS)
def test_alternating_on_one_state_array(mx, port, kind):
    """Two rounds of: swept long, the sequential per-sample entry point, the constant long scan (mxg_scan_long_render, the
    coefficients held at the block's first sample), the sequential one again -- ONE state array.  Each sequential block is the
    oracle's bits from the state left to it, and the whole stream stays within the summed bound."""
    V, n_long, n_seq, n_const = 5, RAGGED, 300, 2 * sl.T + 100
    lens = [n_long, n_seq, n_const, n_seq] * 2
    names = sw.settings(kind)[:V]
    _, par, x, st0 = sw.sweep_case(kind, sum(lens), calls=1, only=names)
    par = tuple(p.copy() for p in par)
    at = 0
    for i, n in enumerate(lens):
        if i % 4 == 2:
            for p in par:
                p[at:at + n] = p[at]           # the constant block: the parameters stand still
        at += n
    coef = sw.coef_ps(kind, par)               # [N][3][V] / [N][2][V]
    D = mx.DeviceBuffer
    dev = _Dev(mx, kind, sw.full_state(kind, st0))
    L = mx.lib()
    got, at = [], 0
    for i, n in enumerate(lens):
        xb, cb = np.ascontiguousarray(x[at:at + n]), np.ascontiguousarray(coef[at:at + n])
        if i % 4 == 0:
            got.append(dev.render(xb, cb))
        elif i % 4 == 2:
            dxb, dcoef, dout = D.from_numpy(xb), D.from_numpy(np.ascontiguousarray(cb[0, :2])), D((n, V))
            mx._lib.check(L.mxg_scan_long_render(sw.KIND_ID[kind], V, n, dxb.ptr, dcoef.ptr, dev.st.ptr, dout.ptr, None), "mxg_scan_long_render")
            got.append(dout.numpy())
        else:
            before = dev.state()
            dout = D((n, V))
            _sequential_swept(mx, kind, V, n, D.from_numpy(xb), D.from_numpy(cb), dev.st, dout)
            exp, est = sw.oracle_seq(port, kind, xb, tuple(p[at:at + n] for p in par), before[:sw.NSTATE[kind]])
            assert_bits_equal(dout.numpy(), exp, "%s block %d: the sequential block from the state left to it" % (kind, i))
            assert_bits_equal(dev.state()[:sw.NSTATE[kind]], est, "%s block %d: its state" % (kind, i))
            got.append(dout.numpy())
        at += n
    exp, _ = sw.oracle_seq(port, kind, x, par, st0)
    sw.assert_stable(exp, names, kind)
    err = sh.scaled_err(np.concatenate(got), exp).max()
    print("%s alternating: max |err| / peak = %.3e" % (kind, err))
    assert err <= SWEPT_RTOL[kind] + sl.SCAN_LONG_RTOL[kind]


def test_streams(mx):
    """Two banks on two streams, launched back to back without a synchronisation between them, give the default stream's bits:
    scratch is per stream."""
    kind, V, N = "lores", 2, 9 * TS + 100
    L = mx.lib()
    s1, s2 = L.mxg_stream_create(), L.mxg_stream_create()
    try:
        cases = [_case(kind, V, N, 2 + i, seed=40 + i) for i in range(2)]
        banks = [mx.maxiLongScanBank(V, kind, stream=s) for s in (None, None, s1, s2)]
        ref = [banks[i].process_swept(cases[i][2][:N], cases[i][1][:N]).numpy() for i in range(2)]   # default stream, one after the other
        dx = [mx.DeviceBuffer.from_numpy(np.ascontiguousarray(c[2][:N])) for c in cases]
        dc = [mx.DeviceBuffer.from_numpy(np.ascontiguousarray(c[1][:N])) for c in cases]
        outs = [banks[2 + i].process_swept(dx[i], dc[i], coef_rows=2 + i) for i in range(2)]        # two streams, in flight together
        for i in range(2):
            assert_bits_equal(outs[i].numpy(), ref[i], "stream %d" % (i + 1))
            assert_bits_equal(banks[2 + i].state(), banks[i].state(), "stream %d: state" % (i + 1))
            exp, _ = sw.host_swept(kind, cases[i][2][:N], cases[i][1][:N], np.zeros((5, V)))
            assert_bits_equal(ref[i], exp, "the host twin")
    finally:
        mx._lib.check(L.mxg_sync(), "mxg_sync")
        L.mxg_stream_destroy(s1)
        L.mxg_stream_destroy(s2)


def test_looper_slot_filtered_in_place_by_a_sweep(mx, port):
    """End to end: noise recorded into a maxiLooperBank slot, the slot filtered in place through maxiLongScanBank(1, "lores") with a
    cutoff on a 2 Hz LFO by its slot_pointer, downloaded: within the bound of the oracle's lores with that cutoff per sample."""
    n = 5 * TS + 300
    rng = np.random.default_rng(4)
    noise = rng.uniform(-1, 1, (n, 1))
    looper = mx.maxiLooperBank(1, n)
    looper.trigger()
    looper.setRecordMix(0.0)
    looper.loopRecord(mx.DeviceBuffer.from_numpy(noise), 1.0, n)
    recorded = looper.download(0)
    assert np.abs(recorded).max() > 0.5, "the slot holds the recording"
    cutoff = sw._lfo(np.arange(n, dtype=np.float64), 2.0, 200.0, 8000.0)[:, None]
    res = np.full((n, 1), 30.0)
    bank = mx.maxiLongScanBank(1, "lores")
    out = bank.process_swept(looper.slot_pointer(0), mx.sweep_lores(cutoff, res), N=n, out=looper.slot_pointer(0))
    assert out == looper.slot_pointer(0)
    got = looper.download(0)
    exp, est = sw.oracle_seq(port, "lores", recorded[:, None], (cutoff, res), np.zeros((2, 1)))
    err = sh.scaled_err(got[:, None], exp).max()
    print("looper slot through a swept maxiLongScanBank: max |err| / peak = %.3e" % err)
    assert err <= SWEPT_RTOL["lores"]
    assert sw.state_err(port, "lores", (cutoff, res), bank.state()[:2], est, exp).max() <= SWEPT_RTOL["lores"]
    looper.free()


def test_facade_longsweep_smoke():
    """The C++ facade's maxiLongScanBank::processSwept (include/maximilian_bank.hpp) through host/facade_longsweep_smoke."""
    exe = os.path.join(ROOT, "host", "facade_longsweep_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_longsweep_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade_longsweep_smoke: ok" in r.stdout
