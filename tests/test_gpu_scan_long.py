"""GPU (-m gpu): K28, the long time-parallel scan (csrc/scan_long.hip, mxg_scan_long_render, maxiLongScanBank): three launches --
chunk summaries, the scan over the chunks, the render -- over signals of any length.  Its arithmetic (csrc/mxg_scan_long.h) is
+ - * in a fixed order with contraction off, so the device is held to the library's host twin mxg_scan_long_host BIT FOR BIT; the
twin is held to the sequential recurrence within SCAN_LONG_RTOL per kind in tests/test_scan_long_host.py, and the device once more
here on the sweep."""
import os
import subprocess

import numpy as np
import pytest

import scan_host as sh
import scan_long_host as sl
from conftest import ROOT, assert_bits_equal
from scan_long_host import RAGGED, SCAN_LONG_RTOL, T

pytestmark = pytest.mark.gpu

# (V, N): the smallest shapes that cross a chunk, a lane run of phase B, the Kogge-Stone of phase B with runs of more than one chunk,
# the ragged tail, more than one wavefront of voices, and the V limit
SHAPES = [(1, 2 * T), (3, 65 * T), (1, (64 * 64 + 1) * T), (5, RAGGED), (65, 2 * T + 64), (4096, T + 1)]
GUARD = 777.5


def _settings(kind, V, rng):
    full = sl.sweep_params(kind)
    return np.ascontiguousarray(full[:, rng.choice(full.shape[1], V, replace=V > full.shape[1])])


class _Dev:
    """Coefficient rows and a state array on the device; render() is one mxg_scan_long_render between guard bands."""

    def __init__(self, mx, kind, coef, st):
        self.mx, self.kind, self.L = mx, kind, mx.lib()
        self.V = coef.shape[1]
        self.coef = mx.DeviceBuffer.from_numpy(np.ascontiguousarray(coef))
        self.st = mx.DeviceBuffer.from_numpy(np.ascontiguousarray(st))

    def render(self, x, inplace=False, stream=None, pad=64):
        N, V = x.shape
        D = self.mx.DeviceBuffer
        buf = np.full(N * V + 2 * pad, GUARD)
        if inplace:
            buf[pad:pad + N * V] = x.ravel()
        dout = D.from_numpy(buf)
        din = dout if inplace else D.from_numpy(np.ascontiguousarray(x))
        po = dout.ptr + 8 * pad
        self.mx._lib.check(self.L.mxg_scan_long_render(sl.KIND_ID[self.kind], V, N, po if inplace else din.ptr, self.coef.ptr, self.st.ptr, po, stream),
                           "mxg_scan_long_render")
        got = dout.numpy()
        assert np.all(got[:pad] == GUARD) and np.all(got[-pad:] == GUARD), "guard bands round d_out"
        return got[pad:-pad].reshape(N, V)

    def state(self):
        return self.st.numpy()


@pytest.mark.parametrize("V,N", SHAPES)
@pytest.mark.parametrize("kind", sl.KINDS)
def test_device_equals_host_twin_bit_for_bit(mx, port, kind, V, N):
    rng = np.random.default_rng(V * 7 + N)
    par = _settings(kind, V, rng)
    coef = sl.coef_rows(port, kind, par)
    x = rng.uniform(-1, 1, (2 * N, V))
    st0 = rng.uniform(-1, 1, (sl.NROWS[kind], V))
    dev = _Dev(mx, kind, coef, st0)
    got = np.concatenate([dev.render(x[:N]), dev.render(x[N:])])    # two calls, the state carried
    exp, est = sl.host_long(kind, x, coef, st0, 2)
    what = "%s V=%d N=%d" % (kind, V, N)
    assert_bits_equal(got, exp, what + ": output")
    assert_bits_equal(dev.state(), est, what + ": state (the rows the kind does not own among them)")
    assert_bits_equal(est[sl.NSTATE[kind]:], st0[sl.NSTATE[kind]:], what + ": rows the kind does not own")


@pytest.mark.parametrize("kind", sl.KINDS)
def test_sweep_on_device_within_the_bound(mx, port, kind):
    """The sweep of tests/test_scan_long_host.py at 65 chunks, one voice per setting, from random states."""
    par, x, st0 = sl.sweep_case(kind, 65 * T, calls=1)
    coef = sl.coef_rows(port, kind, par)
    dev = _Dev(mx, kind, coef, sl.full_state(kind, st0))
    got = dev.render(x)
    gst = dev.state()[:sl.NSTATE[kind]]
    exp, est = sl.oracle_seq(port, kind, x, par, st0)
    err, serr = sh.scaled_err(got, exp), sl.state_err(port, kind, par, gst, est, exp)
    w = int(err.argmax())
    print("%s, 65 chunks, %d settings: max |err| / peak = %.3e at %s; continued from the final state %.3e (bound %.0e)"
          % (kind, par.shape[1], err.max(), par[:, w].tolist(), serr.max(), SCAN_LONG_RTOL[kind]))
    assert err.max() <= SCAN_LONG_RTOL[kind] and serr.max() <= SCAN_LONG_RTOL[kind]


@pytest.mark.parametrize("V,N", [(1, 3 * T + 64 + 5), (6, RAGGED)])
@pytest.mark.parametrize("kind", sl.KINDS)
def test_in_place_equals_out_of_place(mx, port, kind, V, N):
    rng = np.random.default_rng(N + V)
    par = _settings(kind, V, rng)
    coef = sl.coef_rows(port, kind, par)
    x, st0 = rng.uniform(-1, 1, (N, V)), rng.uniform(-1, 1, (sl.NROWS[kind], V))
    a, b = _Dev(mx, kind, coef, st0), _Dev(mx, kind, coef, st0)
    out = a.render(x)
    assert_bits_equal(b.render(x, inplace=True), out, kind + ": in place")
    assert_bits_equal(b.state(), a.state(), kind + ": in place, state")
    assert_bits_equal(a.state()[sl.NSTATE[kind]:], st0[sl.NSTATE[kind]:], kind + ": rows the kind does not own")


def _sequential(mx, kind, V, N, dx, coef3, dst, dout):
    """The sequential entry point of the kind on the same state array."""
    L = mx.lib()
    if kind in ("dc", "svf", "biquad"):
        rc = L.mxg_filter2_render(sl.KIND_ID[kind], V, N, dx.ptr, coef3.ptr, dst.ptr, dout.ptr, None)
    elif kind == "lag":
        rc = L.mxg_lag_render(V, N, dx.ptr, coef3.ptr, coef3.ptr + 8 * V, 0, dst.ptr, dout.ptr, None)
    else:
        cut = mx.DeviceBuffer(V)   # (unread: the coefficients are given)
        rc = L.mxg_filter_render(0 if kind == "lores" else 1, V, N, dx.ptr, cut.ptr, 0, cut.ptr, 0, coef3.ptr, dst.ptr, dout.ptr, None)
    mx._lib.check(rc, "sequential entry point")


@pytest.mark.parametrize("kind", sl.KINDS)
def test_alternating_with_the_sequential_entry_point(mx, port, kind):
    """long, sequential, long, sequential on ONE state array: each sequential block is the oracle's bits from the state the long call
    left, and the whole stream stays within the bound."""
    V, n_long, n_seq = 5, RAGGED, 300
    rng = np.random.default_rng(77)
    par = _settings(kind, V, rng)
    coef = sl.coef_rows(port, kind, par)
    coef3 = np.concatenate([coef, np.zeros((1, V))]) if kind in ("lores", "hires") else coef   # mxg_filter_render reads [3][V]
    st0 = sl.full_state(kind, rng.uniform(-1, 1, (sl.NSTATE[kind], V)))
    dev = _Dev(mx, kind, coef3, st0)
    D = mx.DeviceBuffer
    x = rng.uniform(-1, 1, (2 * (n_long + n_seq), V))
    got, at = [], 0
    for _ in range(2):
        got.append(dev.render(x[at:at + n_long]))
        at += n_long
        before = dev.state()
        dout = D((n_seq, V))
        _sequential(mx, kind, V, n_seq, D.from_numpy(np.ascontiguousarray(x[at:at + n_seq])), dev.coef, dev.st, dout)
        exp, est = sl.oracle_seq(port, kind, x[at:at + n_seq], par, before[:sl.NSTATE[kind]])
        assert_bits_equal(dout.numpy(), exp, kind + ": the sequential block from the state the long call left")
        assert_bits_equal(dev.state()[:sl.NSTATE[kind]], est, kind + ": its state")
        got.append(dout.numpy())
        at += n_seq
    exp, _ = sl.oracle_seq(port, kind, x, par, st0[:sl.NSTATE[kind]])
    assert sh.scaled_err(np.concatenate(got), exp).max() <= SCAN_LONG_RTOL[kind]


def test_streams(mx, port):
    """A non-default stream gives the default stream's bits, and two banks on two streams, launched back to back without a
    synchronisation between them, do not disturb each other: scratch is per stream."""
    kind, V, N = "biquad", 2, 9 * T + 100
    rng = np.random.default_rng(12)
    par = _settings(kind, V, rng)
    L = mx.lib()
    s1, s2 = L.mxg_stream_create(), L.mxg_stream_create()
    try:
        xs = [rng.uniform(-1, 1, (N, V)) for _ in range(2)]
        banks = []
        for s in (None, None, s1, s2):
            b = mx.maxiLongScanBank(V, kind, stream=s)
            b.setBiquad(par[0], par[1], par[2], par[3])
            banks.append(b)
        ref = [banks[i].process(xs[i]).numpy() for i in range(2)]               # default stream, one after the other
        dx = [mx.DeviceBuffer.from_numpy(x) for x in xs]
        outs = [banks[2 + i].process(dx[i]) for i in range(2)]                 # two streams, in flight together
        for i in range(2):
            assert_bits_equal(outs[i].numpy(), ref[i], "stream %d" % (i + 1))
            assert_bits_equal(banks[2 + i].state(), banks[i].state(), "stream %d: state" % (i + 1))
            exp, _ = sl.host_long(kind, xs[i], banks[i].coef, np.zeros((3, V)))
            assert_bits_equal(ref[i], exp, "the host twin")
    finally:
        mx._lib.check(L.mxg_sync(), "mxg_sync")
        L.mxg_stream_destroy(s1)
        L.mxg_stream_destroy(s2)


def test_looper_slot_filtered_in_place(mx, port):
    """End to end: noise recorded into a maxiLooperBank slot, the slot filtered in place through maxiLongScanBank(1, "biquad") by its
    slot_pointer, downloaded: within the bound of the oracle's biquad over the recorded samples."""
    n = 5 * T + 300
    rng = np.random.default_rng(4)
    noise = rng.uniform(-1, 1, (n, 1))
    looper = mx.maxiLooperBank(1, n)
    looper.trigger()
    looper.setRecordMix(0.0)
    looper.loopRecord(mx.DeviceBuffer.from_numpy(noise), 1.0, n)
    recorded = looper.download(0)
    assert np.abs(recorded).max() > 0.5, "the slot holds the recording"
    bank = mx.maxiLongScanBank(1, "biquad")
    par = np.array([[0.0], [1200.0], [0.7], [0.0]])
    bank.setBiquad(par[0], par[1], par[2], par[3])
    out = bank.process(looper.slot_pointer(0), N=n, out=looper.slot_pointer(0))
    assert out == looper.slot_pointer(0)
    got = looper.download(0)
    exp, est = sl.oracle_seq(port, "biquad", recorded[:, None], par, np.zeros((3, 1)))
    err = sh.scaled_err(got[:, None], exp).max()
    print("looper slot through maxiLongScanBank: max |err| / peak = %.3e" % err)
    assert err <= SCAN_LONG_RTOL["biquad"]
    assert sl.state_err(port, "biquad", par, bank.state(), est, exp).max() <= SCAN_LONG_RTOL["biquad"]
    looper.free()


def test_the_existing_knob_is_untouched(mx, port):
    """time_parallel = 1 and N = 4096: mxg_filter2_render still takes the exact kernel -- K28 is not routed to."""
    V, N = 3, 4096
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (N, V))
    par = np.stack([np.zeros(V), np.full(V, 1200.0), np.full(V, 0.7), np.zeros(V)])
    exp, est, _ = port.filter2(2, x, par)
    prev = mx.lib().mxg_tune(b"time_parallel", 1)
    try:
        bank = mx.maxiBiquadBank(V)
        bank.set(par[0].astype(np.int32), par[1], par[2], par[3])
        assert_bits_equal(bank.play(mx.DeviceBuffer.from_numpy(x)).numpy(), exp, "N = 4096 with the knob on")
        assert_bits_equal(bank.state.numpy(), est, "state")
    finally:
        mx.lib().mxg_tune(b"time_parallel", prev)


def test_facade_longscan_smoke():
    """The C++ facade's maxiLongScanBank (include/maximilian_bank.hpp) through host/facade_longscan_smoke."""
    exe = os.path.join(ROOT, "host", "facade_longscan_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_longscan_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade_longscan_smoke: ok" in r.stdout
