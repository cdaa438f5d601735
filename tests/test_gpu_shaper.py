"""GPU: the K18 entry points (mxg_shape_render, mxg_xfade_render, mxg_select_render, mxg_line_render) against the reference's
own bits (tests/golden/shaper.npz) and, on shapes the file does not hold, against the numpy model of tests/shaper_host.py
(pinned to the same file by tests/test_shaper_host.py).  hardclip, fastatan, fastAtanDist, the clipped branches, NaN positions,
the cross-fade, both selects and the line with its state are compared bit for bit; softclip bit for bit with the model and
within 2^-52 of the reference; atanDist and asymclip in ULPs of the reference value against the a-priori bounds of
tests/shaper_host.py (13 / 26 / 17).

Measured on an MI355X (the golden cases; the bounds were fixed before the run): see DESIGN.md section 4, K18."""
import itertools

import numpy as np
import pytest

import shaper_host as sh
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

MODEL = sh.ModelBackend()
VS, NS = [1, 3, 63, 64, 65, 130], [1, 7, 8, 9, 71]
SHAPES = list(itertools.product(VS, NS))   # odd N * V among them: (1, 1), (3, 7), (63, 9), (65, 71) ...
CANARY = 0x5A


@pytest.fixture(scope="module")
def gpu(mx):
    return sh.GpuBackend(mx)


@pytest.fixture(scope="module")
def g(golden):
    return golden("shaper.npz")


def gpu_prepare(mx):
    def prepare(par, st, v, start, end, ms, oneshot, sr):
        V = par.shape[1]
        mask = np.zeros(V, np.int32)
        mask[v] = 1
        a, b, c = (np.full(V, t, np.float64) for t in (start, end, ms))
        one = np.full(V, oneshot, np.int32)
        mx._lib.check(mx.lib().mxg_line_prepare_host(V, a.ctypes.data, b.ctypes.data, c.ctypes.data, one.ctypes.data, mask.ctypes.data,
                                                     float(sr), par.ctypes.data, st.ctypes.data), "mxg_line_prepare_host")
    return prepare


def test_golden_shaping(gpu, g):
    """Every mode, parameters per voice and per sample, cut as stored; the measured figures are printed next to the bounds."""
    res = sh.play_shape_cases(gpu, g)
    print("measured:", {"%s/%s" % (m, "ps" if ps else "pv"): v for (m, ps), v in res.items() if v})


def test_golden_xfade_select_line(mx, gpu, g):
    sh.play_xfade_cases(gpu, g)
    sh.play_select_cases(gpu, g)
    sh.play_line_case(gpu, g, gpu_prepare(mx), extra=(777,))


def test_softclip_is_the_host_builds_bits(gpu, g):
    xu = g["softclip_u/x"]
    assert_bits_equal(gpu.shape("softclip", xu), MODEL.shape("softclip", xu), "softclip, uniform draws")
    x = sh.signal(g)
    assert_bits_equal(gpu.shape("softclip", x), MODEL.shape("softclip", x), "softclip, the signal")


_cases = {}


def edge_inputs(V, N):
    if (V, N) not in _cases:
        rng = np.random.default_rng(1000 * V + N)
        x = rng.uniform(-1.5, 1.5, (N, V))
        x.flat[::5] = rng.choice([1.0, -1.0, 0.0, -0.0, float("nan")], x.flat[::5].size)
        p = dict(x=x, y=rng.uniform(-1.5, 1.5, (2, N, V)), shape=rng.uniform(0.5, 50.0, V), xf=rng.uniform(-1.5, 1.5, (N, V)),
                 index=rng.uniform(-1.0, 6.0, (N, V)), cvals=rng.uniform(-2, 2, (5, V)), svals=rng.uniform(-2, 2, (5, N, V)),
                 trig=rng.choice([-1.0, 0.0, 0.5, 1.0], (N, V), p=[0.4, 0.1, 0.2, 0.3]))
        par, st = sh.line_fresh(V)
        for v in range(V):
            sh.line_prepare_model(par, st, v, *rng.choice([-1.0, 0.0, 0.5, 2.0], 2), float(rng.choice([0.0, 3.0, 7.5, 20.0])), int(rng.integers(0, 2)), 1000.0)
        par[4] = rng.integers(0, 5, V) > 0
        p.update(par=par, st=st)
        exp = dict(hardclip=MODEL.shape("hardclip", x), softclip=MODEL.shape("softclip", x), fastatan=MODEL.shape("fastatan", x),
                   dist=MODEL.shape("fastAtanDist", x, p["shape"]), xfade=MODEL.xfade(p["y"], p["y"][::-1], p["xf"]),
                   xfade_pv=MODEL.xfade(p["y"][0], x, p["xf"][0]))
        for interp in (0, 1):
            exp["sel%d" % interp] = MODEL.select(interp, p["index"], p["cvals"], False)[0]
            exp["sig%d" % interp] = MODEL.select(interp, p["index"] / 5.0, p["svals"], True)[0]
        stm = st.copy()
        exp["line"] = MODEL.line(p["trig"], N, par, stm)
        exp["line_st"] = stm
        stc = st.copy()
        exp["line_const"] = MODEL.line(1.0, N, par, stc)
        exp["line_const_st"] = stc
        _cases[(V, N)] = (p, exp)
    return _cases[(V, N)]


@pytest.mark.parametrize("knob", [0, 1])
def test_edge_shapes(mx, gpu, knob):
    """V = 1 .. 130 x N = 1 .. 71, odd N * V among them: the tail, the shadow lanes, a chunk remainder, the pair rows; with the
    16-byte accesses (knob 0) and the 8-byte ones (rw_store = 1)."""
    lib = mx.lib()
    mx._lib.check(lib.mxg_tune(b"rw_store", knob), "mxg_tune")
    try:
        for V, N in SHAPES:
            p, exp = edge_inputs(V, N)
            what = "rw_store %d V %d N %d: " % (knob, V, N)
            x = p["x"]
            for mode in ("hardclip", "softclip", "fastatan"):
                assert_bits_equal(gpu.shape(mode, x), exp[mode], what + mode)
            assert_bits_equal(gpu.shape("fastAtanDist", x, p["shape"]), exp["dist"], what + "fastAtanDist")
            assert_bits_equal(gpu.xfade(p["y"], p["y"][::-1], p["xf"]), exp["xfade"], what + "xfade C = 2")
            assert_bits_equal(gpu.xfade(p["y"][0], x, p["xf"][0]), exp["xfade_pv"], what + "xfade per voice")
            for interp in (0, 1):
                assert_bits_equal(gpu.select(interp, p["index"], p["cvals"], False)[0], exp["sel%d" % interp], what + "select constants %d" % interp)
                assert_bits_equal(gpu.select(interp, p["index"] / 5.0, p["svals"], True)[0], exp["sig%d" % interp], what + "select signals %d" % interp)
            st = p["st"].copy()
            assert_bits_equal(gpu.line(p["trig"], N, p["par"], st), exp["line"], what + "line")
            assert_bits_equal(st, exp["line_st"], what + "line state")
            st = p["st"].copy()
            assert_bits_equal(gpu.line(1.0, N, p["par"], st), exp["line_const"], what + "line.play(1)")
            assert_bits_equal(st, exp["line_const_st"], what + "line.play(1) state")
    finally:
        mx._lib.check(lib.mxg_tune(b"rw_store", 0), "mxg_tune")


def test_line_pair_rows(mx, gpu):
    """The line's 16-byte pair rows (rw_store = 2): even V with shadow lanes, whole chunks and a ragged last one."""
    lib = mx.lib()
    mx._lib.check(lib.mxg_tune(b"rw_store", 2), "mxg_tune")
    try:
        for V, N in ((64, 71), (130, 71), (130, 8)):
            p, exp = edge_inputs(V, N)
            st = p["st"].copy()
            assert_bits_equal(gpu.line(p["trig"], N, p["par"], st), exp["line"], "pair rows V %d N %d" % (V, N))
            assert_bits_equal(st, exp["line_st"], "pair rows V %d N %d: state" % (V, N))
    finally:
        mx._lib.check(lib.mxg_tune(b"rw_store", 0), "mxg_tune")


def padded(mx, a, off=0):
    """A device block holding `a` at an offset of `off` bytes, canary bytes before and after -> (buffer, pointer, check)."""
    a = np.ascontiguousarray(a)
    raw = np.full(a.nbytes + 64, CANARY, np.uint8)
    raw[16 + off:16 + off + a.nbytes] = a.view(np.uint8).ravel()
    buf = mx.DeviceBuffer.from_numpy(raw)

    def read():
        back = buf.numpy()
        assert (back[:16 + off] == CANARY).all() and (back[16 + off + a.nbytes:] == CANARY).all(), "a call wrote outside its block"
        return back[16 + off:16 + off + a.nbytes].view(a.dtype).reshape(a.shape)
    return buf, buf.ptr + 16 + off, read


@pytest.mark.parametrize("off", [0, 8])
def test_in_place_offset_pointers_and_canaries(mx, off):
    """In place (d_out == d_in), an output 8 bytes off a 16-byte boundary (the 8-byte path), and nothing written before or after
    any block."""
    lib = mx.lib()
    for V, N in ((65, 71), (64, 9), (3, 7), (130, 71)):
        p, exp = edge_inputs(V, N)
        x = p["x"]
        dx = mx.DeviceBuffer.from_numpy(x)
        _, ptr, read = padded(mx, np.zeros((N, V)), off)
        mx._lib.check(lib.mxg_shape_render(0, V, N, dx.ptr, None, None, 0, ptr, None), "mxg_shape_render")
        assert_bits_equal(read(), exp["hardclip"], "offset %d V %d N %d: hardclip" % (off, V, N))
        _, ptr, read = padded(mx, x, off)   # in place
        ds = mx.DeviceBuffer.from_numpy(p["shape"])
        mx._lib.check(lib.mxg_shape_render(3, V, N, ptr, ds.ptr, None, 0, ptr, None), "mxg_shape_render")
        assert_bits_equal(read(), exp["dist"], "offset %d V %d N %d: fastAtanDist in place" % (off, V, N))
        d1, d2, dxf = (mx.DeviceBuffer.from_numpy(np.ascontiguousarray(a)) for a in (p["y"], p["y"][::-1], p["xf"]))
        _, ptr, read = padded(mx, np.zeros((2, N, V)), off)
        mx._lib.check(lib.mxg_xfade_render(2, V, N, d1.ptr, d2.ptr, dxf.ptr, 1, ptr, None), "mxg_xfade_render")
        assert_bits_equal(read(), exp["xfade"], "offset %d V %d N %d: xfade" % (off, V, N))
        di, dv = mx.DeviceBuffer.from_numpy(p["index"] / 5.0), mx.DeviceBuffer.from_numpy(p["svals"])
        _, ptr, read = padded(mx, np.zeros((N, V)), off)
        _, cptr, cread = padded(mx, np.zeros(V, np.uint32))
        mx._lib.check(lib.mxg_select_render(1, 5, V, N, di.ptr, dv.ptr, 1, 1, cptr, ptr, None), "mxg_select_render")
        assert_bits_equal(read(), exp["sig1"], "offset %d V %d N %d: SelectX" % (off, V, N))
        assert not cread().any()
        dt, dpar = mx.DeviceBuffer.from_numpy(p["trig"]), mx.DeviceBuffer.from_numpy(p["par"])
        _, ptr, read = padded(mx, np.zeros((N, V)), off)
        _, sptr, sread = padded(mx, p["st"])
        mx._lib.check(lib.mxg_line_render(V, N, dt.ptr, 0.0, dpar.ptr, sptr, ptr, None), "mxg_line_render")
        assert_bits_equal(read(), exp["line"], "offset %d V %d N %d: line" % (off, V, N))
        assert_bits_equal(sread(), exp["line_st"], "offset %d V %d N %d: line state" % (off, V, N))


def test_per_sample_parameters_that_repeat_the_per_voice_value(gpu, g):
    """A block that repeats the per-voice value gives the per-voice bits.  atanDist is the exception by design: per voice its
    factor comes from the host libm, per sample from the device's atan, so the repeated block is held to the per-sample bound
    against the reference instead."""
    x = sh.signal(g)[:300]
    N, V = x.shape
    shape = g["shape/pv/shape"]
    blk = np.ascontiguousarray(np.broadcast_to(shape, (N, V)))
    assert_bits_equal(gpu.shape("fastAtanDist", x, blk), gpu.shape("fastAtanDist", x, shape), "fastAtanDist")
    xa = np.ascontiguousarray(x[:, :2])
    a, b = g["shape/pv/asym_a"], g["shape/pv/asym_b"]
    pa, pb = (np.ascontiguousarray(np.broadcast_to(t, (N, 2))) for t in (a, b))
    assert_bits_equal(gpu.shape("asymclip", xa, pa, pb), gpu.shape("asymclip", xa, a, b), "asymclip")
    xf = np.array([-1.2, 0.3, 1.0])
    ch = np.stack([x, x[::-1]])
    assert_bits_equal(gpu.xfade(ch, ch[::-1], np.ascontiguousarray(np.broadcast_to(xf, (N, V)))), gpu.xfade(ch, ch[::-1], xf), "xfade")
    ref = g["shape/pv/atanDist"][:300]
    sh.check_shape("repeated block", "atanDist", gpu.shape("atanDist", x, blk), ref, 1)


@pytest.mark.parametrize("K", [1, 2, 64])
def test_select_sizes_and_the_nan_departure(gpu, K):
    """K = 1, 2 and 64; a NaN index reads element 0 and is counted per voice, the count accumulates over calls."""
    rng = np.random.default_rng(K)
    N, V = 71, 5
    index = rng.uniform(-1.0, K + 1.0, (N, V))
    index[0] = [-0.0, float("inf"), float("-inf"), K, K - 1e-12]
    index[3, 1] = index[9, 1] = index[70, 4] = float("nan")
    for values in (rng.uniform(-2, 2, (K, V)), rng.uniform(-2, 2, (K, N, V))):
        for interp, normalised in itertools.product((0, 1), (False, True)):
            ix = index / K if normalised else index
            got, cnt = gpu.select(interp, ix, values, normalised)
            exp, ecnt = MODEL.select(interp, ix, values, normalised)
            assert_bits_equal(got, exp, "K %d interpolate %d normalised %s" % (K, interp, normalised))
            assert cnt.tolist() == ecnt.tolist() == [0, 2, 0, 0, 1]
            if not interp:
                v0 = values[0] if values.ndim == 3 else np.broadcast_to(values[0], (N, V))
                assert_bits_equal(got[np.isnan(ix)], v0[np.isnan(ix)], "a NaN index reads element 0")


@pytest.mark.parametrize("C", [1, 2, 8])
def test_xfade_channels(gpu, C):
    rng = np.random.default_rng(80 + C)
    N, V = 9, 65
    ch1, ch2, xf = rng.uniform(-1, 1, (C, N, V)), rng.uniform(-1, 1, (C, N, V)), rng.uniform(-1.5, 1.5, (N, V))
    xf[0, :3] = [1.0, -1.0, float("nan")]
    assert_bits_equal(gpu.xfade(ch1, ch2, xf), MODEL.xfade(ch1, ch2, xf), "C = %d" % C)
    assert_bits_equal(gpu.xfade(ch1, ch2, xf[0]), MODEL.xfade(ch1, ch2, xf[0]), "C = %d, per voice" % C)


def test_python_banks(mx, g):
    """maxiShaperBank, maxiXFadeBank, maxiSelectBank and maxiLineBank give the entry points' bits; a chain stays on the device."""
    x = sh.signal(g)[:600]
    N, V = x.shape
    D = mx.DeviceBuffer
    dx = D.from_numpy(x)
    bank = mx.maxiShaperBank(V)
    assert_bits_equal(bank.hardclip(dx).numpy(), g["shape/pv/hardclip"][:600].astype(np.float64), "hardclip")
    assert_bits_equal(bank.fastAtanDist(dx, g["shape/pv/shape"]).numpy(), g["shape/pv/fastAtanDist"][:600], "fastAtanDist")
    sh.check_shape("bank", "atanDist", bank.atanDist(dx, g["shape/pv/shape"]).numpy(), g["shape/pv/atanDist"][:600], 0)
    shape_ps, _, _ = sh.per_sample_params(g)
    sh.check_shape("bank", "atanDist", bank.atanDist(D.from_numpy(x[:sh.NPS]), shape_ps).numpy(), g["shape/ps/atanDist"], 1)
    ch1, ch2, xf = sh.xfade_inputs(g)
    assert_bits_equal(mx.maxiXFadeBank(V).xfade(D.from_numpy(ch1), D.from_numpy(ch2), xf).numpy(), g["xfade/ps"], "xfade")
    index, values, normalised = sh.select_inputs(g)["const"]
    sel = mx.maxiSelectBank(V, interpolate=True)
    assert_bits_equal(sel.play(D.from_numpy(index), values, normalised).numpy(), g["sel/const/selectx"], "SelectX")
    assert not sel.nan_count.numpy().any()
    # oscillator -> distortion -> cross-fade by a line, no host array in between
    mx.maxiSettings.setup(1000, 2, 1024)
    try:
        line = mx.maxiLineBank(V)
        line.prepare(-1.0, 1.0, 100.0, False)
        line.triggerEnable(1)
        ramp = line.play(1.0, N=600)
        shaped = bank.softclip(dx)
        mixed = mx.maxiXFadeBank(V).xfade(dx, shaped, ramp).numpy()
        par, st = sh.line_fresh(V)
        for v in range(V):
            sh.line_prepare_model(par, st, v, -1.0, 1.0, 100.0, 0, 1000.0)
        par[4] = 1.0
        assert_bits_equal(mixed, MODEL.xfade(x, MODEL.shape("softclip", x), MODEL.line(1.0, 600, par, st)), "chain")
        assert not line.isLineComplete().any() and np.isfinite(mixed).all()
    finally:
        mx.maxiSettings.setup(44100, 2, 1024)
