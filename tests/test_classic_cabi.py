"""CPU (-m "not gpu"): the K23 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package, and the classes are present in the three headers and the package; the host helpers and the mxg_*_host forms give the
reference's bits without a device; the render entry points refuse bad arguments with a message that names the argument -- their
checks run before the device is touched -- and otherwise fail loudly here (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

import classic_host as ch
from conftest import ROOT, assert_bits_equal

RENDER = ["mxg_dyn_gate_render", "mxg_dyn_compress_render", "mxg_envelope_line_render", "mxg_lag_render", "mxg_map_render"]
HOST = ["mxg_dyn_coeff_host", "mxg_dyn_makeup_host", "mxg_envelope_trigger_host", "mxg_map_range_host", "mxg_dyn_gate_host",
        "mxg_dyn_compress_host", "mxg_envelope_line_host", "mxg_lag_host", "mxg_map_host"]
BANKS = ["maxiDynBank", "maxiEnvelopeBank", "maxiLagExpBank", "maxiMapBank"]
DROPIN = ["maxiDyn", "maxiEnvelope", "maxiLagExp", "maxiMap", "maxiConvert"]


class LibHostBackend(ch.HostBackend):
    """The mxg_*_host entry points of the library behind the HostBackend interface."""
    name = "lib"

    def __init__(self, m):
        lib = m.lib()

        class L:
            cls_h_gate = lib.mxg_dyn_gate_host
            cls_h_compress = lib.mxg_dyn_compress_host
            cls_h_lag = lib.mxg_lag_host
            cls_h_map = lib.mxg_map_host
            cls_h_makeup = lib.mxg_dyn_makeup_host
            cls_h_coeff = lib.mxg_dyn_coeff_host

            @staticmethod
            def cls_h_line(V, N, S, seg, count, trig, tindex, tamp, sr, dst, ist, out):
                assert int(lib.mxg_sample_rate()) == int(sr)
                return lib.mxg_envelope_line_host(V, N, S, seg, count, trig, tindex, tamp, dst, ist, out)

            @staticmethod
            def cls_h_explin_den(a, b):
                r, aux = np.array([[a], [b], [0.0], [0.0]]), np.zeros(1)
                assert lib.mxg_map_range_host(2, 1, r.ctypes.data, aux.ctypes.data) == 0
                return float(aux[0])
        self.L = L


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in RENDER + HOST:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    for name, val in ch.MAP_MODES.items():
        assert re.search(r"#define MXG_MAP_%s %d\b" % (name.upper(), val), hdr), name
        assert m.MAP_MODES[name] == val
    for name, val in (("THRESHOLD", ch.PS_THRESHOLD), ("ATTACK", ch.PS_ATTACK), ("RELEASE", ch.PS_RELEASE), ("RATIO", ch.PS_RATIO)):
        assert re.search(r"#define MXG_CLASSIC_PS_%s %d\b" % (name, val), hdr), name
        assert m.CLASSIC_PS[name.lower()] == val
    assert re.search(r"#define MXG_ENVELOPE_MAX_S 64\b", hdr)
    bank_hpp = open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read()
    dropin = open(os.path.join(ROOT, "include", "maximilian.h")).read()
    for cls in BANKS:
        assert hasattr(m, cls), cls
        assert re.search(r"\bclass %s\b" % cls, bank_hpp), cls
    for cls in DROPIN:
        assert re.search(r"\bclass %s\b" % cls, dropin), cls


def test_host_forms_give_the_reference_bits(golden):
    """Every golden case through the library's own mxg_*_host entry points, envelope triggers through mxg_envelope_trigger_host:
    no device is needed."""
    import maximilian_amd as m
    g = golden("classic.npz")
    lib = m.lib()
    be = LibHostBackend(m)
    ch.play_gate_case(be, g)
    ch.play_compress_case(be, g, (7, 777))
    ch.play_lag_case(be, g)
    res = ch.play_map_cases(be, g)
    assert res["linlin"] == 0 and res["clamp"] == 0
    assert_bits_equal(be.explin_den(g["map/range"]), g["map/aux"], "mxg_map_range_host")
    assert_bits_equal(be.makeup(g["comp/ratio"]), g["comp/makeup"], "mxg_dyn_makeup_host")
    assert_bits_equal([be.coeff(g["comp/setters"][2], 44100.0), be.coeff(g["comp/setters"][3], 44100.0)], g["comp/members"][2:], "mxg_dyn_coeff_host")

    def trigger(v, index, amp, count, dst, ist):
        V = dst.shape[1]
        mask = np.zeros(V, np.int32)
        mask[v] = 1
        ix, am = np.full(V, index, np.int32), np.full(V, amp)
        cnt = np.ascontiguousarray(count, np.int32)
        assert lib.mxg_envelope_trigger_host(V, ix.ctypes.data, am.ctypes.data, mask.ctypes.data, cnt.ctypes.data, dst.ctypes.data, ist.ctypes.data) == 0

    for sr, key in ((44100, "env"), (48000, "env48")):
        lib.mxg_settings(sr, 2, 1024)
        try:
            ch.play_env_case(be, g, trigger, (7,), key=key, sr=float(sr))
        finally:
            lib.mxg_settings(44100, 2, 1024)


def test_trigger_host_refuses_an_index_outside_the_table():
    import maximilian_amd as m
    lib = m.lib()
    V = 3
    count = np.array([4, 2, 8], np.int32)
    amp = np.full(V, 0.5)
    for index, ok in (([0, 0, 0], True), ([2, 0, 6], True), ([3, 0, 0], False), ([0, 1, 0], False), ([0, 0, 7], False), ([-1, 0, 0], False)):
        dst, ist = ch.env_fresh(V)
        ix = np.array(index, np.int32)
        s = lib.mxg_envelope_trigger_host(V, ix.ctypes.data, amp.ctypes.data, None, count.ctypes.data, dst.ctypes.data, ist.ctypes.data)
        if ok:
            assert s == 0 and ist[0].tolist() == index and ist[1].tolist() == [1, 1, 1] and dst[0].tolist() == [0.5] * 3
        else:
            assert s < 0 and b"index" in lib.mxg_last_error() and not ist.any() and not dst.any(), index   # nothing is changed
    # a masked-out voice may hold any index
    dst, ist = ch.env_fresh(V)
    ix, mask = np.array([0, 99, 0], np.int32), np.array([1, 0, 1], np.int32)
    assert lib.mxg_envelope_trigger_host(V, ix.ctypes.data, amp.ctypes.data, mask.ctypes.data, count.ctypes.data, dst.ctypes.data, ist.ctypes.data) == 0
    assert ist[1].tolist() == [1, 0, 1]


def _callers(lib, p):
    def caller(fn, **defaults):
        return lambda **kw: fn(*{**defaults, **kw}.values())
    q = p + 4096   # a second block: the outputs are distinct from the inputs
    gate = caller(lib.mxg_dyn_gate_render, V=4, N=4, d_in=p, d_threshold=p, d_attack=p, d_release=p, ps=0, d_holdtime=p, d_dst=p, d_ist=p, d_out=q, stream=None)
    comp = caller(lib.mxg_dyn_compress_render, V=4, N=4, d_in=p, d_ratio=p, d_makeup=p, d_threshold=p, d_attack=p, d_release=p, ps=0, d_dst=p, d_ist=p,
                  d_out=q, stream=None)
    line = caller(lib.mxg_envelope_line_render, V=4, N=4, S=8, d_segments=p, d_count=p, d_trig=None, d_trig_index=None, d_trig_amp=None, d_dst=p,
                  d_ist=p, d_out=q, stream=None)
    lag = caller(lib.mxg_lag_render, V=4, N=4, d_in=p, d_alpha=p, d_alpha_reciprocal=p, ps=0, d_val=p, d_out=q, stream=None)
    mp = caller(lib.mxg_map_render, mode=0, V=4, N=4, d_in=p, d_range=p, d_aux=p, d_out=q, stream=None)
    return gate, comp, line, lag, mp, q


def test_renders_refuse_bad_arguments_before_touching_the_device():
    """Host addresses stand in for device pointers: every call below is refused before anything is dereferenced."""
    import maximilian_amd as m
    lib = m.lib()
    buf = np.zeros(2048)
    p = buf.ctypes.data
    gate, comp, line, lag, mp, q = _callers(lib, p)
    cases = [(gate, dict(d_in=None), b"input"), (gate, dict(d_threshold=None), b"threshold"), (gate, dict(d_attack=None), b"attack"),
             (gate, dict(d_release=None), b"release"), (gate, dict(d_holdtime=None), b"holdtime"), (gate, dict(d_dst=None), b"dst"),
             (gate, dict(d_ist=None), b"ist"), (gate, dict(d_out=None), b"output"), (gate, dict(ps=8), b"ps_flags"), (gate, dict(ps=16), b"ps_flags"),
             (gate, dict(d_out=p), b"distinct"),
             (comp, dict(d_in=None), b"input"), (comp, dict(d_ratio=None), b"ratio"), (comp, dict(d_makeup=None), b"makeup"),
             (comp, dict(d_threshold=None), b"threshold"), (comp, dict(d_dst=None), b"dst"), (comp, dict(d_out=None), b"output"),
             (comp, dict(ps=16), b"ps_flags"), (comp, dict(ps=-1), b"ps_flags"), (comp, dict(d_out=p), b"distinct"),
             (line, dict(S=1), b"S "), (line, dict(S=65), b"S "), (line, dict(d_segments=None), b"segment"), (line, dict(d_count=None), b"count"),
             (line, dict(d_trig=p), b"trig_index"), (line, dict(d_trig=p, d_trig_index=p), b"trig_amp"), (line, dict(d_dst=None), b"dst"),
             (line, dict(d_ist=None), b"ist"), (line, dict(d_out=None), b"output"), (line, dict(d_trig=q, d_trig_index=p, d_trig_amp=p), b"distinct"),
             (lag, dict(d_in=None), b"d_in"), (lag, dict(d_alpha=None), b"d_alpha"), (lag, dict(d_alpha_reciprocal=None), b"d_alpha_reciprocal"),
             (lag, dict(d_val=None), b"d_val"), (lag, dict(d_out=None), b"d_out"), (lag, dict(d_out=p), b"distinct"),
             (mp, dict(mode=6), b"mode"), (mp, dict(mode=-1), b"mode"), (mp, dict(d_in=None), b"input"), (mp, dict(d_out=None), b"output"),
             (mp, dict(mode=0, d_range=None), b"range"), (mp, dict(mode=3, d_range=None), b"range"), (mp, dict(mode=2, d_aux=None), b"aux")]
    for fn, kw, word in cases:
        assert fn(**kw) < 0, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    # arguments a mode does not read may be null: the refusal, if any, is then not about them
    for mode in (4, 5):
        assert mp(mode=mode, d_range=None, d_aux=None, d_out=None) < 0 and b"output" in lib.mxg_last_error()
    assert mp(mode=1, d_aux=None, d_out=None) < 0 and b"output" in lib.mxg_last_error()
    # the host forms refuse the same way
    assert lib.mxg_map_host(7, 4, 4, p, p, p, q) < 0 and b"mode" in lib.mxg_last_error()
    assert lib.mxg_lag_host(4, 4, p, None, p, 0, p, q) < 0 and b"h_alpha" in lib.mxg_last_error()
    assert lib.mxg_envelope_line_host(4, 4, 0, p, p, None, None, None, p, p, q) < 0 and b"S " in lib.mxg_last_error()
    assert lib.mxg_map_range_host(9, 4, p, p) < 0 and b"mode" in lib.mxg_last_error()


def test_empty_banks_and_blocks_are_accepted_by_the_host_forms():
    import maximilian_amd as m
    lib = m.lib()
    buf = np.zeros(64)
    p, q = buf.ctypes.data, buf.ctypes.data + 256
    for V, N in ((0, 4), (4, 0)):
        assert lib.mxg_dyn_gate_host(V, N, p, p, p, p, 0, p, p, p, q) == 0
        assert lib.mxg_dyn_compress_host(V, N, p, p, p, p, p, p, 0, p, p, q) == 0
        assert lib.mxg_lag_host(V, N, p, p, p, 0, p, q) == 0
        assert lib.mxg_map_host(0, V, N, p, p, p, q) == 0
        assert lib.mxg_envelope_line_host(V, N, 2, p, p, None, None, None, p, p, q) == 0
    assert not buf.any()


def test_compute_fails_loudly_without_a_device():
    import maximilian_amd as m
    lib = m.lib()
    if lib.mxg_init(-1) >= 0:
        return  # a device is present: the GPU suite covers the calls
    buf = np.zeros(2048)
    gate, comp, line, lag, mp, _ = _callers(lib, buf.ctypes.data)
    for fn in (gate, comp, line, lag, mp):
        assert fn() < 0 and lib.mxg_last_error()
    for make in (lambda: m.maxiDynBank(4), lambda: m.maxiEnvelopeBank(4, [1.0, 1.0]), lambda: m.maxiLagExpBank(4), lambda: m.maxiMapBank(4)):
        with pytest.raises(m.MaxiGpuError):
            make()
