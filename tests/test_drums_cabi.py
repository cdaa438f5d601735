"""CPU (-m "not gpu"): the K21 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package, the kind and flag numbers agree in the header, the arithmetic header and the package, the bank classes are present in the
package and in the C++ facade; mxg_drum_render / mxg_drum_host and mxg_clock_render / mxg_clock_host refuse bad arguments with
MXG_ERR_INVALID and a message that names the argument -- the checks run before the device is touched -- and the render otherwise
fails loudly here (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ["mxg_drum_render", "mxg_drum_host", "mxg_clock_render", "mxg_clock_host"]
MXG_ERR_INVALID = -1


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    arith = open(os.path.join(ROOT, "maximilian_amd", "csrc", "mxg_drums.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    for name, val in (("KICK", 0), ("SNARE", 1), ("HATS", 2)):
        assert re.search(r"\bMXG_DRUM_%s = %d\b" % (name, val), hdr) and re.search(r"#define MXG_DRUM_%s %d\b" % (name, val), arith)
        assert m.DRUM_KINDS[name.lower()] == val
    for name, val in (("INVERSE", 1), ("DISTORTION", 2), ("FILTER", 4), ("LIMITER", 8)):
        assert re.search(r"#define MXG_DRUM_%s %d\b" % (name, val), hdr) and re.search(r"#define MXG_DRUM_%s %d\b" % (name, val), arith)
    hpp = open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read()
    for cls in ("maxiKickBank", "maxiSnareBank", "maxiHatsBank", "maxiClockBank"):
        assert hasattr(m, cls), cls
        assert re.search(r"\b(class|struct|using) %s\b" % cls, hpp), cls
    m_err = re.search(r"MXG_ERR_INVALID\s*=\s*(-?\d+)", hdr)
    assert m_err and int(m_err.group(1)) == MXG_ERR_INVALID


def test_drum_calls_refuse_bad_arguments_before_touching_anything():
    """Host addresses stand in for device pointers: every render call below is refused before anything is dereferenced."""
    import maximilian_amd as m
    lib = m.lib()
    buf = np.zeros(4096)
    p = buf.ctypes.data
    other = np.zeros(64)
    q = other.ctypes.data
    base = dict(kind=1, flags=15, V=4, N=4, trig=q, tpv=1, rand=q, pitch=q, par=q, hold=q, shape=q, coef=q, gain=q, phase=q, dst=q,
                ist=q, fst=q, out=p)
    cases = [(dict(V=0), b"V and N"), (dict(N=0), b"V and N"), (dict(kind=3), b"kind"), (dict(kind=-1), b"kind"), (dict(flags=16), b"flags"),
             (dict(rand=None), b"required for snare and hats"), (dict(kind=2, rand=None), b"required for snare and hats"),
             (dict(kind=0), b"kick draws no rand"), (dict(pitch=None), b"pitch"), (dict(par=None), b"envelope"),
             (dict(hold=None), b"envelope"), (dict(shape=None), b"shape"), (dict(coef=None), b"coefficient"),
             (dict(phase=None), b"state"), (dict(dst=None), b"state"), (dict(ist=None), b"state"), (dict(fst=None), b"state"),
             (dict(out=None), b"output"), (dict(trig=p), b"overlaps"), (dict(trig=p + 8 * 15), b"overlaps"), (dict(rand=p + 8), b"overlaps"),
             (dict(tpv=0, trig=p + 8 * 16 - 8), b"overlaps")]
    for kw, word in cases:
        args = list({**base, **kw}.values())
        assert lib.mxg_drum_render(*args, None) == MXG_ERR_INVALID, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
        assert lib.mxg_drum_host(*args) == MXG_ERR_INVALID, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    assert (buf == 0).all() and (other == 0).all()
    # what may be null: the trigger block, the gain, and shape / coef when their switch is off
    V, N = 3, 9
    par = np.array([[1.0] * V, [0.9] * V, [0.5] * V, [0.99] * V])
    hold, pitch, rnd = np.ones(V, np.int64), np.full(V, 800.0), np.full((N, V), 123456789, np.int32)
    st = [np.zeros(V), np.zeros((2, V)), np.zeros((6, V), np.int64), np.zeros((3, V))]
    out = np.ones((N, V))
    assert lib.mxg_drum_host(1, 0, V, N, None, 0, rnd.ctypes.data, pitch.ctypes.data, par.ctypes.data, hold.ctypes.data, None, None, None,
                             *[a.ctypes.data for a in st], out.ctypes.data) == 0, lib.mxg_last_error()
    assert (out == 0).all(), "never triggered: silence"
    assert lib.mxg_drum_host(0, 0, V, N, None, 0, None, pitch.ctypes.data, par.ctypes.data, hold.ctypes.data, None, None, None,
                             *[a.ctypes.data for a in st], out.ctypes.data) == 0, lib.mxg_last_error()


def test_clock_calls_refuse_bad_arguments():
    import maximilian_amd as m
    lib = m.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    base = dict(V=2, N=4, bps=p, clk=p + 64, last=p + 128, playhead=p + 192, count=p + 256, tick=p + 320)
    for kw, word in [(dict(V=0), b"V and N"), (dict(N=0), b"V and N"), (dict(bps=None), b"bps"), (dict(clk=None), b"clk"),
                     (dict(playhead=None), b"playhead"), (dict(count=None), b"count"), (dict(tick=None), b"tick")]:
        args = list({**base, **kw}.values())
        assert lib.mxg_clock_render(*args, None) == MXG_ERR_INVALID, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
        assert lib.mxg_clock_host(*args) == MXG_ERR_INVALID, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    tick = np.zeros(64)   # V * N = 8 doubles of it are the tick block: it may overlap none of the other arrays
    t = tick.ctypes.data
    for name, off in (("bps", 0), ("clk", 56), ("last", 60), ("playhead", 8), ("count", 0)):
        args = list({**base, "tick": t, name: t + off}.values())
        assert lib.mxg_clock_render(*args, None) == MXG_ERR_INVALID and b"overlaps" in lib.mxg_last_error(), name
        assert lib.mxg_clock_host(*args) == MXG_ERR_INVALID and b"overlaps" in lib.mxg_last_error(), name
    assert (buf == 0).all() and (tick == 0).all()
    # a null lastcount is 0
    bps, clk, ph, cnt, tick = np.full(1, 600.0), np.zeros(1), np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros((200, 1))
    assert lib.mxg_clock_host(1, 200, bps.ctypes.data, clk.ctypes.data, None, ph.ctypes.data, cnt.ctypes.data, tick.ctypes.data) == 0
    assert tick.sum() == ph[0] == 2 and tick[74, 0] == 1.0


def test_render_fails_loudly_without_a_device():
    import maximilian_amd as m
    lib = m.lib()
    if lib.mxg_init(-1) >= 0:
        return  # a device is present: the GPU suite covers the calls
    buf = np.zeros(256)
    p = buf.ctypes.data
    assert lib.mxg_drum_render(0, 0, 4, 4, None, 0, None, p, p, p, None, None, None, p, p, p, p, p + 1024, None) < 0 and lib.mxg_last_error()
    assert lib.mxg_clock_render(2, 4, p, p + 64, None, p + 128, p + 192, p + 256, None) < 0 and lib.mxg_last_error()
    for cls in (m.maxiKickBank, m.maxiSnareBank, m.maxiHatsBank, m.maxiClockBank):
        with pytest.raises(m.MaxiGpuError):
            cls(4)
