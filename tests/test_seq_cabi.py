"""CPU (-m "not gpu"): the K15 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package; the host-only one works without a device; the compute ones refuse bad arguments with a message that names the
argument -- their checks run before the device is touched -- and otherwise fail loudly here (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

NEW = ["mxg_seq_ratio_host", "mxg_seq_render", "mxg_seq_signal"]
CLASSES = ["maxiSeqBank", "maxiTriggerBank", "maxiCounterBank", "maxiStepBank", "maxiIndexBank", "maxiZXToPulseBank"]


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert len(m._lib.SIGNATURES["mxg_seq_render"][1]) == 25
    assert len(m._lib.SIGNATURES["mxg_seq_signal"][1]) == 15
    for cls in CLASSES:
        assert hasattr(m, cls), cls
    for name, val in (("ONZX", 0), ("COUNTER", 1), ("STEP", 2), ("INDEX", 3), ("ZXTOPULSE", 4), ("VAL_VALUES", 0), ("VAL_STEP", 1),
                      ("MAX_RATIOS", 64)):
        assert re.search(r"#define MXG_SEQ_%s %d\b" % (name, val), hdr), name
    assert [getattr(m, c).KIND for c in CLASSES[1:]] == [0, 1, 2, 3, 4]
    bank_hpp = open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read()
    dropin = open(os.path.join(ROOT, "include", "maximilian.h")).read()
    for cls in CLASSES:
        assert re.search(r"\bclass %s\b" % cls, bank_hpp), cls
    for cls in ("maxiRatioSeq", "maxiStep", "maxiCounter", "maxiIndex", "maxiZXToPulse"):
        assert re.search(r"\bclass %s\b" % cls, dropin), cls


def test_ratio_host_needs_no_device_and_refuses():
    import maximilian_amd as m
    lib = m.lib()
    norm, lens = m.seq_ratio_tables([[3, 3, 2], [1], [4, 4, 4, 1, 1, 1, 1]])
    assert lens.tolist() == [3, 1, 7] and norm.shape == (3, 7)
    assert norm[0, :3].tolist() == [3.0 / 8.0, 6.0 / 8.0, 0.0] and np.isnan(norm[0, 3:]).all()   # the boundary 1.0 becomes 0.0
    assert norm[1, 0] == 0.0
    assert norm[2, :7].tolist() == [4 / 16, 8 / 16, 12 / 16, 13 / 16, 14 / 16, 15 / 16, 0.0]
    t65, n65 = np.ones((1, 65)), np.zeros((1, 65))
    one = np.array([1], np.int32)
    assert lib.mxg_seq_ratio_host(1, 65, one.ctypes.data, t65.ctypes.data, n65.ctypes.data) < 0      # L = 65
    assert b"64" in lib.mxg_last_error()
    t, n = np.ones((2, 4)), np.zeros((2, 4))
    for bad in ([4, 0], [5, 1], [-1, 2]):                                                          # a length < 1, or > L
        ln = np.array(bad, np.int32)
        assert lib.mxg_seq_ratio_host(2, 4, ln.ctypes.data, t.ctypes.data, n.ctypes.data) < 0
        assert b"length" in lib.mxg_last_error()
    assert lib.mxg_seq_ratio_host(2, 4, None, t.ctypes.data, n.ctypes.data) < 0
    assert b"null" in lib.mxg_last_error()
    assert lib.mxg_seq_ratio_host(0, 4, one.ctypes.data, t.ctypes.data, n.ctypes.data) < 0


def _dummy():
    """Host addresses standing in for device pointers: the calls below are refused before anything is dereferenced."""
    buf = np.zeros(64)
    return buf, buf.ctypes.data


def test_render_refuses_bad_arguments_before_touching_the_device():
    import maximilian_amd as m
    lib = m.lib()
    buf, p = _dummy()
    INVALID = -1

    def render(freq=p, clk=p, phase=None, P=1, L=3, dst=p, ist=p, trig=p, val=None, values=None, vlen=None, PV=0, LV=0, mode=0):
        return lib.mxg_seq_render(4, 4, freq, clk, phase, 0, p, p, P, L, None, mode, values, vlen, PV, LV, None, None, None, dst, ist,
                                  trig, val, None, None)

    for kw, word in ((dict(dst=None), b"state"), (dict(ist=None), b"state"), (dict(L=65), b"64"), (dict(L=0), b"64"), (dict(P=0), b"pattern"),
                     (dict(trig=None), b"no output"), (dict(phase=p), b"not both"), (dict(freq=None, clk=None), b"not both"),
                     (dict(val=p), b"value lists"), (dict(val=p, values=p, vlen=p, PV=1, LV=0), b"value lists"), (dict(mode=7), b"val_mode"),
                     (dict(P=1000, L=64), b"48 KB")):
        st = render(**kw)
        assert st < 0, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
    # mxg_seq_signal
    def signal(kind=0, a=p, b=None, values=None, vlen=None, PV=0, LV=0, dst=p, ist=p, out=p):
        return lib.mxg_seq_signal(kind, 4, 4, a, b, values, vlen, PV, LV, None, None, dst, ist, out, None)

    for kw, word in ((dict(dst=None), b"state"), (dict(ist=None), b"state"), (dict(kind=5), b"kind"), (dict(kind=-1), b"kind"),
                     (dict(a=None), b"null"), (dict(out=None), b"null"), (dict(kind=1), b"second input"), (dict(kind=3, values=p, vlen=p, PV=1, LV=4), b"second input"),
                     (dict(kind=2), b"value lists"), (dict(kind=2, values=p, vlen=p, PV=1, LV=0), b"value lists")):
        st = signal(**kw)
        assert st < 0, kw
        assert word in lib.mxg_last_error(), (kw, lib.mxg_last_error())
