"""CPU (-m "not gpu"): the K30 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package; the layout helper works without a device, answers the offsets and ring doubles of hand-computed topologies and rejects
what the kernel does not take; the compute entry point refuses bad arguments or fails loudly (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

import revnet_cases as rc
from conftest import ROOT

NEW = ["mxg_revnet_layout_host", "mxg_revnet_render"]


def u32(a):
    return np.asarray(list(a) + [0], np.uint32)


def layout_status(lib, combs, aps, lowp=None):
    cs, ap = u32(combs), u32(aps)
    lp = None if lowp is None else u32(lowp)
    return lib.mxg_revnet_layout_host(len(combs), len(aps), cs.ctypes.data, ap.ctypes.data, None if lp is None else lp.ctypes.data,
                                      None, None)


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert len(m._lib.SIGNATURES["mxg_revnet_layout_host"][1]) == 7
    assert len(m._lib.SIGNATURES["mxg_revnet_render"][1]) == 16
    assert hasattr(m, "maxiReverbNetBank") and hasattr(m, "revnet_layout")
    assert re.search(r"#define MXG_REVNET_MAX_STAGES %d\b" % rc.MAX_STAGES, hdr)


def test_layout_of_hand_computed_topologies():
    import maximilian_amd as m
    # maxiSatReverb's numbers: 778 + 901 + 1011 + 1123 + 125 + 42 + 12
    assert m.revnet_layout([778, 901, 1011, 1123], [125, 42, 12]) == ([0, 778, 1679, 2690, 3813, 3938, 3980], 3992)
    # maxiFreeVerb::play(x)
    offs, S = m.revnet_layout(rc.FV_COMBS, rc.FV_APS, [1] * 8)
    assert S == 12587 and offs[:3] == [0, 1557, 3174] and offs[8] == 11024 and offs[-1] == 12246
    assert m.revnet_layout([], [1]) == ([0], 1)
    assert m.revnet_layout([1], []) == ([0], 1)
    assert m.revnet_layout([1, 2, 63], [64, 65]) == ([0, 1, 3, 66, 130], 195)
    assert m.revnet_layout([44100], [44100, 1]) == ([0, 44100, 88200], 88201)
    offs, S = m.revnet_layout([64] * 32, [3] * 32, [1] * 32)   # the most stages there are
    assert S == 32 * 67 and offs == [64 * c for c in range(32)] + [2048 + 3 * a for a in range(32)]
    for case in rc.CASES:
        combs, aps, lowp = rc.topology(case)
        assert m.revnet_layout(combs, aps, lowp) == rc.layout(combs, aps), case["name"]


def test_layout_rejects_what_the_kernel_does_not_take():
    import maximilian_amd as m
    lib = m.lib()
    assert layout_status(lib, [64], [1], [1]) == 0            # a low-pass comb of exactly one tile
    assert layout_status(lib, [63], [1], [0]) == 0            # plain, it may be shorter
    assert layout_status(lib, [1] * 32, [1] * 32) == 0
    bad = [
        (([0], [5], None), "length"),                          # length 0
        (([5], [0], None), "length"),
        (([44101], [], None), "length"),                       # beyond the reference's ring
        (([], [44101], None), "length"),
        (([], [], None), "at least 1"),                        # P + A = 0
        (([70] * 33, [5], None), "32"),                        # P = 33
        (([70], [5] * 33, None), "32"),
        (([100, 63], [5], [0, 1]), "low-pass"),                # a low-pass comb of 63
    ]
    for (combs, aps, lowp), word in bad:
        assert layout_status(lib, combs, aps, lowp) < 0, (combs, aps, lowp)
        assert word in lib.mxg_last_error().decode(), lib.mxg_last_error()
        with pytest.raises(m.MaxiGpuError):
            m.revnet_layout(combs, aps, lowp)
    with pytest.raises(ValueError):
        m.revnet_layout([10.5], [3])
    with pytest.raises(ValueError):
        m.revnet_layout([100, 100], [3], [1])


def test_render_without_valid_arguments_fails_loudly():
    """No device here, or a refused argument on a GPU box: either way a negative status and a message, never a quiet success."""
    import maximilian_amd as m
    lib = m.lib()
    z = np.zeros(4096)
    p = z.ctypes.data
    cs, ap, lp = u32([100, 64]), u32([7]), u32([0, 1])

    def refused(*args):
        return lib.mxg_revnet_render(*args) < 0 and len(lib.mxg_last_error()) > 0

    topo = (2, 1, cs.ctypes.data, ap.ctypes.data, lp.ctypes.data)
    for k in range(8):  # each device pointer by itself: this topology needs all eight
        args = [p] * 8
        args[k] = None
        assert refused(*topo, 1, 1, *args, None), k
    zero_len = u32([100, 0])
    assert refused(2, 1, zero_len.ctypes.data, ap.ctypes.data, None, 1, 1, *([p] * 8), None)
    assert b"length" in lib.mxg_last_error()
    assert refused(0, 0, None, None, None, 1, 1, *([p] * 8), None)
    if lib.mxg_init(-1) != 0:
        assert refused(*topo, 1, 1, *([p] * 8), None)  # no device: an error, not a CPU rendering
        with pytest.raises(m.MaxiGpuError):
            m.maxiReverbNetBank(8, [100], [7])
    with pytest.raises(m.MaxiGpuError):
        m.maxiReverbNetBank(8, [100], [0])
