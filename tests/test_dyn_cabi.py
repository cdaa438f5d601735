"""CPU (-m "not gpu"): the K12 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package; the host-only one works without a device, the compute ones refuse bad arguments or fail loudly (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

NEW = ["mxg_dynamics_render", "mxg_rms_render", "mxg_envgen_set_time_host"]


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert len(m._lib.SIGNATURES["mxg_dynamics_render"][1]) == 32
    assert len(m._lib.SIGNATURES["mxg_rms_render"][1]) == 11
    for cls in ("maxiDynamicsBank", "maxiRMSBank"):
        assert hasattr(m, cls)
    for flag, bit in (("THRESHOLD_HIGH", 1), ("RATIO_HIGH", 2), ("KNEE_HIGH", 4), ("THRESHOLD_LOW", 8), ("RATIO_LOW", 16), ("KNEE_LOW", 32)):
        assert re.search(r"#define MXG_DYN_PS_%s %d\b" % (flag, bit), hdr)
    assert sorted(m.banks.DYN_PS.values()) == [1, 2, 4, 8, 16, 32]


def test_set_time_host_needs_no_device():
    import maximilian_amd as m
    lib = m.lib()
    m.maxiSettings.setup(44100, 2, 1024)
    tab = m.banks._DynControl._asr()
    assert tab[:, 4].tolist() == [441.0, 0.0, 441.0] and tab[:, 5].tolist() == [0.0, 1.0, 0.0]
    assert lib.mxg_envgen_set_time_host(tab.ctypes.data, 3, 0, 20.0) == 0
    assert tab[0, 4] == 882.0 and tab[0, 2] == 1.0 / 882.0
    assert lib.mxg_envgen_set_time_host(tab.ctypes.data, 3, 2, -46692.0) == 1   # a second HOLD stage
    assert lib.mxg_envgen_set_time_host(tab.ctypes.data, 3, 3, 5.0) == 1        # past the table
    assert lib.mxg_envgen_set_time_host(None, 3, 0, 5.0) < 0                     # refused argument
    assert b"null" in lib.mxg_last_error()


def test_render_without_valid_arguments_fails_loudly():
    """No device here, or a null pointer on a GPU box: either way a negative status and a message, never a quiet success."""
    import maximilian_amd as m
    lib = m.lib()
    z = [None] * 8
    st = lib.mxg_dynamics_render(4, 4, *z, 0, None, None, None, None, None, 3, None, 16, None, 16, *([None] * 11))
    assert st < 0 and lib.mxg_last_error()
    assert lib.mxg_rms_render(4, 4, None, None, None, 16, None, None, None, None, None) < 0
