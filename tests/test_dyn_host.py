"""CPU (-m "not gpu"): mxg_dyn.h -- the arithmetic dyn.hip's kernels run -- compiled for the host with g++ under the oracle's
FPFLAGS (tests/host_dyn.cpp) reproduces tests/golden/dyn.npz BIT FOR BIT: outputs, detector levels, every state array at every
stored cut, ring contents, for every case, with the blocks cut at the stored cuts and at further uneven ones.  On the host the
header calls the same glibc log10 / pow / sqrt as the reference, so no tolerance applies.  Also: the ring index logic and
mxg_envgen_set_time_host against step-by-step restatements, and the reference's 17.Compressor example against the drop-in header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dyn_host
from conftest import ROOT, assert_bits_equal

CASES = ["compress", "play", "persample"]


def ref_example():
    """17.Compressor of the reference checkout oracle/Makefile names (REF), read in place."""
    import re
    ref = os.environ.get("MAXI_REF") or re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    return os.path.join(ref, "cpp", "commandline", "maximilian_examples", "17.Compressor", "main.cpp")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    import maximilian_amd as mx
    mx.maxiSettings.setup(44100, 2, 1024)
    return dyn_host.build(tmp_path_factory.mktemp("dyn"))


@pytest.fixture(scope="module")
def g(golden):
    return golden("dyn.npz")


def assert_same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        assert_bits_equal(a, b, what)
    else:
        assert np.array_equal(a, b), what


@pytest.mark.parametrize("extra", [(), (1, 64, 777, 1501, 3999)])
@pytest.mark.parametrize("name", CASES)
def test_host_reproduces_golden(L, g, name, extra):
    c = dyn_host.load_case(g, name)
    bank = dyn_host.construct(c, lambda V: dyn_host.host_bank(L, V))
    out, lvl, states = dyn_host.play_case(bank, c, extra)
    assert_same(out, c["out"], name + " out")
    assert not np.isnan(out).any()
    assert (out == 0.0).mean() > 0.05  # the exact zeros of outDB = NaN are in the data
    assert_same(lvl.astype(np.float32).astype(np.float64), c["level_db"].astype(np.float64), name + " level_db")
    ncut = len(c["cuts"]) - 1
    assert sorted(states) == list(range(ncut))
    for i in range(ncut):
        exp = dyn_host.expected_state(c, i, i == ncut - 1)
        for k, e in exp.items():
            got = states[i][k]
            if k.endswith("_ring"):
                assert not got[e.shape[0]:].any(), (name, k)
                got = got[:e.shape[0]]
            assert_same(got, e, "%s cut %d %s" % (name, i, k))
    assert not bank.overflow.any()
    # the setters left what the reference's did
    assert_same(bank.window, c["snap%d/window" % (ncut - 1)], "window")
    assert_same(bank.lookahead, c["snap%d/look" % (ncut - 1)], "look")
    for v in range(c["sig"].shape[1]):
        assert_same(bank.stages_high, c["snap%d/stages_h" % (ncut - 1)][v], "stages_h")
        assert_same(bank.stages_low, c["snap%d/stages_l" % (ncut - 1)][v], "stages_l")
    assert (dyn_host.tie_start(lvl, c["pars"]) == c["sig"].shape[0]).all()  # the generator's assertion, re-made on the checker's levels
    assert (c["margin_db"] > dyn_host.NEAR_DB).all()


def test_golden_pins_peak_detector_below_one(g):
    """The PEAK detector is the double abs: |control| < 1 must not collapse to 0 (an int abs would give level 0 = -inf dB)."""
    c = dyn_host.load_case(g, "play")
    peak = np.flatnonzero(c["analyser"] == 0)
    assert peak.size
    lvl = c["level_db"][:, peak]
    ctl = np.abs(c["control"][:, peak])
    m = (ctl > 0) & (ctl < 1)
    assert m.any() and np.isfinite(lvl[m]).all() and (lvl[m] < 0).all()


def test_rms_host_reproduces_golden(L, g):
    x, cap, cuts = g["rms/in_q"] / 32768.0, int(g["rms/cap"]), [int(c) for c in g["rms/cuts"]]
    N, V = x.shape
    sr = int(g["rms/sr"])
    ring, pos, run, ovf = np.zeros((cap, V)), np.zeros(V, np.int32), np.zeros(V), np.zeros(V, np.uint32)
    win = np.full(V, int(10.0 / 1000.0 * sr), np.uint32)
    out = np.zeros((N, V))
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        for n, v, ms in g["rms/ops"]:
            if int(n) == a:  # maxiRMS::setWindowSize
                s = int(ms / 1000.0 * sr)
                if s <= cap:
                    win[int(v)] = s
                run[int(v)] = 0.0
        assert_same(win, g["rms/window"][i], "window")
        xb, ob = np.ascontiguousarray(x[a:b]), np.zeros((b - a, V))
        L.rms_host_render(V, b - a, xb.ctypes.data, win.ctypes.data, ring.ctypes.data, cap, pos.ctypes.data, run.ctypes.data,
                          ovf.ctypes.data, ob.ctypes.data)
        out[a:b] = ob
    for got, key in ((out, "out"), (ring, "ring"), (pos, "pos"), (run, "running")):
        assert_same(got, g["rms/" + key], key)
    assert not ovf.any()


def test_ring_index_logic_fuzz(L):
    """push / tail / head against a list that is rotated step by step."""
    rng = np.random.default_rng(11)
    for trial in range(200):
        size = int(rng.choice([1, 2, 3, 7, 64, 500]))
        buf, idx = [0.0] * size, 0
        hist = []  # every pushed value, oldest first
        for step in range(int(rng.integers(1, 4 * size + 20))):
            x = float(step + 1)
            buf[idx] = x
            hist.append(x)
            nxt = L.dyn_host_ring_advance(idx, size)
            assert nxt == (idx + 1) % size
            idx = nxt
            assert buf[L.dyn_host_ring_head(idx, size)] == hist[-1]
            n = int(rng.integers(0, size + 1))
            slot = L.dyn_host_ring_tail(idx, size, n)
            assert 0 <= slot < size
            # tail(n): the value pushed n pushes ago (0 if the ring is not that full yet); tail(0) is the slot about to be written
            if n == 0:
                assert slot == idx
            else:
                assert buf[slot] == (hist[-n] if n <= len(hist) else 0.0)


def test_set_time_matches_restatement_and_golden(L, g):
    import maximilian_amd as mx
    lib = mx.lib()
    HOLD = -46692.0

    def asr(sr):
        mx.maxiSettings.setup(sr, 2, 1024)
        return mx.banks._DynControl._asr()

    try:
        for row in g["set_time"]:  # setupASR(10, 10) + setTime in the compiled reference
            sr, idx, ms, err = int(row[0]), int(row[1]), row[2], int(row[3])
            tab = asr(sr)
            assert lib.mxg_envgen_set_time_host(tab.ctypes.data, 3, idx, ms) == err
            assert_same(tab, row[4:].reshape(3, 6), "set_time %s" % row[:4])
        rng = np.random.default_rng(12)
        for trial in range(300):
            sr = int(rng.choice([8000, 44100, 48000, 96000]))
            tab = asr(sr)
            exp = tab.copy()
            for call in range(4):
                idx = int(rng.integers(0, 5))
                ms = float(rng.choice([HOLD, 0.0, 0.01, 1.0, 200.0, rng.uniform(0.0, 500.0)]))
                # the restatement, step by step
                has_hold = bool((exp[:, 5] != 0).any())
                if idx >= 3 or (ms == HOLD and has_hold):
                    err = 1
                else:
                    err = 0
                    if ms == HOLD:
                        exp[idx, 4], exp[idx, 5], exp[idx, 2] = 0.0, 1.0, 0.0
                    else:
                        length = float(np.floor(ms / 1000.0 * sr))
                        with np.errstate(divide="ignore"):
                            exp[idx, 4], exp[idx, 2], exp[idx, 5] = length, np.float64(1.0) / np.float64(length), 0.0
                host = tab.copy()
                assert lib.mxg_envgen_set_time_host(tab.ctypes.data, 3, idx, ms) == err
                assert L.dyn_host_set_time(host.ctypes.data, 3, idx, ms, float(sr)) == err
                assert_same(tab, exp, "library")
                assert_same(host, exp, "host build")
    finally:
        mx.maxiSettings.setup(44100, 2, 1024)


def test_reference_compressor_example_compiles_against_dropin_header():
    REF_EXAMPLE = ref_example()
    if not os.path.exists(REF_EXAMPLE):
        pytest.skip("the reference checkout is not present")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), REF_EXAMPLE])
