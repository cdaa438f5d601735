"""CPU (-m "not gpu"): mxg_dattaro.h -- the arithmetic, the length rule and the tile rule dattaro.hip runs -- compiled for the
host.  It reproduces every case of tests/golden/dattaro.npz (the unmodified reference, tools/gen/gen_golden_dattaro.py) bit for
bit: outputs, ring contents, indices and the five state doubles, replayed in the case's blocks of changing length and again in
blocks of 1, 63, 64, 65 and 512.  The lengths and tap positions equal the reference constructor's at the five rates and at both
ends of the accepted range.  The kernel's way through a tile (every read before any write, sub-tiles over the input rings) is
fuzzed against the step-by-step walk from random full states at rates on both sides of the sub-tile threshold."""
import numpy as np
import pytest

import dattaro_cases as dc
import dattaro_host as dh
from conftest import assert_bits_equal


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return dh.build(tmp_path_factory.mktemp("dattaro"))


@pytest.fixture(scope="module")
def g():
    return dh.load_golden()


def host_layout(host, rate):
    lens, offs = np.zeros(dc.RINGS, np.int32), np.zeros(dc.RINGS, np.int32)
    taps, rings = np.zeros(dc.TAPS, np.int32), np.zeros(dc.TAPS, np.int32)
    S = host.dt_host_layout(rate, lens.ctypes.data, offs.ctypes.data, taps.ctypes.data, rings.ctypes.data)
    return S, lens.tolist(), offs.tolist(), taps.tolist(), rings.tolist()


def test_lengths_are_the_reference_constructors(host, g):
    rates = g["rates"].tolist()
    assert rates[:5] == dc.RATES and rates[5:] == list(dc.accepted_ends()) == g["accepted_ends"].tolist()
    for k, rate in enumerate(rates):
        S, lens, offs, taps, rings = host_layout(host, rate)
        assert lens == g["lengths"][k].tolist() == dc.lengths(rate), rate
        assert taps == g["taps"][k].tolist() == dc.taps(rate), rate
        assert (lens, offs, S) == dc.layout(rate) and rings == dc.TAP_RING
    # the issue's check values
    k = rates.index(44100)
    assert g["lengths"][k][6:].tolist() == dc.CHECK_44100["D"] and g["fbap"][k].tolist() == dc.CHECK_44100["fbap"]
    assert g["taps"][k].tolist() == dc.CHECK_44100["taps"]
    k = rates.index(48000)
    assert g["lengths"][k][6:].tolist() == dc.CHECK_48000["D"] and g["fbap"][k].tolist() == dc.CHECK_48000["fbap"]
    # the smallest tap distance at 44 100 Hz
    lens, taps = dc.lengths(44100), dc.taps(44100)
    assert min(lens[dc.TAP_RING[j]] - 1 - taps[j] for j in range(dc.TAPS)) == 845


def test_acceptance_rule_against_brute_force(host):
    rates = np.arange(1, 400001)
    exp = dc.accepted(rates)
    got = np.array([host.dt_host_layout(int(r), None, None, None, None) >= 0 for r in rates])
    assert np.array_equal(got, exp)
    lo, hi = dc.accepted_ends()
    assert not exp[lo - 2] and exp[lo - 1] and exp[hi - 1] and not exp[hi]
    assert max(dc.lengths(hi)) == dc.MAX_LEN


def test_golden_file_is_what_the_issue_asks(g):
    assert sorted(g["cases"].tolist()) == sorted(c["name"] for c in dc.CASES)
    assert {dc.case_rate(c) for c in dc.CASES} == set(dc.RATES) | set(dc.accepted_ends())
    assert {c["signal"] for c in dc.CASES} == {"impulse", "noise", "tail"}
    for case in dc.CASES:
        y = g[case["name"] + "/out"]
        assert y.shape == (2, case["N"], case["V"]) and int(g[case["name"] + "/rate"]) == dc.case_rate(case)
        assert not np.isnan(y).any() and (y != 0).any(axis=1).all()
        if case["signal"] == "tail":
            assert case["N"] - case["noise"] > 2 * max(dc.lengths(case["rate"]))
            assert (y[:, -100:] != 0).any()  # still ringing after every ring has wrapped twice
    assert any(len(set(c["blocks"])) > 4 for c in dc.CASES)  # a block sequence with changing N
    assert "reference sources" in str(g["provenance"])


@pytest.mark.parametrize("case", dc.CASES, ids=[c["name"] for c in dc.CASES])
def test_host_build_reproduces_golden(host, g, case):
    x = dh.case_inputs(case, g)
    st = dh.State(dc.case_rate(case), case["V"])
    exp = g[case["name"] + "/out"]
    got = np.zeros_like(exp)
    for a, b in dc.block_edges(case):
        got[:, a:b] = dh.host_render(host, st, np.ascontiguousarray(x[a:b]))
    assert_bits_equal(got, exp, case["name"] + ": output")
    dh.check_case_state(case, g, st, case["name"])


@pytest.mark.parametrize("block", [1, 63, 64, 65, 512])
def test_block_length_does_not_matter(host, g, block):
    """One block or many: the state carries everything."""
    case = [c for c in dc.CASES if c["name"] == "r8000"][0]
    x = dh.case_inputs(case, g)
    whole = dh.State(case["rate"], case["V"])
    exp = dh.host_render(host, whole, x)
    st = dh.State(case["rate"], case["V"])
    got = np.concatenate([dh.host_render(host, st, np.ascontiguousarray(x[n:n + block])) for n in range(0, case["N"], block)], axis=1)
    assert_bits_equal(got, exp, "r8000 in blocks of %d" % block)
    assert_bits_equal(got, g["r8000/out"], "r8000 in blocks of %d against the golden file" % block)
    for (name, a), (_, e) in zip(st.parts(), whole.parts()):
        assert_bits_equal(a.astype(np.float64), e.astype(np.float64), name)
    dh.check_case_state(case, g, st, "r8000 in blocks of %d" % block)


def test_tile_walk_matches_step_by_step(host):
    rng = np.random.default_rng(9)
    lo, hi = dc.accepted_ends()
    sub = 0
    for trial, rate in enumerate([lo, 3400, 8000, 16000, 22050, 35000, 35700, 36000, 44100, 48000, 96000, hi] * 2):
        lens, offs, S = dc.layout(rate)
        for N in (1, 63, 64, 65, 300):
            x = np.ascontiguousarray(rng.uniform(-1, 1, N))
            rings = np.ascontiguousarray(rng.uniform(-1, 1, S))
            idx = (rng.integers(0, 1 << 30, dc.RINGS) % np.array(lens)).astype(np.int32)
            if trial % 3 == 0:
                idx[rng.integers(0, dc.RINGS)] = [-1, 1 << 20][trial % 2]  # outside its ring: restarts at 0
            state = np.ascontiguousarray(rng.uniform(-1, 1, dc.STATE))
            bad = host.dt_tile_fuzz(rate, 64, N, x.ctypes.data, rings.ctypes.data, idx.ctypes.data, state.ctypes.data)
            assert bad == 0, (rate, N, bad)
        sub += min(lens[:2]) < 128
    assert 8 <= sub < 24  # both paths over the input rings
