"""CPU (-m "not gpu"): mxg_reverb.h -- the arithmetic and the topology reverb.hip runs -- compiled for the host.
It reproduces every case of tests/golden/reverb.npz (the unmodified reference, tools/gen/gen_golden_reverb.py) bit for bit:
outputs, ring contents, indices, low-pass states and (w, cut).  The tile machinery of the kernel that is plain arithmetic (slots
of a tile, the wrap, sub-tiles over a ring shorter than the tile, the index advance) is fuzzed against the step-by-step
recurrence over random ring lengths including D < T, D = T and D = 1, start indices, block lengths and steps per sample."""
import ctypes

import numpy as np
import pytest

import reverb_cases as rc
import reverb_host as rh
from conftest import assert_bits_equal


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return rh.build(tmp_path_factory.mktemp("reverb"))


@pytest.fixture(scope="module")
def g():
    return rh.load_golden()


def test_topology_tables(host):
    for kind in (rc.SAT, rc.FREEVERB, rc.STEREO):
        lens, offs, S = rc.layout(kind)
        la, oa = np.zeros(len(lens), np.int32), np.zeros(len(lens), np.int32)
        assert host.rv_layout(kind, la.ctypes.data, oa.ctypes.data) == S == rc.RING_DOUBLES[kind]
        assert la.tolist() == lens and oa.tolist() == offs


def test_golden_file_is_what_the_issue_asks(g):
    assert sorted(g["cases"].tolist()) == sorted(c["name"] for c in rc.CASES)
    tiny = np.finfo(np.float64).tiny
    for case in rc.CASES:
        y = g[case["name"] + "/out"]
        assert y.shape == (rc.CHANNELS[case["kind"]], case["N"], case["V"])
        assert case["N"] >= 6000 and case["N"] > 3 * max(rc.LENGTHS[case["kind"]])
        assert (y[:, case["noise"] + 100:] != 0).any()  # the tail after the input went silent
        if case.get("subnormal"):
            a = np.abs(y)
            assert ((a > 0) & (a < tiny)).sum() >= 100
    assert "reference sources" in str(g["provenance"])


@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_host_build_reproduces_golden(host, g, case):
    st = rh.State(case["kind"], case["V"])
    exp = g[case["name"] + "/out"]
    got = np.zeros_like(exp)
    for a, b, m, x, room, absorb, ps in rh.case_blocks(case, g):
        o = rh.host_render(host, st, m, x, room, absorb, ps)
        got[:, a:b] = o if case["kind"] == rc.STEREO else o[None]
    assert_bits_equal(got, exp, case["name"] + ": output")
    rh.check_case_state(case, g, st, case["name"])


def test_block_boundaries_do_not_matter(host, g):
    """One block or many: the state carries everything (fv_ps cut at odd places against the golden output)."""
    case = [c for c in rc.CASES if c["name"] == "fv_ps"][0]
    x, mode, room, absorb = rc.inputs(case)
    st = rh.State(case["kind"], case["V"])
    got, n = [], 0
    for ln in [1, 63, 64, 65, 512, 4096, 10 ** 6]:
        s = slice(n, min(n + ln, case["N"]))
        got.append(rh.host_render(host, st, 1, np.ascontiguousarray(x[s]), np.ascontiguousarray(room[s]),
                                  np.ascontiguousarray(absorb[s]), 3))
        n = s.stop
    assert_bits_equal(np.concatenate(got)[None], g["fv_ps/out"], "fv_ps in uneven blocks")
    rh.check_case_state(case, g, st, "fv_ps in uneven blocks")


def test_tile_machinery_matches_recurrence(host):
    rng = np.random.default_rng(5)
    short = 0
    for trial in range(600):
        T = int(rng.choice([8, 64]))
        steps = int(rng.choice([1, 1, 2]))
        D = int(rng.choice([1, 2, 3, 12, 42, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 125, 225, 1617]))
        D = max(D, steps)
        N = int(rng.integers(1, 5 * T + 3 * D if D < 300 else 4000))
        idx0 = int(rng.choice([0, 0, D - 1, D // 2, D, D + 5, -1]))
        x = np.ascontiguousarray(rng.uniform(-1, 1, (steps, N)))
        bad = host.rv_tile_fuzz(T, D, steps, idx0, N, x.ctypes.data)
        assert bad == 0, (trial, T, D, steps, idx0, N)
        short += D < steps * T
    assert short > 100  # rings shorter than a tile were exercised
    # the rings of the three classes, as the kernel steps them
    for kind in (rc.SAT, rc.FREEVERB, rc.STEREO):
        steps = 2 if kind == rc.STEREO else 1
        for D in rc.LENGTHS[kind][rc.NCOMB[kind]:]:
            x = np.ascontiguousarray(rng.uniform(-1, 1, (steps, 3 * D + 70)))
            assert host.rv_tile_fuzz(64, D, steps, int(rng.integers(0, D)), x.shape[1], x.ctypes.data) == 0, (kind, D)
