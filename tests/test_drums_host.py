"""CPU (-m "not gpu"): mxg_drums.h -- the arithmetic drums.hip's kernels run -- on the host, twice: compiled with g++ under the
oracle's FPFLAGS (tests/host_drums.cpp) and through the library's mxg_drum_host / mxg_clock_host, against tests/golden/drums.npz
under the numerics contract (tests/drums_host.py check_case): snare, hats, the clock and every state row BIT FOR BIT, the kick's
output under its derived bound -- with the blocks cut as stored and at 1, 2, 7, 8, 9, 64, 65, 333, 1199.  Also the numpy model
against the same file, a seeded fuzz of each drum's step, host build against the model, on full-mantissa parameters and states,
and the two denormal cases (a flush to zero would show in both).  (tests/host_drums.cpp built as a program is the stand-alone run
under -fsanitize=address,undefined.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import drums_host as dh
from conftest import ROOT

EXTRA = (1, 2, 7, 8, 9, 64, 65, 333, 1199)


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


class GxxBackend(dh.HostBackend):
    name = "g++"

    def __init__(self, tmpdir):
        super().__init__()
        so = os.path.join(str(tmpdir), "libdrums_host.so")
        subprocess.check_call(["g++", "-std=c++17"] + fpflags() + ["-w", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                               "-o", so, os.path.join(ROOT, "tests", "host_drums.cpp")])
        self.so = ctypes.CDLL(so)
        S, I, D, P = ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_void_p
        self.so.dr_host_render.argtypes = [I, I, S, S, P, I] + [P] * 7 + [D] + [P] * 5
        self.so.dr_host_clock.argtypes = [S, S, P, D] + [P] * 5
        self.fn = lambda *a: self.so.dr_host_render(*a[:13], float(self.L.mxg_sample_rate()), *a[13:])

    def clock(self, bps, clk, last, playhead, n):
        V = len(bps)
        bps, clk = np.ascontiguousarray(bps, np.float64), np.ascontiguousarray(clk, np.float64).copy()
        last = None if last is None else np.ascontiguousarray(last, np.int32)
        ph, cnt, tick = np.ascontiguousarray(playhead, np.int64).copy(), np.zeros(V, np.int32), np.zeros((n, V))
        assert self.so.dr_host_clock(V, n, bps.ctypes.data, float(self.L.mxg_sample_rate()), clk.ctypes.data,
                                     None if last is None else last.ctypes.data, ph.ctypes.data, cnt.ctypes.data, tick.ctypes.data) == 0
        return tick, clk, ph, cnt


@pytest.fixture(scope="module")
def backends(tmp_path_factory):
    return {"g++": GxxBackend(tmp_path_factory.mktemp("drums")), "lib": dh.HostBackend()}


@pytest.fixture(scope="module")
def g(golden):
    return golden("drums.npz")


@pytest.mark.parametrize("which", ["g++", "lib"])
@pytest.mark.parametrize("extra", [(), EXTRA])
@pytest.mark.parametrize("tpv", [0, 1])
def test_host_build_against_golden(backends, g, which, extra, tpv):
    be, worst = backends[which], {}
    for sr in dh.RATES:
        with dh.at_rate(be.L, sr):
            for kind in dh.KINDS:
                for variant in dh.VARIANTS:
                    out, states = dh.play_case(be, g, kind, variant, sr, cuts=extra, tpv=tpv)
                    r = dh.check_case(be.L, g, kind, variant, sr, out, states, which)
                    if r:
                        worst[dh.key(kind, variant, sr)] = r
    print("kick, measured (worst error, bound there, samples within the bound of +-1):", worst)


def test_the_two_host_builds_agree_bit_for_bit(backends, g):
    """g++ and the library's host pass run the same text: the same bits, the kick's sine included."""
    for sr in dh.RATES:
        with dh.at_rate(backends["lib"].L, sr):
            for kind in dh.KINDS:
                for variant in dh.VARIANTS:
                    a, sa = dh.play_case(backends["g++"], g, kind, variant, sr)
                    b, sb = dh.play_case(backends["lib"], g, kind, variant, sr)
                    dh.bits_equal(a, b, dh.key(kind, variant, sr))
                    dh.bits_equal(dh.state_rows(sa[dh.N]), dh.state_rows(sb[dh.N]), dh.key(kind, variant, sr) + " state")


def test_model_against_golden(backends, g):
    class Model:
        L = backends["lib"].L

        def __init__(self, sr):
            self.sr = sr

        def render(self, p, trig, rnd, state, n=None, tpv=None):
            return dh.model_render(p, trig, rnd, state, self.sr)

    for sr in dh.RATES:
        with dh.at_rate(Model.L, sr):
            for kind in ("snare", "hats"):
                for variant in dh.VARIANTS:
                    out, states = dh.play_case(Model(sr), g, kind, variant, sr)
                    dh.check_case(Model.L, g, kind, variant, sr, out, states, "model")


def test_golden_is_not_trivial(g):
    """What the generator asserted, seen from here."""
    assert g["cuts"].tolist() == list(dh.CUTS) and g["trig_at"].tolist() == list(dh.TRIG_AT)
    assert len(np.unique(g["draws"])) == dh.N
    for sr in dh.RATES:
        for kind in dh.KINDS:
            o = dh.ref_out(g, kind, "full", sr)
            assert (np.abs(o) == 1.0).sum() >= 30 and len(np.unique(o)) > 200 and np.isfinite(o).all()
            assert (dh.ref_out(g, kind, "plain", sr)[:3] == 0).all()
            assert g["envpar/" + dh.key(kind, "plain", sr)][0] == 1.0
        assert g["clock/%d/0/tick" % sr].sum() >= 14
    assert g["clock/44100/0/tick"].sum() == 16 and int(np.argmax(g["clock/44100/0/tick"])) == 74


def test_env_coefficients_are_the_references(backends, g):
    L = backends["lib"].L
    for sr in dh.RATES:
        with dh.at_rate(L, sr):
            for kind in dh.KINDS:
                for variant in dh.VARIANTS:
                    p = dh.Params.of_case(L, kind, variant)
                    dh.bits_equal(p.par[:, 0], g["envpar/" + dh.key(kind, variant, sr)][:4], dh.key(kind, variant, sr))


@pytest.mark.parametrize("which", ["g++", "lib"])
@pytest.mark.parametrize("kind", dh.KINDS)
def test_fuzz_step_against_the_model(backends, which, kind):
    """Random parameters, states and draws with full mantissas, every combination of the four switches, four samples with random
    triggers: the host build and the numpy model give the same bits for the output (snare, hats) and for every state row (all
    three; the kick's filter state only with the filter off, its output never: numpy's sine is another sine)."""
    be = backends[which]
    rng = np.random.default_rng(2121 + dh.KIND[kind])
    Vf, Nf = 4000, 4
    for flags in range(16):
        sr = int(rng.choice(dh.RATES))
        with dh.at_rate(be.L, sr):
            p = dh.Params.of_case(be.L, kind, "plain", Vf)
            p.flags = flags
            p.pitch = rng.uniform(20.0, 15000.0, Vf)
            p.par = np.array([rng.choice([1.0, 0.37, 0.011], Vf) * rng.uniform(0.5, 1.0, Vf), rng.uniform(0.5, 1.0, Vf), rng.uniform(0.0, 0.9, Vf),
                              rng.uniform(0.3, 1.0, Vf)])
            p.par[0, ::5] = 1.0
            p.holdtime = rng.integers(0, 4, Vf).astype(np.int64)
            p.shape = rng.uniform(0.1, 5.0, Vf)
            p.gain = rng.uniform(0.2, 3.0, Vf)
            p.coef = rng.uniform(0.01, 0.9, p.coef.shape)
            st = dh.fresh_state(Vf)
            st[0] = rng.uniform(0.0, 1.0, Vf) if kind != "hats" else rng.uniform(0.0, 510.0, Vf)
            stage = rng.integers(0, 5, Vf)   # rest, attack, decay, hold, release
            st[1][0] = np.where(stage == 0, 0.0, rng.uniform(0.0, 1.0, Vf))
            st[1][1] = rng.uniform(0.0, 1.0, Vf)
            st[2][0] = np.where(stage == 4, p.holdtime, 0)
            for r, s in ((1, 1), (2, 2), (4, 3), (5, 4)):
                st[2][r] = (stage == s).astype(np.int64)
            st[3] = rng.uniform(-1.0, 1.0, (3, Vf))
            trig = (rng.uniform(0, 1, (Nf, Vf)) < 0.3).astype(np.float64)
            rnd = None if kind == "kick" else rng.integers(0, 2 ** 31 - 1, (Nf, Vf)).astype(np.int32)
            got, sg = be.render(p, trig, rnd, st)
            exp, se = dh.model_render(p, trig, rnd, st, sr)
            what = "%s flags %d" % (kind, flags)
            if kind != "kick":
                dh.bits_equal(got, exp, what)
            dh.bits_equal(sg[0], se[0], what + " phase")
            dh.bits_equal(sg[1], se[1], what + " envelope")
            assert np.array_equal(sg[2], se[2]), what + " envelope flags"
            if kind != "kick" or not flags & dh.FILTER:
                dh.bits_equal(sg[3], se[3], what + " filter state")
            assert len(np.unique(got)) > Vf // 2


@pytest.mark.parametrize("which", ["g++", "lib"])
def test_denormal_amplitudes_survive(backends, which):
    """An uploaded envelope amplitude of 3 * 2^-1074 in release: with a release coefficient near 0.97 it stays exactly 3 * 2^-1074 for
    ever (3 * 0.97 rounds back to 3 steps), with 0.3 it goes 3 -> 1 -> 0 steps.  A flush to zero would show in both."""
    be = backends[which]
    dh.denormal_cases(be)


@pytest.mark.parametrize("which", ["g++", "lib"])
def test_clock_against_golden(backends, g, which):
    be = backends[which]
    for sr in dh.RATES:
        with dh.at_rate(be.L, sr):
            for last in (0, 1):
                for cuts in ((0, dh.N), (0,) + EXTRA + (dh.N,)):
                    clk, ph, ticks = np.zeros(1), np.zeros(1, np.int64), []
                    for a, b in zip(cuts[:-1], cuts[1:]):
                        t, clk, ph, cnt = be.clock([600.0], clk, [last], ph, b - a)
                        ticks.append(t)
                        dh.bits_equal(clk, g["clock/%d/%d/phase" % (sr, last)][b - 1:b], "clock phase at %d" % b)
                    dh.check_clock(g, sr, last, np.concatenate(ticks), ph[0], cnt[0])
