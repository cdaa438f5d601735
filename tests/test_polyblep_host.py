"""CPU (-m "not gpu"): mxg_polyblep.h -- the arithmetic polyblep.hip's kernel runs -- on the host, twice: compiled with g++ under
the oracle's FPFLAGS (tests/host_polyblep.cpp) and through the library's mxg_polyblep_host, against tests/golden/polyblep.npz
under the contract of DESIGN.md section 4 (tests/polyblep_host.py check_contract): the phase and the ten exact waveforms BIT FOR
BIT, SINE / COSINE and every fallback sample within 1 ULP, the two rectified sines within 2^-50 absolute -- with the blocks
cut as stored and at further uneven positions.  Also the numpy model against the same file, and a seeded fuzz of the phase
recurrence and of each exact waveform, host build against the step-by-step model, on t, dt and pw with full mantissas and dt
up to 0.25.  (tests/host_polyblep.cpp built as a program is the stand-alone run under -fsanitize=address,undefined.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import polyblep_host as ph
from conftest import ROOT, assert_bits_equal

EXTRA = (2, 64, 65, 199, 333, 602, 777, 1001, 1199)


def fpflags():
    txt = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*=\s*(.*)$", txt, re.M).group(1).split()


class GxxBackend(ph.HostBackend):
    name = "g++"

    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libpolyblep_host.so")
        subprocess.check_call(["g++", "-std=c++17"] + fpflags() + ["-w", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"),
                               "-o", so, os.path.join(ROOT, "tests", "host_polyblep.cpp")])
        self.so = ctypes.CDLL(so)
        S, I, D, P = ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_void_p
        self.so.pb_host_render.argtypes = [I, S, S, P, I, P, D, P, P]
        self.so.pb_host_sync.restype, self.so.pb_host_sync.argtypes = D, [D]

    def render(self, wf, freq, pw, sr, t, n=None):
        freq = np.ascontiguousarray(freq, np.float64)
        fps = freq.ndim == 2
        n = freq.shape[0] if fps else n
        out, t = np.zeros((n, t.shape[0])), np.ascontiguousarray(t, np.float64).copy()
        pwa = None if pw is None else np.ascontiguousarray(pw, np.float64)
        assert self.so.pb_host_render(ph.WF[wf], t.shape[0], n, freq.ctypes.data, int(fps), None if pwa is None else pwa.ctypes.data,
                                      float(sr), t.ctypes.data, out.ctypes.data) == 0
        return out, t


@pytest.fixture(scope="module")
def backends(tmp_path_factory):
    return {"g++": GxxBackend(tmp_path_factory.mktemp("polyblep")), "lib": ph.HostBackend()}


@pytest.fixture(scope="module")
def g(golden):
    return golden("polyblep.npz")


@pytest.mark.parametrize("which", ["g++", "lib"])
@pytest.mark.parametrize("extra", [(), EXTRA])
def test_host_build_against_golden(backends, g, which, extra):
    worst = {}
    for wf in ph.WAVEFORMS:
        out, phases = ph.play_case(backends[which], g, wf, cuts=extra, fps=bool(extra))
        worst[wf] = ph.check_contract(g, wf, out, phases, which)
    print({wf: r for wf, r in worst.items() if wf not in ph.EXACT})
    assert all(worst[wf]["ulp"] <= 1 for wf in ph.WAVEFORMS)


def test_the_two_host_builds_agree_bit_for_bit(backends, g):
    """g++ and the library's host pass run the same text with every product that may fuse spelled as an fma(): the same bits,
    the sine waveforms included."""
    for wf in ph.WAVEFORMS:
        a, pa = ph.play_case(backends["g++"], g, wf)
        b, pb = ph.play_case(backends["lib"], g, wf)
        assert_bits_equal(a, b, wf)
        assert_bits_equal(pa, pb, wf + " phase")


def test_model_against_golden(g):
    m = ph.ModelBackend()
    fb = ph.fallback(ph.freqs(g))
    for wf in ph.EXACT:
        out, phases = ph.play_case(m, g, wf)
        assert_bits_equal(phases, g["t/" + wf], wf + " phase")
        assert_bits_equal(out[~fb], ph.ref_out(g, wf)[~fb], wf)


def test_golden_is_not_trivial(g):
    """What the generator asserted, seen from here: no constant column or row, the fallback on and off, a negative phase."""
    fb = ph.fallback(ph.freqs(g))
    assert fb[:, 2].any() and not fb[:, 2].all() and not fb[:, [0, 1, 3, 4, 5]].any()
    assert g["enum/values"].tolist() == list(range(14))
    for wf in ph.WAVEFORMS:
        o = ph.ref_out(g, wf)
        assert all(len(np.unique(o[:, v])) > 3 for v in range(ph.V)) and all(len(np.unique(o[n])) > 1 for n in range(1, ph.N)), wf
        assert (g["t/" + wf][1:, 1] < 0).all()


def test_sync_wraps_like_the_reference(backends, g):
    so = backends["g++"].so
    for p, want in ((2.75, 0.75), (-0.25, 0.75), (-3.0, 1.0), (0.0, 0.0), (0.5, 0.5), (-0.0, 0.0)):
        assert so.pb_host_sync(p) == want and float(ph.sync_wrap(p)) == want
    import maximilian_amd as m
    assert m.polyblep_sync([2.75, -0.25, -3.0]).tolist() == [0.75, 0.75, 1.0]


@pytest.mark.parametrize("which", ["g++", "lib"])
def test_fuzz_phase_and_exact_waveforms_against_the_model(backends, which):
    """Random t in (-1, 1), dt in (-0.25, 0.25) and pw in [-0.1, 1.1] with full mantissas, three samples each: the host build
    and the step-by-step model give the same bits for the phase and for every exact waveform.  The frequency is dt * sr rounded,
    so the dt both sides form is freq / sr; sr is drawn per run."""
    rng = np.random.default_rng(2020)
    Vf, Nf = 20000, 3
    m = ph.ModelBackend()
    for wf in ph.EXACT:
        sr = float(rng.choice([1000.0, 44100.0, 48000.0, 96000.0, 22050.5]))
        t0 = rng.uniform(-1.0, 1.0, Vf)
        t0[:2000] = rng.uniform(0.0, 1.0, 2000) * 2.0 ** -rng.integers(0, 40, 2000)   # phases next to 0
        t0[2000:4000] = 1.0 - rng.uniform(0.0, 1.0, 2000) * 2.0 ** -rng.integers(1, 40, 2000)   # and next to 1
        dt = rng.uniform(-0.25, 0.25, (Nf, Vf))
        dt[:, ::7] = rng.uniform(0.0, 0.25, (Nf, len(range(0, Vf, 7)))) * 2.0 ** -rng.integers(0, 30, (Nf, len(range(0, Vf, 7))))
        freq = dt * sr
        freq = np.where(ph.fallback(freq, sr), 0.2 * sr, freq)   # (stay below the fallback: the exact arithmetic is the subject)
        pw = rng.uniform(-0.1, 1.1, Vf)
        pw[::11] = rng.choice([0.0, 0.0001, 0.9999, 1.0, 0.5], len(range(0, Vf, 11)))
        got, tg = backends[which].render(wf, freq, pw, sr, t0)
        exp, te = m.render(wf, freq, pw, sr, t0)
        assert not np.isnan(exp).all(axis=0).any()
        assert_bits_equal(tg, te, wf + " phase")
        assert_bits_equal(got, exp, wf)
        assert len(np.unique(got)) > Vf
