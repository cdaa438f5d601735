"""CPU (-m "not gpu"): the host build of mxg_kuramoto.h for sets of up to 1024 oscillators (tests/host_kuramoto_wide.cpp, the
arithmetic of kernel K26) against the narrow host build (tests/host_kuramoto.cpp, K17's) bit for bit where both apply, and
against the UNMODIFIED reference (tests/golden/kuramoto_wide.npz, tools/gen/gen_golden_kuramoto_wide.py) on sets of 65 .. 1024.

Bounds.  As in test_kuramoto_host.py the only yardstick of the exact form is the reference's own accumulated rounding:
"<case>/tol" is the reference's largest distance from a long double restatement of the same recurrence (6.7e-15 .. 5.1e-13 in this
file), and the host build must stay within 1 x tol of the file on the mix at every sample and the phases at every cut.  Measured
here: the host build differs from the file by 0 .. 5.3e-15 (at most 0.27 x tol; 2 of 8 cases are the reference's bits).

The mean-field form rounds differently on every term and shares no summation order with the exact form.  Measured over the wide
cases (host exact against host mean field, phases and mix at every sample): at most MEANFIELD_WIDE_MEASURED (case sync1024).  The
bound is 8 x that -- the margin rule MEANFIELD_BOUND was set with for N <= 64 -- and never above 1e-10."""
import os
import subprocess

import numpy as np
import pytest

import kuramoto_host as kh
import kuramoto_wide_host as kw
from conftest import ROOT, assert_bits_equal

MEANFIELD_WIDE_MEASURED = 1.10e-13   # host exact vs host mean field over the wide golden cases, see the docstring
MEANFIELD_WIDE_BOUND = min(8 * MEANFIELD_WIDE_MEASURED, 1e-10)
TWOPI = kh.TWOPI
MODES = [0, kh.MEANFIELD, kh.ASYNC, kh.ASYNC | kh.MEANFIELD]


@pytest.fixture(scope="module")
def W(tmp_path_factory):
    return kw.WideHostBackend(kw.build(tmp_path_factory.mktemp("kuramoto_wide_host")))


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return kh.HostBackend(kh.build(tmp_path_factory.mktemp("kuramoto_host")))


@pytest.fixture(scope="module")
def g(golden):
    return golden("kuramoto_wide.npz")


@pytest.fixture(scope="module")
def exact(W, g):
    """The wide host build's exact form on every golden case, computed once."""
    return {name: kh.play_case(W, kh.case(g, name)) for name in g["cases"]}


def spread(p):
    s = np.sort(np.asarray(p) % TWOPI)
    gaps = np.diff(np.concatenate([s, [s[0] + TWOPI]]))
    return float(TWOPI - gaps.max())


def test_golden_file_is_not_trivial(g):
    """What the generator asserted, re-asserted from the file."""
    assert list(g["cases"]) == kw.CASES
    assert [int(g[n + "/N"]) for n in kw.CASES] == [65, 128, 129, 1000, 1024, 1024, 200, 200]
    for n in kw.CASES:
        c = kh.case(g, n)
        N, tol, ns = int(c["N"]), float(c["tol"]), int(c["cuts"][-1])
        assert 0 < tol <= 1e-10, (n, tol)
        assert ns == (96 if N >= 1000 else 300) and c["mix"].shape == (ns,) and np.isfinite(c["mix"]).all()
        assert int(c["sr"]) == 1000
        lens = np.diff(c["cuts"])
        assert 1 in lens and 7 in lens
        assert float(c["margin"]) > 1000 * tol, n
        assert min(c["snap_phase"].min(), (TWOPI - c["snap_phase"]).min()) > 1000 * tol, n
        assert int(c["wraps"]) >= 3, n
        assert ("phases" in c) == (n == "n65")
    s = g["n65/phases"]   # the one whole stream: the margin and the wraps from the data themselves
    assert min(s.min(), (TWOPI - s).min()) > 1000 * float(g["n65/tol"])
    assert (np.abs(np.diff(s, axis=0)) > np.pi).sum(axis=0).min() >= 3
    assert float(g["desync1024/K"]) < 0 and spread(g["desync1024/snap_phase"][-1]) > 1
    assert float(g["sync1024/K"]) > 0 and spread(g["sync1024/snap_phase"][-1]) < 1e-6
    assert g["ps1000/K_q"].min() < 0 < g["ps1000/K_q"].max() and len(np.unique(g["ps1000/freq_q"])) > 30
    ev = g["async_raise/events"]
    assert len(set(ev[:, 0])) == 2 and int(ev[:, 1].max()) >= 192   # told at two cuts; once in the set's last wavefront
    assert int(g["async_raise/raise0"]) == 1 and int(g["async_raise/async"]) == 1
    assert g["async_never/events"].shape[0] == 0 and int(g["async_never/raise0"]) == 0 and int(g["async_never/async"]) == 1
    assert not g["async_never/snap_gathered"].any() and not g["async_never/snap_update"].any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kuramoto_wide.npz")) < os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "kuramoto.npz"))


@pytest.mark.parametrize("mode", MODES)
def test_wide_host_is_the_narrow_host_up_to_64(W, H, mode):
    """N = 1 .. 64: kura_wide_host_render == kura_host_render bit for bit -- mix, phases_out and state over three carried blocks with
    freq and K per set and per sample, flags raised on a subset of the sets."""
    for N in range(1, 65):
        S = 3
        rng = np.random.default_rng(100 * N + mode)
        p0, g0 = rng.uniform(0, TWOPI, (S, N)), rng.uniform(0, TWOPI, (S, N))
        sts = []
        for be in (W, H):
            st = kh.fresh(S, N, p0)
            st["gathered"][...] = g0
            st["update"][:] = [1, 0, 0]
            sts.append(st)
        r = np.random.default_rng(7 * N + mode)
        for k, B in enumerate((1, 5, 9)):
            f = r.uniform(-40, 40, (B, S) if k & 1 else (S,))
            K = r.uniform(-10, 60, (B, S) if k & 2 else (S,))
            if k == 2:
                for st in sts:
                    st["update"][2] = 1
                    st["phase"][2, N // 2] = 1.5
            ow, oh = W.render(1000, mode, sts[0], B, f, K), H.render(1000, mode, sts[1], B, f, K)
            what = "N %d mode %d block %d" % (N, mode, k)
            assert_bits_equal(ow["mix"], oh["mix"], what + ": mix")
            assert_bits_equal(ow["phases"], oh["phases"], what + ": phases_out")
            for key in ("phase", "gathered"):
                assert_bits_equal(sts[0][key], sts[1][key], what + ": " + key)
            assert np.array_equal(sts[0]["update"], sts[1]["update"]), what


def test_wide_host_refuses_what_the_entry_point_refuses(W):
    for N in (0, 1025):
        one = np.zeros(max(N, 1))
        assert W.L.kura_wide_host_render(1000.0, 0, 1, N, 1, one.ctypes.data, 0, one.ctypes.data, 0, one.ctypes.data, None, None, 0, None,
                                         None) != 0


def test_host_build_against_golden(g, exact):
    worst = 0.0
    for name in g["cases"]:
        c = kh.case(g, name)
        dev = kh.case_deviation(c, *exact[name])
        print("%-12s wide host build: max |difference| %.3e, tol %.3e (%.2f x)" % (name, dev, float(c["tol"]), dev / float(c["tol"])))
        worst = max(worst, dev / float(c["tol"]))
        assert dev <= float(c["tol"]), name
    print("largest: %.2f x tol" % worst)


def test_blocks_do_not_matter(W, g, exact):
    """The same case cut at other positions gives the same bits: nothing but the state arrays crosses a call."""
    for name in ("n129", "async_raise"):
        mix, ph, _ = kh.play_case(W, kh.case(g, name), extra=(2, 3, 77, 298))
        assert_bits_equal(mix, exact[name][0], name + ": mix")
        assert_bits_equal(ph, exact[name][1], name + ": phases")


def test_meanfield_against_exact(W, g, exact):
    worst = 0.0
    for name in g["cases"]:
        mix, ph, _ = kh.play_case(W, kh.case(g, name), mode=kh.MEANFIELD)
        dev = max(float(np.abs(mix - exact[name][0]).max()), float(np.abs(ph - exact[name][1]).max()))
        print("%-12s mean field against exact: %.3e" % (name, dev))
        worst = max(worst, dev)
    print("largest: %.3e (allowed %.3e)" % (worst, MEANFIELD_WIDE_BOUND))
    assert worst <= MEANFIELD_WIDE_BOUND, worst
    assert worst > 0   # it is another computation, not the same one under another name


@pytest.mark.parametrize("mode", MODES)
def test_nan_or_stray_phase_in_the_last_wavefront(W, mode):
    """A set of 200 whose oscillator 199 is NaN: with the flag up (or a sync set) every oscillator of the set is NaN after the next
    sample, and so is the mix; the neighbouring set is untouched.  A stray phase there (setPhase(1000)) moves oscillator 0."""
    N = 200
    p0 = np.random.default_rng(3).uniform(0, TWOPI, (2, N))
    st = kh.fresh(2, N, p0)
    st["phase"][0, N - 1] = np.nan
    st["update"][:] = 1
    o = W.render(1000, mode, st, 2, 2.0, 7.0)
    assert np.isnan(o["phases"][0, 0]).all() and np.isnan(o["mix"][:, 0]).all()
    assert np.isfinite(o["phases"][:, 1]).all() and np.isfinite(o["mix"][:, 1]).all()
    a, b = kh.fresh(1, N, p0[0]), kh.fresh(1, N, p0[0])
    b["phase"][0, N - 1] = 1000.0
    a["update"][:] = b["update"][:] = 1
    oa, ob = W.render(1000, mode, a, 1, 2.0, 7.0), W.render(1000, mode, b, 1, 2.0, 7.0)
    assert np.isfinite(ob["phases"]).all() and oa["phases"][0, 0, 0] != ob["phases"][0, 0, 0]


def test_standalone_program_under_sanitizers(tmp_path):
    """tests/host_kuramoto_wide.cpp with its own main under AddressSanitizer + UndefinedBehaviorSanitizer, run once as its own
    process."""
    exe = str(tmp_path / "host_kuramoto_wide_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DKURA_WIDE_HOST_MAIN", kw.INC, "-o", exe, kw.SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_kuramoto_wide: ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
