"""GPU: mxg_kuramoto_wide_render (kernel K26) against the host build of the same arithmetic (tests/host_kuramoto_wide.cpp over
maximilian_amd/csrc/mxg_kuramoto.h) BIT FOR BIT -- phases, gathered phases, flags, mix and phases_out, in both forms and both
modes -- on the cases of tests/golden/kuramoto_wide.npz, where the exact form is also held to the UNMODIFIED reference within
each case's `tol` (the reference's own distance from a long double restatement; tests/test_kuramoto_wide_host.py holds the host
build to the same bound), and on shapes the file does not hold; against mxg_kuramoto_render bit for bit up to N = 64.

Shapes are the smallest at which the kernel can go wrong: N on both sides of every wavefront count that matters (one, two, three
wavefronts, the last one full, one lane over, one lane short; 1000, 1023 and 1024 for the sixteenth), S = 1 and 3 sets (one
workgroup each), blocks of 1 and 5 samples carried over four calls.  From N = 1000 on the host twin's N * N sines per set and
sample cost 50 ms: there S is 1 and 2 and the blocks are 1 and 3 samples."""
import os
import subprocess

import numpy as np
import pytest

import kuramoto_host as kh
import kuramoto_wide_host as kw
from conftest import ROOT, assert_bits_equal
from test_gpu_kuramoto import MODES, drive, same_run, same_state
from test_kuramoto_wide_host import MEANFIELD_WIDE_BOUND

pytestmark = pytest.mark.gpu

TWOPI = kh.TWOPI
EXTRA = (2, 3, 50, 77, 298)   # further cuts (those beyond a case's length are dropped)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return kw.WideHostBackend(kw.build(tmp_path_factory.mktemp("kuramoto_wide_host")))


@pytest.fixture(scope="module")
def gpu(mx):
    return kw.WideGpuBackend(mx)


@pytest.fixture(scope="module")
def g(golden):
    return golden("kuramoto_wide.npz")


@pytest.fixture(scope="module")
def host_exact():
    """The host build's exact form per golden case, computed once (both golden tests need it)."""
    return {}


def _host_exact(cache, host, c, name, extra):
    if name not in cache:
        cache[name] = kh.play_case(host, c, extra=extra)
    return cache[name]


def _extra(c):
    return tuple(x for x in EXTRA if x < int(c["cuts"][-1]))


@pytest.mark.parametrize("name", kw.CASES)
def test_golden_cases(gpu, host, g, host_exact, name):
    c = kh.case(g, name)
    extra = _extra(c)
    got, exp = kh.play_case(gpu, c, extra=extra), _host_exact(host_exact, host, c, name, extra)
    dev = kh.case_deviation(c, *got)
    print("%-12s gpu: max |difference| from the reference %.3e, tol %.3e" % (name, dev, float(c["tol"])))
    same_run(got, exp, name)
    assert dev <= float(c["tol"])


@pytest.mark.parametrize("name", kw.CASES)
def test_golden_cases_meanfield(gpu, host, g, host_exact, name):
    c = kh.case(g, name)
    extra = _extra(c)
    got, exp = kh.play_case(gpu, c, mode=kh.MEANFIELD, extra=extra), kh.play_case(host, c, mode=kh.MEANFIELD, extra=extra)
    same_run(got, exp, name + " (mean field)")
    exact = _host_exact(host_exact, host, c, name, extra)
    dev = max(float(np.abs(got[0] - exact[0]).max()), float(np.abs(got[1] - exact[1]).max()))
    print("%-12s gpu mean field against the exact form: %.3e (allowed %.3e)" % (name, dev, MEANFIELD_WIDE_BOUND))
    assert dev <= MEANFIELD_WIDE_BOUND


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", [64, 65, 127, 128, 129, 191, 1000, 1023, 1024])
def test_shapes(gpu, host, N, S):
    """test_gpu_kuramoto.py's drive(): four carried blocks, freq per sample in blocks 1 and 3 and K per sample in blocks 2 and 3,
    async flags raised (and a phase written) on every third set before blocks 0 and 2."""
    big = N >= 1000
    if big:
        S = min(S, 2)
    for B in ((1, 3) if big else (1, 5)):
        for mode in MODES:
            seed = 1000 * N + 10 * S + B + mode
            got, exp = drive(gpu, S, N, B, mode, seed), drive(host, S, N, B, mode, seed)
            for k, ((gm, gp, gs), (em, ep, es)) in enumerate(zip(got, exp)):
                what = "S %d N %d B %d mode %d block %d" % (S, N, B, mode, k)
                assert_bits_equal(gm, em, what + ": mix")
                assert_bits_equal(gp, ep, what + ": phases_out")
                same_state(gs, es, what)
            assert len(np.unique(exp[-1][1])) > 1


@pytest.mark.parametrize("S", [1, 17])
@pytest.mark.parametrize("N", [1, 3, 33, 64])
def test_wide_is_narrow_up_to_64(mx, gpu, N, S):
    """mxg_kuramoto_wide_render == mxg_kuramoto_render bit for bit, one set per workgroup against 64 / W sets per wavefront."""
    narrow = kw.WideGpuBackend(mx, entry="mxg_kuramoto_render")
    for B in (1, 7):
        for mode in MODES:
            seed = 77 * N + S + B + mode
            got, exp = drive(gpu, S, N, B, mode, seed), drive(narrow, S, N, B, mode, seed)
            for k, ((gm, gp, gs), (em, ep, es)) in enumerate(zip(got, exp)):
                what = "S %d N %d B %d mode %d block %d" % (S, N, B, mode, k)
                assert_bits_equal(gm, em, what + ": mix")
                assert_bits_equal(gp, ep, what + ": phases_out")
                same_state(gs, es, what)


@pytest.mark.parametrize("mode", MODES)
def test_every_subset_of_want(mx, host, mode):
    """The outputs of a subset are those of the full run and the state moves the same; a block that is not wanted is not written
    (poisoned beforehand, found untouched) and may be NULL.  A sync call does not touch the async arrays."""
    S, N, B = 3, 200, 5
    rng = np.random.default_rng(77 + mode)
    p0, g0 = rng.uniform(0, TWOPI, (S, N)), rng.uniform(0, TWOPI, (S, N))

    def start():
        st = kh.fresh(S, N, p0)
        st["gathered"][...] = g0
        st["update"][:] = [1, 0, 1]
        return st
    ref_st = start()
    ref = host.render(1000, mode, ref_st, B, [3.0, -2.0, 1.0], 12.0)
    for want in range(4):
        for nulls in (True, False):
            st = start()
            o = kw.WideGpuBackend(mx, nulls=nulls).render(1000, mode, st, B, [3.0, -2.0, 1.0], 12.0, want)
            what = "mode %d want %d nulls %s" % (mode, want, nulls)
            assert (o["mix"] is not None) == bool(want & kh.MIX) and (o["phases"] is not None) == bool(want & kh.PHASES)
            if want & kh.MIX:
                assert_bits_equal(o["mix"], ref["mix"], what)
            if want & kh.PHASES:
                assert_bits_equal(o["phases"], ref["phases"], what)
            same_state(st, ref_st, what)


@pytest.mark.parametrize("mode", MODES)
def test_nan_and_stray_phases_in_the_last_wavefront(gpu, host, mode):
    """Three sets of 200 (four wavefronts each); oscillator 199 of set 1 -- in the set's LAST wavefront -- is NaN, or far outside
    [0, 2 pi) (setPhase(1000)).  The first wavefront reads that phase through LDS and must leave the trusted sine with it.
    NaN: the set equals the host build bit for bit (NaN where the host has it), and so do the launch's other sets.  Stray: its
    sines come from the platform's sin() above |x| = 64, within 1 ULP per term but not bit-identical, so that set is held to 1e-12
    (test_gpu_kuramoto.py's bound) and its neighbours to the bits; and oscillator 0 of the set must differ from a run without the
    stray phase -- a kernel that ignored it would pass everything else."""
    S, N, B = 3, 200, 5
    rng = np.random.default_rng(123)
    p0 = rng.uniform(0, TWOPI, (S, N))
    freq = [2.0, -3.0, 4.0]

    def run(be, bad):
        st = kh.fresh(S, N, p0)
        if bad is not None:
            st["phase"][1, N - 1] = bad
        st["update"][:] = 1
        return be.render(1000, mode, st, B, freq, 9.0), st
    clean, _ = run(gpu, None)
    for bad, tol in ((np.nan, None), (1000.0, 1e-12)):
        (og, sg), (oh, sh) = run(gpu, bad), run(host, bad)
        for s in (0, 2):
            assert_bits_equal(og["phases"][:, s], oh["phases"][:, s], "set %d beside %r" % (s, bad))
            assert_bits_equal(og["mix"][:, s], oh["mix"][:, s], "mix of set %d beside %r" % (s, bad))
            assert_bits_equal(og["phases"][:, s], clean["phases"][:, s], "set %d beside %r, against a clean launch" % (s, bad))
        if tol is None:
            assert_bits_equal(og["phases"], oh["phases"], "NaN set")
            assert_bits_equal(og["mix"], oh["mix"], "NaN set, mix")
            same_state(sg, sh, "NaN set, state")
            assert np.isnan(og["phases"][0, 1]).all() and np.isnan(og["mix"][:, 1]).all()
        else:
            assert np.isfinite(og["phases"]).all()
            dev = max(float(np.abs(og["phases"][:, 1] - oh["phases"][:, 1]).max()), float(np.abs(og["mix"][:, 1] - oh["mix"][:, 1]).max()))
            print("mode %d: the set with the stray phase against the host build: %.3e (allowed %.3e)" % (mode, dev, tol))
            assert dev <= tol
            assert og["phases"][0, 1, 0] != clean["phases"][0, 1, 0]


def test_facade_kuramoto_wide_smoke():
    exe = os.path.join(ROOT, "host", "facade_kuramoto_wide_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_kuramoto_wide_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("meanfield,asynchronous", [(False, False), (True, True)])
def test_python_bank_against_host_build(mx, host, meanfield, asynchronous):
    mode = (kh.MEANFIELD if meanfield else 0) | (kh.ASYNC if asynchronous else 0)
    S, N, B = 3, 130, 6
    rng = np.random.default_rng(3)
    p0 = rng.uniform(0, TWOPI, (S, N))
    freq, K = rng.uniform(-30, 30, S), rng.uniform(0, 50, S)
    fblock = rng.uniform(-30, 30, (B, S))
    mx.maxiSettings.setup(1000, 2, 1024)
    try:
        bank = mx.maxiKuramotoWideBank(S, N, meanfield=meanfield, asynchronous=asynchronous)
        assert not bank.phases().any()
        st = kh.fresh(S, N)
        bank.set_phases(p0)
        st["phase"][...] = p0
        st["update"][:] = 1
        assert_bits_equal(bank.play(freq, K, B).numpy(), host.render(1000, mode, st, B, freq, K)["mix"], "play")
        assert_bits_equal(bank.phases(), st["phase"], "phases")
        bank.set_phase([0.25, 5.5], N - 1, sets=[0, 2])
        st["phase"][[0, 2], N - 1] = [0.25, 5.5]
        st["update"][[0, 2]] = 1
        m2, p2 = bank.render_phases(mx.DeviceBuffer.from_numpy(fblock), K)
        exp = host.render(1000, mode, st, B, fblock, K)
        assert_bits_equal(m2.numpy(), exp["mix"], "render_phases: mix")
        assert_bits_equal(p2.numpy(), exp["phases"], "render_phases: phases")
        assert_bits_equal(bank.phases(), st["phase"], "phases after render_phases")
        if asynchronous:
            assert_bits_equal(bank.gathered.numpy(), st["gathered"], "gathered")
            assert not bank.update.numpy().any()
    finally:
        mx.maxiSettings.setup(44100, 2, 1024)
