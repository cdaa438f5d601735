"""GPU: mxg_kuramoto_render (kernel K17) against the host build of the same arithmetic (tests/host_kuramoto.cpp over
maximilian_amd/csrc/mxg_kuramoto.h) BIT FOR BIT -- phases, gathered phases, flags, mix and phases_out, in both forms and both
modes -- and, on the cases of tests/golden/kuramoto.npz, against the UNMODIFIED reference within each case's `tol` (the
reference's own distance from a long double restatement; tests/test_kuramoto_host.py holds the host build to the same bound).

Shapes are the smallest at which the kernel can go wrong: S = 1, 3, 17 sets (with N = 3 a set takes 4 lanes, so 17 sets leave the
second wavefront with one live segment and fifteen shadows), N on both sides of every segment width, blocks of 1, 7 and 64 samples
carried over four calls, freq and K per set and per sample in all four combinations."""
import numpy as np
import pytest

import kuramoto_host as kh
from conftest import assert_bits_equal
from test_kuramoto_host import MEANFIELD_BOUND

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 5, 31, 32, 33, 63, 64]
MODES = [0, kh.MEANFIELD, kh.ASYNC, kh.ASYNC | kh.MEANFIELD]
TWOPI = kh.TWOPI


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return kh.HostBackend(kh.build(tmp_path_factory.mktemp("kuramoto_host")))


@pytest.fixture(scope="module")
def gpu(mx):
    return kh.GpuBackend(mx)


@pytest.fixture(scope="module")
def g(golden):
    return golden("kuramoto.npz")


def same_run(a, b, what):
    (ma, pa, sa), (mb, pb, sb) = a, b
    assert_bits_equal(ma, mb, what + ": mix")
    assert_bits_equal(pa, pb, what + ": phases_out")
    assert sorted(sa) == sorted(sb)
    for cut in sa:
        same_state(sa[cut], sb[cut], "%s: state at cut %d" % (what, cut))


def same_state(a, b, what):
    assert_bits_equal(a["phase"], b["phase"], what + ", phase")
    assert_bits_equal(a["gathered"], b["gathered"], what + ", gathered")
    assert np.array_equal(a["update"], b["update"]), what + ", update"


@pytest.mark.parametrize("name", ["n1", "n2", "n3", "n5", "n31", "n32", "n33", "n63", "n64", "ps", "setp", "async_raise", "async_never",
                                  "kt"])
def test_golden_cases(gpu, host, g, name):
    c = kh.case(g, name)
    got, exp = kh.play_case(gpu, c), kh.play_case(host, c)
    dev = kh.case_deviation(c, *got)
    print("%-12s gpu: max |difference| from the reference %.3e, tol %.3e" % (name, dev, float(c["tol"])))
    same_run(got, exp, name)
    assert dev <= float(c["tol"])


@pytest.mark.parametrize("name", ["n3", "n33", "n64", "ps", "async_raise"])
def test_golden_cases_meanfield(gpu, host, g, name):
    c = kh.case(g, name)
    got, exp = kh.play_case(gpu, c, mode=kh.MEANFIELD), kh.play_case(host, c, mode=kh.MEANFIELD)
    same_run(got, exp, name + " (mean field)")
    exact = kh.play_case(host, c)
    dev = max(float(np.abs(got[0] - exact[0]).max()), float(np.abs(got[1] - exact[1]).max()))
    print("%-12s gpu mean field against the exact form: %.3e (allowed %.3e)" % (name, dev, MEANFIELD_BOUND))
    assert dev <= MEANFIELD_BOUND


def drive(be, S, N, B, mode, seed):
    """Four carried blocks of B samples; block k has freq per sample when k & 1 and K per sample when k & 2.  Async sets get a
    flag raised before blocks 0 and 2 on every third set (and a phase written, as setPhase does)."""
    rng = np.random.default_rng(seed)
    st = kh.fresh(S, N, rng.uniform(0, TWOPI, (S, N)))
    st["gathered"][...] = rng.uniform(0, TWOPI, (S, N))
    outs = []
    for k in range(4):
        f = rng.uniform(-40, 40, (B, S) if k & 1 else (S,))
        K = rng.uniform(-10, 60, (B, S) if k & 2 else (S,))
        if mode & kh.ASYNC and k in (0, 2):
            st["update"][k // 2::3] = 1
            st["phase"][k // 2::3, N // 2] = rng.uniform(0, TWOPI)
        o = be.render(1000, mode, st, B, f, K)
        outs.append((o["mix"].copy(), o["phases"].copy(), {key: v.copy() for key, v in st.items()}))
    return outs


@pytest.mark.parametrize("N", NS)
def test_shapes(gpu, host, N):
    for S in (1, 3, 17):
        for B in (1, 7, 64):
            for mode in MODES:
                seed = 1000 * N + 10 * S + B + mode
                got, exp = drive(gpu, S, N, B, mode, seed), drive(host, S, N, B, mode, seed)
                for k, ((gm, gp, gs), (em, ep, es)) in enumerate(zip(got, exp)):
                    what = "S %d N %d B %d mode %d block %d" % (S, N, B, mode, k)
                    assert_bits_equal(gm, em, what + ": mix")
                    assert_bits_equal(gp, ep, what + ": phases_out")
                    same_state(gs, es, what)
                assert len(np.unique(exp[-1][1])) > 1 or S * N * B == 1


@pytest.mark.parametrize("mode", MODES)
def test_every_subset_of_want(mx, host, mode):
    """The outputs of a subset are those of the full run and the state moves the same; a block that is not wanted is not written
    (poisoned beforehand, found untouched) and may be NULL.  A sync call does not touch the async arrays."""
    S, N, B = 3, 5, 7
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
            o = kh.GpuBackend(mx, nulls=nulls).render(1000, mode, st, B, [3.0, -2.0, 1.0], 12.0, want)
            what = "mode %d want %d nulls %s" % (mode, want, nulls)
            assert (o["mix"] is not None) == bool(want & kh.MIX) and (o["phases"] is not None) == bool(want & kh.PHASES)
            if want & kh.MIX:
                assert_bits_equal(o["mix"], ref["mix"], what)
            if want & kh.PHASES:
                assert_bits_equal(o["phases"], ref["phases"], what)
            same_state(st, ref_st, what)


@pytest.mark.parametrize("mf", [0, kh.MEANFIELD])
def test_flag_of_one_set_among_several_in_a_wavefront(gpu, host, mf):
    """17 async sets of 3 (16 to a wavefront): the flag is up on set 5 and on set 16 only.  They refresh and play K on the first
    sample; every neighbour keeps its stale gathered phases and runs free."""
    S, N, B = 17, 3, 7
    rng = np.random.default_rng(99)
    p0, g0 = rng.uniform(0, TWOPI, (S, N)), rng.uniform(0, TWOPI, (S, N))
    sts = []
    for be in (gpu, host):
        st = kh.fresh(S, N, p0)
        st["gathered"][...] = g0
        st["update"][[5, 16]] = 1
        o = be.render(1000, kh.ASYNC | mf, st, B, 5.0, 50.0)
        sts.append((o, st))
    (og, sg), (oh, sh) = sts
    assert_bits_equal(og["mix"], oh["mix"], "mix")
    assert_bits_equal(og["phases"], oh["phases"], "phases_out")
    same_state(sg, sh, "state")
    others = [s for s in range(S) if s not in (5, 16)]
    assert_bits_equal(sg["gathered"][others], g0[others], "the neighbours' gathered phases")
    assert_bits_equal(sg["gathered"][[5, 16]], p0[[5, 16]], "the raised sets' gathered phases")
    assert not sg["update"].any()
    free = p0[others] + TWOPI / 1000 * (5.0 + 0.0)
    free = np.where(free >= TWOPI, free - TWOPI, free)
    assert_bits_equal(og["phases"][0][others], free, "the neighbours ran free")
    assert np.abs(og["phases"][0][[5, 16]] - (p0[[5, 16]] + TWOPI / 1000 * 5.0)).max() > 1e-3


@pytest.mark.parametrize("mode", MODES)
def test_nan_and_stray_phases(gpu, host, mode):
    """A NaN phase in one of three sets that share a wavefront: that set is NaN from the next sample on, exactly where the host
    build has it, and the wavefront's other sets -- which take the general sine with it -- keep the host build's bits.  A phase
    far outside [0, 2 pi) (setPhase(1000)) is wrapped once per sample like the reference's; its sines come from the platform's
    sin() above |x| = 64, within 1 ULP per term but not bit-identical, so that set is held to 1e-12 and its neighbours to the bits."""
    S, N, B = 3, 5, 7
    rng = np.random.default_rng(123)
    p0 = rng.uniform(0, TWOPI, (S, N))
    for bad, tol in ((np.nan, None), (1000.0, 1e-12)):
        res = []
        for be in (gpu, host):
            st = kh.fresh(S, N, p0)
            st["phase"][1, 2] = bad
            st["update"][:] = 1
            o = be.render(1000, mode, st, B, [2.0, -3.0, 4.0], 9.0)
            res.append((o, st))
        (og, sg), (oh, sh) = res
        for s in (0, 2):
            assert_bits_equal(og["phases"][:, s], oh["phases"][:, s], "set %d beside %r" % (s, bad))
            assert_bits_equal(og["mix"][:, s], oh["mix"][:, s], "mix of set %d beside %r" % (s, bad))
        if tol is None:
            assert_bits_equal(og["phases"], oh["phases"], "NaN set")
            assert np.isnan(og["phases"][0, 1]).all() and np.isnan(og["mix"][:, 1]).all()
        else:
            assert np.isfinite(og["phases"]).all()
            assert np.abs(og["phases"][:, 1] - oh["phases"][:, 1]).max() <= tol and np.abs(og["mix"][:, 1] - oh["mix"][:, 1]).max() <= tol
