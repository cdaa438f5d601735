"""CPU (-m "not gpu"): mxg_analysis.h -- the arithmetic analysis.hip's kernel runs -- compiled for the host with g++ under the
oracle's FPFLAGS (tests/host_analysis.cpp) reproduces tests/golden/analysis.npz BIT FOR BIT: crossings, rates, follower levels,
held samples, and every state array at every stored cut, with the blocks cut as stored and at further uneven positions.
Everything is compares, + - *, integer counts and indexing, so no tolerance applies anywhere.  Also: the numpy model (a ring of
doubles exactly like maxiRingBuf) against the same file and a seeded fuzz of the bit-packed ring against that model.  (tests/host_analysis.cpp
with -DANA_HOST_MAIN is the stand-alone program for a run under -fsanitize=address,undefined.)"""
import numpy as np
import pytest

import analysis_host as ah
from conftest import assert_bits_equal  # noqa: F401

EXTRA = (2, 64, 65, 777, 1001, 1063, 2001, 3333)
CASES = ["a", "b"]


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    return ah.HostBackend(ah.build(tmp_path_factory.mktemp("analysis")))


@pytest.fixture(scope="module")
def g(golden):
    return golden("analysis.npz")


@pytest.mark.parametrize("extra", [(), EXTRA])
@pytest.mark.parametrize("name", CASES)
def test_host_reproduces_golden(be, g, name, extra):
    c, outs, states = ah.play_case(be, g, name, extra)
    ah.check_case(c, name, outs, states)


@pytest.mark.parametrize("name", CASES)
def test_model_reproduces_golden(g, name):
    c, outs, states = ah.play_case(ah.ModelBackend(), g, name)
    ah.check_case(c, name, outs, states)


def test_golden_holds_the_edges(g):
    """What the file must contain for the tests above to mean something."""
    for name in CASES:
        zx, zcr, cuts = g[name + "/zx"], g[name + "/zcr"].astype(np.int64), g[name + "/cuts"].tolist()
        cap = int(g[name + "/cap"])
        assert cap == 1000 and cap % 64 != 0 and {1, 7} <= set(np.diff(cuts).tolist())
        d = np.diff(zcr, axis=0)
        assert all(len(np.unique(zcr[:, v])) >= 3 for v in range(zcr.shape[1])) and (d > 0).any(axis=0).all() and (d < 0).any(axis=0).all()
        assert zx[cuts[1:-1]].any() and zx[[c - 1 for c in cuts[1:-1]]].any() and zx[cap - 1].any()
    x = ah.signal(g)
    assert np.isnan(x).sum() == 1 and (np.signbit(x) & (x == 0)).any() and ((x == 0) & ~np.signbit(x)).sum() >= 20
    assert g["b/hold"].ndim == 2 and set(np.unique(g["a/hold"]).tolist()) == {0.0, 1.0, 2.5, 37.0, 300.0}
    assert "sha256" in str(g["provenance"])


def test_ring_of_bits_against_ring_of_doubles(be):
    """Seeded fuzz: random ring sizes 1 .. 200, windows 1 .. cap, start positions, ring contents, counts and block cuts."""
    rng = np.random.default_rng(16)
    model = ah.ModelBackend()
    for trial in range(150):
        cap = int(rng.integers(1, 201)) if trial % 5 else int(rng.choice([1, 2, 63, 64, 65, 127, 128, 129, 192, 200]))
        V = int(rng.integers(1, 5))
        N = int(rng.integers(1, 3 * cap + 70))
        window = rng.integers(1, cap + 1, V).astype(np.uint32)
        if trial % 7 == 0:
            window[0] = cap
        if trial % 11 == 0:
            window[-1] = 1
        x = rng.choice([-1.0, -0.25, 0.0, 0.5, 1.0], (N, V))
        st0 = ah.fresh(V, cap)
        st0["zring"][:] = ah.pack_ring(rng.integers(0, 2, (cap, V)))
        st0["zpos"][:] = rng.integers(0, cap, V)
        st0["zcount"][:] = rng.integers(-3, 50, V)
        st0["prev_x"][:] = rng.choice([-1.0, 0.0, 1.0], V)
        cuts = sorted(set([0, N] + rng.integers(0, N + 1, int(rng.integers(0, 6))).tolist()))
        sa, sb = ({k: v.copy() for k, v in st0.items()} for _ in range(2))
        for a, b in zip(cuts[:-1], cuts[1:]):
            oa = be.render(1000, x[a:b], ah.ZX | ah.ZCR, sa, window, cap, None, None, None)
            ob = model.render(1000, x[a:b], ah.ZX | ah.ZCR, sb, window, cap, None, None, None)
            assert np.array_equal(oa["zx"], ob["zx"]) and np.array_equal(oa["zcr"], ob["zcr"]), (trial, cap, window, a, b)
            for k in ("prev_x", "zring", "zpos", "zcount"):
                assert np.array_equal(sa[k], sb[k]), (trial, cap, window, k)


def test_window_above_the_ring_is_held_and_counted(be):
    V, cap, N = 3, 70, 200
    rng = np.random.default_rng(2)
    x = rng.choice([-1.0, 1.0], (N, V))
    held, over = ah.fresh(V, cap), ah.fresh(V, cap)
    a = be.render(1000, x, ah.ZCR, held, np.array([70, 70, 5], np.uint32), cap, None, None, None)
    b = be.render(1000, x, ah.ZCR, over, np.array([71, 4000000000, 5], np.uint32), cap, None, None, None)
    assert np.array_equal(a["zcr"], b["zcr"]) and over["overflow"].tolist() == [1, 1, 0] and not held["overflow"].any()
    be.render(1000, x, ah.ZCR, over, np.array([71, 70, 5], np.uint32), cap, None, None, None)
    assert over["overflow"].tolist() == [2, 1, 0]
    wild = ah.fresh(V, cap)
    wild["zpos"][:] = [-1, 70, 1 << 30]  # a stored position outside the ring restarts at slot 0
    c = be.render(1000, x, ah.ZCR, wild, np.array([70, 70, 5], np.uint32), cap, None, None, None)
    assert np.array_equal(a["zcr"], c["zcr"])


def test_negative_and_nan_hold_times_are_zero_samples(be):
    x = np.arange(1.0, 21.0)[:, None] * np.ones((1, 3))
    st = ah.fresh(3, 1)
    o = be.render(1000, x, ah.SAH, st, None, 1, None, None, np.array([-5.0, float("nan"), 0.0]))
    assert (o["sah"] == 1.0).all()  # hold == 0 samples once, ever


def test_float_follower(be):
    """maxiEnvelopeFollowerF: the recurrence in float, against numpy's float32."""
    rng = np.random.default_rng(3)
    env = np.zeros(1, np.float32)
    e, att, rel = np.float32(0), np.float32(0.37), np.float32(0.93)
    for s in rng.uniform(-1, 1, 500).astype(np.float32):
        a = np.abs(s)
        e = np.float32(np.float32((att if a > e else rel) * np.float32(e - a)) + a)
        got = be.L.ana_host_follow_f(env.ctypes.data, float(att), float(rel), float(s))
        assert np.float32(got).view(np.uint32) == e.view(np.uint32)

