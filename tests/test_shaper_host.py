"""CPU (-m "not gpu"): mxg_shaper.h -- the arithmetic shaper.hip's kernels run -- compiled for the host with g++ under the oracle's
FPFLAGS (tests/host_shaper.cpp) against tests/golden/shaper.npz, with the blocks cut as stored and at further uneven positions:
hardclip, fastatan, fastAtanDist, the clipped branches, NaN positions, the cross-fade, both selects and the line (output,
parameters and state at every cut) BIT FOR BIT; softclip within 2^-52 absolute (the cube is (x * x) * x, the reference's is
pow(x, 3)); atanDist and asymclip within the a-priori ULP bounds of tests/shaper_host.py (on the host they call the same libm as
the reference did, so the measured distance is normally 0).  Also: the numpy model against the same file, and a seeded fuzz of
the line's state machine, host build against the step-by-step model.  (tests/host_shaper.cpp with -DSHP_HOST_MAIN is the
stand-alone program for a run under -fsanitize=address,undefined.)"""
import numpy as np
import pytest

import shaper_host as sh
from conftest import assert_bits_equal

EXTRA = (2, 64, 65, 199, 333, 777, 1001, 1999)


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    return sh.HostBackend(sh.build(tmp_path_factory.mktemp("shaper")))


@pytest.fixture(scope="module")
def g(golden):
    return golden("shaper.npz")


def host_prepare(be):
    def prepare(par, st, v, start, end, ms, oneshot, sr):
        V = par.shape[1]
        mask = np.zeros(V, np.int32)
        mask[v] = 1
        a, b, c = (np.full(V, t, np.float64) for t in (start, end, ms))
        one = np.full(V, oneshot, np.int32)
        be.L.shp_host_line_prepare(V, a.ctypes.data, b.ctypes.data, c.ctypes.data, one.ctypes.data, mask.ctypes.data, float(sr),
                                   par.ctypes.data, st.ctypes.data)
    return prepare


@pytest.mark.parametrize("extra", [(), EXTRA])
def test_host_shaping_against_golden(be, g, extra):
    res = sh.play_shape_cases(be, g, extra)
    assert set(m for m, _ in res) == set(sh.MODES) | {"softclip_u"}


@pytest.mark.parametrize("extra", [(), EXTRA])
def test_host_xfade_select_line_reproduce_golden(be, g, extra):
    sh.play_xfade_cases(be, g, extra)
    sh.play_select_cases(be, g, extra)
    sh.play_line_case(be, g, host_prepare(be), extra)


def test_model_against_golden(g):
    m = sh.ModelBackend()
    sh.play_shape_cases(m, g)
    sh.play_xfade_cases(m, g)
    sh.play_select_cases(m, g)
    sh.play_line_case(m, g, sh.line_prepare_model)


def test_softclip_bound_and_host_model_agreement(be, g):
    """The host build and the numpy model form the same cube, so they agree bit for bit; both stay within 2^-52 of the
    reference's pow(x, 3) stream, and do differ from it somewhere (the bound is not vacuous)."""
    x = sh.signal(g)
    host, model = be.shape("softclip", x), sh.ModelBackend().shape("softclip", x)
    assert_bits_equal(host, model, "softclip: host build against the model")
    ref = g["shape/pv/softclip"]
    ok = ~np.isnan(ref)
    assert np.abs(host[ok] - ref[ok]).max() <= sh.SOFTCLIP_ABS   # (the quantised signal's cubes are exact: normally 0)
    xu, ref = g["softclip_u/x"], g["softclip_u/out"]
    host = be.shape("softclip", xu)
    assert_bits_equal(host, sh.ModelBackend().shape("softclip", xu), "softclip on the stored uniform draws")
    err = np.abs(host - ref)
    print("softclip: max abs error %.3e, %.2f %% of samples differ" % (err.max(), 100.0 * (err > 0).mean()))
    assert 0 < err.max() <= sh.SOFTCLIP_ABS
    rng = np.random.default_rng(18)
    u = rng.uniform(-1.0, 1.0, (20000, 1))
    assert_bits_equal(be.shape("softclip", u), sh.ModelBackend().shape("softclip", u), "softclip on uniform draws")


def test_golden_holds_the_edges(g):
    """What the file must contain for the tests above to mean something."""
    x = sh.signal(g)
    cuts = g["cuts"].tolist()
    assert {1, 7} <= set(np.diff(cuts).tolist()) and x.shape == (2000, 3)
    assert np.isnan(x).sum() == 1 and (np.signbit(x) & (x == 0)).any() and ((x == 0) & ~np.signbit(x)).any()
    assert not (np.signbit(x[:, :sh.ASYM_V]) & (x[:, :sh.ASYM_V] == 0)).any()   # -0.0 stays out of the voices played through asymclip
    for v in range(3):
        assert (x[:, v] == 1).any() and (x[:, v] == -1).any() and (x[:, v] > 1).any() and (x[:, v] < -1).any()
    shape_ps, a_ps, b_ps = sh.per_sample_params(g)
    assert shape_ps.min() >= 0.5 and shape_ps.max() <= 50 and a_ps.min() >= 0.25 and a_ps.max() <= 8 and b_ps.min() >= 0.25
    _, _, xf = sh.xfade_inputs(g)
    assert (xf > 1).any() and (xf < -1).any()
    ev = sh.line_events(g)
    assert set(ev) <= set(cuts) and len(ev) >= 3 and g["line/out"].shape[1] == 5
    st = np.stack([g["line/snap%d/st" % i] for i in range(len(cuts) - 1)])
    assert (st[:, 2] == 1).any() and (st[:, 3] == 1).any()   # a cut falls inside a running line and after a completed one
    assert np.signbit(g["asym_zero/out"]).ravel().tolist() == [True, False, False]
    assert "sha256" in str(g["provenance"])


def test_line_state_machine_fuzz(be):
    """Seeded fuzz, host build against the step-by-step model: random parameters (ascending, descending, inc of 0, +-Inf and NaN
    from a duration of 0), flags, start states and trigger blocks with exact zeros, cut at random positions; constant triggers."""
    rng = np.random.default_rng(1818)
    model = sh.ModelBackend()
    prepare = host_prepare(be)
    for trial in range(120):
        V = int(rng.integers(1, 6))
        N = int(rng.integers(1, 150))
        pa, sa = sh.line_fresh(V)
        pb, sb = pa.copy(), sa.copy()
        for v in range(V):
            start, end = rng.choice([-1.0, 0.0, 0.5, 1.0, 2.0], 2)
            ms = float(rng.choice([0.0, 3.0, 10.0, 17.5, 40.0]))
            one = int(rng.integers(0, 2))
            prepare(pa, sa, v, start, end, ms, one, 1000.0)
            sh.line_prepare_model(pb, sb, v, start, end, ms, one, 1000.0)
        en = rng.integers(0, 4, V) > 0
        pa[4] = pb[4] = en
        if trial % 3 == 0:   # any state, not only a fresh one
            sa[1] = sb[1] = rng.choice([-1.0, 0.0, 1.0], V)
            sa[2] = sb[2] = rng.integers(0, 2, V)
            sa[3] = sb[3] = rng.integers(0, 2, V)
        assert_bits_equal(pa, pb, "prepare: parameters")
        assert_bits_equal(sa, sb, "prepare: state")
        trig = rng.choice([-1.0, 0.0, -0.0, 0.25, 1.0], (N, V), p=[0.35, 0.1, 0.05, 0.2, 0.3])
        cuts = sorted(set([0, N] + rng.integers(0, N + 1, int(rng.integers(0, 5))).tolist()))
        for a, b in zip(cuts[:-1], cuts[1:]):
            if trial % 5 == 4:
                oa, ob = be.line(1.0, b - a, pa, sa), model.line(1.0, b - a, pb, sb)
            else:
                oa, ob = be.line(trig[a:b], b - a, pa, sa), model.line(trig[a:b], b - a, pb, sb)
            assert_bits_equal(oa, ob, "trial %d block %d..%d" % (trial, a, b))
            assert_bits_equal(sa, sb, "trial %d state at %d" % (trial, b))


def test_select_edges_host_against_model(be):
    """K = 1, 2 and 64, the clamps, -0.0, +-Inf and the NaN departure (element 0, counted per voice)."""
    rng = np.random.default_rng(64)
    model = sh.ModelBackend()
    for K in (1, 2, 64):
        N, V = 40, 3
        index = rng.uniform(-1.0, K + 1.0, (N, V))
        index[0] = [-0.0, float("inf"), float("-inf")]
        index[1] = [K, K - 1e-12, float(K - 1)]
        index[2, 1] = index[5, 1] = index[7, 2] = float("nan")
        for values in (rng.uniform(-2, 2, (K, V)), rng.uniform(-2, 2, (K, N, V))):
            for interp in (0, 1):
                for normalised in (False, True):
                    ix = index / K if normalised else index
                    a, ca = be.select(interp, ix, values, normalised)
                    b, cb = model.select(interp, ix, values, normalised)
                    assert_bits_equal(a, b, "K %d interp %d normalised %s" % (K, interp, normalised))
                    assert ca.tolist() == cb.tolist() == [0, 2, 1]
                    v0 = values[0] if values.ndim == 2 else values[0][np.isnan(ix)]
                    if values.ndim == 3 and not interp:
                        assert_bits_equal(a[np.isnan(ix)], v0, "a NaN index reads element 0")
