"""GPU: mxg_dattaro_render (K14, dattaro.hip) through the Python bank.
The cases of tests/golden/dattaro.npz (the unmodified reference) bit for bit -- outputs, ring contents, indices, the five state
doubles -- replayed in the cases' blocks of changing length; then against the host build of mxg_dattaro.h
(tests/host_dattaro.cpp, itself pinned to the golden file by tests/test_dattaro_host.py) at shapes the file cannot hold: V in {1,
31, 64, 1000} and one large bank, N in {1, 63, 64, 65, 512, 4096} from a random state (rings full, indices anywhere), a block
sequence that carries state across calls with changing N, each of the five rates (8 000, 22 050: the input rings in sub-tiles
through LDS; 44 100, 48 000, 96 000: whole tiles on the rings) and both ends of the accepted range, and an input with a NaN and an
Inf in one voice.  No tolerance and no excluded samples: the arithmetic is + - * with contraction off, a differing bit is a bug.
(NaNs are compared as positions: IEEE 754 leaves the sign and payload of an arithmetic NaN open, see conftest.assert_bits_equal.)"""
import numpy as np
import pytest

import dattaro_cases as dc
import dattaro_host as dh
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return dh.build(tmp_path_factory.mktemp("dattaro"))


@pytest.fixture(scope="module")
def g():
    return dh.load_golden()


def make_bank(mx, st):
    """A device bank holding a copy of the host state `st`."""
    b = mx.maxiDattaroReverbBank(st.V, st.rate)
    assert (b.lengths, b.offsets, b.ring_doubles) == dc.layout(st.rate)
    b.rings.upload(st.rings)
    b.idx.upload(st.idx)
    b.state.upload(st.state)
    return b


def gpu_render(mx, b, x):
    return b.playStereo(mx.DeviceBuffer.from_numpy(x)).numpy()


def gpu_state(b):
    st = dh.State(b.sample_rate, b.V)
    st.rings, st.idx, st.state = b.rings.numpy(), b.idx.numpy(), b.state.numpy()
    return st


def assert_state_equal(got, exp, what):
    assert np.array_equal(got.idx, exp.idx), what + ": ring indices"
    assert_bits_equal(got.rings, exp.rings, what + ": rings")
    assert_bits_equal(got.state, exp.state, what + ": lp0 lp1 lp2 sigl sigr")


def random_state(rng, rate, V, cheap=False):
    st = dh.State(rate, V)
    S = st.rings.shape[1]
    if cheap:  # a large bank: a repeated block of noise is as good and much faster to make
        st.rings = np.ascontiguousarray(np.resize(rng.uniform(-1, 1, 1000003), (V, S)))
    else:
        st.rings = rng.uniform(-1, 1, (V, S))
    st.idx = (rng.integers(0, 1 << 30, (V, dc.RINGS)) % np.array(st.lens)).astype(np.int32)
    st.state = rng.uniform(-1, 1, (V, dc.STATE))
    return st


def both(mx, host, b, st, x, what):
    """One block on the device bank `b` and on the host state `st`; outputs compared bit for bit."""
    got = gpu_render(mx, b, x)
    exp = dh.host_render(host, st, x)
    assert_bits_equal(got, exp, what + ": output")
    return got


@pytest.mark.parametrize("case", dc.CASES, ids=[c["name"] for c in dc.CASES])
def test_golden_cases(mx, g, case):
    x = dh.case_inputs(case, g)
    b = make_bank(mx, dh.State(dc.case_rate(case), case["V"]))
    exp = g[case["name"] + "/out"]
    got = np.zeros_like(exp)
    for a, e in dc.block_edges(case):
        got[:, a:e] = gpu_render(mx, b, np.ascontiguousarray(x[a:e]))
    assert_bits_equal(got, exp, case["name"] + ": output")
    dh.check_case_state(case, g, gpu_state(b), case["name"])


@pytest.mark.parametrize("V", [1, 31, 64, 1000])
@pytest.mark.parametrize("rate", dc.RATES)
def test_shapes_against_host(mx, host, rate, V):
    rng = np.random.default_rng(100 * V + rate)
    for N in (1, 63, 64, 65, 512, 4096):
        st = random_state(rng, rate, V)
        if N == 65:
            st.idx[0, :] = [-1, 1 << 20, 44100, -5, 1 << 30, -(1 << 31), 50000, 99999, -2, 123456]  # outside their rings: restart at 0
        b = make_bank(mx, st)
        x = rng.uniform(-1, 1, (N, V))
        what = "%d Hz V=%d N=%d" % (rate, V, N)
        both(mx, host, b, st, x, what)
        assert_state_equal(gpu_state(b), st, what)


@pytest.mark.parametrize("end", [0, 1])
def test_ends_of_the_accepted_range(mx, host, end):
    rate = dc.accepted_ends()[end]
    rng = np.random.default_rng(7 + end)
    V = 9
    st = random_state(rng, rate, V)
    b = make_bank(mx, st)
    for N in (65, 700):
        both(mx, host, b, st, rng.uniform(-1, 1, (N, V)), "%d Hz N=%d" % (rate, N))
    assert_state_equal(gpu_state(b), st, "%d Hz" % rate)


@pytest.mark.parametrize("rate", dc.RATES)
def test_block_sequence_carries_state(mx, host, rate):
    """Changing N on one bank from a fresh state."""
    V = 77
    rng = np.random.default_rng(5 + rate)
    st = dh.State(rate, V)
    b = make_bank(mx, st)
    for k, N in enumerate([1, 63, 64, 65, 2, 512, 4096, 7, 1700, 1]):
        x = rng.uniform(-1, 1, (N, V))
        if k == 7:
            x[:] = 0.0  # a silent block: the tail
        both(mx, host, b, st, x, "%d Hz block %d (N=%d)" % (rate, k, N))
    assert_state_equal(gpu_state(b), st, "%d Hz after the sequence" % rate)


def test_large_bank(mx, host):
    """8 320 voices at 44 100 Hz, 2.15 GB of rings: every voice of a large bank, offsets beyond 2^31 bytes included."""
    rate, V = 44100, 8320
    rng = np.random.default_rng(V)
    st = random_state(rng, rate, V, cheap=True)
    b = make_bank(mx, st)
    for N in (512, 65):
        both(mx, host, b, st, rng.uniform(-1, 1, (N, V)), "V=%d N=%d" % (V, N))
    got = gpu_state(b)
    del b
    assert_state_equal(got, st, "V=%d" % V)


@pytest.mark.parametrize("rate", [8000, 44100])
def test_nan_and_inf_stay_in_their_voice(mx, host, rate):
    V, N, bad = 31, 2 * max(dc.lengths(rate)) + 500, 7
    rng = np.random.default_rng(40 + rate)
    x = rng.uniform(-1, 1, (N, V))
    clean = gpu_render(mx, make_bank(mx, dh.State(rate, V)), x)
    x[100, bad] = np.nan
    x[300, bad + 2] = np.inf
    st = dh.State(rate, V)
    b = make_bank(mx, st)
    got = gpu_render(mx, b, x)
    exp = dh.host_render(host, st, x)
    # positions of the non-finite values as positions, everything else as bits
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(np.isinf(got), np.isinf(exp))
    assert np.isnan(exp[..., bad]).any() and not np.isfinite(exp[..., bad + 2]).all()
    assert_bits_equal(got, exp, "output with a NaN in voice %d and an Inf in voice %d" % (bad, bad + 2))
    # the neighbouring voices are untouched
    keep = np.ones(V, bool)
    keep[[bad, bad + 2]] = False
    assert np.isfinite(got[..., keep]).all()
    assert_bits_equal(got[..., keep], clean[..., keep], "the other voices")
    gs = gpu_state(b)
    assert np.array_equal(gs.idx, st.idx)
    for (name, a), (_, e) in zip(gs.parts(), st.parts()):
        if name != "idx":
            assert np.array_equal(np.isnan(a), np.isnan(e)), name
            assert_bits_equal(a, e, name)
