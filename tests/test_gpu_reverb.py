"""GPU: mxg_reverb_render (K13, reverb.hip) through the Python banks.
The cases of tests/golden/reverb.npz (the unmodified reference) bit for bit -- outputs, ring contents, indices, low-pass states,
(w, cut) -- then against the host build of mxg_reverb.h (tests/host_reverb.cpp, itself pinned to the golden file by
tests/test_reverb_host.py) at shapes the file cannot hold: V in {1, 31, 64, 1000} and one large bank per kind, N in {1, 63, 64,
65, 512, 4096} from a random state (rings full, indices anywhere), a block sequence that carries state across calls with
changing N and changing overload, per-sample parameters beyond both clamps, and an input with a NaN and an Inf in one voice.
No tolerance and no excluded samples: the arithmetic is + - * with contraction off, a differing bit is a bug.  (NaNs are
compared as positions: IEEE 754 leaves the sign and payload of an arithmetic NaN open, see conftest.assert_bits_equal.)"""
import numpy as np
import pytest

import reverb_cases as rc
import reverb_host as rh
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

FORMS = {"sat": (rc.SAT, 0), "fv4": (rc.FREEVERB, 0), "fv31": (rc.FREEVERB, 1), "stereo": (rc.STEREO, 0)}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return rh.build(tmp_path_factory.mktemp("reverb"))


@pytest.fixture(scope="module")
def g():
    return rh.load_golden()


def make_bank(mx, st):
    """A device bank holding a copy of the host state `st`."""
    cls = {rc.SAT: mx.maxiSatReverbBank, rc.FREEVERB: mx.maxiFreeVerbBank, rc.STEREO: mx.maxiFreeVerbStereoBank}[st.kind]
    b = cls(st.V)
    assert (b.ring_doubles, b.lengths) == (rc.RING_DOUBLES[st.kind], rc.LENGTHS[st.kind])
    b.rings.upload(st.rings)
    b.idx.upload(st.idx)
    if st.kind == rc.FREEVERB:
        b.lp.upload(st.lp)
        b.wc.upload(st.wc)
    return b


def gpu_render(mx, b, kind, mode, x, room=None, absorb=None):
    dx = mx.DeviceBuffer.from_numpy(x)
    if kind == rc.SAT:
        return b.play(dx).numpy()
    if kind == rc.STEREO:
        return b.playStereo(dx).numpy()
    return b.play(dx).numpy() if mode == 0 else b.play(dx, room, absorb).numpy()


def gpu_state(b, kind):
    st = rh.State(kind, b.V)
    st.rings, st.idx = b.rings.numpy(), b.idx.numpy()
    if kind == rc.FREEVERB:
        st.lp, st.wc = b.lp.numpy(), b.wc.numpy()
    return st


def assert_state_equal(got, exp, what):
    assert np.array_equal(got.idx, exp.idx), what + ": ring indices"
    for (name, a), (_, e) in zip(got.parts(), exp.parts()):
        if name != "idx":
            assert_bits_equal(a, e, "%s: %s" % (what, name))


def random_state(rng, kind, V, cheap=False):
    st = rh.State(kind, V)
    S = st.rings.shape[1]
    if cheap:  # a large bank: a repeated block of noise is as good and much faster to make
        st.rings = np.ascontiguousarray(np.resize(rng.uniform(-1, 1, 1000003), (V, S)))
    else:
        st.rings = rng.uniform(-1, 1, (V, S))
    st.idx = (rng.integers(0, 1 << 30, (V, len(rc.LENGTHS[kind]))) % np.array(rc.LENGTHS[kind])).astype(np.int32)
    st.lp = rng.uniform(-1, 1, (V, 8))
    st.wc = np.stack([rng.uniform(0.5, 0.98, V), rng.uniform(0, 1, V)], axis=1)
    return st


def params(rng, N, V, per_sample):
    """roomsize, absorbtion, ps: [N][V] beyond both clamps, or [V]."""
    if per_sample:
        return rng.uniform(-21.0, 3.0, (N, V)), rng.uniform(-1.5, 1.5, (N, V)), 3
    return rng.uniform(-6.0, 1.5, V), rng.uniform(0.0, 1.0, V), 0


def both(mx, host, b, st, kind, mode, x, room=None, absorb=None, ps=0, what=""):
    """One block on the device bank `b` and on the host state `st`; outputs compared bit for bit."""
    got = gpu_render(mx, b, kind, mode, x, room, absorb)
    exp = rh.host_render(host, st, mode, x, None if room is None else np.ascontiguousarray(room),
                         None if absorb is None else np.ascontiguousarray(absorb), ps)
    assert_bits_equal(got, exp, what + ": output")
    return got


@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_golden_cases(mx, g, case):
    kind = case["kind"]
    b = make_bank(mx, rh.State(kind, case["V"]))
    exp = g[case["name"] + "/out"]
    got = np.zeros_like(exp)
    for a, e, m, x, room, absorb, ps in rh.case_blocks(case, g):
        o = gpu_render(mx, b, kind, m, x, room, absorb)
        got[:, a:e] = o if kind == rc.STEREO else o[None]
    assert_bits_equal(got, exp, case["name"] + ": output")
    rh.check_case_state(case, g, gpu_state(b, kind), case["name"])


@pytest.mark.parametrize("V", [1, 31, 64, 1000])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_shapes_against_host(mx, host, form, V):
    kind, mode = FORMS[form]
    rng = np.random.default_rng(100 * V + kind * 7 + mode)
    for N in (1, 63, 64, 65, 512, 4096):
        st = random_state(rng, kind, V)
        b = make_bank(mx, st)
        x = rng.uniform(-1, 1, (N, V))
        room, absorb, ps = params(rng, N, V, per_sample=N != 512) if mode else (None, None, 0)
        what = "%s V=%d N=%d" % (form, V, N)
        both(mx, host, b, st, kind, mode, x, room, absorb, ps, what)
        assert_state_equal(gpu_state(b, kind), st, what)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_block_sequence_carries_state(mx, host, form):
    """Changing N, and for maxiFreeVerb the two overloads and the three parameter layouts, on one bank from a fresh state."""
    kind, mode0 = FORMS[form]
    V = 77
    rng = np.random.default_rng(5 + kind)
    st = rh.State(kind, V)
    b = make_bank(mx, st)
    for k, N in enumerate([1, 63, 64, 65, 2, 512, 4096, 7, 1700, 1]):
        x = rng.uniform(-1, 1, (N, V))
        if k == 5:
            x[:] = 0.0  # a silent block: the tail
        mode = (k % 2 if form == "fv31" else mode0) if kind == rc.FREEVERB else 0
        room = absorb = None
        ps = 0
        if mode:
            ps = k % 4
            room = rng.uniform(-21.0, 3.0, (N, V) if ps & 1 else V)
            absorb = rng.uniform(-1.5, 1.5, (N, V) if ps & 2 else V)
        both(mx, host, b, st, kind, mode, x, room, absorb, ps, "%s block %d (N=%d)" % (form, k, N))
    assert_state_equal(gpu_state(b, kind), st, form + " after the sequence")


@pytest.mark.parametrize("form,V", [("sat", 65536), ("stereo", 16384), ("fv31", 16384)])
def test_large_bank(mx, host, form, V):
    """2.1 / 1.6 / 2.5 GB of rings: every voice of a full-size bank, offsets beyond 2^31 bytes included."""
    kind, mode = FORMS[form]
    rng = np.random.default_rng(V + kind)
    st = random_state(rng, kind, V, cheap=True)
    b = make_bank(mx, st)
    for N in (512, 65):
        x = rng.uniform(-1, 1, (N, V))
        room, absorb, ps = params(rng, N, V, per_sample=N == 65) if mode else (None, None, 0)
        both(mx, host, b, st, kind, mode, x, room, absorb, ps, "%s V=%d N=%d" % (form, V, N))
    got = gpu_state(b, kind)
    del b
    assert_state_equal(got, st, "%s V=%d" % (form, V))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_nan_and_inf_stay_in_their_voice(mx, host, form):
    kind, mode = FORMS[form]
    V, N, bad = 31, 2500, 7
    rng = np.random.default_rng(40 + kind + mode)
    x = rng.uniform(-1, 1, (N, V))
    room, absorb, ps = params(rng, N, V, per_sample=True) if mode else (None, None, 0)
    clean = gpu_render(mx, make_bank(mx, rh.State(kind, V)), kind, mode, x, room, absorb)
    x[100, bad] = np.nan
    x[300, bad] = np.inf
    if mode:
        absorb[50, bad + 2] = np.nan  # a NaN parameter passes the clamp and poisons that voice too
    st = rh.State(kind, V)
    b = make_bank(mx, st)
    got = gpu_render(mx, b, kind, mode, x, room, absorb)
    exp = rh.host_render(host, st, mode, x, room, absorb, ps)
    # positions of the non-finite values as positions, everything else as bits
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(np.isinf(got), np.isinf(exp))
    assert np.isnan(exp[..., bad]).any()
    assert_bits_equal(got, exp, form + ": output with a NaN and an Inf in voice %d" % bad)
    # the neighbouring voices are untouched
    keep = np.ones(V, bool)
    keep[bad] = False
    if mode:
        keep[bad + 2] = False
    assert np.isfinite(got[..., keep]).all()
    assert_bits_equal(got[..., keep], clean[..., keep], form + ": the other voices")
    gs = gpu_state(b, kind)
    assert np.array_equal(gs.idx, st.idx)
    for (name, a), (_, e) in zip(gs.parts(), st.parts()):
        if name != "idx":
            assert np.array_equal(np.isnan(a), np.isnan(e)), name
            assert_bits_equal(a, e, form + ": " + name)
