"""GPU: mxg_analysis_render (kernel K16) against the reference's own bits (tests/golden/analysis.npz) and, on shapes the file does
not hold, against the numpy model of tests/analysis_host.py (pinned to the same file by tests/test_analysis_host.py).  Everything
is compares, + - *, integer counts and indexing: every comparison is bit for bit, outputs and state arrays alike."""
import itertools

import numpy as np
import pytest

import analysis_host as ah
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

MODEL = ah.ModelBackend()


@pytest.fixture(scope="module")
def gpu(mx):
    return ah.GpuBackend(mx)


@pytest.fixture(scope="module")
def g(golden):
    return golden("analysis.npz")


def same_state(a, b, keys, what):
    for k in keys:
        if a[k].dtype == np.float64:
            assert_bits_equal(a[k], b[k], "%s: %s" % (what, k))
        else:
            assert np.array_equal(a[k], b[k]), "%s: %s" % (what, k)


@pytest.mark.parametrize("name", ["a", "b"])
def test_golden_cases(gpu, g, name):
    """All four outputs and every state array at every cut are the reference's bits."""
    c, outs, states = ah.play_case(gpu, g, name)
    assert c["zx"].sum() > 1000 and len(np.unique(c["zcr"])) > 50
    ah.check_case(c, name, outs, states)


@pytest.fixture(scope="module")
def all_stages(gpu, g):
    c, outs, states = ah.play_case(gpu, g, "a", extra=(777,))
    return outs, states


@pytest.mark.parametrize("want", range(1, 16))
def test_every_subset_of_want(mx, g, all_stages, want):
    """The outputs of a subset equal the all-stages run; the state arrays of stages that are not asked for, filled with a canary,
    are untouched; null pointers for them are accepted."""
    full, full_states = all_stages
    x = ah.signal(g)
    c = {k[2:]: g[k] for k in g.files if k.startswith("a/")}
    N, V = x.shape
    cap = int(c["cap"])
    used = set()
    for b, keys in ah.STAGE_STATE.items():
        if want & b:
            used |= set(keys)
    for nulls in (True, False):
        be = ah.GpuBackend(mx, nulls=nulls)
        st = ah.fresh(V, cap)
        canary = {}
        for k in ah.STATE_KEYS:
            if k not in used:
                st[k].view(np.uint8)[...] = 0x5A
                canary[k] = st[k].copy()
        outs = {n: [] for b, n in ah.NAMES.items() if want & b}
        for a, b in ((0, 777), (777, N)):
            o = be.render(int(c["sr"]), x[a:b], want, st, c["window"], cap, c["attack"], c["release"], c["hold"])
            assert set(o) == set(outs)
            for n in outs:
                outs[n].append(o[n])
        for n in outs:
            assert_bits_equal(np.concatenate(outs[n]), full[n], "want %d nulls %s: %s" % (want, nulls, n))
        same_state(st, full_states[N], [k for k in used if k != "overflow"], "want %d" % want)
        for k, v in canary.items():
            assert st[k].tobytes() == v.tobytes(), "want %d: %s of a stage that was not asked for changed" % (want, k)


EDGES = [(1, 1), (2, 1), (63, 63), (64, 64), (65, 65), (65, 1), (130, 128), (1000, 1000), (1000, 999), (1000, 64), (1000, 37), (1000, 1)]


@pytest.mark.parametrize("cap,W", EDGES)
def test_ring_edges(gpu, cap, W):
    """The shared head / tail word, the partial last word and the wrap: V = 3 at staggered start positions (one of them cap - 1),
    N = 2 * cap + 5 in blocks of 1, 7, 64 and the rest."""
    x, st, window, cuts = ah.edge_case(cap, W)
    sg, sm = ({k: v.copy() for k, v in st.items()} for _ in range(2))
    assert (cap - 1) in sg["zpos"].tolist()
    crossings = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        og = gpu.render(1000, x[a:b], ah.ZX | ah.ZCR, sg, window, cap, None, None, None)
        om = MODEL.render(1000, x[a:b], ah.ZX | ah.ZCR, sm, window, cap, None, None, None)
        crossings += int(om["zx"].sum())
        assert_bits_equal(og["zx"], om["zx"], "cap %d W %d block %d..%d: zx" % (cap, W, a, b))
        assert_bits_equal(og["zcr"], om["zcr"], "cap %d W %d block %d..%d: zcr" % (cap, W, a, b))
        same_state(sg, sm, ("prev_x", "zring", "zpos", "zcount", "overflow"), "cap %d W %d at %d" % (cap, W, b))
    assert crossings >= 1 and (W == 1 or cap < 3 or sm["zcount"].any())


SHAPES = list(itertools.product([1, 2, 63, 64, 65, 130], [1, 8, 9, 512]))
_expected = {}


def store_case(V, N):
    if (V, N) not in _expected:
        rng = np.random.default_rng(100 * V + N)
        cap = 100
        x = rng.choice([-0.5, 0.25, 0.75, -0.125, 0.0, 1.0], (N, V)) * rng.uniform(0.5, 1.0, (N, V))
        par = dict(window=rng.integers(1, cap + 1, V).astype(np.uint32), attack=rng.uniform(0.1, 0.9, V), release=rng.uniform(0.9, 0.999, V),
                   hold=rng.choice([0.0, 1.0, 2.5, 37.0], (N, V)) if N % 2 else rng.choice([0.0, 1.0, 2.5, 37.0], V))
        st = ah.fresh(V, cap)
        st["zpos"][:] = rng.integers(0, cap, V)
        st["env"][:] = rng.uniform(0, 1, V)
        sm = {k: v.copy() for k, v in st.items()}
        exp = MODEL.render(1000, x, ah.ALL, sm, par["window"], cap, par["attack"], par["release"], par["hold"])
        _expected[(V, N)] = (x, par, st, exp, sm)
    return _expected[(V, N)]


@pytest.mark.parametrize("knob", [1, 2])
def test_store_paths(mx, gpu, knob):
    """8-byte stores and 16-byte pair rows, the odd tail, shadow lanes and a chunk remainder."""
    lib = mx.lib()
    mx._lib.check(lib.mxg_tune(b"rw_store", knob), "mxg_tune")
    try:
        for V, N in SHAPES:
            x, par, st, exp, sm = store_case(V, N)
            sg = {k: v.copy() for k, v in st.items()}
            got = gpu.render(1000, x, ah.ALL, sg, par["window"], 100, par["attack"], par["release"], par["hold"])
            for n in exp:
                assert_bits_equal(got[n], exp[n], "rw_store %d V %d N %d: %s" % (knob, V, N, n))
            same_state(sg, sm, ah.STATE_KEYS, "rw_store %d V %d N %d" % (knob, V, N))
    finally:
        mx._lib.check(lib.mxg_tune(b"rw_store", 0), "mxg_tune")


def test_window_above_the_ring(gpu):
    """Held at cap, d_overflow increased by exactly one per call, other voices unaffected."""
    V, cap, N = 5, 70, 300
    rng = np.random.default_rng(5)
    x = rng.choice([-1.0, 1.0], (N, V))
    held, over = ah.fresh(V, cap), ah.fresh(V, cap)
    wh, wo = np.array([70, 70, 5, 70, 33], np.uint32), np.array([71, 4000000000, 5, 70, 33], np.uint32)
    for i in range(3):
        a = gpu.render(1000, x[i * 100:(i + 1) * 100], ah.ZCR, held, wh, cap, None, None, None)
        b = gpu.render(1000, x[i * 100:(i + 1) * 100], ah.ZCR, over, wo, cap, None, None, None)
        assert_bits_equal(a["zcr"], b["zcr"], "call %d" % i)
        assert over["overflow"].tolist() == [i + 1, i + 1, 0, 0, 0] and not held["overflow"].any()
    m = ah.fresh(V, cap)
    exp = MODEL.render(1000, x, ah.ZCR, m, wo, cap, None, None, None)
    assert exp["zcr"].max() > 10
    same_state(over, m, ("prev_x", "zring", "zpos", "zcount"), "held window")


def test_crossings_trigger_an_envelope_bank_on_the_device(mx):
    """The zx block is the trigger of mxg_envgen_render (tpv = 1) with no host array in between: the same render fed a
    host-computed trigger block gives the same bits."""
    V, N, B = 130, 512, 3
    rng = np.random.default_rng(9)
    n = np.arange(N * B)[:, None]
    x = np.sin(2 * np.pi * n * rng.uniform(20.0, 400.0, V)[None, :] / 44100.0 + rng.uniform(0, 6, V)[None, :]) - 0.1
    ana = mx.maxiAnalysisBank(V, cap=1000)
    e1, e2 = mx.maxiEnvGenBank(V), mx.maxiEnvGenBank(V)
    for e in (e1, e2):
        assert e.setup([0, 1, 0.2, 0], [5, 4, 2], [1, 1, 1], False, True)
    prev = np.vstack([np.zeros((1, V)), x[:-1]])
    trig = ((prev <= 0) & (x > 0)).astype(np.float64)
    assert trig.sum(axis=0).min() >= 1
    for i in range(B):
        blk = mx.DeviceBuffer.from_numpy(x[i * N:(i + 1) * N])
        t = ana.render(blk, want="zx")["zx"]
        a = e1.play(t).numpy()
        b = e2.play(mx.DeviceBuffer.from_numpy(trig[i * N:(i + 1) * N])).numpy()
        assert_bits_equal(t.numpy(), trig[i * N:(i + 1) * N], "zx block %d" % i)
        assert_bits_equal(a, b, "envelope block %d" % i)
    assert a.max() > 0


def test_python_bank(mx, g):
    """maxiAnalysisBank: render(x, want=...) returns the requested blocks, reset() starts over, a window of 0 is refused."""
    x = ah.signal(g)[:600]
    c = {k[2:]: g[k] for k in g.files if k.startswith("a/")}
    V = x.shape[1]
    mx.maxiSettings.setup(1000, 2, 1024)
    try:
        bank = mx.maxiAnalysisBank(V)
        assert bank.cap == 1000 and bank.zring.shape == (16, V)
        bank.setWindow(c["window"])
        bank.attack.upload(c["attack"])
        bank.release.upload(c["release"])
        for rnd in range(2):
            o = bank.render(mx.DeviceBuffer.from_numpy(x), hold_ms=c["hold"])
            assert sorted(o) == ["env", "sah", "zcr", "zx"]
            assert_bits_equal(o["zcr"].numpy(), c["zcr"][:600].astype(np.float64), "zcr")
            assert_bits_equal(o["env"].numpy(), c["env"][:600], "env")
            assert_bits_equal(o["sah"].numpy(), c["sah"][:600].astype(np.float64), "sah")
            bank.reset()
        assert sorted(bank.render(mx.DeviceBuffer.from_numpy(x), want=("env", "zx"))) == ["env", "zx"]
        with pytest.raises(mx.MaxiGpuError, match="window"):
            bank.setWindow(0)
    finally:
        mx.maxiSettings.setup(44100, 2, 1024)
