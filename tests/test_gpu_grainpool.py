"""GPU (-m gpu): K27, mxg_granular_pool_render (maximilian_amd/csrc/grainpool.hip), against the reference's bits
(tests/golden/grainpool.npz), against the library's host twin on shapes the file does not hold, against mxg_granular_render where the
two contracts meet, and behind maxiGrainPoolBank over loops that maxiLooperBank recorded on the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import grainpool_host as gh
from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("grainpool.npz")


@pytest.fixture(scope="module")
def gpu(mx):
    return gh.GpuBackend(mx)


@pytest.fixture(scope="module")
def twin(mx):
    return gh.TwinBackend(mx)


@pytest.fixture(params=[1, 2, 0], ids=["walk", "tiles", "auto"])
def form(mx, request):
    """Knob grain_pool_tiles: 1 = the walk only, 2 = the tile form wherever it can run (calls of one sample too), 0 = automatic."""
    prev = mx.lib().mxg_tune(b"grain_pool_tiles", request.param)
    yield request.param
    mx.lib().mxg_tune(b"grain_pool_tiles", prev)


def test_golden_table_cut_by_cut(gpu, g, form):
    gh.check_table(gpu, g)


def _both(gpu, twin, mode, S, T, cuts, seed, ov=3):
    rng = np.random.default_rng(seed)
    mem, lens = gh.pool_array(), np.array(gh.LENS, np.uint64)
    ps, a, b, pm, slot, loop, rnd, st0 = gh.random_case(rng, mode, S, T)
    slot[:] = np.arange(S) % gh.R          # every slot, in turn
    for j in range(S):
        loop[:, j] = np.minimum(loop[:, j], gh.LENS[slot[j]])
        if loop[0, j] >= loop[1, j]:
            loop[:, j] = (0, gh.LENS[slot[j]])
    st0[0] = np.minimum(st0[0], np.array(gh.LENS)[slot] - 1.0)

    def run(be, cuts):
        st, gst, out = st0.copy(), np.zeros((4, 8, S)), []
        for n0, n1 in zip(cuts[:-1], cuts[1:]):
            sl = lambda x, per: None if x is None else (np.ascontiguousarray(x[n0:n1]) if per else x)
            o, rc = be.call(mode, ov, "hann", n1 - n0, mem, lens, slot, loop, sl(a, mode == 2 or ps & 1), sl(b, ps & 2), sl(pm, ps & 4), ps, rnd, st, gst)
            assert rc == 0, (be.name, mode, rc, be.lib.mxg_last_error().decode())
            out.append(o)
        return np.concatenate(out), st, gst

    want = run(twin, [0, T])
    got = run(gpu, cuts)
    for x, y, name in zip(got, want, ("output", "state", "grains")):
        assert_bits_equal(x, y, "mode %d, S %d, T %d, cuts %r: %s" % (mode, S, T, cuts, name))


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_device_equals_twin_on_a_ragged_bank(gpu, twin, mode, form):
    """S = 130 over the 5 slots (three wavefronts, the last with 2 lanes), T = 700 in one call and in three."""
    _both(gpu, twin, mode, 130, 700, [0, 700], 2710 + mode)
    _both(gpu, twin, mode, 130, 700, [0, 1, 66, 700], 2720 + mode)


@pytest.mark.parametrize("T", [1, 65])
def test_device_equals_twin_on_short_calls(gpu, twin, T, form):
    for mode in range(5):
        _both(gpu, twin, mode, 130, T, [0, T], 2730 + mode + T)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_one_uploaded_sample_equals_mxg_granular_render(mx, mode, form):
    """All streams on one sample from mxg_sample_upload (R = 1, stride = 0, a one-element d_len), d_loop = NULL, ps_flags = 0: the
    output and both state arrays of mxg_granular_render."""
    L, D = mx.lib(), mx.DeviceBuffer
    rng = np.random.default_rng(2740 + mode)
    S, T, n = 130, 900, 5000
    sb = mx.maxiSampleBank(1)
    sb.setSample(rng.uniform(-1, 1, n))
    a = rng.uniform(0, 1, (T, S)) if mode == 2 else rng.uniform(0.3, 1.8, S) * np.where(np.arange(S) % 3 == 2, -1.0, 1.0)
    b = rng.uniform(0.2, 2.0, S) if mode == 1 else None
    pm = None if mode == 2 else rng.uniform(0, 0.2, S)
    rnd = rng.integers(0, 10, (S, 64)).astype(np.int32) if mode < 2 else None
    plan = L.mxg_grain_plan_create(0, gh.GRAIN_LENGTH, 44100)
    up = lambda x: None if x is None else D.from_numpy(np.ascontiguousarray(x))
    ptr = lambda x: None if x is None else x.ptr
    da, db, dp, dr = up(a), up(b), up(pm), up(rnd)
    dlen, dslot = D.from_numpy(np.array([n], np.uint64)), D(S, np.uint32)
    res = []
    for pool in (False, True):
        st, gst, out = D((4, S)), D((4, 8, S)), D((T, S))
        if pool:
            rc = L.mxg_granular_pool_render(plan, mode, S, T, sb.d_samples, 0, n, 1, dlen.ptr, dslot.ptr, None, 3, da.ptr, ptr(db), ptr(dp), 0,
                                            ptr(dr), 64 if rnd is not None else 0, st.ptr, gst.ptr, out.ptr, None)
        else:
            rc = L.mxg_granular_render(plan, mode, S, T, sb.d_samples, n, 3, da.ptr, ptr(db), ptr(dp), ptr(dr), 64 if rnd is not None else 0,
                                       st.ptr, gst.ptr, out.ptr, None)
        assert rc == 0, L.mxg_last_error().decode()
        res.append((out.numpy(), st.numpy(), gst.numpy()))
        assert L.mxg_last_async_error() == 0
    L.mxg_grain_plan_destroy(plan)
    assert res[0][0].any()
    for x, y, name in zip(res[1], res[0], ("output", "state", "grains")):
        assert_bits_equal(x, y, name)


def test_both_forms_give_the_same_bits(mx, gpu):
    """grain_pool_tiles 1 (the walk) against 2 (the tile form) on a call long enough for grains to wrap, die and be carried over a
    cut that is no multiple of the tile: negative steps and slots shorter than a grain among the streams."""
    L = mx.lib()
    res = []
    for knob in (1, 2, 0):
        prev = L.mxg_tune(b"grain_pool_tiles", knob)
        try:
            res.append(gh.run_table(gpu, [0, 777, gh.T]))
        finally:
            L.mxg_tune(b"grain_pool_tiles", prev)
    for other in res[1:]:
        assert_bits_equal(other[0], res[0][0], "output")
        for c in res[0][1]:
            assert_bits_equal(other[1][c][0], res[0][1][c][0], "state at %d" % c)
            assert_bits_equal(other[1][c][1], res[0][1][c][1], "grains at %d" % c)


def test_record_then_stretch(mx, twin):
    """maxiLooperBank.loopRecord into two slots on the device, then maxiGrainPoolBank.stretch with loop points over them: what the
    twin computes on the download()ed slots."""
    D = mx.DeviceBuffer
    R, cap, N, S, T = 2, 1500, 1500, 4, 800
    n = np.arange(N)
    x = np.stack([np.sin(n * 0.05) * 0.7, ((n * 53) % 601 - 300) / 300.0], 1)
    lb = mx.maxiLooperBank(R, cap)
    lb.setLength(1, 1100)
    lb.trigger()
    lb.setRecordMix(0.0)
    lb.loopRecord(D.from_numpy(x), 1.0, N)
    gp = mx.maxiGrainPoolBank(S, lb, "hann")
    gp.setSlot(2, 1)
    gp.setSlot(3, 1)
    gp.setSlot(1, 0)
    gp.setLoop(0.25, 0.5, 0)
    gp.setLoopStart(0.5, 3)
    gp.setLoopEnd(0.75, 3)
    assert list(gp.getLoopEnd()) == [750, 1500, 1100, 825]
    pitch, rate = np.array([1.0, 0.5, 1.7, -1.0]), np.array([1.0, 0.25, -1.0, 2.0])
    rnd = ((np.arange(S)[:, None] * 3 + np.arange(40)[None, :]) % 10).astype(np.int32)
    out = np.concatenate([gp.stretch(pitch, rate, gh.GRAIN_LENGTH, 3, k, rnd=rnd).numpy() for k in (300, 500)])
    st, gst = gp.state.numpy(), gp.grains.numpy()
    slots = [lb.download(r) for r in range(R)]
    assert all(np.abs(s).max() > 0.5 for s in slots), "the loops were recorded"
    mem = np.zeros(8 + 2 * 1600)
    for r in range(R):
        mem[8 + r * 1600:8 + r * 1600 + slots[r].size] = slots[r]
    lens = np.array([1500, 1100], np.uint64)
    est, egst, eout = np.zeros((4, S)), np.zeros((4, 8, S)), np.zeros((T, S))
    rc = twin.lib.mxg_granular_pool_host(twin.plan("hann"), 1, S, T, mem.ctypes.data + 64, 1600, 1500, R, lens.ctypes.data, gp.slot.ctypes.data,
                                         gp.loop.ctypes.data, 3, pitch.ctypes.data, rate.ctypes.data, None, 0, rnd.ctypes.data, 40, est.ctypes.data,
                                         egst.ctypes.data, eout.ctypes.data)
    assert rc == 0, twin.lib.mxg_last_error().decode()
    assert_bits_equal(out, eout, "output")
    assert_bits_equal(st, est, "state")
    assert_bits_equal(gst, egst, "grains")
    assert np.abs(out).max(axis=0).min() > 0.05
    pos = gp.getPosition()
    assert 375 <= pos[0] < 750 and 550 <= pos[3] < 825, "the positions are inside their loops"


def test_bank_modulated_inside_a_block(mx, twin):
    """A device block [N][S] (as an LFO bank writes it) as the timestretch and as posMod: the flag bits follow from the shapes."""
    D = mx.DeviceBuffer
    S, T = 5, 600
    mem, lens = gh.pool_array(), np.array(gh.LENS, np.uint64)
    gpu = gh.GpuBackend(mx)
    p, stride, dl = gpu._pool(mem, lens)
    gp = mx.maxiGrainPoolBank(S, (p, stride, gh.CAP, lens), "hann")
    n = np.arange(T)
    rate = np.stack([gh.tri(n + 37 * j) for j in range(S)], 1)
    pm = np.stack([((n * (3 + j)) % 64) / 512.0 for j in range(S)], 1)
    out = gp.stretch(np.linspace(0.5, 1.5, S), D.from_numpy(rate), gh.GRAIN_LENGTH, 2, T, posMod=D.from_numpy(pm)).numpy()
    est, egst = np.zeros((4, S)), np.zeros((4, 8, S))
    pitch = np.linspace(0.5, 1.5, S)
    eout, rc = twin.call(1, 2, "hann", T, mem, lens, np.arange(S, dtype=np.uint32), None, pitch, rate, pm, gh.PS_B | gh.PS_POSMOD, None, est, egst)
    assert rc == 0
    assert_bits_equal(out, eout, "output")
    assert_bits_equal(gp.state.numpy(), est, "state")
    assert_bits_equal(gp.grains.numpy(), egst, "grains")
    o4 = gp.stretchAtPosition(1.0, D.from_numpy(np.ascontiguousarray(pm * 4.0)), gh.GRAIN_LENGTH, 2).numpy()
    assert o4.shape == (T, S) and o4.any()


def test_refused_arguments_launch_nothing(mx, gpu):
    L, D = mx.lib(), mx.DeviceBuffer
    mem, lens = gh.pool_array(), np.array(gh.LENS, np.uint64)
    p, stride, dl = gpu._pool(mem, lens)
    S, T = 3, 16
    plan = gpu.plan("hann")
    a, st, gst = D.from_numpy(np.ones(S)), D((4, S)), D((4, 8, S))
    out = D.from_numpy(np.full((T, S), 7.0))
    bad = D.from_numpy(np.array([0, 5, 2], np.uint32))

    def call(**kw):
        v = dict(plan=plan, mode=0, S=S, T=T, pool=p, stride=stride, cap=gh.CAP, R=gh.R, len=dl.ptr, slot=None, loop=None, ov=2, a=a.ptr, b=None,
                 pm=None, ps=0, rnd=None, Rn=0, st=st.ptr, gst=gst.ptr, out=out.ptr, stream=None)
        v.update(kw)
        return L.mxg_granular_pool_render(*v.values()), L.mxg_last_error().decode()

    for kw, word in ((dict(slot=bad.ptr), "slot[1] = 5 is outside the pool of R = 5 slots"), (dict(S=6, slot=None), "S is larger than R"),
                     (dict(mode=5), "mode must be"), (dict(mode=1), "timestretch"), (dict(pool=None), "pool is null"), (dict(ov=0), "overlaps"),
                     (dict(ps=8), "ps_flags"), (dict(R=0), "R is 0"), (dict(out=None), "out is null")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert L.mxg_last_async_error() == 0
    assert (out.numpy() == 7.0).all() and not st.numpy().any() and not gst.numpy().any(), "a refused call writes nothing"
    rc, msg = call()
    assert rc == 0, msg
    assert (out.numpy() != 7.0).all()


def test_a_crowded_stream_reports_and_the_others_are_untouched(mx, gpu, form):
    """overlaps 12: stream 0 draws zeros and runs past eight live grains -- the async error; streams 1 and 2 draw 40 and are what they
    are in a call without stream 0."""
    L = mx.lib()
    mem, lens = gh.pool_array(), np.array(gh.LENS, np.uint64)
    S, T = 3, 1200
    slot, a = np.array([3, 4, 2], np.uint32), np.array([1.0, 0.5, -1.0])
    rnd = np.zeros((S, 64), np.int32)
    rnd[1:] = 40
    st, gst = np.zeros((4, S)), np.zeros((4, 8, S))
    o, rc = gpu.call(0, 12, "hann", T, mem, lens, slot, None, a, None, None, 0, rnd, st, gst)
    assert rc == -1 and "more than 8 grains" in L.mxg_last_error().decode(), (rc, L.mxg_last_error().decode())
    assert L.mxg_last_async_error() == 0, "reported once"
    st2, gst2 = np.zeros((4, 2)), np.zeros((4, 8, 2))
    o2, rc = gpu.call(0, 12, "hann", T, mem, lens, slot[1:], None, a[1:], None, None, 0, np.ascontiguousarray(rnd[1:]), st2, gst2)
    assert rc == 0 and o2.any()
    assert_bits_equal(o[:, 1:], o2, "the neighbours' output")
    assert_bits_equal(st[:, 1:], st2, "the neighbours' state")
    assert_bits_equal(gst[:, :, 1:], gst2, "the neighbours' grains")
    # a foreign grain (a position that fits the 4096 slot, not the 130 one the stream reads) and an exhausted draw queue
    st, gst = np.zeros((4, 2)), np.zeros((4, 8, 2))
    gst[:, 0, 0] = (200.0, 1.0, 3.0, 441.0)
    o, rc = gpu.call(0, 2, "hann", 50, mem, lens, np.array([0, 4], np.uint32), None, np.ones(2), None, None, 0, None, st, gst)
    assert rc == -1 and "could not have made" in L.mxg_last_error().decode()
    st, gst = np.zeros((4, 2)), np.zeros((4, 8, 2))
    o, rc = gpu.call(0, 2, "hann", 2000, mem, lens, np.array([0, 4], np.uint32), None, np.ones(2), None, None, 0, np.zeros((2, 2), np.int32), st, gst)
    assert rc == -1 and "d_rnd exhausted" in L.mxg_last_error().decode()


def test_facade_grainpool_smoke():
    """The C++ maxiGrainPoolBank: two loops recorded with maxiLooperBank, stretched with loop points, against the host twin."""
    exe = os.path.join(ROOT, "host", "facade_grainpool_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_grainpool_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade_grainpool_smoke: ok" in r.stdout and "checksum" in r.stdout
