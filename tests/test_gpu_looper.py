"""GPU: K25 (mxg_looprec_render, mxg_sample_pool_normalise over a pool from mxg_sample_pool_alloc) against the reference's own
bits (tests/golden/looper.npz: the outputs, and at every cut recordPosition, the lag's val, position and the content of every slot)
and, on shapes the file does not hold, against the library's host twin (mxg_looprec_host, pinned to the same file by
tests/test_looper_host.py).  Everything is compared bit for bit; the pool comes back whole after every call, so guards, the tails
of short slots and the padding between slots are compared too.  No GPU run is compared with another GPU run, except where the
subject is that a split of the samples into calls changes nothing -- and there the unsplit call is held to the file as well."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import looper_host as lh
from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(mx):
    return lh.GpuBackend(mx)


@pytest.fixture(scope="module")
def twin(mx):
    return lh.TwinBackend(mx)


@pytest.fixture(scope="module")
def g(golden):
    return golden("looper.npz")


@pytest.mark.parametrize("key", ["loop", "play"])
def test_golden_at_every_cut(gpu, g, key):
    lh.check_cuts(gpu, g, key)


def test_golden_normalise(gpu, g):
    lh.check_normalise(gpu, g)


@pytest.mark.parametrize("key", ["loop", "play"])
def test_splits_change_nothing(mx, gpu, g, key):
    """The unsplit call (2000 samples: the library cuts it into pieces of P) and other splits -- one of P + 1 samples, one longer than
    P, pieces of 1 -- give the file's output and the same bank."""
    P = mx.lib().mxg_looprec_piece()
    whole_out, whole = lh.run_case(gpu, g, key, [])           # cut only where the events are
    assert_bits_equal(whole_out, g[key + "/out"], "unsplit output")
    for cuts in ([P + 1, P + 1 + 3 * P + 5, 1000, 1001, 1002], [1, 2, 3, P, 2 * P, 2 * P + 1, 1999]):
        out, b = lh.run_case(gpu, g, key, cuts)
        assert_bits_equal(out, whole_out, "split at %s" % cuts)
        lh.same_bank(b, whole, "split at %s" % cuts)


@pytest.mark.parametrize("Nn", [1, 7, 63, 64, 65, 512])
def test_shapes_against_the_host_twin(mx, gpu, twin, Nn):
    """R in {1, 5, one more than the slot tile, 37}, every play mode, enables per sample and per slot; the output block lies between
    sentinel bands, and the bank has two slots more than the call addresses, filled with a pattern."""
    tile = mx.lib().mxg_looprec_tile()
    rng = np.random.default_rng(2600 + Nn)
    for Rr in (1, 5, tile + 1, 37):
        for mode in (lh.PLAY_NONE, lh.PLAY, lh.PLAYLOOP):
            b0, x, en = lh.random_case(rng, Rr + 2, Nn, cap=int(rng.choice([3, 64, 200])))
            for r in (Rr, Rr + 1):
                b0.slot(r)[:] = 1234.5
            x, en = np.ascontiguousarray(x[:, :Rr]), np.ascontiguousarray(en[:, :Rr] if en.ndim == 2 else en[:Rr])
            ref, got = b0.copy(), b0.copy()
            pre = lh._Prefix(ref, Rr)
            for k in ("len", "mix", "start", "end", "recpos", "lag", "pstart", "pend", "position", "dropped", "pool_ptr"):
                setattr(pre, k, getattr(ref, k))
            o = twin.render(pre, x, en, mode)
            p = gpu.render(got, x, en, mode, band=64, R=Rr)
            what = "R %d, N %d, mode %d" % (Rr, Nn, mode)
            lh.same_bank(got, ref, what)
            if mode != lh.PLAY_NONE:
                assert_bits_equal(p, o, what + ": output")
            assert not got.outside().any(), what + ": a guard, a tail or the padding was written"
            assert (got.slot(Rr) == 1234.5).all() and (got.slot(Rr + 1) == 1234.5).all(), what + ": a slot the call does not address"


@pytest.mark.parametrize("case", ["start1", "end2", "nan", "recpos", "negative"])
def test_outside_the_domain(gpu, twin, case):
    b = lh.Bank([50, 50, 300], 300)
    for r in range(3):
        b.set_sample(r, lh.ramp(int(b.len[r])))
    b.trigger()
    n = 300
    rng = np.random.default_rng(2601)
    x = rng.uniform(-1, 1, (n, 3))
    en = np.ones((n, 3))
    en[1::3, 0] = 0.0
    if case == "start1":
        b.start[0] = 1.0
    elif case == "end2":
        b.end[0] = 2.0
    elif case == "nan":
        b.start[0] = lh.NAN
    elif case == "recpos":
        b.recpos[0], b.position[2] = 1e9, -5.0
    else:
        b.start[0], b.end[0] = -0.5, 0.0
    ref, got = b.copy(), b.copy()
    o = twin.render(ref, x, en, lh.PLAYLOOP)
    p = gpu.render(got, x, en, lh.PLAYLOOP, band=8)
    lh.same_bank(got, ref, case)
    assert_bits_equal(p, o, case + ": output")
    assert got.dropped[0] > 0 and not got.dropped[1:].any()
    assert not got.outside().any()


def test_long_slots_normalise_and_record(gpu, twin):
    """Slots longer than one normalise chunk and than a piece, of different lengths in one pool."""
    rng = np.random.default_rng(2602)
    b = lh.Bank([5000, 2048, 2049, 1, 4097], 5000)
    for r in range(b.R):
        b.set_sample(r, np.round(rng.uniform(-3e4, 3e4, int(b.len[r]))))
    b.slot(2)[2048] = -32768.0      # the peak in the last, one-element chunk
    b.trigger()
    x, en = rng.uniform(-1, 1, (700, b.R)), np.ones(b.R)
    ref, got = b.copy(), b.copy()
    assert_bits_equal(gpu.render(got, x, en, lh.PLAY), twin.render(ref, x, en, lh.PLAY), "output")
    lh.same_bank(got, ref, "record")
    level = np.array([0.99, 200.0, 1.0, 3.0, 32767.0])
    gpu.normalise(got, level)
    twin.normalise(ref, level)
    lh.same_bank(got, ref, "normalise")
    assert np.abs(got.slot(2)).max() == 1.0 and not got.outside().any()


def test_recorded_slot_through_the_sample_players(mx, gpu):
    """A slot recorded on the device, handed to the existing players as it lies in the pool (PLAYLOOP, PLAYATSPEED), against the same
    players over mxg_sample_upload of the downloaded slot."""
    L = mx.lib()
    rng = np.random.default_rng(2603)
    bank = mx.maxiLooperBank(6, 777)
    for r, n in enumerate((777, 300, 50, 441, 2, 129)):
        bank.setSample(r, lh.ramp(n))
    bank.trigger()
    bank.setLoop(0.1003, 0.6)
    x = mx.DeviceBuffer.from_numpy(rng.uniform(-1, 1, (600, 6)))
    bank.loopRecord(x, 1.0)
    a = bank.download(3)
    assert (a != lh.ramp(441)).sum() > 200
    up = L.mxg_sample_upload(a.ctypes.data, a.size)
    assert up
    V, M = 5, 400
    speed = mx.DeviceBuffer.from_numpy(np.array([1.0, 0.5, 2.25, -1.0, 0.013]))
    ps, pe = mx.DeviceBuffer.from_numpy(np.array([0.0, 0.25, 0.5, 0.1, 0.9])), mx.DeviceBuffer.from_numpy(np.array([1.0, 0.75, 0.9, 0.2, 1.0]))
    for mode in (2, 4):
        res = []
        for ptr in (bank.slot_pointer(3), up):
            pos, out = mx.DeviceBuffer.from_numpy(np.array([0.0, 10.0, 220.5, 440.0, 439.0])), mx.DeviceBuffer((M, V))
            mx._lib.check(L.mxg_sample_render(mode, V, M, ptr, a.size, 44100, speed.ptr, 0, ps.ptr, pe.ptr, pos.ptr, out.ptr, None), "mxg_sample_render")
            res.append((out.numpy(), pos.numpy()))
        assert_bits_equal(res[0][0], res[1][0], "mode %d from the pool" % mode)
        assert_bits_equal(res[0][1], res[1][1], "mode %d position" % mode)
        assert len(np.unique(res[0][0])) > 100
    mx._lib.check(L.mxg_sample_free(up), "mxg_sample_free")


def test_python_bank_against_the_c_abi(mx, twin):
    rng = np.random.default_rng(2604)
    lens = [300, 64, 129, 2, 500]
    ref = lh.Bank(lens, 500)
    bank = mx.maxiLooperBank(5, 500)
    for r, n in enumerate(lens):
        a = np.round(rng.uniform(-3e4, 3e4, n))
        ref.set_sample(r, a)
        bank.setSample(r, a)
    assert [bank.length(r) for r in range(5)] == lens
    assert_bits_equal(bank.position.numpy(), ref.position, "position after setSample")
    bank.trigger()
    ref.trigger()
    bank.setRecordMix([0.5, 0.0, 1.0, 0.5, 0.3])
    ref.mix[:] = [0.5, 0.0, 1.0, 0.5, 0.3]
    bank.setLoop(0.1, [0.6, 1.0, 0.1, 0.9, 0.35])
    ref.start[:], ref.end[:] = 0.1, [0.6, 1.0, 0.1, 0.9, 0.35]
    bank.setPlayLoop(0.0, 0.5)
    ref.pstart[:], ref.pend[:] = 0.0, 0.5
    x = rng.uniform(-1, 1, (700, 5))
    gate = (rng.uniform(0, 1, (700, 5)) < 0.7) * 3.0
    dx, dg = mx.DeviceBuffer.from_numpy(x), mx.DeviceBuffer.from_numpy(gate)
    o1 = bank.playLoop(dx, dg).numpy()
    assert_bits_equal(o1, twin.render(ref, x, gate, lh.PLAYLOOP), "playLoop, a gate block")
    o2 = bank.play(dx, 1.0).numpy()
    assert_bits_equal(o2, twin.render(ref, x, np.ones(5), lh.PLAY), "play, enabled for the call")
    assert bank.loopRecord(dx, [1, 0, 1, 0, 1]) is None
    twin.render(ref, x, np.array([1.0, 0, 1, 0, 1]), lh.PLAY_NONE)
    bank.normalise(200.0)
    twin.normalise(ref, np.full(5, 200.0))
    for r in range(5):
        assert_bits_equal(bank.download(r), ref.slot(r), "slot %d" % r)
    for k, buf in (("recpos", bank.recpos), ("lag", bank.lagval), ("position", bank.position)):
        assert_bits_equal(buf.numpy(), getattr(ref, k), k)
    assert not bank.dropped.numpy().any()
    with pytest.raises(Exception, match="larger than cap"):
        bank.setLength(1, 501)
    assert bank.length(1) == 64


def test_facade_looper_smoke():
    exe = os.path.join(ROOT, "host", "facade_looper_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_looper_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade_looper_smoke: ok" in r.stdout
