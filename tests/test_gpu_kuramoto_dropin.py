"""GPU: host/facade_kuramoto_smoke exits 0; the Python bank (maxiKuramotoBank: play, render_phases, phases, set_phase, set_phases,
meanfield=, asynchronous=) gives the host build's bits (tests/host_kuramoto.cpp); tests/patches/kuramoto_patch.cpp built as
host/dropin_ku -- the Kuramoto classes on the host, their mix mapped onto the pitch of a maxiOsc::sawn on the device -- gives the
stream the same patch gives with the reference (tests/golden/kuramoto.npz["patch"])."""
import os
import platform
import subprocess

import numpy as np
import pytest

import kuramoto_host as kh
from conftest import GOLDEN, ROOT, assert_bits_equal
from test_kuramoto_dropin_cpu import PATCH_TOL

pytestmark = pytest.mark.gpu
TWOPI = kh.TWOPI


def test_facade_kuramoto_smoke():
    exe = os.path.join(ROOT, "host", "facade_kuramoto_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_kuramoto_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("meanfield,asynchronous", [(False, False), (True, False), (False, True), (True, True)])
def test_python_bank_against_host_build(mx, tmp_path_factory, meanfield, asynchronous):
    H = kh.HostBackend(kh.build(tmp_path_factory.mktemp("kuramoto_host")))
    mode = (kh.MEANFIELD if meanfield else 0) | (kh.ASYNC if asynchronous else 0)
    S, N, B = 5, 6, 20
    rng = np.random.default_rng(3)
    p0 = rng.uniform(0, TWOPI, (S, N))
    freq, K = rng.uniform(-30, 30, S), rng.uniform(0, 50, S)
    fblock = rng.uniform(-30, 30, (B, S))
    mx.maxiSettings.setup(1000, 2, 1024)
    try:
        bank = mx.maxiKuramotoBank(S, N, meanfield=meanfield, asynchronous=asynchronous)
        assert not bank.phases().any()
        st = kh.fresh(S, N)
        bank.set_phases(p0)
        st["phase"][...] = p0
        st["update"][:] = 1
        mix = bank.play(freq, K, B).numpy()
        exp = H.render(1000, mode, st, B, freq, K)
        assert_bits_equal(mix, exp["mix"], "play")
        assert_bits_equal(bank.phases(), st["phase"], "phases")
        # setPhase on two sets, then a block with freq per sample from a device block
        bank.set_phase([0.25, 5.5], 2, sets=[1, 4])
        st["phase"][[1, 4], 2] = [0.25, 5.5]
        st["update"][[1, 4]] = 1
        m2, p2 = bank.render_phases(mx.DeviceBuffer.from_numpy(fblock), K)
        exp = H.render(1000, mode, st, B, fblock, K)
        assert_bits_equal(m2.numpy(), exp["mix"], "render_phases: mix")
        assert_bits_equal(p2.numpy(), exp["phases"], "render_phases: phases")
        assert_bits_equal(bank.phases(), st["phase"], "phases after render_phases")
        if asynchronous:
            assert_bits_equal(bank.gathered.numpy(), st["gathered"], "gathered")
            assert not bank.update.numpy().any()
        bank.set_phases(p0[0], sets=[3])
        st["phase"][3] = p0[0]
        st["update"][3] = 1
        assert_bits_equal(bank.play(freq, K, 7).numpy(), H.render(1000, mode, st, 7, freq, K)["mix"], "after set_phases on one set")
        with pytest.raises(ValueError, match="want"):
            bank.render(4, freq, K, want=("mix", "rms"))
        with pytest.raises(IndexError):
            bank.set_phase(0.0, N)
    finally:
        mx.maxiSettings.setup(44100, 2, 1024)


def test_kuramoto_patch_against_reference(tmp_path):
    g = np.load(os.path.join(GOLDEN, "kuramoto.npz"))
    exp = g["patch"]
    exe = os.path.join(ROOT, "host", "dropin_ku")
    if not os.path.exists(exe):
        pytest.fail("host/dropin_ku is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)")
    out = str(tmp_path / "o.f64")
    r = subprocess.run([exe, str(exp.shape[0]), out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert b"ERROR" not in r.stderr, r.stderr.decode()
    got = np.fromfile(out, np.float64).reshape(exp.shape)
    assert len(np.unique(exp[:, 1])) > 0.9 * exp.shape[0] and np.abs(exp[:, 1]).max() <= 1.0   # a saw that moves
    same_libc = " ".join(platform.libc_ver()) == str(g["libc"])
    print("kuramoto_patch: max |difference| channel 0 %.3e, channel 1 %.3e (libc %s the recorded one)"
          % (np.abs(got[:, 0] - exp[:, 0]).max(), np.abs(got[:, 1] - exp[:, 1]).max(), "is" if same_libc else "is NOT"))
    if same_libc:
        assert_bits_equal(got[:, 0], exp[:, 0], "the sets (host)")
        assert_bits_equal(got[:, 1], exp[:, 1], "sawn at the pair's pitch (device)")
    else:
        # another libm: the pitch moves by 880 * ln 8 / (2 pi) Hz per radian of mix, 2e-10 Hz for a mix within PATCH_TOL; over the
        # run that is 2e-11 cycles of the saw, 4e-11 of its output -- except on the sample of a wrap that falls the other way
        assert np.abs(got[:, 0] - exp[:, 0]).max() <= PATCH_TOL
        assert (np.abs(got[:, 1] - exp[:, 1]) <= 1e-10).mean() >= 0.999
