"""GPU (-m gpu): maxiDynamicsBank / maxiRMSBank (K12, dyn.hip) against tests/golden/dyn.npz and against the host build of the
same arithmetic (tests/dyn_host.py, pinned bit for bit to dyn.npz by tests/test_dyn_host.py).

Bit-identical: ring contents, ring positions, runningRMS, both envelopes' state arrays, the overflow counts, the positions of NaN
and of exact 0.0 in the output, and mxg_rms_render's output.  The companded output (device log10 and pow) is compared as a relative
error, the optional dB output as an absolute one.  A voice in which the CHECKER's detector level comes within 1e-9 dB of a boundary
it is compared with may take the other branch on the device; it is left out from that sample on, at most 0.1 % of a test's voices."""
import numpy as np
import pytest

import dyn_host
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

# Relative tolerance of the companded output: |got - exp| <= TOL * |exp|.
# measured on the MI355X over every test of this file and of tests/test_gpu_dyn_dropin.py (each block prints its figure): largest
# relative error 1.217e-14 (16 x 512 x 65 536, a voice in an expansion regime: ratio 0.3 multiplies an error of the dB value by
# 1 / ratio before pow); golden cases <= 3.2e-15, the drop-in patch <= 2.3e-15.
# allowed 8 x that = 9.74e-14 (the device log10 / pow error varies with the argument and the tests sample only part of the range);
# the cap of 1e-11, the loosest transcendental tolerance the project states (mode B), is two orders above.
MEASURED_REL = 1.217e-14
TOL = 8 * MEASURED_REL
# Absolute tolerance of the dB output: measured 5.684e-14 dB (4 ULP of a level near -100 dB); allowed 8 x that = 4.55e-13 dB.
MEASURED_DB = 5.684e-14
TOL_DB = 8 * MEASURED_DB
MAX_EXCLUDED = 0.001

CASES = ["compress", "play", "persample"]


@pytest.fixture(scope="module")
def L(tmp_path_factory, mx):
    return dyn_host.build(tmp_path_factory.mktemp("dyn"))


@pytest.fixture(scope="module")
def g(golden):
    return golden("dyn.npz")


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        assert_bits_equal(a, b, what)
    else:
        assert np.array_equal(a, b), what


def check_block(got, exp, lvl_got, lvl_exp, start, n0, what):
    """Output and dB output of one block whose first sample is n0; start [V] = first excluded sample per voice."""
    N, V = exp.shape
    valid = (n0 + np.arange(N))[:, None] < start[None, :]
    rel = dyn_host.compare_output(got, exp, valid, what)
    lg, le = lvl_got[valid], lvl_exp[valid]
    fin = np.isfinite(le)
    assert np.array_equal(np.isnan(lg), np.isnan(le)), what + ": dB NaN positions"
    assert np.array_equal(lg[~fin & ~np.isnan(le)], le[~fin & ~np.isnan(le)]), what + ": dB infinities"
    db = float(np.abs(lg[fin] - le[fin]).max()) if fin.any() else 0.0
    print("%s: rel %.3e  dB %.3e" % (what, rel, db))
    assert rel <= TOL, "%s: relative error %.3e > %.1e" % (what, rel, TOL)
    assert db <= TOL_DB, "%s: dB error %.3e > %.1e" % (what, db, TOL_DB)
    return rel, db


def check_state(got, exp, keep, what):
    """State arrays, bit for bit, over the voices that were never excluded."""
    for k, e in exp.items():
        a = got[k]
        if k.endswith("_ring") and a.shape[0] != e.shape[0]:  # a golden ring stored without its never-written rows
            assert not a[e.shape[0]:].any(), (what, k)
            a = a[:e.shape[0]]
        same(a[..., keep], e[..., keep], "%s %s" % (what, k))


def excluded_ok(start, total, what):
    n = int((start < total).sum())
    print("%s: %d of %d voices excluded by the near-tie rule" % (what, n, start.size))
    assert n <= MAX_EXCLUDED * start.size, "%s: %d voices excluded" % (what, n)
    return start >= total


# ---- golden ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [(), (1, 64, 777, 1501, 3999)])
@pytest.mark.parametrize("name", CASES)
def test_bank_against_golden(mx, L, g, name, extra):
    c = dyn_host.load_case(g, name)
    N, V = c["sig"].shape
    bank = dyn_host.construct(c, lambda V: dyn_host.GpuBank(mx, V))
    out, lvl, states = dyn_host.play_case(bank, c, extra)
    # the file keeps the level as float32; the doubles come from the host checker, which test_dyn_host.py pins to the file
    _, lvl_exp, _ = dyn_host.play_case(dyn_host.construct(c, lambda V: dyn_host.host_bank(L, V)), c)
    start = np.full(V, N)  # the generator asserted that no level is within 1e-9 dB of a boundary
    check_block(out, c["out"], lvl, lvl_exp, start, 0, name)
    ncut = len(c["cuts"]) - 1
    for i in range(ncut):
        check_state(states[i], dyn_host.expected_state(c, i, i == ncut - 1), slice(None), "%s cut %d" % (name, i))
    assert not bank.overflow.numpy().any()


def test_rms_bank_against_golden(mx, g):
    x, cap, cuts = g["rms/in_q"] / 32768.0, int(g["rms/cap"]), [int(c) for c in g["rms/cuts"]]
    N, V = x.shape
    mx.maxiSettings.setup(int(g["rms/sr"]), 2, 1024)
    try:
        bank = mx.maxiRMSBank(V, 1)
        bank.setup(100.0, 10.0)
        assert bank.cap == cap
        out = np.zeros((N, V))
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            for n, v, ms in g["rms/ops"]:
                if int(n) == a:
                    bank.setWindowSize(ms, voices=[int(v)])
            same(bank.window, g["rms/window"][i], "window")
            out[a:b] = bank.play(mx.DeviceBuffer.from_numpy(np.ascontiguousarray(x[a:b]))).numpy()
    finally:
        mx.maxiSettings.setup(44100, 2, 1024)
    for got, key in ((out, "out"), (bank.ring.numpy(), "ring"), (bank.pos.numpy(), "pos"), (bank.running.numpy(), "running")):
        same(got, g["rms/" + key], key)
    assert not bank.overflow.numpy().any()


# ---- randomized, against the host checker ------------------------------------------------------------------------------
def random_signal(rng, N, V, n0, kind, rate):
    """[N][V]: per voice noise / amplitude-modulated noise / noise with gaps of exact zeros, continuing at sample n0."""
    n = (n0 + np.arange(N))[:, None]
    x = rng.uniform(-1.0, 1.0, (N, V))
    amp = 10.0 ** ((-55.0 + 55.0 * (0.5 - 0.5 * np.cos(n * rate[None, :]))) / 20.0)
    x = np.where(kind[None, :] == 0, x, x * amp)
    gap = (kind[None, :] == 2) & ((n // 97) % 3 == 1)
    return np.ascontiguousarray(np.where(gap, 0.0, x))


class Regimes:
    """Mixed regimes per voice: analyser, window, look-ahead, ratios below / above 1 and off, knees on and off."""

    def __init__(self, rng, V, cap_r, cap_l, per_sample):
        self.rng, self.V, self.per_sample = rng, V, per_sample
        self.kind = rng.integers(0, 3, V)
        self.rate = rng.uniform(0.002, 0.05, V)
        self.analyser = rng.integers(0, 2, V)
        self.window = rng.choice([1, 2, 17, cap_r // 3, cap_r], V).astype(np.uint32)
        self.look = rng.choice([0, 0, 1, 5, cap_l // 2, cap_l], V).astype(np.uint32)
        self.th = rng.uniform(-30.0, -5.0, V)
        self.rh = rng.choice([0.0, 0.3, 0.7, 2.0, 6.0], V)
        self.kh = rng.choice([0.0, 0.0, 3.0, 8.0], V)
        self.tl = rng.uniform(-55.0, -35.0, V)
        self.rl = rng.choice([0.0, 0.0, 0.5, 2.0, 4.0], V)
        self.kl = rng.choice([0.0, 4.0], V)

    def apply(self, bank):
        bank.analyser[:] = self.analyser
        bank.window[:] = self.window
        bank.lookahead[:] = self.look
        bank.invalidate()

    def pars(self, N, n0):
        if not self.per_sample:
            return [self.th, self.rh, self.kh, self.tl, self.rl, self.kl]
        n = (n0 + np.arange(N))[:, None]
        th = self.th[None, :] + 6.0 * np.sin(n * 0.01 + np.arange(self.V)[None, :])
        rh = np.where(self.rh[None, :] > 0, self.rh[None, :] * (1.0 + 0.5 * np.cos(n * 0.003)), 0.0)
        return [np.ascontiguousarray(th), np.ascontiguousarray(rh), self.kh, self.tl, self.rl, self.kl]


def run_pair(mx, L, V, blocks, seed, cap_r=600, cap_l=300, per_sample=False, sidechain=True, stream=None, mid=None):
    """The same random stream through a GPU bank and the host checker, block after block; compares every block and the state after
    each.  mid(i, gpu, host): called between blocks.  Returns (gpu bank wrapper, host bank, largest rel, largest dB)."""
    rng = np.random.default_rng(seed)
    reg = Regimes(rng, V, cap_r, cap_l, per_sample)
    gpu = dyn_host.GpuBank(mx, V, cap_r, cap_l, stream=stream)
    host = dyn_host.host_bank(L, V, cap_r, cap_l)
    for b in (gpu, host):
        reg.apply(b)
        b.setAttackHigh(3.0)
        b.setReleaseLow(1.0)
    total = sum(blocks)
    start = np.full(V, total)
    n0, worst = 0, (0.0, 0.0)
    outs = []
    for i, N in enumerate(blocks):
        sig = random_signal(rng, N, V, n0, reg.kind, reg.rate)
        ctl = random_signal(rng, N, V, n0, reg.kind[::-1].copy(), reg.rate) if sidechain else None
        pars = reg.pars(N, n0)
        eo, el = host.play(sig, ctl, *pars)
        go, gl = gpu.play(sig, ctl, *pars)
        ts = dyn_host.tie_start(el, pars)
        start = np.minimum(start, np.where(ts < N, n0 + ts, total))
        r = check_block(go, eo, gl, el, start, n0, "V=%d block %d (N=%d)" % (V, i, N))
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        keep = start >= total
        check_state(gpu.state(), host.state(), keep, "V=%d after block %d" % (V, i))
        outs.append(go)
        n0 += N
        if mid is not None and i + 1 < len(blocks):
            mid(i, gpu, host)
    excluded_ok(start, total, "V=%d" % V)
    return gpu, host, worst, outs


@pytest.mark.parametrize("N", [1, 7, 64, 515])
@pytest.mark.parametrize("V", [1, 63, 777, 65536])
def test_bank_against_host_checker(mx, L, V, N):
    run_pair(mx, L, V, [N, N], seed=V * 1000 + N, per_sample=(N % 2 == 1), sidechain=(V != 63))


def test_sixteen_carried_blocks_at_65536_voices(mx, L):
    _, _, worst, _ = run_pair(mx, L, 65536, [512] * 16, seed=16, cap_r=300, cap_l=200)
    print("16 x 512 x 65536: largest rel %.3e, dB %.3e" % worst)


def test_setters_mid_stream_and_overflow(mx, L):
    """Setter calls between blocks; a window and a look-ahead above the capacity (edited in place: the setters clamp them as the
    reference does) are held at the capacity and counted."""
    def mid(i, gpu, host):
        for b in (gpu, host):
            if i == 0:
                b.setRMSWindowSize(2.0, voices=[1, 5, 9])
                b.setLookAhead(0.5, voices=slice(0, 40))
                b.setReleaseHigh(150.0)
            else:
                b.window[3] = b.cap_rms + 7
                b.lookahead[4] = b.cap_lookahead + 1
                b.lookahead[3] = b.cap_lookahead + 9
                b.invalidate()

    gpu, host, _, _ = run_pair(mx, L, 200, [300, 301, 130], seed=5, mid=mid)
    ovf = gpu.overflow.numpy()
    assert ovf[3] == 2 and ovf[4] == 1 and ovf.sum() == 3
    same(ovf, host.overflow, "overflow")


def test_state_uploaded_mid_stream_on_a_stream(mx, L):
    """A bank on a non-default stream plays one block; its whole state is read back and uploaded into a fresh bank on the same stream,
    which plays the next block: same samples as a bank that played both (and as the checker, inside run_pair)."""
    s = mx.lib().mxg_stream_create()
    try:
        V, blocks = 300, [257, 190]
        ref_gpu, _, _, outs = run_pair(mx, L, V, blocks, seed=77, stream=s)
        # replay: the same draws
        rng = np.random.default_rng(77)
        reg = Regimes(rng, V, 600, 300, False)
        a = dyn_host.GpuBank(mx, V, 600, 300, stream=s)
        reg.apply(a)
        a.setAttackHigh(3.0)
        a.setReleaseLow(1.0)
        sig = [None, None]
        ctl = [None, None]
        n0 = 0
        for i, N in enumerate(blocks):
            sig[i] = random_signal(rng, N, V, n0, reg.kind, reg.rate)
            ctl[i] = random_signal(rng, N, V, n0, reg.kind[::-1].copy(), reg.rate)
            n0 += N
        o0, _ = a.play(sig[0], ctl[0], *reg.pars(blocks[0], 0))
        same(o0, outs[0], "first block")
        st = a.state()
        b = dyn_host.GpuBank(mx, V, 600, 300, stream=s)
        reg.apply(b)
        b.setAttackHigh(3.0)
        b.setReleaseLow(1.0)
        b.rms_ring.upload(st["rms_ring"]); b.la_ring.upload(st["la_ring"])
        b.rms_pos.upload(st["rms_pos"]); b.la_pos.upload(st["la_pos"]); b.running.upload(st["running"])
        b.env_high[0].upload(st["dst_h"]); b.env_high[1].upload(st["ist_h"])
        b.env_low[0].upload(st["dst_l"]); b.env_low[1].upload(st["ist_l"])
        o1, _ = b.play(sig[1], ctl[1], *reg.pars(blocks[1], blocks[0]))
        same(o1, outs[1], "second block after the upload")
        final, want = b.state(), ref_gpu.state()
        for k in want:
            if k != "overflow":
                same(final[k], want[k], k)
    finally:
        mx.lib().mxg_stream_sync(s)
        mx.lib().mxg_stream_destroy(s)


def test_rms_bank_against_host_checker(mx, L):
    rng = np.random.default_rng(3)
    V, cap = 1000, 257
    bank = mx.maxiRMSBank(V, cap)
    bank.window[:] = rng.choice([1, 2, 100, cap, cap + 3], V)
    ring, pos, run, ovf = np.zeros((cap, V)), np.zeros(V, np.int32), np.zeros(V), np.zeros(V, np.uint32)
    for N in (1, 300, 515):
        x = np.ascontiguousarray(rng.uniform(-1, 1, (N, V)) * rng.choice([0.0, 1e-3, 1.0], V)[None, :])
        exp = np.zeros((N, V))
        L.rms_host_render(V, N, x.ctypes.data, bank.window.ctypes.data, ring.ctypes.data, cap, pos.ctypes.data, run.ctypes.data,
                          ovf.ctypes.data, exp.ctypes.data)
        same(bank.play(mx.DeviceBuffer.from_numpy(x)).numpy(), exp, "rms out")
    for got, e, k in ((bank.ring, ring, "ring"), (bank.pos, pos, "pos"), (bank.running, run, "running"), (bank.overflow, ovf, "overflow")):
        same(got.numpy(), e, k)
    assert ovf.sum() == 3 * int((bank.window > cap).sum()) > 0


def test_device_inputs_are_type_checked(mx):
    V, N = 8, 16
    bank = mx.maxiDynamicsBank(V, 64, 64)
    D = mx.DeviceBuffer
    x = D((N, V))
    with pytest.raises(TypeError):
        bank.compress(D((N, V), np.float32), -20, 4, 0)
    with pytest.raises(TypeError):
        bank.sidechainCompress(x, D((N, V), np.int64), -20, 4, 0)
    with pytest.raises(ValueError):
        bank.sidechainCompress(x, D((N - 1, V)), -20, 4, 0)
    with pytest.raises(TypeError):
        bank.compress(x, D(V, np.float32), 4, 0)
    with pytest.raises(ValueError):
        bank.compress(x, -20, D(V + 1), 0)
    with pytest.raises(ValueError):
        bank.setLookAhead([1.0, 2.0])
    rms = mx.maxiRMSBank(V, 32)
    with pytest.raises(TypeError):
        rms.play(D((N, V), np.float32))
    with pytest.raises(ValueError):
        rms.play(D((N, V + 1)))
    import torch
    t = torch.zeros((N, V), dtype=torch.float32, device="cuda")
    with pytest.raises(TypeError):
        bank.compress(t, -20, 4, 0)
    # and a well-formed call with torch tensors runs: the four methods are play() with the reference's argument order
    t64 = torch.full((N, V), 0.5, dtype=torch.float64, device="cuda")
    a = bank.compandAbove(t64, t64, -20.0, 4.0, 0.0).numpy()
    b = mx.maxiDynamicsBank(V, 64, 64).compress(t64, -20.0, 4.0, 0.0).numpy()
    same(a, b, "compandAbove(x, x) == compress(x)")
    c = mx.maxiDynamicsBank(V, 64, 64).compandBelow(t64, t64, -3.0, 2.0, 0.0).numpy()
    d = mx.maxiDynamicsBank(V, 64, 64).play(t64, t64, 0, 0, 0, -3.0, 2.0, 0.0).numpy()
    same(c, d, "compandBelow")
