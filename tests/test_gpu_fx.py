"""GPU: maxiFlangerBank / maxiChorusBank (fx.hip, K11) against the numpy checker tests/fx_port.py and against the
reference's own output tests/golden/fx.npz, bit for bit: outputs, and every carried state (ring phases, LFO phase,
lores x / y, the rings themselves, the overflow counter) after each call."""
import numpy as np
import pytest

import fx_port
from test_fx_cpu import bits_equal, cases, load

pytestmark = pytest.mark.gpu


def params(V, N, rng, short=False, cap=None, ps=False):
    """A mix of regimes per voice: long / short / size 1 / sizes <= 0 / NaN depth; feedback 0..1.2."""
    dl = rng.choice([0, 1, 5, 20, 63, 64, 100, 200] if short else [0, 1, 20, 100, 200, 400], V).astype(np.uint32)
    fb = rng.choice([0.0, 0.5, 0.99, 1.2], V)
    sp = rng.choice([0.2, 1.0, 5.0, 10.0, 11.0, 300.0], V)
    dp = rng.choice([0.0, 0.5, 1.0, 1.5], V)
    dp[::97] = np.nan
    if ps:
        n = np.arange(N)[:, None]
        dl = (dl[None, :] + (n * 3) % 50).astype(np.uint32)
        fb = np.clip(fb[None, :] + 0.0001 * n, 0.0, 1.2)
        sp = sp[None, :] * (1.0 + 0.01 * n)
        dp = np.where(np.isnan(dp), dp, 0.0)[None, :] + 1.5 * ((n * (1 + np.arange(V) % 5)) % 97) / 96.0  # a real ramp 0..1.5
    return dl, fb, sp, dp


def check_flanger_state(bank, f):
    assert bits_equal(bank.memory.numpy()[0], f.ring.mem)
    assert np.array_equal(bank.phase.numpy()[0], f.ring.phase)
    assert bits_equal(bank.lfo_phase.numpy(), f.lfo_phase)
    assert np.array_equal(bank.overflow.numpy(), f.overflow)


def check_chorus_state(bank, c):
    mem, ph, lp = bank.memory.numpy(), bank.phase.numpy(), bank.lp.numpy()
    for r in range(2):
        assert bits_equal(mem[r], c.rings[r].mem)
        assert np.array_equal(ph[r], c.rings[r].phase)
    assert bits_equal(lp[0], c.lx) and bits_equal(lp[1], c.ly)
    assert np.array_equal(bank.overflow.numpy(), c.overflow)


def sl(p, a, b):
    p = np.asarray(p)
    return p[a:b] if p.ndim == 2 else p


@pytest.mark.parametrize("V", [1, 63, 777, 65536])
@pytest.mark.parametrize("N", [1, 7, 64, 515])
def test_flanger_bank_matches_port(mx, V, N):
    rng = np.random.default_rng(V * 1000 + N)
    cap = 256 if V == 65536 else 512
    dl, fb, sp, dp = params(V, N, rng, short=V < 1000)
    bank, f = mx.maxiFlangerBank(V, cap), fx_port.Flanger(V, cap)
    for blk in range(2):
        x = rng.uniform(-1, 1, (N, V))
        y = bank.flange(mx.DeviceBuffer.from_numpy(x), dl, fb, sp, dp).numpy()
        assert bits_equal(y, f.flange(x, dl, fb, sp, dp)), blk
        check_flanger_state(bank, f)


@pytest.mark.parametrize("V", [1, 63, 777, 65536])
@pytest.mark.parametrize("N", [1, 7, 64, 515])
def test_chorus_bank_matches_port(mx, V, N):
    from maximilian_amd.banks import chorus_coeffs
    rng = np.random.default_rng(V * 1000 + N + 7)
    cap = 256 if V == 65536 else 512
    dl, fb, sp, dp = params(V, N, rng, short=V < 1000)
    coef = chorus_coeffs(sp)
    bank, c = mx.maxiChorusBank(V, cap), fx_port.Chorus(V, cap)
    for blk in range(2):
        x = rng.uniform(-1, 1, (N, V))
        rd = rng.integers(0, 2 ** 31 - 1, (N, V), dtype=np.int32)
        y = bank.chorus(mx.DeviceBuffer.from_numpy(x), dl, fb, sp, dp, rd).numpy()
        assert bits_equal(y, c.chorus(x, dl, fb, coef, dp, rd)), blk
        check_chorus_state(bank, c)


@pytest.mark.parametrize("chorus", [False, True])
def test_per_sample_parameters_and_coefficients(mx, chorus):
    from maximilian_amd.banks import chorus_coeffs
    rng = np.random.default_rng(31 + chorus)
    V, N, cap = 300, 200, 400
    dl, fb, sp, dp = params(V, N, rng, short=True, ps=True)
    x = rng.uniform(-1, 1, (N, V))
    if chorus:
        rd = rng.integers(0, 2 ** 31 - 1, (N, V), dtype=np.int32)
        bank, c = mx.maxiChorusBank(V, cap), fx_port.Chorus(V, cap)
        y = bank.chorus(mx.DeviceBuffer.from_numpy(x), dl, fb, sp, dp, rd).numpy()
        assert bits_equal(y, c.chorus(x, dl, fb, chorus_coeffs(sp), dp, rd))
        check_chorus_state(bank, c)
    else:
        bank, f = mx.maxiFlangerBank(V, cap), fx_port.Flanger(V, cap)
        y = bank.flange(mx.DeviceBuffer.from_numpy(x), dl, fb, sp, dp).numpy()
        assert bits_equal(y, f.flange(x, dl, fb, sp, dp))
        check_flanger_state(bank, f)


@pytest.mark.parametrize("name", cases("fl") + cases("ch"))
def test_bank_matches_reference_golden(mx, name):
    from maximilian_amd.banks import chorus_coeffs
    g = load(name)
    N, V = g["in"].shape
    chorus = name.startswith("ch")
    bank = (mx.maxiChorusBank if chorus else mx.maxiFlangerBank)(V, 4096)
    cuts = [0, 333, 397, 1000]  # carried state across uneven blocks
    ys = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        x = mx.DeviceBuffer.from_numpy(g["in"][a:b])
        args = [sl(g[k], a, b) for k in ("delay", "feedback", "speed", "depth")]
        if chorus:
            ys.append(bank.chorus(x, *args, g["rand"][a:b]).numpy())
        else:
            ys.append(bank.flange(x, *args).numpy())
    assert bits_equal(np.concatenate(ys), g["out"])
    assert np.array_equal(bank.phase.numpy()[:2 if chorus else 1].reshape(g["phase"].shape), g["phase"])
    if chorus:
        assert bits_equal(bank.lp.numpy(), g["lp"])
    else:
        assert bits_equal(bank.lfo_phase.numpy(), g["lfo_phase"])
    assert not bank.overflow.numpy().any()
    # the chorus's per-sample coefficient form gives the same bits
    if chorus:
        b2 = mx.maxiChorusBank(V, 4096)
        sp = np.broadcast_to(g["speed"], (N, V)) if np.ndim(g["speed"]) == 1 else g["speed"]
        coef = chorus_coeffs(np.ascontiguousarray(sp))
        y = b2.chorus(mx.DeviceBuffer.from_numpy(g["in"]), g["delay"], g["feedback"], None, g["depth"], g["rand"],
                      coef=coef).numpy()
        assert bits_equal(y, g["out"])


def test_long_carried_stream_65536(mx):
    """>= 16 carried blocks of 512 at 65 536 voices, the large-delay regime with clamping above cap."""
    V, N, cap = 65536, 512, 300
    rng = np.random.default_rng(5)
    dl = rng.choice([100, 200, 250], V).astype(np.uint32)
    fb, sp, dp = rng.uniform(0, 0.99, V), rng.uniform(0.1, 20, V), rng.uniform(0, 1.0, V)
    bank, f = mx.maxiFlangerBank(V, cap), fx_port.Flanger(V, cap)
    for blk in range(16):
        x = rng.uniform(-1, 1, (N, V))
        y = bank.flange(mx.DeviceBuffer.from_numpy(x), dl, fb, sp, dp).numpy()
        assert bits_equal(y, f.flange(x, dl, fb, sp, dp)), blk
    check_flanger_state(bank, f)
    assert f.overflow.any()  # sizes up to 501 against cap 300: clamped, and counted exactly


def test_long_carried_stream_65536_chorus(mx):
    """The chorus's >= 16 carried blocks of 512 at 65 536 voices, per-sample coefficients in half the blocks."""
    from maximilian_amd.banks import chorus_coeffs
    V, N, cap = 65536, 512, 300
    rng = np.random.default_rng(6)
    dl = rng.choice([100, 200, 290], V).astype(np.uint32)
    fb, sp, dp = rng.uniform(0, 0.99, V), rng.uniform(0.1, 20, V), rng.uniform(0, 1.0, V)
    coef = chorus_coeffs(sp)
    bank, c = mx.maxiChorusBank(V, cap), fx_port.Chorus(V, cap)
    for blk in range(16):
        x = rng.uniform(-1, 1, (N, V))
        rd = rng.integers(0, 2 ** 31 - 1, (N, V), dtype=np.int32)
        cps = np.ascontiguousarray(np.broadcast_to(coef, (N, 2, V))) if blk % 2 else coef
        y = bank.chorus(mx.DeviceBuffer.from_numpy(x), dl, fb, None, dp, rd, coef=cps).numpy()
        assert bits_equal(y, c.chorus(x, dl, fb, cps, dp, rd)), blk
    check_chorus_state(bank, c)


def test_device_inputs_are_type_checked(mx):
    import torch
    V, N = 64, 8
    bank = mx.maxiFlangerBank(V, 128)
    x = mx.DeviceBuffer.from_numpy(np.zeros((N, V)))
    with pytest.raises(TypeError):
        bank.flange(x, torch.full((V,), 10, dtype=torch.int64, device="cuda"), 0.5, 1.0, 0.5)
    with pytest.raises(TypeError):
        bank.flange(torch.zeros((N, V), dtype=torch.float32, device="cuda"), 10, 0.5, 1.0, 0.5)
    with pytest.raises(TypeError):
        bank.flange(x, 10, torch.zeros((V, 2), dtype=torch.float64, device="cuda")[:, 0], 1.0, 0.5)
    with pytest.raises(ValueError):
        bank.flange(x, 10, mx.DeviceBuffer.from_numpy(np.zeros(V + 1)), 1.0, 0.5)


def test_state_uploaded_mid_stream_and_streams(mx):
    import torch
    V, N, cap = 500, 300, 256
    rng = np.random.default_rng(77)
    dl, fb, sp, dp = params(V, N, rng, short=True)
    c = fx_port.Chorus(V, cap)
    from maximilian_amd.banks import chorus_coeffs
    coef = chorus_coeffs(sp)
    x0, r0 = rng.uniform(-1, 1, (N, V)), rng.integers(0, 2 ** 31 - 1, (N, V), dtype=np.int32)
    c.chorus(x0, dl, fb, coef, dp, r0)
    s = torch.cuda.Stream()
    bank = mx.maxiChorusBank(V, cap, stream=s.cuda_stream)
    bank.memory.upload(np.stack([r.mem for r in c.rings]))
    bank.phase.upload(np.stack([r.phase for r in c.rings]).astype(np.int32))
    bank.lp.upload(np.stack([c.lx, c.ly]))
    bank.overflow.upload(c.overflow.astype(np.uint32))
    x1, r1 = rng.uniform(-1, 1, (N, V)), rng.integers(0, 2 ** 31 - 1, (N, V), dtype=np.int32)
    xt = torch.from_numpy(x1).cuda()
    torch.cuda.synchronize()
    y = bank.chorus(xt, dl, fb, sp, dp, r1).numpy()
    assert bits_equal(y, c.chorus(x1, dl, fb, coef, dp, r1))
    check_chorus_state(bank, c)
    # the flanger on the library's default stream (NULL), state uploaded mid-stream
    f = fx_port.Flanger(V, cap)
    f.flange(x0, dl, fb, sp, dp)
    fb_ = mx.maxiFlangerBank(V, cap, stream=None)
    fb_.memory.upload(f.ring.mem[None])
    fb_.phase.upload(f.ring.phase[None].astype(np.int32))
    fb_.lfo_phase.upload(f.lfo_phase)
    fb_.overflow.upload(f.overflow.astype(np.uint32))
    y = fb_.flange(mx.DeviceBuffer.from_numpy(x1), dl, fb, sp, dp).numpy()
    assert bits_equal(y, f.flange(x1, dl, fb, sp, dp))
    check_flanger_state(fb_, f)
