"""GPU: mxg_drum_render / mxg_clock_render (kernel K21) and the drum and clock banks against tests/golden/drums.npz under the
numerics contract (tests/drums_host.py check_case): snare, hats, the clock and every state row BIT FOR BIT (the kick's filter
state excepted), the kick's output under its derived bound.  Each drum x variant x rate through the C-ABI at V in {1, 63, 64, 65,
130} -- surplus lanes, odd V, pair rows, more than one wavefront -- with the recorded voice on the even voices and a second
parameter set on the odd ones, which is checked against mxg_drum_host; the 1200 samples cut into blocks of 1, 7, 8, 9 and 512 over
and over (shorter than a chunk, ragged last chunks, many chunks) plus the stored cuts, where the carried state must equal the
recorded rows; one shared trigger signal and one per voice.  The clock bank alone, clock -> drum chained on the device, the two
denormal cases, the Python banks.  d_out and every state array sit in a guard band of NaN bit patterns that must come back
untouched (drums_host.GpuBackend checks it on every call).

Measured on an MI355X (the printout of test_case_through_the_cabi): see DESIGN.md section 4."""
import itertools

import numpy as np
import pytest

import drums_host as dh

pytestmark = pytest.mark.gpu

VS = (1, 63, 64, 65, 130)
BLOCKS = (1, 7, 8, 9, 512)
CUTS = tuple(c for c in itertools.accumulate(itertools.islice(itertools.cycle(BLOCKS), 12)) if c < dh.N)
# the odd voices' parameters (the kick's second set moves the pitch alone: its bound does not depend on the pitch)
SECOND = {"kick": dict(pitch=433.7), "snare": dict(pitch=1234.5, release=9, distortion=1.25, cutoff=1777.0, resonance=5.0, gain=0.8),
          "hats": dict(pitch=9876.5, release=5, distortion=0.7, gain=1.3, svf=(5100.0, 3.0))}


@pytest.fixture(scope="module")
def g(golden):
    return golden("drums.npz")


@pytest.fixture(scope="module")
def be(mx):
    return dh.GpuBackend(mx)


@pytest.fixture(scope="module")
def host():
    return dh.HostBackend()


def second_set(L, kind, variant, V):
    c, ct = dict(dh.CASES[(kind, variant)]), dh.CTOR[kind]
    c.update(SECOND[kind])
    return dh.Params(L, kind, ct[4] if c["pitch"] is None else c["pitch"], ct[0], ct[1] if c["decay"] is None else c["decay"], ct[2],
                     c["release"], c["distortion"], c["cutoff"], c["resonance"], c["gain"], dh.flags_of(kind, variant), c["svf"], V)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("kind", dh.KINDS)
def test_case_through_the_cabi(be, host, g, kind, V):
    worst = {}
    for sr, variant, tpv in itertools.product(dh.RATES, dh.VARIANTS, (0, 1)):
        with dh.at_rate(be.L, sr):
            odd = second_set(be.L, kind, variant, V) if V > 1 else None
            out, states = dh.play_case(be, g, kind, variant, sr, cuts=CUTS, V=V, tpv=tpv, odd=odd)
            what = "V=%d tpv=%d" % (V, tpv)
            for v in sorted({0, (V - 1) & ~1}):   # the first and the last voice that carries the recorded parameters
                r = dh.check_case(be.L, g, kind, variant, sr, out, states, what, v=v)
            if r:
                worst[dh.key(kind, variant, sr)] = r
            dh.bits_equal(out[:, 0::2], np.repeat(out[:, :1], (V + 1) // 2, 1), what + ": the even voices are one voice")
            if odd is not None:
                exp, est = dh.play_case(host, g, kind, variant, sr, cuts=CUTS, V=V, tpv=tpv, odd=odd)
                if kind == "kick":
                    env = dh.unshuffle(g["envout/" + dh.key(kind, variant, sr)], (dh.N,))
                    bound = dh.kick_bound(be.L, variant, env)
                    err = np.abs(out[:, 1::2] - exp[:, 1::2])
                    ok = err <= bound[:, None]   # (or one side of the limiter each, both within the bound of +-1: at most 1 % of the case)
                    near = ~ok & (np.abs(np.abs(out[:, 1::2]) - 1) <= bound[:, None]) & (np.abs(np.abs(exp[:, 1::2]) - 1) <= bound[:, None])
                    assert (ok | near).all() and near.sum() <= 0.01 * near.size, what
                    rows = [0, 1, 2]
                else:
                    dh.bits_equal(out[:, 1::2], exp[:, 1::2], what + " odd voices against mxg_drum_host")
                    rows = [0, 1, 2, 3]
                for c in est:
                    for r_ in rows[:3]:
                        dh.bits_equal(states[c][r_][..., 1::2].astype(np.float64), est[c][r_][..., 1::2].astype(np.float64), "%s odd state %d at %d" % (what, r_, c))
                    if kind != "kick":
                        dh.bits_equal(states[c][3][..., 1::2], est[c][3][..., 1::2], "%s odd filter state at %d" % (what, c))
    if worst:
        print("kick, measured (worst error, bound there, samples within the bound of +-1):", worst)


@pytest.mark.parametrize("rw", [2, 3, 4])
def test_pair_row_stores_give_the_same_bits(mx, be, g, rw):
    """Knob rw_store: the 16-byte pair rows (plain / write-through / non-temporal) on an even bank, against the stored reference."""
    L = mx.lib()
    prev = L.mxg_tune(b"rw_store", rw)
    try:
        for kind in dh.KINDS:
            for V in (2, 130):
                out, states = dh.play_case(be, g, kind, "full", 44100, cuts=CUTS, V=V, tpv=1)
                dh.check_case(be.L, g, kind, "full", 44100, out, states, "rw_store=%d V=%d" % (rw, V), v=V - 1)
    finally:
        L.mxg_tune(b"rw_store", prev)


def test_no_trigger_block_is_silence(be):
    for kind in ("kick", "hats"):
        p = dh.Params.of_case(be.L, kind, "plain", 65)
        rnd = None if kind == "kick" else np.full((17, 65), 1234567, np.int32)
        out, st = be.render(p, None, rnd, dh.fresh_state(65), n=17)
        assert (out == 0).all() and (st[1] == 0).all()


def test_denormal_amplitudes_survive(be):
    dh.denormal_cases(be)


@pytest.mark.parametrize("V", (1, 65))
def test_clock_alone(be, g, V):
    for sr in dh.RATES:
        with dh.at_rate(be.L, sr):
            for last in (0, 1):
                cuts = (0,) + CUTS + (dh.N,)
                clk, ph, ticks = np.zeros(V), np.zeros(V, np.int64), []
                for a, b in zip(cuts[:-1], cuts[1:]):
                    t, clk, ph, cnt = be.clock(np.full(V, 600.0), clk, np.full(V, last, np.int32), ph, b - a)
                    ticks.append(t)
                    dh.bits_equal(clk, np.full(V, g["clock/%d/%d/phase" % (sr, last)][b - 1]), "clock phase at %d" % b)
                tick = np.concatenate(ticks)
                assert (tick == tick[:, :1]).all() and (ph == ph[0]).all() and (cnt == cnt[0]).all()
                dh.check_clock(g, sr, last, tick, ph[0], cnt[0])


def test_clock_into_drum_on_the_device(mx, host):
    """maxiClockBank's tick block is the kick bank's trigger block, device to device; against the two host calls."""
    V, N = 65, 600
    clock, kick, hats = mx.maxiClockBank(V), mx.maxiKickBank(V), mx.maxiHatsBank(V)
    clock.setTicksPerBeat(4)
    clock.setTempo(np.linspace(6000.0, 12000.0, V))
    for b in (kick, hats):
        b.setRelease(4)
    draws = np.random.default_rng(5).integers(0, 2 ** 31 - 1, (N, V)).astype(np.int32)
    tick = clock.render(N)
    ok, oh = kick.render(N, trig=tick).numpy(), hats.render(N, trig=tick, rand=draws).numpy()
    et, eclk, eph, ecnt = host.clock(clock.bps, np.zeros(V), None, np.zeros(V, np.int64), N)
    assert np.array_equal(tick.numpy(), et) and et.sum() > 3 * V
    assert np.array_equal(clock.playHead.numpy(), eph) and np.array_equal(clock.currentCount.numpy(), ecnt)
    dh.bits_equal(clock.clk.numpy(), eclk, "clock phase")
    ph = dh.Params.of_case(host.L, "hats", "plain", V)
    ph.par[:] = hats.env
    eh, _ = host.render(ph, et, draws, dh.fresh_state(V))
    dh.bits_equal(oh, eh, "hats after the clock")
    pk = dh.Params.of_case(host.L, "kick", "plain", V)
    pk.par[:] = kick.env
    ek, _ = host.render(pk, et, None, dh.fresh_state(V))
    assert np.abs(ok - ek).max() <= 2.0 ** -52 and np.abs(ok).max() > 0.5   # (the kick's bound with every switch off: one sine, two roundings)


@pytest.mark.parametrize("kind", dh.KINDS)
def test_python_bank(mx, g, kind):
    """The bank classes: the reference's setters in the reference's units, the state carried from call to call."""
    cls = {"kick": mx.maxiKickBank, "snare": mx.maxiSnareBank, "hats": mx.maxiHatsBank}[kind]
    L = mx.lib()
    for variant in dh.VARIANTS:
        c, fl = dh.CASES[(kind, variant)], dh.flags_of(kind, variant)
        bank = cls(3)
        assert bank.useFilter == (kind == "snare")
        bank.setRelease(c["release"])
        if c["decay"] is not None:
            bank.setDecay(c["decay"])
        if c["pitch"] is not None:
            bank.setPitch(c["pitch"])
        bank.setDistortion(c["distortion"]), bank.setCutoff(c["cutoff"]), bank.setResonance(c["resonance"]), bank.setGain(c["gain"])
        if c["svf"]:
            bank.setFilterCutoff(c["svf"][0]), bank.setFilterResonance(c["svf"][1])
        bank.inverse, bank.useDistortion, bank.useFilter, bank.useLimiter = (bool(fl & b) for b in (1, 2, 4, 8))
        tr, out, states = dh.triggers(), np.zeros((dh.N, 3)), {}
        draws = None if kind == "kick" else np.repeat(g["draws"][:, None], 3, 1)
        for a, b in zip(dh.CUTS[:-1], dh.CUTS[1:]):
            states[a] = [bank.phase.numpy(), bank.dstate.numpy(), bank.istate.numpy(), bank.fstate.numpy()]
            out[a:b] = bank.render(b - a, trig=tr[a:b], rand=None if draws is None else draws[a:b]).numpy()
        states[dh.N] = [bank.phase.numpy(), bank.dstate.numpy(), bank.istate.numpy(), bank.fstate.numpy()]
        dh.check_case(L, g, kind, variant, 44100, out, states, "bank", v=2)
    if kind != "kick":
        with pytest.raises(mx.MaxiGpuError):
            cls(3).render(8)   # snare and hats need the draws


def test_facade_drums_smoke():
    """host/facade_drums_smoke: the C++ banks of include/maximilian_bank.hpp, clock -> drums, against the host arithmetic."""
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "host", "facade_drums_smoke")
    if not os.path.exists(exe):
        pytest.fail("host/facade_drums_smoke is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
