"""GPU: kernel K15 (seq.hip) through mxg_seq_render and mxg_seq_signal, BIT FOR BIT everywhere -- compares, + - / floor and
indexing have no tolerance.

  * every case of tests/golden/seq.npz (the reference's own triggers, values, gates and state snapshots) through both entry
    points, with the blocks cut as stored and cut at (1, 7, 9, 513) as well; the carried state equals the snapshots;
  * the internal clock's phase equals mxg_osc_render(MXG_OSC_PHASOR) on the same frequencies;
  * random banks against the host build of mxg_seq.h (tests/host_seq.cpp, pinned to the golden file by tests/test_seq_host.py;
    the reference is not on the GPU machine) over V in {1, 2, 63, 64, 65, 130, 1000} x N in {1, 7, 8, 9, 512, 513} -- the lane,
    pair-row and chunk edges -- with per-voice pattern and value-list selection, every subset of the three outputs, the three
    clock forms, both value modes, and the 16-byte pair-row stores forced on (knob rw_store);
  * an output that is not asked for leaves its stage's state bytes alone;
  * the chain mxg_seq_render -> mxg_envgen_render(tpv = 1) -> mxg_osc_render(MXG_OSC_SAW, fps = 1, d_freq = d_val) over 1000
    voices x 3 blocks of 512 with no host array uploaded per block, against the same chain per voice on the host; its voice 0
    is the second channel of tests/patches/seq_patch.cpp as the reference plays it."""
import itertools

import numpy as np
import pytest

import seq_host
from seq_host import assert_same

pytestmark = pytest.mark.gpu

GPU_CUTS = (1, 7, 9, 513)
VS = [1, 2, 63, 64, 65, 130, 1000]
NS = [1, 7, 8, 9, 512, 513]
SUBSETS = [s for s in itertools.product([False, True], repeat=3) if any(s)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return seq_host.HostBackend(seq_host.build(tmp_path_factory.mktemp("seq")))


@pytest.fixture(scope="module")
def gpu(mx):
    return seq_host.GpuBackend(mx)


@pytest.fixture(scope="module")
def g(golden):
    return golden("seq.npz")


@pytest.mark.parametrize("extra", [(), GPU_CUTS])
@pytest.mark.parametrize("name", seq_host.FUSED_CASES)
def test_golden_fused(gpu, g, name, extra):
    c = seq_host.load_case(g, name)
    trig, val, gate, states = seq_host.play_fused(gpu, c, extra)
    seq_host.check_fused(c, name, trig, val, gate, states)


@pytest.mark.parametrize("extra", [(), GPU_CUTS])
@pytest.mark.parametrize("kind", sorted(seq_host.KIND_NAMES))
def test_golden_signal(gpu, g, kind, extra):
    out, states = seq_host.play_signal(gpu, g, kind, extra)
    seq_host.check_signal(g, kind, out, states)


def test_internal_clock_is_the_phasor_render(mx):
    """d_clk after every block = maxiOscBank.phase after render('phasor') on the same frequencies; the triggers of the internal
    clock = the triggers of the external form fed with that render's output."""
    V = 130
    rng = np.random.default_rng(150)
    freq = rng.uniform(0.0, 3000.0, V)
    freq[:3] = [0.0, 22050.0, 441.0]
    times = [[3, 3, 2], [4, 4, 4, 1, 1, 1, 1]]
    a, b = mx.maxiSeqBank(V, times=times), mx.maxiSeqBank(V, times=times)
    sel = rng.integers(0, 2, V)
    a.setPattern(sel)
    b.setPattern(sel)
    osc = mx.maxiOscBank(V)
    fired = 0
    for N in (7, 512, 9, 513):
        ta, _, _ = a.render(N, freq=freq)
        ph = osc.render("phasor", freq, N)
        tb, _, _ = b.render(N, phase=ph)
        assert_same(a.clock.numpy(), osc.phase.numpy(), "clock phase after %d" % N)
        assert_same(ta.numpy(), tb.numpy(), "internal against external clock")
        assert_same(a.dstate.numpy(), b.dstate.numpy(), "state")
        fired += int(ta.numpy().sum())
    assert fired > 100


def random_bank(rng, V):
    """Tables and per-voice selections that use every row; one pattern of 64 ratios, a zero ratio, a zero sum."""
    pats = [[3, 3, 2], [1], [4, 4, 4, 1, 1, 1, 1], list(rng.uniform(0.0, 5.0, 64)), [2, 0, 1, 0.001, 1], [0, 0]]
    times, plen = seq_host.table(pats, 64)
    vals, vlen = seq_host.table([[440.0], [40.0, 80.0, 170.0], list(rng.uniform(20.0, 4000.0, 6)), list(rng.uniform(20.0, 4000.0, 10))], 10)
    d = dict(norm=seq_host.ratio_tables(times, plen), plen=plen, values=vals, vlen=vlen,
             pat=rng.integers(0, len(pats), V).astype(np.int32), vpat=rng.integers(0, 4, V).astype(np.int32),
             freq=rng.uniform(20.0, 9000.0, V), hold=rng.choice([0.0, 1.0, 2.5, 7.0, 300.0], V))
    d["pat"][0] = 0  # voice 0 always carries a pattern that fires ({0, 0} never does): the tests' "something fired" checks hold for V = 1
    n = vlen[d["vpat"]].astype(np.float64)
    d["step"] = np.choose(rng.integers(0, 6, V), [np.ones(V), 2 * np.ones(V), -np.ones(V), 0.5 * np.ones(V), n + 3, -n])
    return d


def run_random(be, d, V, blocks, phases, subset, clock, mode):
    dst, ist = seq_host.fresh_seq(V)
    clk = np.zeros(V)
    outs, a = [], 0
    for N in blocks:
        ph = None if clock == 0 else (phases[a:a + N] if clock == 1 else np.ascontiguousarray(phases[a:a + N, 0]))
        outs.append(be.render(44100, V, N, d["freq"] if clock == 0 else None, clk, ph, d["norm"], d["plen"], d["pat"], mode, d["values"],
                              d["vlen"], d["vpat"], d["step"], d["hold"], dst, ist, subset))
        a += N
    return outs, dst, ist, clk


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("V", VS)
def test_random_banks_against_host_build(gpu, host, V, N):
    rng = np.random.default_rng(1000 * V + N)
    d = random_bank(rng, V)
    blocks = (N, 9, N)
    total = sum(blocks)
    # external phases: phasors with wraps, a few voices with noise and values outside [0, 1]
    phases = (rng.uniform(0, 1, V)[None, :] + np.arange(total)[:, None] * rng.uniform(0.001, 0.3, V)[None, :]) % 1.0
    phases[:, ::7] = rng.uniform(-0.2, 1.2, (total, len(range(0, V, 7))))
    fired = 0
    for k, subset in enumerate(SUBSETS):
        clock, mode = k % 3, (k // 2) % 2
        got, gd, gi, gc = run_random(gpu, d, V, blocks, phases, subset, clock, mode)
        exp, ed, ei, ec = run_random(host, d, V, blocks, phases, subset, clock, mode)
        what = "V %d N %d outputs %s clock %d mode %d" % (V, N, subset, clock, mode)
        for gb, eb in zip(got, exp):
            for o, e, nm in zip(gb, eb, ("trig", "val", "gate")):
                assert (o is None) == (e is None)
                if o is not None:
                    assert_same(o, e, what + " " + nm)
                    fired += int(nm == "trig") * int(e.sum())
        assert_same(gd, ed, what + " dst")
        assert_same(gi, ei, what + " ist")
        assert_same(gc, ec, what + " clk")
    if V * N >= 500:
        assert fired > 0
    # the signal kinds on the same shape, two blocks
    trig = (rng.uniform(0, 1, (2 * N, V)) < 0.3).astype(np.float64)
    second = rng.uniform(-0.3, 1.3, (2 * N, V))
    for kind in sorted(seq_host.KIND_NAMES):
        res = []
        for be in (gpu, host):
            dst, ist = seq_host.fresh_sig(kind, V)
            tab = kind in (seq_host.STEP, seq_host.INDEX)
            par = d["step"] if kind == seq_host.STEP else (d["hold"] if kind == seq_host.ZXTOPULSE else None)
            a = second - 0.5 if kind == seq_host.ONZX else trig
            b = second if kind == seq_host.INDEX else (second - 0.5 if kind == seq_host.COUNTER else None)
            out = [be.signal(kind, V, N, a[i * N:(i + 1) * N], None if b is None else b[i * N:(i + 1) * N], d["values"] if tab else None,
                             d["vlen"] if tab else None, d["vpat"] if tab else None, par, dst, ist) for i in range(2)]
            res.append((np.concatenate(out), dst, ist))
        for x, y, nm in zip(res[0], res[1], ("out", "dst", "ist")):
            assert_same(x, y, "signal %s V %d N %d %s" % (seq_host.KIND_NAMES[kind], V, N, nm))


@pytest.mark.parametrize("knob", [2, 3, 4])
def test_pair_row_stores(mx, gpu, host, knob):
    """rw_store 2 / 3 / 4 = 16-byte pair rows with plain / write-through / non-temporal stores (automatic only from 64 MB blocks):
    the same bits, for even banks whose last wavefront is partly shadow lanes, with whole and ragged chunks."""
    lib = mx.lib()
    mx._lib.check(lib.mxg_tune(b"rw_store", knob), "mxg_tune")
    try:
        for V, N in ((2, 9), (64, 8), (130, 513), (1000, 16)):
            rng = np.random.default_rng(77 * V + N + knob)
            d = random_bank(rng, V)
            phases = (rng.uniform(0, 1, V)[None, :] + np.arange(N)[:, None] * rng.uniform(0.001, 0.3, V)[None, :]) % 1.0
            for clock, mode in ((0, 0), (1, 1), (2, 0)):
                got, gd, gi, gc = run_random(gpu, d, V, (N,), phases, (True, True, True), clock, mode)
                exp, ed, ei, ec = run_random(host, d, V, (N,), phases, (True, True, True), clock, mode)
                for o, e, nm in zip(got[0], exp[0], ("trig", "val", "gate")):
                    assert_same(o, e, "pair rows %d V %d N %d clock %d %s" % (knob, V, N, clock, nm))
                assert_same(gd, ed, "dst")
                assert_same(gi, ei, "ist")
            trig = (rng.uniform(0, 1, (N, V)) < 0.3).astype(np.float64)
            res = []
            for be in (gpu, host):
                dst, ist = seq_host.fresh_sig(seq_host.STEP, V)
                res.append(be.signal(seq_host.STEP, V, N, trig, None, d["values"], d["vlen"], d["vpat"], d["step"], dst, ist))
            assert_same(res[0], res[1], "pair rows %d signal V %d N %d" % (knob, V, N))
    finally:
        mx._lib.check(lib.mxg_tune(b"rw_store", 0), "mxg_tune")


def test_null_output_leaves_state_bytes(mx):
    V, N = 65, 100
    rng = np.random.default_rng(3)
    bank = mx.maxiSeqBank(V, times=[[3, 3, 2], [1]], values=[[1.0, 2.0, 3.0], [5.0, 6.0]])
    bank.setPattern(rng.integers(0, 2, V))
    bank.setValueList(rng.integers(0, 2, V))
    bank.setHold(3.0)
    freq = rng.uniform(500.0, 5000.0, V)
    # recognisable bytes in every state row, then renders that leave stages out
    d0 = rng.uniform(-1, 1, (5, V))
    i0 = rng.integers(0, 2, (6, V)).astype(np.int64)
    i0[1] = rng.integers(0, 2, V)
    i0[2] = rng.integers(2, 4, V)
    for kw, drows, irows in ((dict(trig=True), [0], [0]),
                             (dict(trig=False, val="values"), [0], [0, 1, 2]),
                             (dict(trig=False, val="step"), [0, 1, 2], [0, 3, 4]),
                             (dict(trig=False, gate=True), [0, 3, 4], [0, 5])):
        bank.dstate.upload(d0)
        bank.istate.upload(i0)
        bank.render(N, freq=freq, **kw)
        d1, i1 = bank.dstate.numpy(), bank.istate.numpy()
        for r in range(5):
            if r not in drows:
                assert d1[r].tobytes() == d0[r].tobytes(), (kw, "dst row", r)
        for r in range(6):
            if r not in irows:
                assert i1[r].tobytes() == i0[r].tobytes(), (kw, "ist row", r)
        assert d1[0].tobytes() != d0[0].tobytes()  # playTrig always runs


def test_gpu_seq_chain(mx, host, g, tmp_path_factory):
    """mxg_seq_render -> mxg_envgen_render(tpv = 1) -> mxg_osc_render(MXG_OSC_SAW, fps = 1, d_freq = d_val): 1000 voices x 3 blocks
    of 512, every block handed on as a device array."""
    V, N, B = 1000, 512, 3
    E = seq_host.build_envgen(tmp_path_factory.mktemp("eg"))
    rng = np.random.default_rng(47)
    times = [[4, 4, 4, 1, 1, 1, 1], [3, 3, 2], [1], [33, 991, 13, 153]]
    values = [[40.0, 80.0, 170.0, 350.0, 900.0, 3888.0], [110.0, 220.0, 330.0], [55.0]]
    pat, vpat = rng.integers(0, 4, V).astype(np.int32), rng.integers(0, 3, V).astype(np.int32)
    freq, step = rng.uniform(20.0, 400.0, V), rng.choice([1.0, 2.0, -1.0, 0.5], V)
    pat[0], vpat[0], freq[0], step[0] = 0, 0, 47.0, 1.0          # voice 0 = channel 1 of tests/patches/seq_patch.cpp
    levels, ms, curves = [0, 1, 0.2, 0], [5, 4, 2], [1, 1, 1]
    seq = mx.maxiSeqBank(V, times=times, values=values)
    seq.setPattern(pat)
    seq.setValueList(vpat)
    seq.setStep(step)
    env = mx.maxiEnvGenBank(V)
    assert env.setup(levels, ms, curves, False, True)
    osc = mx.maxiOscBank(V)
    dfreq = mx.DeviceBuffer.from_numpy(freq)                     # uploaded once; nothing goes up per block
    got_e, got_o = [], []
    for _ in range(B):
        t, x, _ = seq.render(N, freq=dfreq, val="step")
        e = env.play(t)
        o = osc.render("saw", x, N, per_sample=True)
        got_e.append(e.numpy())
        got_o.append(o.numpy())
    got_e, got_o = np.concatenate(got_e), np.concatenate(got_o)
    # the same chain on the host, per voice
    tv, plen = seq_host.table(times, 7)
    vals, vlen = seq_host.table(values, 6)
    assert tv.shape == seq.host_norm.shape
    norm = seq_host.ratio_tables(tv, plen)
    dst, ist = seq_host.fresh_seq(V)
    clk = np.zeros(V)
    t, x, _ = host.render(44100, V, N * B, freq, clk, None, norm, plen, pat, 1, vals, vlen, vpat, step, None, dst, ist, (True, True, False))
    ed, ei = np.zeros((5, V)), np.zeros((7, V), np.int64)
    ed[2:5] = 1.0
    ei[4:7] = 1
    exp_e = np.zeros((N * B, V))
    st = env.host_stages
    E.envgen_host(V, N * B, t.ctypes.data, 1, st.ctypes.data, st.shape[0], 0, 1, ed.ctypes.data, ei.ctypes.data, exp_e.ctypes.data, 0)
    exp_o, ph = np.zeros((N * B, V)), np.zeros(V)
    host.L.seq_host_saw(44100.0, V, N * B, x.ctypes.data, ph.ctypes.data, exp_o.ctypes.data)
    assert t.sum() > 3 * V and len(np.unique(x)) >= 8 and exp_e.max() == 1.0
    assert_same(got_e, exp_e, "envelope leg")
    assert_same(got_o, exp_o, "oscillator leg")
    assert_same(seq.clock.numpy(), clk, "clock")
    assert_same(osc.phase.numpy(), ph, "oscillator phase")
    # voice 0 against the reference's own stream of the patch
    patch = g["patch"][:N * B, 1]
    assert (patch != 0).mean() > 0.3
    assert_same(got_e[:, 0] * got_o[:, 0], patch, "voice 0 = envelope * oscillator of the patch, as the reference plays it")
