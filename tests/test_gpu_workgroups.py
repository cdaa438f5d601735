"""GPU: every "one lane = one voice" kernel at every workgroup size voice_block() (csrc/mxg_stream.h) can give it.

The knob voice_block takes multiples of 64 and is capped at 256, so these kernels run with 64, 128, 192 or 256 lanes per
workgroup; the small64 families (polyblep, drums, clock, line, analysis) are held at 64 lanes up to 16 384 voices.  What differs
between those sizes is the delicate part: LDS tables staged with a blockDim.x stride in front of a barrier, whole surplus
wavefronts returned after it (bank_wave_idle), shadow lanes and shadow pairs beside full or idle wavefronts, the per-wavefront
LDS windows and part counters of sample.hip, the pair parity taken from threadIdx.x.

  Part A  the small64 kernels with several wavefronts per workgroup: V in {16 385, 16 514} x voice_block in {128, 192, 256}
          (the rule cannot be switched off below 16 385 voices).
  Part B  the other per-voice kernels at voice_block in {64, 128, 192} (256 is what every other test runs) x V in {1, 65, 130,
          193, 386}: 193 = 192 + 1, 386 = 2 * 192 + 2, 130 puts two live lanes into a third wavefront.

Every case: each voice has its own parameters, drawn from a seeded generator (a bank of repeated voices is invisible to a shift
by a whole number of periods); two carried blocks of 9 and 16 samples (a whole chunk and a ragged one, then whole chunks); the
output AND every state array compared after each block; output and state inside guard bands of 64 NaN patterns that must come back
untouched; rw_store 0 (automatic: 8-byte stores at these sizes) and, for even V, 2 (pair rows).  The expectation is always the
reference side -- the plain-C port for the core families, the host build of the shared header for the others -- under each
family's existing contract: bit for bit, except the polyblep sine waveforms (polyblep_host.check_against), the kick's output and
filter state (drums_host.kick_bound) and the fused voice's mode B (1e-11 of the voice's peak, as tests/test_gpu_voice.py).
No GPU run is compared with another GPU run.  Before the launches of each knob setting the LDS of every compute unit is overwritten
with NaNs (scrub_lds): a table staged short would otherwise be completed by what an earlier launch left at the same addresses."""
import contextlib

import numpy as np
import pytest

import analysis_host as ah
import drums_host as dh
import polyblep_host as ph
import seq_host as sq
import shaper_host as sh
from conftest import assert_bits_equal, assert_close_scaled
from maximilian_amd import banks

pytestmark = pytest.mark.gpu

CUTS = ((0, 9), (9, 25))   # two carried blocks, of 9 then 16 samples
TOTAL = 25
A_SHAPES = [(V, vb) for V in (16385, 16514) for vb in (128, 192, 256)]
B_SHAPES = [(V, vb) for V in (1, 65, 130, 193, 386) for vb in (64, 128, 192)]
GUARD = 64
PAT = np.uint64(0x7FF8DEADBEEF0001)
MOD_FILTER_RTOL = 1e-11   # the fused voice's mode B (tests/test_gpu_voice.py, DESIGN.md "Numerics")
ENVGEN_HOLD = -46692.0

_expected = {}


def cached(key, make):
    """The expectation of a case: computed once, shared by every workgroup size and store flavour, never written to."""
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


def stores(V):
    return (0, 2) if V % 2 == 0 else (0,)


@contextlib.contextmanager
def knobs(L, **kv):
    """mxg_tune inside try / finally; every knob goes back to the value mxg_tune returned."""
    prev = []
    try:
        for k, v in kv.items():
            p = L.mxg_tune(k.encode(), v)
            assert p >= 0, "mxg_tune(%s, %d) was refused" % (k, v)
            prev.append((k, p))
        yield
    finally:
        for k, p in reversed(prev):
            L.mxg_tune(k.encode(), p)


class Guarded:
    """A device array the kernel writes, between two bands of GUARD NaN patterns (and padded to whole doubles)."""

    def __init__(self, mx, a):
        self.like = np.ascontiguousarray(a)
        raw = self.like.reshape(-1).view(np.uint8)
        self.pad = (-raw.size) % 8
        band = np.full(GUARD, PAT, np.uint64).view(np.uint8)
        self.buf = mx.DeviceBuffer.from_numpy(np.concatenate([band, raw, np.full(self.pad, 0xA5, np.uint8), band]))
        self.ptr = self.buf.ptr + GUARD * 8

    def back(self, what):
        raw, n, g8 = self.buf.numpy().reshape(-1), self.like.nbytes, GUARD * 8
        assert (raw[:g8].view(np.uint64) == PAT).all(), "the guard band in front of %s was written" % what
        assert (raw[g8 + n:g8 + n + self.pad] == 0xA5).all() and (raw[g8 + n + self.pad:].view(np.uint64) == PAT).all(), \
            "the guard band behind %s was written" % what
        return raw[g8:g8 + n].copy().view(self.like.dtype).reshape(self.like.shape)


class Dev:
    """The device arrays of one call: plain inputs and guarded in / out arrays, kept alive until the results are back."""

    def __init__(self, mx):
        self.mx, self.keep = mx, []

    def inp(self, a, dtype=np.float64):
        if a is None:
            return None
        self.keep.append(self.mx.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype)))
        return self.keep[-1].ptr

    def io(self, a):
        if a is None:
            return None
        self.keep.append(Guarded(self.mx, a))
        return self.keep[-1]

    def out(self, n, V):
        return self.io(np.full((n, V), -7.5))

    def call(self, fn, *args):
        L = self.mx.lib()
        st = fn(*[a.ptr if isinstance(a, Guarded) else a for a in args])
        assert st == 0, L.mxg_last_error()
        self.mx._lib.check(L.mxg_stream_sync(None), "mxg_stream_sync")


SCRUB_V, SCRUB_L = 262144, 6000


def scrub_lds(mx):
    """Fills the first 48 KB of every compute unit's LDS with NaNs: mxg_seq_signal stages a value table of 6000 NaNs per workgroup,
    over enough workgroups to visit every compute unit several times.  A table that a kernel under test stages short would
    otherwise be completed by what the previous launch left at the same LDS addresses -- the same table, staged whole at another
    workgroup size -- and pass.  Nothing is read back."""
    def make():
        D = mx.DeviceBuffer
        dst, ist = sq.fresh_sig(sq.STEP, SCRUB_V)
        return dict(x=D((1, SCRUB_V)), out=D((1, SCRUB_V)), values=D.from_numpy(np.full((1, SCRUB_L), np.nan)),
                    vlen=D.from_numpy(np.array([SCRUB_L], np.int32)), dst=D.from_numpy(dst), ist=D.from_numpy(ist))
    b, L = cached("scrub", make), mx.lib()
    st = L.mxg_seq_signal(sq.STEP, SCRUB_V, 1, b["x"].ptr, None, b["values"].ptr, b["vlen"].ptr, 1, SCRUB_L, None, None, b["dst"].ptr,
                          b["ist"].ptr, b["out"].ptr, None)
    assert st == 0, L.mxg_last_error()
    mx._lib.check(L.mxg_stream_sync(None), "mxg_stream_sync")


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float64:
        assert_bits_equal(a, b, what)
    else:
        assert np.array_equal(a, b), what


# =====================================================================================================================
# Part A: the small64 kernels above 16 384 voices
# =====================================================================================================================
PB_SR = 1000.0


def pb_case(V):
    """A sixth of the voices at or above sr / 4 (the sine fallback, whatever the waveform), two fifths running backwards, pulse
    widths over [0, 1] with both ends present, phases anywhere in [0, 1)."""
    rng = np.random.default_rng(7000 + V)
    f0 = rng.uniform(-300.0, 300.0, V)
    f = f0[None, :] * rng.uniform(0.8, 1.2, (TOTAL, V))
    pw = rng.uniform(0.0, 1.0, V)
    pw[rng.integers(0, V, 16)] = 0.0
    pw[rng.integers(0, V, 16)] = 1.0
    t0 = rng.uniform(0.0, 1.0, V)
    host, exp = ph.HostBackend(), {}
    for wf in ph.WAVEFORMS:
        for fps in (0, 1):
            t, blocks = t0, []
            for a, b in CUTS:
                o, t = host.render(wf, f[a:b] if fps else f0, pw, PB_SR, t, n=b - a)
                blocks.append((o, t))
            exp[wf, fps] = blocks
    assert ph.fallback(f0, PB_SR).sum() > V // 16 and len(np.unique(exp["SINE", 1][1][0])) > V
    return dict(f0=f0, f=f, pw=pw, t0=t0, exp=exp)


@pytest.mark.parametrize("V,vb", A_SHAPES)
def test_polyblep(mx, V, vb):
    """mxg_polyblep_render, fps 0 and 1, every waveform: the arithmetic ones bit for bit, SINE / COSINE and every fallback sample
    within 1 ULP, the rectified sines within 2^-50 -- all three groups read the 16 KB LDS table staged by the whole workgroup."""
    c = cached(("polyblep", V), lambda: pb_case(V))
    be, L = ph.GpuBackend(mx), mx.lib()
    for rw in stores(V):
        with knobs(L, voice_block=vb, rw_store=rw):
            scrub_lds(mx)
            for (wf, fps), blocks in c["exp"].items():
                t = c["t0"]
                for (a, b), (eo, et) in zip(CUTS, blocks):
                    fr = c["f"][a:b] if fps else c["f0"]
                    o, t = be.render(wf, fr, c["pw"], PB_SR, t, n=b - a)
                    fb = np.broadcast_to(ph.fallback(fr, PB_SR), o.shape)
                    ph.check_against(wf, o, t, eo, et, fb, "V=%d voice_block=%d rw_store=%d fps=%d block %d..%d" % (V, vb, rw, fps, a, b))


DRUM_TRIG_AT = (1, 4, 5, 12, 20)


def drum_params(L, rng, kind, variant, V):
    """The recorded case's parameters with every voice's pitch and envelope its own; snare and hats also their distortion, gain and
    filter.  The kick keeps the case's distortion, filter and gain: its bound (drums_host.kick_bound) is derived from them, and
    takes each voice's own envelope."""
    p = dh.Params.of_case(L, kind, variant, V)
    p.pitch[:] = p.pitch * rng.uniform(0.5, 1.5, V)
    p.par[1], p.par[2], p.par[3] = rng.uniform(0.6, 0.99, V), rng.uniform(0.05, 0.6, V), rng.uniform(0.6, 0.99, V)
    p.holdtime[:] = rng.integers(1, 4, V)
    if kind != "kick":
        p.shape[:], p.gain[:] = rng.uniform(0.5, 3.0, V), rng.uniform(0.5, 2.0, V)
        if kind == "hats":
            a, b = rng.uniform(3000.0, 9000.0, V), rng.uniform(0.5, 3.0, V)
            assert L.mxg_svf_coeffs_host(V, a.ctypes.data, b.ctypes.data, p.coef.ctypes.data) == 0
        else:
            a, b = rng.uniform(500.0, 5000.0, V), rng.uniform(1.0, 5.0, V)
            assert L.mxg_filter_coeffs_host(0, V, a.ctypes.data, b.ctypes.data, p.coef.ctypes.data) == 0
    return p


def kick_envelopes(p, trig):
    """[n][V]: the envelope of every voice over the case, from the numpy model of maxiEnv::adsr (drums_host.model_adsr)."""
    V = p.V
    dst, ist = np.zeros((2, V)), np.zeros((6, V), np.int64)
    e = dict(amplitude=dst[0], output=dst[1], holdcount=ist[0], attackphase=ist[1], decayphase=ist[2], sustainphase=ist[3],
             holdphase=ist[4], releasephase=ist[5])
    env = np.zeros((len(trig), V))
    with np.errstate(all="ignore"):
        for i in range(len(trig)):
            env[i] = dh.model_adsr(e, p.par, p.holdtime, np.broadcast_to(np.asarray(trig[i]) != 0, (V,)))
    return env


def drum_cases(V):
    import maximilian_amd as m
    L = m.lib()
    host, cases = dh.HostBackend(), []
    for ki, kind in enumerate(dh.KINDS):
        for vi, variant in enumerate(dh.VARIANTS):
            for tpv in (0, 1):
                rng = np.random.default_rng(8000 + V + 100 * ki + 10 * vi + tpv)
                p = drum_params(L, rng, kind, variant, V)
                if tpv:
                    trig = (rng.uniform(0, 1, (TOTAL, V)) < 0.15).astype(np.float64)
                else:
                    trig = np.zeros(TOTAL)
                    trig[list(DRUM_TRIG_AT)] = 1.0
                draws = None if kind == "kick" else rng.integers(0, 2 ** 31 - 1, (TOTAL, V)).astype(np.int32)
                state, blocks = dh.fresh_state(V), []
                for a, b in CUTS:
                    o, state = host.render(p, trig[a:b], None if draws is None else draws[a:b], state, tpv=tpv)
                    blocks.append((o, state))
                bound = dh.kick_bound(L, variant, kick_envelopes(p, trig), TOTAL) if kind == "kick" else None
                assert len(np.unique(np.concatenate([o for o, _ in blocks]))) > V // 4
                cases.append(dict(kind=kind, variant=variant, tpv=tpv, p=p, trig=trig, draws=draws, blocks=blocks, bound=bound))
    return cases


def check_drum_block(c, a, b, o, st, eo, est, what):
    if c["kind"] != "kick":
        dh.bits_equal(o, eo, what)
        for i in range(4):
            same(st[i], est[i], "%s: state array %d" % (what, i))
        return
    # the kick: the output under its bound; where the limiter returned +-1 on one side and the other lies within the bound of
    # +-1, either passes, for at most 1 % of the samples (drums_host.check_kick)
    fl, bound = c["p"].flags, c["bound"]
    err = np.abs(o - eo)
    ok = err <= bound[a:b]
    near = np.zeros_like(ok)
    if fl & dh.LIMITER:
        near = ~ok & (np.abs(np.abs(o) - 1.0) <= bound[a:b]) & (np.abs(np.abs(eo) - 1.0) <= bound[a:b])
    assert (ok | near).all(), "%s: %d samples over the bound, worst %.3g" % (what, (~(ok | near)).sum(), err[~(ok | near)].max())
    assert near.sum() <= 0.01 * near.size, "%s: %d samples within the bound of +-1" % (what, near.sum())
    for i in range(3):
        same(st[i], est[i], "%s: state array %d" % (what, i))
    if fl & dh.FILTER:
        # y is the output of the block's last sample before the gain; x = (y_n - y_n-1) * r (drums_host.check_case)
        g, r = c["p"].gain, np.abs(c["p"].coef[1])
        assert (np.abs(st[3][1] - est[3][1]) <= bound[b - 1] / g).all(), what + ": filter y"
        assert (np.abs(st[3][0] - est[3][0]) <= (bound[b - 1] + bound[b - 2]) / g * r).all(), what + ": filter x"
        same(st[3][2], est[3][2], what + ": filter state row 2")
    else:
        same(st[3], est[3], what + ": filter state")


@pytest.mark.parametrize("V,vb", A_SHAPES)
def test_drums(mx, V, vb):
    """mxg_drum_render: kick (the 16 KB sine table in LDS), snare (no table), hats (the 515-entry sineBuffer), plain and full
    variant, one shared trigger signal and one per voice."""
    cases = cached(("drums", V), lambda: drum_cases(V))
    be, L = dh.GpuBackend(mx), mx.lib()
    for rw in stores(V):
        with knobs(L, voice_block=vb, rw_store=rw):
            scrub_lds(mx)
            for c in cases:
                state = dh.fresh_state(V)
                for (a, b), (eo, est) in zip(CUTS, c["blocks"]):
                    o, state = be.render(c["p"], c["trig"][a:b], None if c["draws"] is None else c["draws"][a:b], state, tpv=c["tpv"])
                    check_drum_block(c, a, b, o, state, eo, est, "%s %s tpv=%d V=%d voice_block=%d rw_store=%d block %d..%d" % (
                        c["kind"], c["variant"], c["tpv"], V, vb, rw, a, b))


def clock_case(V):
    rng = np.random.default_rng(8500 + V)
    bps = rng.uniform(2000.0, 20000.0, V)    # a tick every 2 .. 22 samples at 44 100 Hz
    last = rng.integers(0, 2, V).astype(np.int32)
    clk, ph_ = rng.uniform(0.0, 1.0, V), rng.integers(0, 100, V).astype(np.int64)
    host, blocks = dh.HostBackend(), []
    c, p = clk, ph_
    for a, b in CUTS:
        tick, c, p, cnt = host.clock(bps, c, last, p, b - a)
        blocks.append((tick, c, p, cnt))
    assert blocks[0][0].sum() + blocks[1][0].sum() > V
    return dict(bps=bps, last=last, clk=clk, ph=ph_, blocks=blocks)


@pytest.mark.parametrize("V,vb", A_SHAPES)
def test_clock(mx, V, vb):
    """mxg_clock_render: the tick block, the phase, playHead and currentCount, bit for bit mxg_clock_host."""
    c = cached(("clock", V), lambda: clock_case(V))
    be, L = dh.GpuBackend(mx), mx.lib()
    for rw in stores(V):
        with knobs(L, voice_block=vb, rw_store=rw):
            clk, ph_ = c["clk"], c["ph"]
            for (a, b), (et, ec, ep, en) in zip(CUTS, c["blocks"]):
                tick, clk, ph_, cnt = be.clock(c["bps"], clk, c["last"], ph_, b - a)
                what = "clock V=%d voice_block=%d rw_store=%d block %d..%d" % (V, vb, rw, a, b)
                same(tick, et, what + ": tick")
                same(clk, ec, what + ": phase")
                same(ph_, ep, what + ": playhead")
                same(cnt, en, what + ": count")


@pytest.fixture(scope="module")
def line_host(tmp_path_factory):
    return sh.HostBackend(sh.build(tmp_path_factory.mktemp("wg_shaper")))


def line_case(host, V):
    """Ramps of 2 .. 13 samples (up and down), one-shot and repeating, a sixth of the lines with trigEnable off; an uploaded state
    in mid-flight; a trigger block that crosses zero often."""
    rng = np.random.default_rng(9000 + V)
    start, end = rng.uniform(-1.0, 1.0, V), rng.uniform(-1.0, 1.0, V)
    par = np.ascontiguousarray(np.stack([start, end, (end - start) / rng.integers(2, 14, V), (rng.uniform(0, 1, V) < 0.5) * 1.0,
                                         (rng.uniform(0, 1, V) < 0.85) * 1.0]))
    st0 = np.ascontiguousarray(np.stack([rng.uniform(-1.0, 1.0, V), rng.choice([-1.0, 0.0, 1.0], V), (rng.uniform(0, 1, V) < 0.3) * 1.0,
                                         np.zeros(V)]))
    trig = rng.choice([-1.0, 0.0, 0.5, 1.0], (TOTAL, V))
    exp = {}
    for tb in (True, False):
        st, blocks = st0.copy(), []
        for a, b in CUTS:
            o = host.line(trig[a:b] if tb else 1.0, b - a, par, st)
            blocks.append((o, st.copy()))
        assert len(np.unique(blocks[1][0])) > V // 4
        exp[tb] = blocks
    return dict(par=par, st0=st0, trig=trig, exp=exp)


@pytest.mark.parametrize("V,vb", A_SHAPES)
def test_line(mx, line_host, V, vb):
    """mxg_line_render with a trigger block and with the constant trigger of line.play(1)."""
    c = cached(("line", V), lambda: line_case(line_host, V))
    L = mx.lib()
    for rw in stores(V):
        with knobs(L, voice_block=vb, rw_store=rw):
            for tb, blocks in c["exp"].items():
                st = c["st0"]
                for (a, b), (eo, est) in zip(CUTS, blocks):
                    d = Dev(mx)
                    gs, go = d.io(st), d.out(b - a, V)
                    d.call(L.mxg_line_render, V, b - a, d.inp(c["trig"][a:b]) if tb else None, 0.0 if tb else 1.0, d.inp(c["par"]), gs, go, None)
                    what = "line trigger block %s V=%d voice_block=%d rw_store=%d block %d..%d" % (tb, V, vb, rw, a, b)
                    o, st = go.back(what + ": d_out"), gs.back(what + ": d_st")
                    same(o, eo, what)
                    same(st, est, what + ": state")


@pytest.fixture(scope="module")
def ana_host(tmp_path_factory):
    return ah.HostBackend(ah.build(tmp_path_factory.mktemp("wg_analysis")))


ANA_CAP = 70
ANA_WANTS = (ah.ALL, ah.ZCR | ah.ENV)


def ana_case(host, V):
    """cap 70 (two ring words, the second partial), windows over 1 .. cap, positions anywhere in the ring, hold times of 0 .. 8
    samples per sample; all four outputs, and zcr + env alone."""
    rng = np.random.default_rng(9500 + V)
    x = rng.choice([-0.5, 0.25, 0.75, -0.125, 0.0, 1.0], (TOTAL, V)) * rng.uniform(0.5, 1.0, (TOTAL, V))
    par = dict(window=rng.integers(1, ANA_CAP + 1, V).astype(np.uint32), attack=rng.uniform(0.1, 0.9, V), release=rng.uniform(0.9, 0.999, V),
               hold=rng.choice([0.0, 0.05, 0.1, 0.2], (TOTAL, V)))
    st0 = ah.fresh(V, ANA_CAP)
    st0["zpos"][:] = rng.integers(0, ANA_CAP, V)
    st0["env"][:] = rng.uniform(0, 1, V)
    exp = {}
    for want in ANA_WANTS:
        st, blocks = {k: v.copy() for k, v in st0.items()}, []
        for a, b in CUTS:
            o = host.render(44100, x[a:b], want, st, par["window"], ANA_CAP, par["attack"], par["release"], par["hold"][a:b])
            blocks.append((o, {k: v.copy() for k, v in st.items()}))
        assert blocks[1][0]["zcr"].max() >= 2
        exp[want] = blocks
    return dict(x=x, par=par, st0=st0, exp=exp)


def gpu_analysis(mx, x, want, st, par, hold):
    """mxg_analysis_render with every wanted state array and output guarded; the stages that are not wanted get NULL."""
    L, d = mx.lib(), Dev(mx)
    n, V = x.shape
    used = set()
    for bit, keys in ah.STAGE_STATE.items():
        if want & bit:
            used |= set(keys)
    gs = {k: d.io(st[k]) for k in ah.STATE_KEYS if k in used}
    go = {name: d.out(n, V) for bit, name in ah.NAMES.items() if want & bit}
    zcr, env, sah = want & ah.ZCR, want & ah.ENV, want & ah.SAH
    d.call(L.mxg_analysis_render, V, n, d.inp(x), want, gs.get("prev_x"), d.inp(par["window"], np.uint32) if zcr else None, gs.get("zring"),
           ANA_CAP, gs.get("zpos"), gs.get("zcount"), gs.get("overflow"), d.inp(par["attack"]) if env else None,
           d.inp(par["release"]) if env else None, gs.get("env"), d.inp(hold) if sah else None, 1, gs.get("sah_phase"), gs.get("sah_value"),
           go.get("zx"), go.get("zcr"), go.get("env"), go.get("sah"), None)
    new = {k: v.copy() for k, v in st.items()}
    for k, g in gs.items():
        new[k] = g.back("the state array " + k)
    return {name: g.back("the output " + name) for name, g in go.items()}, new


@pytest.mark.parametrize("V,vb", A_SHAPES)
def test_analysis(mx, ana_host, V, vb):
    """mxg_analysis_render with all four outputs and with a subset, against the host build of mxg_analysis.h."""
    c = cached(("analysis", V), lambda: ana_case(ana_host, V))
    L = mx.lib()
    for rw in stores(V):
        with knobs(L, voice_block=vb, rw_store=rw):
            for want, blocks in c["exp"].items():
                st = c["st0"]
                for (a, b), (eo, est) in zip(CUTS, blocks):
                    o, st = gpu_analysis(mx, c["x"][a:b], want, st, c["par"], c["par"]["hold"][a:b])
                    what = "analysis want=%d V=%d voice_block=%d rw_store=%d block %d..%d" % (want, V, vb, rw, a, b)
                    assert sorted(o) == sorted(eo)
                    for name in eo:
                        same(o[name], eo[name], "%s: %s" % (what, name))
                    for k in ah.STATE_KEYS:
                        same(st[k], est[k], "%s: state %s" % (what, k))


# =====================================================================================================================
# Part B: the other per-voice kernels at 64, 128 and 192 lanes
# =====================================================================================================================
def two_blocks(V, vb, run, expected, what):
    """run(a, b, state) -> (outputs, state) block after block from expected["state0"], under every store flavour; outputs and
    states are tuples, compared entry by entry with expected["blocks"] (a state array with more rows than its expectation is
    compared on those rows)."""
    import maximilian_amd as m
    for rw in stores(V):
        with knobs(m.lib(), voice_block=vb, rw_store=rw):
            scrub_lds(m)
            state = expected["state0"]
            for (a, b), (eo, est) in zip(CUTS, expected["blocks"]):
                o, state = run(a, b, state)
                w = "%s V=%d voice_block=%d rw_store=%d block %d..%d" % (what, V, vb, rw, a, b)
                for i, (x, y) in enumerate(zip(o, eo)):
                    same(x, y, "%s: output %d" % (w, i))
                for i, (x, y) in enumerate(zip(state, est)):
                    same(x[:len(y)], y, "%s: state array %d" % (w, i))


def filter_case(port, kind, V):
    rng = np.random.default_rng(1100 + 10 * V + kind)
    x = rng.uniform(-1, 1, (TOTAL, V))
    c = rng.uniform(0, 1, V) if kind >= 3 else rng.uniform(1, 30000, V)
    r = None if kind >= 3 else (rng.uniform(0.01, 1.3, V) if kind == 2 else rng.uniform(0.2, 25, V))
    st, blocks = np.zeros((5, V)), []
    for a, b in CUTS:
        o, st = port.filter(kind, x[a:b], c, r, state=st)
        blocks.append(((o,), (st,)))
    return dict(x=x, c=c, r=r, coef=banks.filter_coeffs(kind, c, r) if kind < 3 else None, state0=(np.zeros((5, V)),), blocks=blocks)


@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_filter(mx, port, V, vb):
    """maxiFilter, all five kinds, block-constant parameters (the pair-row kernel takes its parity from threadIdx.x)."""
    L = mx.lib()
    for kind in range(5):
        c = cached(("filter", kind, V), lambda: filter_case(port, kind, V))

        def run(a, b, state):
            d = Dev(mx)
            gs, go = d.io(state[0]), d.out(b - a, V)
            d.call(L.mxg_filter_render, kind, V, b - a, d.inp(c["x"][a:b]), d.inp(c["c"]), 0, d.inp(c["r"]), 0, d.inp(c["coef"]), gs, go, None)
            return (go.back("d_out"),), (gs.back("d_st"),)
        two_blocks(V, vb, run, c, "filter kind %d" % kind)


def env_trig(rng, V, tpv):
    n = np.arange(TOTAL)
    if tpv:
        return ((n[:, None] + rng.integers(0, 11, V)[None, :]) % 11 < rng.integers(2, 9, V)[None, :]).astype(np.int32)
    return ((n % 11) < 6).astype(np.int32)


def env_pars(rng, V):
    par = np.stack([rng.uniform(0.05, 0.6, V), rng.uniform(0.5, 0.95, V), rng.uniform(0.2, 0.9, V), rng.uniform(0.5, 0.95, V)])
    return np.ascontiguousarray(par), rng.integers(1, 5, V).astype(np.int64)


def env_case(port, mode, tpv, hasin, V):
    rng = np.random.default_rng(1200 + 10 * V + 4 * mode + 2 * tpv + hasin)
    x = rng.uniform(-1, 1, (TOTAL, V)) if hasin else None
    trig = env_trig(rng, V, tpv)
    par, hold = env_pars(rng, V)
    dst, ist, blocks = None, None, []
    for a, b in CUTS:
        o, dst, ist = port.env(mode, None if x is None else x[a:b], trig[a:b], par, hold, dstate=dst, istate=ist, N=b - a)
        blocks.append(((o,), (dst, ist)))
    assert len(np.unique(blocks[1][0][0])) > V
    return dict(x=x, trig=trig, par=par, hold=hold, state0=(np.zeros((2, V)), np.zeros((6, V), np.int64)), blocks=blocks)


@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_env(mx, port, V, vb):
    """maxiEnv adsr and ar: a shared gate over a constant input, per-voice gates over an input block."""
    L = mx.lib()
    for mode in (0, 1):
        for tpv, hasin in ((0, 0), (1, 1)):
            c = cached(("env", mode, tpv, V), lambda: env_case(port, mode, tpv, hasin, V))

            def run(a, b, state):
                d = Dev(mx)
                gd, gi, go = d.io(state[0]), d.io(state[1]), d.out(b - a, V)
                d.call(L.mxg_env_render, mode, V, b - a, d.inp(None if c["x"] is None else c["x"][a:b]), d.inp(c["trig"][a:b], np.int32), tpv,
                       d.inp(c["par"]), d.inp(c["hold"], np.int64), gd, gi, go, None)
                return (go.back("d_out"),), (gd.back("d_dst"), gi.back("d_ist"))
            two_blocks(V, vb, run, c, "env mode %d tpv %d" % (mode, tpv))


def voice_case(port, mode, tpv, V):
    rng = np.random.default_rng(1300 + 10 * V + 2 * mode + tpv)
    freq, res = rng.uniform(50.0, 4000.0, V), rng.uniform(1.0, 6.0, V)
    cutoff = rng.uniform(300.0, 6000.0, V)
    trig = env_trig(rng, V, tpv)
    par, hold = env_pars(rng, V)
    st, blocks = (None, None, None, None), []
    for a, b in CUTS:
        o, *st = port.voice(mode, freq, cutoff, res, trig[a:b], par, hold, *st)
        blocks.append((o, tuple(st)))
    state0 = (np.zeros((2, V)), np.zeros((5, V)), np.zeros((2, V)), np.zeros((6, V), np.int64))
    return dict(freq=freq, cutoff=cutoff, res=res, coef=banks.filter_coeffs(0, cutoff, res), trig=trig, par=par, hold=hold, state0=state0,
                blocks=blocks)


@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_voice(mx, port, V, vb):
    """The fused voice (the plain form; the mixdown form sets its own workgroup).  Mode A bit for bit; mode B's cutoff follows the
    envelope through device cos / sqrt: the block within 1e-11 of the voice's peak, oscillator and envelope state bit for bit
    (the filter state has the block's tolerance and is not compared, as in tests/test_gpu_voice.py)."""
    L = mx.lib()
    for mode in (0, 1):
        for tpv in (0, 1):
            c = cached(("voice", mode, tpv, V), lambda: voice_case(port, mode, tpv, V))
            for rw in stores(V):
                with knobs(L, voice_block=vb, rw_store=rw, voice_store=0 if rw == 0 else 3):
                    state = c["state0"]
                    for (a, b), (eo, est) in zip(CUTS, c["blocks"]):
                        d = Dev(mx)
                        gs, go = [d.io(s) for s in state], d.out(b - a, V)
                        d.call(L.mxg_voice_render, mode, V, b - a, d.inp(c["freq"]), d.inp(c["cutoff"]), d.inp(c["res"]), d.inp(c["coef"]),
                               d.inp(c["trig"][a:b], np.int32), tpv, d.inp(c["par"]), d.inp(c["hold"], np.int64), *gs, go, None)
                        what = "voice mode %d tpv %d V=%d voice_block=%d store %d block %d..%d" % (mode, tpv, V, vb, rw, a, b)
                        o = go.back(what + ": d_out")
                        state = tuple(g.back("%s: state array %d" % (what, i)) for i, g in enumerate(gs))
                        if mode == 0:
                            same(o, eo, what)
                            same(state[1], est[1], what + ": filter state")
                        else:
                            assert_close_scaled(o, eo, MOD_FILTER_RTOL, what)
                        same(state[0], est[0], what + ": osc state")
                        same(state[2], est[2], what + ": envelope amplitude / output")
                        same(state[3], est[3], what + ": envelope flags")


def filter2_case(port, L, kind, V):
    rng = np.random.default_rng(1400 + 10 * V + kind)
    x = rng.uniform(-1, 1, (TOTAL, V))
    if kind == 0:
        par = rng.uniform(0.9, 0.9999, (1, V))
        coef = par.copy()
    elif kind == 1:
        cutoff, res = rng.uniform(20.0, 20000.0, V), rng.uniform(0.3, 12.0, V)
        mix = rng.uniform(0.0, 1.0, (4, V))
        par = np.vstack([cutoff[None], res[None], mix])
        coef = np.zeros((9, V))
        assert L.mxg_svf_coeffs_host(V, cutoff.ctypes.data, res.ctypes.data, coef.ctypes.data) == 0
        coef[5:] = mix
    else:
        typ = rng.integers(0, 7, V).astype(np.int32)
        cutoff, q, gain = rng.uniform(50.0, 15000.0, V), rng.uniform(0.3, 8.0, V), rng.uniform(-12.0, 12.0, V)
        par = np.stack([typ.astype(np.float64), cutoff, q, gain])
        coef = np.zeros((5, V))
        assert L.mxg_biquad_coeffs_host(V, typ.ctypes.data, cutoff.ctypes.data, q.ctypes.data, gain.ctypes.data, coef.ctypes.data) == 0
    st, blocks = None, []
    for a, b in CUTS:
        o, st, ecoef = port.filter2(kind, x[a:b], par, st)
        blocks.append(((o,), (st[:2] if kind == 0 else st,)))   # (maxiDCBlocker has two state members: row 2 is unused)
    if kind:
        assert_bits_equal(coef[:5], ecoef, "the host coefficients of kind %d" % kind)
    return dict(x=x, coef=np.ascontiguousarray(coef), state0=(np.zeros((3, V)),), blocks=blocks)


@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_filter2(mx, port, V, vb):
    """maxiDCBlocker, maxiSVF, maxiBiquad (filter2_pairs_kernel takes its parity from threadIdx.x)."""
    L = mx.lib()
    for kind in range(3):
        c = cached(("filter2", kind, V), lambda: filter2_case(port, L, kind, V))

        def run(a, b, state):
            d = Dev(mx)
            gs, go = d.io(state[0]), d.out(b - a, V)
            d.call(L.mxg_filter2_render, kind, V, b - a, d.inp(c["x"][a:b]), d.inp(c["coef"]), gs, go, None)
            return (go.back("d_out"),), (gs.back("d_st"),)
        two_blocks(V, vb, run, c, "filter2 kind %d" % kind)


EG_SHAPE = ([0, 1, 0.4, 0.4, 0], [0.05, 0.1, ENVGEN_HOLD, 0.08], [1, 1, 1, 1])   # 2, 4 and 3 samples around a hold: all curves 1


def envgen_case(port, tpv, V):
    rng = np.random.default_rng(1500 + 10 * V + tpv)
    lv, tm, cv = EG_SHAPE
    if tpv:
        trig = np.sign(np.sin(np.arange(TOTAL)[:, None] * rng.uniform(0.2, 1.5, V)[None, :] + rng.uniform(0, 6, V)[None, :]))
        trig[:, ::5] = (rng.uniform(0, 1, (TOTAL, len(range(0, V, 5)))) < 0.2) * 1.0
    else:
        trig = np.where(np.arange(TOTAL) % 12 < 7, 1.0, -1.0)
    dst, ist, blocks = None, None, []
    for a, b in CUTS:
        o, dst, ist, stages = port.envgen(trig[a:b], lv, tm, cv, 1, 1, dst=dst, ist=ist, V=V)
        blocks.append(((o,), (dst, ist)))
    assert np.concatenate([bl[0][0] for bl in blocks]).max() > 0
    return dict(trig=trig, stages=stages, state0=port.envgen_fresh(V), blocks=blocks)


@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_envgen(mx, port, V, vb):
    """mxg_envgen_render (the stage table staged into LDS by the workgroup): a shared gate and per-voice triggers, loop and
    retrigger on, every curve 1 -- bit for bit, the state machine included."""
    L = mx.lib()
    lv, tm, cv = (np.array(a, np.float64) for a in EG_SHAPE)
    stages = np.zeros((len(lv) - 1, 6))
    assert L.mxg_envgen_stages_host(len(lv), lv.ctypes.data, tm.ctypes.data, cv.ctypes.data, stages.ctypes.data) == len(lv) - 1
    for tpv in (0, 1):
        c = cached(("envgen", tpv, V), lambda: envgen_case(port, tpv, V))
        assert_bits_equal(stages, c["stages"], "stage table")

        def run(a, b, state):
            d = Dev(mx)
            gd, gi, go = d.io(state[0]), d.io(state[1]), d.out(b - a, V)
            d.call(L.mxg_envgen_render, V, b - a, d.inp(c["trig"][a:b]), tpv, d.inp(stages), len(stages), 1, 1, gd, gi, go, None)
            return (go.back("d_out"),), (gd.back("d_dst"), gi.back("d_ist"))
        two_blocks(V, vb, run, c, "envgen tpv %d" % tpv)


@pytest.fixture(scope="module")
def seq_be(tmp_path_factory):
    return sq.HostBackend(sq.build(tmp_path_factory.mktemp("wg_seq")))


class GuardedSeq:
    """seq_host.GpuBackend's interface with the state arrays and the outputs inside guard bands."""

    def __init__(self, mx):
        self.mx = mx

    def render(self, sr, V, N, freq, clk, phase, norm, plen, pat, mode, values, vlen, vpat, step, hold, dst, ist, want):
        mx, d, f64, i32 = self.mx, Dev(self.mx), np.float64, np.int32
        assert int(sr) == mx.maxiSettings.sampleRate
        gd, gi, gc = d.io(dst), d.io(ist), d.io(clk) if freq is not None else None
        out = [d.out(N, V) if w else None for w in want]
        pv = 0 if phase is None else int(np.ndim(phase) == 2)
        d.call(mx.lib().mxg_seq_render, V, N, d.inp(freq), gc, d.inp(phase), pv, d.inp(norm), d.inp(plen, i32), norm.shape[0], norm.shape[1],
               d.inp(pat, i32), mode, d.inp(values), d.inp(vlen, i32), 0 if values is None else values.shape[0],
               0 if values is None else values.shape[1], d.inp(vpat, i32), d.inp(step), d.inp(hold), gd, gi, *out, None)
        dst[...], ist[...] = gd.back("d_dst"), gi.back("d_ist")
        if gc is not None:
            clk[...] = gc.back("d_clk")
        return [None if o is None else o.back("output %d" % i) for i, o in enumerate(out)]

    def signal(self, kind, V, N, a, b, values, vlen, vpat, par, dst, ist):
        mx, d, i32 = self.mx, Dev(self.mx), np.int32
        gd, gi, go = d.io(dst), d.io(ist), d.out(N, V)
        d.call(mx.lib().mxg_seq_signal, kind, V, N, d.inp(a), d.inp(b), d.inp(values), d.inp(vlen, i32), 0 if values is None else values.shape[0],
               0 if values is None else values.shape[1], d.inp(vpat, i32), d.inp(par), gd, gi, go, None)
        dst[...], ist[...] = gd.back("d_dst"), gi.back("d_ist")
        return go.back("d_out")


def seq_bank(V):
    """Tables and per-voice selections that use every row (tests/test_gpu_seq.py random_bank): a pattern of 64 ratios, a zero ratio,
    a zero sum; clocks fast enough for several steps in 25 samples."""
    rng = np.random.default_rng(1600 + V)
    pats = [[3, 3, 2], [1], [4, 4, 4, 1, 1, 1, 1], list(rng.uniform(0.0, 5.0, 64)), [2, 0, 1, 0.001, 1], [0, 0]]
    times, plen = sq.table(pats, 64)
    vals, vlen = sq.table([[440.0], [40.0, 80.0, 170.0], list(rng.uniform(20.0, 4000.0, 6)), list(rng.uniform(20.0, 4000.0, 10))], 10)
    d = dict(norm=sq.ratio_tables(times, plen), plen=plen, values=vals, vlen=vlen, pat=rng.integers(0, len(pats), V).astype(np.int32),
             vpat=rng.integers(0, 4, V).astype(np.int32), freq=rng.uniform(1000.0, 15000.0, V), hold=rng.choice([0.0, 1.0, 2.5, 7.0, 300.0], V))
    n = vlen[d["vpat"]].astype(np.float64)
    d["step"] = np.choose(rng.integers(0, 6, V), [np.ones(V), 2 * np.ones(V), -np.ones(V), 0.5 * np.ones(V), n + 3, -n])
    d["phases"] = (rng.uniform(0, 1, V)[None, :] + np.arange(TOTAL)[:, None] * rng.uniform(0.03, 0.4, V)[None, :]) % 1.0
    d["phases"][:, ::7] = rng.uniform(-0.2, 1.2, (TOTAL, len(range(0, V, 7))))
    d["trig"] = (rng.uniform(0, 1, (TOTAL, V)) < 0.3).astype(np.float64)
    d["second"] = rng.uniform(-0.3, 1.3, (TOTAL, V))
    return d


def seq_render_run(be, d, V, clock, mode):
    """Both blocks through a backend, all three outputs: [(outputs, dst, ist, clk) after each block]."""
    dst, ist = sq.fresh_seq(V)
    clk, res = np.zeros(V), []
    for a, b in CUTS:
        ph_ = None if clock == 0 else (d["phases"][a:b] if clock == 1 else np.ascontiguousarray(d["phases"][a:b, 0]))
        o = be.render(44100, V, b - a, d["freq"] if clock == 0 else None, clk, ph_, d["norm"], d["plen"], d["pat"], mode, d["values"], d["vlen"],
                      d["vpat"], d["step"], d["hold"], dst, ist, (True, True, True))
        res.append((o, dst.copy(), ist.copy(), clk.copy()))
    return res


def seq_signal_run(be, d, V, kind):
    dst, ist = sq.fresh_sig(kind, V)
    tab = kind in (sq.STEP, sq.INDEX)
    par = d["step"] if kind == sq.STEP else (d["hold"] if kind == sq.ZXTOPULSE else None)
    x = d["second"] - 0.5 if kind == sq.ONZX else d["trig"]
    y = d["second"] if kind == sq.INDEX else (d["second"] - 0.5 if kind == sq.COUNTER else None)
    res = []
    for a, b in CUTS:
        o = be.signal(kind, V, b - a, x[a:b], None if y is None else y[a:b], d["values"] if tab else None, d["vlen"] if tab else None,
                      d["vpat"] if tab else None, par, dst, ist)
        res.append((o, dst.copy(), ist.copy()))
    return res


SEQ_RENDERS = ((0, sq.VAL_VALUES), (0, sq.VAL_STEP), (1, sq.VAL_STEP), (2, sq.VAL_VALUES))   # (clock form, value mode)


def seq_case(host, V):
    d = seq_bank(V)
    exp = {("render", cm): seq_render_run(host, d, V, *cm) for cm in SEQ_RENDERS}
    exp.update({("signal", kind): seq_signal_run(host, d, V, kind) for kind in sorted(sq.KIND_NAMES)})
    if V >= 65:
        assert sum(r[0][0].sum() for r in exp["render", SEQ_RENDERS[0]]) > 0
    return d, exp


@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_seq(mx, seq_be, V, vb):
    """mxg_seq_render (internal clock, an external phase per voice, one shared external phase; all three outputs; both value
    modes) and mxg_seq_signal (every kind): the tables go to dynamic LDS with a blockDim.x stride.  Against the host build of
    mxg_seq.h, bit for bit."""
    d, exp = cached(("seq", V), lambda: seq_case(seq_be, V))
    gpu, L = GuardedSeq(mx), mx.lib()
    for rw in stores(V):
        with knobs(L, voice_block=vb, rw_store=rw):
            scrub_lds(mx)
            for key, want in exp.items():
                got = seq_render_run(gpu, d, V, *key[1]) if key[0] == "render" else seq_signal_run(gpu, d, V, key[1])
                for (a, b), g, e in zip(CUTS, got, want):
                    what = "seq %s %s V=%d voice_block=%d rw_store=%d block %d..%d" % (key[0], key[1], V, vb, rw, a, b)
                    outs = zip(g[0], e[0]) if key[0] == "render" else [(g[0], e[0])]
                    for i, (x, y) in enumerate(outs):
                        same(x, y, "%s: output %d" % (what, i))
                    for i, (x, y) in enumerate(zip(g[1:], e[1:])):
                        same(x, y, "%s: state array %d" % (what, i))


DELAY_CAP = 12


def delay_case(port, mode, V):
    """Rings of 12 slots, sizes over 1 .. 12: every ring wraps inside the 25 samples."""
    rng = np.random.default_rng(1700 + 10 * V + mode)
    x = rng.uniform(-1, 1, (TOTAL, V))
    size, fb = rng.integers(1, DELAY_CAP + 1, V).astype(np.int32), rng.uniform(0, 0.9, V)
    pos = rng.integers(0, DELAY_CAP, V).astype(np.int32) if mode else None
    mem, ph_, blocks = None, None, []
    for a, b in CUTS:
        o, mem, ph_ = port.delay(mode, x[a:b], size, fb, DELAY_CAP, position=pos, mem=mem, phase=ph_)
        blocks.append(((o,), (mem, ph_)))
    return dict(x=x, size=size, fb=fb, pos=pos, state0=(np.zeros((DELAY_CAP, V)), np.zeros(V, np.int32)), blocks=blocks)


@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_delay(mx, port, V, vb):
    """mxg_delay_render, dl and dlFromPosition: output, ring memory and phase."""
    L = mx.lib()
    for mode in (0, 1):
        c = cached(("delay", mode, V), lambda: delay_case(port, mode, V))

        def run(a, b, state):
            d = Dev(mx)
            gm, gp, go = d.io(state[0]), d.io(state[1]), d.out(b - a, V)
            d.call(L.mxg_delay_render, mode, V, b - a, d.inp(c["x"][a:b]), d.inp(c["size"], np.int32), d.inp(c["fb"]), d.inp(c["pos"], np.int32),
                   gm, DELAY_CAP, gp, go, None)
            return (go.back("d_out"),), (gm.back("d_mem"), gp.back("d_phase"))
        two_blocks(V, vb, run, c, "delay mode %d" % mode)


SMP_LEN = 1500


def sample_data():
    def make():
        rng, n = np.random.default_rng(1800), np.arange(SMP_LEN)
        return np.round((0.5 * np.sin(2 * np.pi * 110 * n / 44100) + 0.25 * np.sin(2 * np.pi * 331 * n / 44100)
                         + 0.05 * rng.uniform(-1, 1, SMP_LEN)) * 32767) / 32767.0
    return cached("samples", make)


@pytest.fixture(scope="module")
def d_samples(mx):
    smp = sample_data()
    ptr = mx.lib().mxg_sample_upload(smp.ctypes.data, smp.size)
    assert ptr
    yield ptr
    mx.lib().mxg_sample_free(ptr)


def sample_pars(rng, mode, V):
    """Per voice, in the ranges of oracle/gen_golden.py: heads anywhere in the sample (integers for play / playOnce), speeds over
    0.2 .. 3, loop points as fractions; play4 / playAtSpeedBetweenPoints take a frequency of either sign and points in samples."""
    pos0 = rng.uniform(1, SMP_LEN - 5, V)
    pos0[0] = SMP_LEN - 1.0
    if mode in (0, 1):
        pos0 = np.floor(pos0)
    a = rng.uniform(0.2, 3.0, V)
    st, en = rng.uniform(0, 0.4, V), rng.uniform(0.5, 1.1, V)
    if mode == 2:
        en = np.minimum(en, 1.0)
    if mode in (7, 8):
        a = rng.uniform(0.5, 60, V) * np.where(rng.uniform(0, 1, V) < 0.4, -1, 1)
        st, en = np.floor(rng.uniform(2, 400, V)), np.floor(rng.uniform(500, SMP_LEN - 1, V))
    return pos0, a, st, en


def sample_case(port, mode, V, cuts=CUTS, seed=0):
    rng = np.random.default_rng(1900 + 100 * V + mode + seed)
    pos0, a, st, en = sample_pars(rng, mode, V)
    pos, blocks = pos0, []
    for c0, c1 in cuts:
        o, pos = port.sample(mode, sample_data(), c1 - c0, pos, a=a, start=st, end=en)
        blocks.append((o, pos))
    return dict(pos0=pos0, a=a, st=st, en=en, blocks=blocks)


def gpu_sample(mx, d_samples, mode, V, n, c, pos):
    L, d = mx.lib(), Dev(mx)
    gp, go = d.io(pos), d.out(n, V)
    d.call(L.mxg_sample_render, mode, V, n, d_samples, SMP_LEN, 44100, d.inp(c["a"]), 0, d.inp(c["st"]), d.inp(c["en"]), gp, go, None)
    return go.back("d_out"), gp.back("d_position")


@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_sample(mx, port, d_samples, V, vb):
    """mxg_sample_render, modes 0 - 8: output and head, bit for bit."""
    L = mx.lib()
    for mode in range(9):
        c = cached(("sample", mode, V), lambda: sample_case(port, mode, V))
        for rw in stores(V):
            with knobs(L, voice_block=vb, rw_store=rw):
                pos = c["pos0"]
                for (a, b), (eo, ep) in zip(CUTS, c["blocks"]):
                    o, pos = gpu_sample(mx, d_samples, mode, V, b - a, c, pos)
                    what = "sample mode %d V=%d voice_block=%d rw_store=%d block %d..%d" % (mode, V, vb, rw, a, b)
                    same(o, eo, what)
                    same(pos, ep, what + ": head")


PART_CUTS = ((0, 73),)


@pytest.mark.parametrize("pipe", [0, 1])
@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_sample_time_parts(mx, port, d_samples, V, vb, pipe):
    """playAtSpeed / playOnceAtSpeed / playUntilAtSpeed cut into time parts (smp_split 3: a block of 64 + 9 samples gives two parts):
    sample_parts_kernel's LDS windows are indexed by the wavefront of the workgroup, its part counters sized per wavefront."""
    L = mx.lib()
    for mode in (4, 5, 6):
        c = cached(("sample parts", mode, V), lambda: sample_case(port, mode, V, PART_CUTS, seed=50))
        eo, ep = c["blocks"][0]
        for rw in stores(V):
            with knobs(L, voice_block=vb, rw_store=rw, smp_split=3, smp_pipe=pipe):
                o, pos = gpu_sample(mx, d_samples, mode, V, 73, c, c["pos0"])
            what = "sample mode %d in time parts, smp_pipe=%d V=%d voice_block=%d rw_store=%d" % (mode, pipe, V, vb, rw)
            same(o, eo, what)
            same(pos, ep, what + ": head")
            assert L.mxg_last_async_error() == 0, what


def sample_trig_case(port, mode, V):
    """Modes 9 - 13 (tests/test_gpu_sample.py _zx_case): sines and sparse impulses as triggers; mode 14: phasors forward, backward,
    in steps, stuck at 0."""
    rng = np.random.default_rng(2000 + 100 * V + mode)
    n = np.arange(TOTAL)[:, None]
    if mode == 14:
        trig = (n * rng.uniform(0.003, 0.1, V)[None, :] + rng.uniform(0, 1, V)) % 1.0
        trig[:, 1::4] = 1.0 - trig[:, 1::4]
        trig[:, 2::4] = np.round(trig[:, 2::4] * 8) / 8
        trig[:, 3::16] = 0.0
        state, blocks = (None, None), []
        for a, b in CUTS:
            o, *state = port.sample_phasor(sample_data(), trig[a:b], *state)
            blocks.append((o, (None, state[0], state[1])))
        return dict(trig=trig, a=None, p0=None, p1=None, state0=(None, np.zeros(V), np.ones(V, np.int32)), blocks=blocks)
    trig = np.sin(n * rng.uniform(0.2, 1.5, V)[None, :] + rng.uniform(0, 6, V))
    trig[:, ::5] = np.where(rng.uniform(size=(TOTAL, (V + 4) // 5)) < 0.2, 1.0, 0.0)
    a, p0, p1 = rng.uniform(0.3, 2.5, V), rng.uniform(0, 0.6, V), rng.uniform(0.1, 0.5, V)
    pos0 = rng.uniform(0, SMP_LEN - 1, V)
    state, blocks = (pos0, None, None), []
    for c0, c1 in CUTS:
        o, *state = port.sample_zx(mode - 9, sample_data(), trig[c0:c1], state[0], a=a, p0=p0, p1=p1, zx_prev=state[1], zx_first=state[2])
        blocks.append((o, tuple(state)))
    return dict(trig=trig, a=a if mode in (10, 11, 12) else None, p0=p0 if mode >= 11 else None, p1=p1 if mode == 12 else None,
                state0=(pos0, np.ones(V), np.ones(V, np.int32)), blocks=blocks)


@pytest.mark.parametrize("V,vb", B_SHAPES)
def test_sample_trig(mx, port, d_samples, V, vb):
    """mxg_sample_render_trig, modes 9 - 14: output, head and the trigger detector's state, bit for bit."""
    L = mx.lib()
    for mode in range(9, 15):
        c = cached(("sample trig", mode, V), lambda: sample_trig_case(port, mode, V))
        for rw in stores(V):
            with knobs(L, voice_block=vb, rw_store=rw):
                state = c["state0"]
                for (a, b), (eo, est) in zip(CUTS, c["blocks"]):
                    d = Dev(mx)
                    gs, go = [d.io(s) for s in state], d.out(b - a, V)
                    d.call(L.mxg_sample_render_trig, mode, V, b - a, d_samples, SMP_LEN, 44100, d.inp(c["trig"][a:b]), d.inp(c["a"]), 0,
                           d.inp(c["p0"]), d.inp(c["p1"]), *gs, go, None)
                    what = "sample mode %d V=%d voice_block=%d rw_store=%d block %d..%d" % (mode, V, vb, rw, a, b)
                    same(go.back(what + ": d_out"), eo, what)
                    state = tuple(None if g is None else g.back("%s: state array %d" % (what, i)) for i, g in enumerate(gs))
                    for i, (x, y) in enumerate(zip(state, est)):
                        if y is not None:
                            same(x, y, "%s: state array %d" % (what, i))
