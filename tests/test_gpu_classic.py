"""GPU: the K23 entry points (mxg_dyn_gate_render, mxg_dyn_compress_render, mxg_envelope_line_render, mxg_lag_render,
mxg_map_render) against the reference's own bits (tests/golden/classic.npz: outputs and every state array at every cut) and, on
shapes the file does not hold, against the host build of mxg_classic.h (tests/host_classic.cpp, pinned to the same file by
tests/test_classic_host.py).  Everything is compared bit for bit except linexp, explin, ampToDbs and dbsToAmp, which are held to
the a-priori bounds of tests/classic_host.py (35 / 17 ULP of the reference value; an absolute bound per element), fixed before the
first GPU run; positions of NaN and +-Inf agree exactly.  No GPU run is compared with another GPU run.

Measured on an MI355X: see DESIGN.md section 4, K23."""
import itertools

import numpy as np
import pytest

import classic_host as ch
from conftest import assert_bits_equal
from test_gpu_workgroups import Dev, Guarded, knobs, same, stores

pytestmark = pytest.mark.gpu

VS, NS = [1, 3, 63, 64, 65, 130], [1, 7, 8, 9, 71]
SHAPES = list(itertools.product(VS, NS))
WG_CUTS = ((0, 9), (9, 25))   # two carried blocks, of 9 then 16 samples
A_SHAPES = [(V, vb) for V in (16385, 16514) for vb in (128, 192, 256)]   # every stateful kernel here passes small64
B_SHAPES = [(V, vb) for V in (1, 65, 130, 193, 386) for vb in (64, 128, 192)]
ENV_S = 8
SPECIAL = np.array([1.0, -1.0, 0.0, -0.0, 0.5, float("nan"), float("inf"), float("-inf"), 1e-310])


@pytest.fixture(scope="module")
def gpu(mx):
    return ch.GpuBackend(mx)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ch.HostBackend(ch.build(tmp_path_factory.mktemp("classic_host")))


@pytest.fixture(scope="module")
def g(golden):
    return golden("classic.npz")


# ---- the golden cases, through the C-ABI as stored ---------------------------------------------------------------------------
def test_golden_dynamics_and_lag(gpu, g):
    ch.play_gate_case(gpu, g)
    ch.play_compress_case(gpu, g, (777,))
    ch.play_lag_case(gpu, g)


def test_golden_envelope(mx, gpu, g):
    lib = mx.lib()

    def trigger(v, index, amp, count, dst, ist):
        V = dst.shape[1]
        mask = np.zeros(V, np.int32)
        mask[v] = 1
        ix, am, cnt = np.full(V, index, np.int32), np.full(V, amp), np.ascontiguousarray(count, np.int32)
        mx._lib.check(lib.mxg_envelope_trigger_host(V, ix.ctypes.data, am.ctypes.data, mask.ctypes.data, cnt.ctypes.data, dst.ctypes.data,
                                                    ist.ctypes.data), "mxg_envelope_trigger_host")
    ch.play_env_case(gpu, g, trigger, (777,))
    mx.maxiSettings.setup(48000, 2, 1024)
    try:
        ch.play_env_case(gpu, g, trigger, key="env48", sr=48000.0)
    finally:
        mx.maxiSettings.setup(44100, 2, 1024)


def test_golden_maps(gpu, g):
    """Every mode, cut as stored; the measured figures are printed next to the bounds."""
    res = ch.play_map_cases(gpu, g, (7,))
    print("measured:", res)


# ---- shapes the file does not hold, against the host build ------------------------------------------------------------------
class GuardedGpu:
    """The entry points with every array they write -- outputs and state -- between guard bands of NaN patterns that must come
    back untouched; the interface of classic_host.HostBackend."""

    def __init__(self, mx):
        self.mx, self.L = mx, mx.lib()

    def gate(self, x, thr, hold, att, rel, dst, ist):
        N, V = x.shape
        d = Dev(self.mx)
        thr, att, rel = (np.ascontiguousarray(p) for p in (thr, att, rel))
        o, sd, si = d.out(N, V), d.io(dst), d.io(ist)
        d.call(self.L.mxg_dyn_gate_render, V, N, d.inp(x), d.inp(thr), d.inp(att), d.inp(rel), ch.ps_flags(thr, att, rel), d.inp(hold, np.int64), sd, si, o, None)
        dst[...], ist[...] = sd.back("gate dst"), si.back("gate ist")
        return o.back("gate out")

    def compress(self, x, ratio, thr, att, rel, dst, ist, makeup):
        N, V = x.shape
        d = Dev(self.mx)
        ratio, thr, att, rel = (np.ascontiguousarray(p) for p in (ratio, thr, att, rel))
        o, sd, si = d.out(N, V), d.io(dst), d.io(ist)
        d.call(self.L.mxg_dyn_compress_render, V, N, d.inp(x), d.inp(ratio), d.inp(makeup), d.inp(thr), d.inp(att), d.inp(rel),
               ch.ps_flags(thr, att, rel, ratio), sd, si, o, None)
        dst[...], ist[...] = sd.back("compressor dst"), si.back("compressor ist")
        return o.back("compressor out")

    def line(self, N, seg, count, trig, tindex, tamp, sr, dst, ist):
        S, V = seg.shape
        assert int(self.L.mxg_sample_rate()) == int(sr)
        d = Dev(self.mx)
        o, sd, si = d.out(N, V), d.io(dst), d.io(ist)
        d.call(self.L.mxg_envelope_line_render, V, N, S, d.inp(seg), d.inp(count, np.int32), d.inp(trig), d.inp(tindex, np.int32), d.inp(tamp), sd, si, o, None)
        dst[...], ist[...] = sd.back("line dst"), si.back("line ist")
        return o.back("line out")

    def lag(self, x, alpha, recip, val):
        N, V = x.shape
        d = Dev(self.mx)
        alpha, recip = np.ascontiguousarray(alpha), np.ascontiguousarray(recip)
        o, sv = d.out(N, V), d.io(val)
        d.call(self.L.mxg_lag_render, V, N, d.inp(x), d.inp(alpha), d.inp(recip), int(alpha.ndim == 2), sv, o, None)
        val[...] = sv.back("lag val")
        return o.back("lag out")

    def map(self, mode, x, rng, aux, in_place=False):
        N, V = x.shape
        d = Dev(self.mx)
        o = d.io(x) if in_place else d.out(N, V)
        d.call(self.L.mxg_map_render, ch.MAP_MODES[mode], V, N, o if in_place else d.inp(x), d.inp(rng), d.inp(aux), o, None)
        return o.back("map out")


_cases = {}


def make_case(V, N, host):
    """Inputs with every voice's parameters different, per voice (key 0) and per sample (key 1), and the host build's outputs
    and states over `cuts`; computed once per shape and shared by every knob setting, never written to."""
    if (V, N) in _cases:
        return _cases[(V, N)]
    rng = np.random.default_rng(100000 + 1000 * V + N)
    x = rng.uniform(-1.5, 1.5, (N, V))
    x.flat[::7] = rng.choice(SPECIAL, x.flat[::7].size)

    def both(lo, hi):
        return {0: rng.uniform(lo, hi, V), 1: rng.uniform(lo, hi, (N, V))}
    c = dict(x=x, thr=both(0.1, 1.2), att=both(0.0, 1.0), rel=both(0.8, 1.0), ratio=both(0.5, 9.0), hold=rng.integers(0, 12, V),
             alpha=both(0.0, 1.0), recip=both(0.0, 1.0), val=rng.uniform(-1, 1, V))
    c["makeup"] = {k: host.makeup(r) for k, r in c["ratio"].items()}
    seg = rng.choice([0.0, 0.25, 0.5, 1.0, -0.5], (ENV_S, V))
    seg[1::2] = rng.choice([0.0, 0.02, 0.1, 4 / 48.51], seg[1::2].shape)   # segments of a few samples: tables run to their end
    count = rng.integers(2, ENV_S + 1, V).astype(np.int32)
    c.update(seg=seg, count=count, trig=rng.choice([0.0, 1.0, -2.0, float("nan")], (N, V), p=[0.9, 0.05, 0.03, 0.02]),
             tindex=(rng.integers(0, ENV_S, V) % (count - 1)).astype(np.int32), tamp=rng.uniform(-0.5, 1.0, V))
    # the kernel's one defined departure: a trigger index outside [0, count - 2] and a count outside [1, S] are held (the host build
    # holds them by the same statements; the facades refuse them before a launch)
    tix, cnt = c["tindex"], c["count"]
    if V >= 3:
        tix[0], tix[1], cnt[2] = -1, ENV_S, 0
        if V >= 4:
            cnt[3], tix[3] = ENV_S + 1, ENV_S + 5
    else:
        tix[0], cnt[0] = (-1, ENV_S + 1) if N % 2 else (ENV_S, 0)
    c["env0"] = (rng.uniform(-0.2, 1.0, (2, V)), np.stack([rng.integers(0, ENV_S + 2, V), rng.integers(0, 2, V)]).astype(np.int32))
    r = np.stack([rng.uniform(-1.0, 0.5, V), rng.uniform(0.6, 1.4, V), rng.uniform(1.0, 50.0, V), rng.uniform(60.0, 4000.0, V)])
    r[:, ::5] = r[[1, 0, 3, 2], ::5]    # every fifth voice: reversed ranges
    pos = r.copy()
    pos[0] = np.abs(r[0]) + 0.05        # explin: a positive inMin, so that the logs are finite
    c.update(range=r, range_pos=pos, aux=host.explin_den(pos))
    _cases[(V, N)] = c
    return c


def run_stateful(be, c, ps, cuts, env_trigger):
    """gate, then the compressor on the state the gate left (the two share the members of one maxiDyn), the line with or
    without its trigger block, the lag: outputs and the states after every block."""
    V = c["x"].shape[1]
    sl = lambda p, a, b: p[a:b] if np.ndim(p) == 2 else p  # noqa: E731
    res = []
    dyn, env, val = ch.dyn_fresh(V), (c["env0"][0].copy(), c["env0"][1].copy()), c["val"].copy()
    for a, b in cuts:
        x = c["x"][a:b]
        thr, att, rel, ratio, mk = (sl(c[k][ps], a, b) for k in ("thr", "att", "rel", "ratio", "makeup"))
        res.append(("gate", be.gate(x, thr, c["hold"], att, rel, *dyn), dyn[0].copy(), dyn[1].copy()))
        res.append(("compressor", be.compress(x, ratio, thr, att, rel, *dyn, mk), dyn[0].copy(), dyn[1].copy()))
        trig = c["trig"][a:b] if env_trigger else None
        res.append(("line", be.line(b - a, c["seg"], c["count"], trig, c["tindex"], c["tamp"], 44100.0, *env), env[0].copy(), env[1].copy()))
        res.append(("lag", be.lag(x, sl(c["alpha"][ps], a, b), sl(c["recip"][ps], a, b), val), val.copy()))
    return res


def expected(host, c, ps, cuts, env_trigger):
    key = ("exp", ps, cuts, env_trigger)
    if key not in c:
        c[key] = run_stateful(host, c, ps, cuts, env_trigger)
    return c[key]


def compare(got, exp, what):
    assert len(got) == len(exp)
    for gk, ek in zip(got, exp):
        for i, (a, b) in enumerate(zip(gk[1:], ek[1:])):
            same(a, b, "%s: %s %s" % (what, gk[0], ("output", "state", "integer state")[i]))


@pytest.mark.parametrize("knob", [0, 1])
def test_edge_shapes(mx, host, knob):
    """V = 1 .. 130 x N = 1 .. 71: the tail, the shadow lanes, a chunk remainder; rw_store 0 (automatic) and 1 (8-byte accesses);
    parameters per voice and per sample; the line with and without its trigger block; every map mode, and linlin in place;
    outputs and states between guard bands."""
    be = GuardedGpu(mx)
    with knobs(mx.lib(), rw_store=knob):
        for V, N in SHAPES:
            c = make_case(V, N, host)
            cuts = ((0, N),)
            for ps in (0, 1):
                what = "rw_store %d V %d N %d per %s" % (knob, V, N, "sample" if ps else "voice")
                compare(run_stateful(be, c, ps, cuts, ps == 0), expected(host, c, ps, cuts, ps == 0), what)
            for mode in ch.MAP_MODES:
                rng = c["range_pos"] if mode == "explin" else (c["range"] if mode in ("linlin", "linexp", "clamp") else None)
                aux = c["aux"] if mode == "explin" else None
                xin = np.ascontiguousarray(c["x"] * 40.0) if mode == "dbsToAmp" else c["x"]
                key = ("map", mode)
                if key not in c:
                    c[key] = host.map(mode, xin, rng, aux)
                if mode in ch.EXACT_MAPS:
                    assert_bits_equal(be.map(mode, xin, rng, aux), c[key], "rw_store %d V %d N %d %s" % (knob, V, N, mode))
                    assert_bits_equal(be.map(mode, xin, rng, aux, in_place=True), c[key], "rw_store %d V %d N %d %s in place" % (knob, V, N, mode))
                else:
                    check_quiet(mode, be.map(mode, xin, rng, aux, in_place=(V + N) % 2 == 1), c[key], xin, rng, aux)


def check_quiet(mode, got, ref, x, rng, aux):
    """ch.check_map without its report (hundreds of shapes)."""
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        ch.check_map("edge", mode, got, ref, x, rng, aux)


@pytest.mark.parametrize("V,N", [(64, 71), (130, 71), (130, 8)])
def test_pair_rows(mx, host, V, N):
    """The 16-byte pair rows (rw_store = 2): even V with shadow lanes, whole chunks and a ragged last one."""
    be = GuardedGpu(mx)
    c = make_case(V, N, host)
    with knobs(mx.lib(), rw_store=2):
        for ps in (0, 1):
            compare(run_stateful(be, c, ps, ((0, N),), True), expected(host, c, ps, ((0, N),), True), "pair rows V %d N %d ps %d" % (V, N, ps))


@pytest.mark.parametrize("V,vb", B_SHAPES + A_SHAPES)
def test_workgroup_sizes(mx, host, V, vb):
    """voice_block 64 / 128 / 192 x V in {1, 65, 130, 193, 386}, and -- the stateful kernels are held at one wavefront per
    workgroup up to 16 384 voices -- 128 / 192 / 256 above that: two carried blocks of 9 and 16 samples, every voice's parameters
    different, outputs and states after each block, 8-byte stores and (even V) pair rows."""
    be = GuardedGpu(mx)
    c = make_case(V, 25, host)
    for store in stores(V):
        with knobs(mx.lib(), voice_block=vb, rw_store=store):
            for ps in (0, 1):
                compare(run_stateful(be, c, ps, WG_CUTS, True), expected(host, c, ps, WG_CUTS, True), "voice_block %d V %d rw_store %d ps %d" % (vb, V, store, ps))


def test_a_block_of_repeated_parameters_gives_the_per_voice_bits(mx, host):
    """[N][V] blocks that repeat the per-voice values, under every combination of flags (one kernel serves them all through the
    row strides): the host build's per-voice bits."""
    be = GuardedGpu(mx)
    c = make_case(65, 71, host)
    N, V = c["x"].shape
    exp = expected(host, c, 0, ((0, N),), True)
    blk = lambda p: np.ascontiguousarray(np.broadcast_to(p, (N, V)))  # noqa: E731
    for flags in (1, 2, 4, 8, 5, 10, 15):
        dyn = ch.dyn_fresh(V)
        thr, att, rel, ratio, mk = (c[k][0] for k in ("thr", "att", "rel", "ratio", "makeup"))
        t, a, r = (blk(thr) if flags & 1 else thr), (blk(att) if flags & 2 else att), (blk(rel) if flags & 4 else rel)
        if not flags & 8:
            same(be.gate(c["x"], t, c["hold"], a, r, *dyn), exp[0][1], "gate, flags %d" % flags)
            same(dyn[0], exp[0][2], "gate state, flags %d" % flags)
        else:
            be.gate(c["x"], thr, c["hold"], att, rel, *dyn)
        q, m = (blk(ratio), blk(mk)) if flags & 8 else (ratio, mk)
        same(be.compress(c["x"], q, t, a, r, *dyn, m), exp[1][1], "compressor, flags %d" % flags)
        same(dyn[0], exp[1][2], "compressor state, flags %d" % flags)
        assert np.array_equal(dyn[1], exp[1][3])


def test_python_banks(mx, g):
    """maxiDynBank, maxiEnvelopeBank, maxiLagExpBank and maxiMapBank give the golden bits; a chain stays on the device."""
    D = mx.DeviceBuffer
    x = ch.signal(g["gate/q"])
    N, V = x.shape
    dyn = mx.maxiDynBank(V)
    assert_bits_equal(dyn.gate(D.from_numpy(x), g["gate/thr"], g["gate/hold"], g["gate/att"], g["gate/rel"]).numpy(), g["gate/out"], "gate")
    assert_bits_equal(dyn.dst.numpy(), g["gate/snap7/dst"], "gate state")
    xc = ch.signal(g["comp/q"])
    one = mx.maxiDynBank(1)
    ratio, thr, attack_ms, release_ms = g["comp/setters"]
    one.setRatio(ratio); one.setThreshold(thr); one.setAttack(attack_ms); one.setRelease(release_ms)   # noqa: E702
    assert_bits_equal(one.compress(D.from_numpy(np.ascontiguousarray(xc[:, 3:4]))).numpy(), g["comp/out_members"], "compress() after the setters")
    # a ratio per sample that lives on the device travels with its make-up block: nothing is copied back
    three = mx.maxiDynBank(3)
    rblk = np.ascontiguousarray(np.broadcast_to(g["comp/ratio"], (601, 3)))
    got = three.compressor(D.from_numpy(np.ascontiguousarray(xc[:601, :3])), D.from_numpy(rblk), g["comp/thr"], g["comp/att"], g["comp/rel"],
                           makeup=D.from_numpy(mx.dyn_makeup(rblk)))
    assert_bits_equal(got.numpy(), g["comp/out"][:601], "compressor, ratio and make-up blocks on the device")
    with pytest.raises(ValueError):
        three.compressor(D.from_numpy(np.ascontiguousarray(xc[:601, :3])), D.from_numpy(rblk))
    env = mx.maxiEnvelopeBank(g["env/seg"].shape[1], g["env/seg"], g["env/count"])
    env.trigger(0, 0.0, voices=[3])
    first = env.line(trigger=D.from_numpy(ch.env_trigger_block(g)[:601]), trig_index=g["env/tindex"], trig_amp=g["env/tamp"])
    assert_bits_equal(first.numpy(), g["env/out"][:601], "envelope")
    assert np.array_equal(env.valindex, g["env/snap4/ist"][0]) and np.array_equal(env.amplitude.view(np.uint64), g["env/snap4/dst"][0].view(np.uint64))
    with pytest.raises(mx.MaxiGpuError):
        env.trigger(7, 0.5)   # outside [0, count - 2] for most voices: refused, nothing changes
    lag = mx.maxiLagExpBank(5, g["lag/alpha"], g["lag/val0"])
    lag.setAlphaReciprocal(g["lag/recip"])
    xl = ch.patched(g["lag/q"], g["lag/patches"])
    assert_bits_equal(lag.addSample(D.from_numpy(xl)).numpy(), g["lag/out"], "lag")
    assert_bits_equal(lag.value(), g["lag/snap7/val"], "lag value")
    mp = mx.maxiMapBank(g["map/range"].shape[1])
    xm = D.from_numpy(ch.map_input(g, "linlin"))
    r = g["map/range"]
    assert_bits_equal(mp.linlin(xm, *r).numpy(), g["map/linlin"], "linlin")
    assert_bits_equal(mp.clamp(xm, r[0], r[1]).numpy(), g["map/clamp"], "clamp")
    ch.check_map("bank", "linexp", mp.linexp(xm, *r).numpy(), g["map/linexp"], ch.map_input(g, "linexp"), r, g["map/aux"])
    ch.check_map("bank", "explin", mp.explin(xm, *r).numpy(), g["map/explin"], ch.map_input(g, "explin"), r, g["map/aux"])
    ch.check_map("bank", "ampToDbs", mp.ampToDbs(xm).numpy(), g["map/ampToDbs"], None, None, None)
    # sequencer value -> lag -> range map -> gate threshold per sample, no host array in between
    smooth = mx.maxiLagExpBank(V, 0.05, 0.0).addSample(D.from_numpy(x))
    thr_blk = mx.maxiMapBank(V).linlin(smooth, -0.2, 0.2, 0.3, 0.9)
    got = mx.maxiDynBank(V).gate(D.from_numpy(x), thr_blk, g["gate/hold"], g["gate/att"], g["gate/rel"]).numpy()
    model = ch.ModelBackend()
    val = np.zeros(V)
    t = model.map("linlin", model.lag(x, np.full(V, 0.05), np.full(V, 0.95), val), np.array([[-0.2] * V, [0.2] * V, [0.3] * V, [0.9] * V]))
    assert_bits_equal(got, model.gate(x, t, g["gate/hold"], g["gate/att"], g["gate/rel"], *ch.dyn_fresh(V)), "chain")
    assert len(np.unique(got)) > 1000
