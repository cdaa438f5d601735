"""GPU: mxg_revnet_render (K30, revnet.hip) through maxiReverbNetBank.
The network cases of tests/golden/revnet.npz (arrays of the unmodified reference's maxiReverbFilters objects) bit for bit --
outputs, ring contents, indices, low-pass states -- then against the host build of mxg_revfilt.h (tests/host_revnet.cpp, itself
pinned to the golden file by tests/test_revnet_host.py) from a random state (rings full, indices anywhere) at V in {1, 9, 64} and
N in {1, 63, 64, 65, 200} over topologies without combs, without allpasses, with 32 + 32 short stages, with every length of
{1, 2, 63, 64, 65} as a plain comb and as an allpass, with low-pass combs of 64 and 65 and with both comb kinds mixed; a four-call
sequence whose parameters are rewritten per voice between the calls (feedback beyond 1 and negative, cutoff outside [0, 1]:
nothing clamps them); an input with a NaN and an Inf in one voice; the network given maxiSatReverb's and maxiFreeVerb's numbers
against kernel K13 from the same uploaded state; and one larger bank.
No tolerance and no excluded samples: the arithmetic is + - * with contraction off, a differing bit is a bug.  (NaNs are
compared as positions, see conftest.assert_bits_equal.)  host/facade_revnet_smoke (the C++ facade) exits 0 and prints the checksum
the Python bank gives for the same fixed case."""
import os
import re
import subprocess

import numpy as np
import pytest

import revnet_cases as rc
import revnet_host as rh
from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

SPECIAL = [1, 2, 63, 64, 65]
TOPOLOGIES = {
    "no_combs": dict(combs=[], lowpass=[], aps=SPECIAL + [200]),
    "no_allpasses": dict(combs=SPECIAL + [64, 65, 300], lowpass=[0, 0, 0, 0, 0, 1, 1, 0], aps=[]),
    "wide_32_32": rc.WIDE,
    "special_lengths": dict(combs=SPECIAL, lowpass=[0] * 5, aps=SPECIAL),
    "lowpass_64_65": dict(combs=[64, 65], lowpass=[1, 1], aps=[64]),
    "mixed": dict(combs=[500, 64, 7, 65, 130, 1, 99, 64, 2, 700, 65], lowpass=[1, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0], aps=[33, 640, 1, 65]),
}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return rh.build(tmp_path_factory.mktemp("revnet"))


@pytest.fixture(scope="module")
def g():
    return rh.load_golden()


def make_bank(mx, net):
    """A device bank holding a copy of the host network `net`: topology, parameters and state."""
    b = mx.maxiReverbNetBank(net.V, net.combs, net.aps, net.lowpass, net.comb_fb, net.comb_cut, net.ap_fb)
    assert (b.ring_doubles, b.offsets, b.lengths) == (net.S, net.offsets, net.lengths)
    b.rings.upload(net.rings)
    b.idx.upload(net.idx)
    b.lp.upload(net.lp)
    return b


def bank_parts(b):
    return [("rings", b.rings.numpy()), ("idx", b.idx.numpy()), ("lp", b.lp.numpy())]


def both(mx, host, b, net, x, what):
    """One block on the device bank `b` and on the host network `net`; outputs compared bit for bit."""
    got = b.play(mx.DeviceBuffer.from_numpy(x)).numpy()
    exp = rh.host_render(host, net, x)
    assert_bits_equal(got, exp, what + ": output")
    return got


def scale(V, P):
    """Feedbacks that keep P summed combs and their allpasses lively but finite over a few hundred samples."""
    return 0.9 if P <= 8 else 0.3


def random_net(rng, V, topo):
    P, A = len(topo["combs"]), len(topo["aps"])
    s = scale(V, P)
    return rh.Net(V, topo["combs"], topo["aps"], topo["lowpass"], rng.uniform(-s, s, (V, P)), rng.uniform(0, 1, (V, P)),
                  rng.uniform(-s, s, (V, A))).randomise(rng)


@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_golden_cases(mx, g, case):
    net, x = rh.case_net(case, g)
    b = make_bank(mx, net)
    got, n = [], 0
    for size in (700, 1, 65, len(x)):   # any split into calls
        blk = np.ascontiguousarray(x[n:n + size])
        got.append(b.play(mx.DeviceBuffer.from_numpy(blk)).numpy())
        n += len(blk)
    assert_bits_equal(np.concatenate(got), g[case["name"] + "/out"], case["name"] + ": output")
    rh.check_case_state(case, g, b.rings.numpy(), b.idx.numpy(), b.lp.numpy(), case["name"])


@pytest.mark.parametrize("V", [1, 9, 64])
@pytest.mark.parametrize("topo", sorted(TOPOLOGIES))
def test_shapes_against_host(mx, host, topo, V):
    rng = np.random.default_rng(1000 * V + sorted(TOPOLOGIES).index(topo))
    for N in (1, 63, 64, 65, 200):
        net = random_net(rng, V, TOPOLOGIES[topo])
        b = make_bank(mx, net)
        what = "%s V=%d N=%d" % (topo, V, N)
        both(mx, host, b, net, rng.uniform(-1, 1, (N, V)), what)
        rh.assert_state_equal(bank_parts(b), net.parts(), what)


@pytest.mark.parametrize("topo", ["mixed", "special_lengths"])
def test_call_sequence_with_rewritten_parameters(mx, host, topo):
    """Four calls with changing N on one bank; between them every parameter is rewritten per voice, beyond what a reverb would
    use: the reference clamps none of them here, so neither does the bank."""
    V = 9
    t = TOPOLOGIES[topo]
    P, A = len(t["combs"]), len(t["aps"])
    rng = np.random.default_rng(77)
    net = random_net(rng, V, t)
    net.idx[3, :] = -1            # stored indices outside their rings restart at 0
    net.idx[4, :] = 1 << 24
    b = make_bank(mx, net)
    for k, N in enumerate([65, 1, 200, 63]):
        if k == 1:
            net.comb_fb = rng.uniform(1.0, 1.05, (V, P))       # feedback beyond 1
            net.ap_fb = rng.uniform(-1.1, -0.2, (V, A))        # negative, some beyond -1
            net.comb_cut = rng.uniform(-0.5, 0.0, (V, P))      # cutoff below 0
        elif k == 2:
            net.comb_fb = rng.uniform(-1.05, -0.5, (V, P))
            net.ap_fb = rng.uniform(1.0, 1.1, (V, A))
            net.comb_cut = rng.uniform(1.0, 1.8, (V, P))       # cutoff beyond 1
        elif k == 3:
            net.comb_fb = np.ascontiguousarray(np.broadcast_to(rng.uniform(-0.9, 0.9, P), (V, P)))   # one value per stage
            net.ap_fb = np.full((V, A), 0.5)                                                          # a scalar
            net.comb_cut = rng.uniform(0, 1, (V, P))
        if k:
            b.set_comb_fb(net.comb_fb if k < 3 else net.comb_fb[0])
            b.set_comb_cut(net.comb_cut)
            b.set_ap_fb(net.ap_fb if k < 3 else 0.5)
        both(mx, host, b, net, rng.uniform(-1, 1, (N, V)), "%s call %d (N=%d)" % (topo, k, N))
    rh.assert_state_equal(bank_parts(b), net.parts(), topo + " after the sequence")
    b.clear()
    for name, a in bank_parts(b):
        assert not a.any(), name
    assert_bits_equal(b.comb_fb.numpy(), net.comb_fb, "clear() keeps the parameters")


def test_nan_and_inf_stay_in_their_voice(mx, host):
    V, N, bad = 9, 200, 4
    t = TOPOLOGIES["mixed"]
    rng = np.random.default_rng(41)
    proto = random_net(rng, V, t)
    x = rng.uniform(-1, 1, (N, V))

    def copy():
        n = rh.Net(V, t["combs"], t["aps"], t["lowpass"], proto.comb_fb, proto.comb_cut, proto.ap_fb)
        n.rings, n.idx, n.lp = proto.rings.copy(), proto.idx.copy(), proto.lp.copy()
        return n

    clean = make_bank(mx, copy()).play(mx.DeviceBuffer.from_numpy(x)).numpy()
    x[20, bad] = np.nan
    x[90, bad] = np.inf
    net = copy()
    b = make_bank(mx, net)
    got = both(mx, host, b, net, x, "a NaN and an Inf in voice %d" % bad)
    assert np.isnan(got[:, bad]).any()
    keep = np.arange(V) != bad
    assert np.isfinite(got[:, keep]).all()
    assert_bits_equal(got[:, keep], clean[:, keep], "the other voices")
    for (name, a), (_, e) in zip(bank_parts(b), net.parts()):
        if name == "idx":
            assert np.array_equal(a, e)
        else:
            assert np.array_equal(np.isnan(a), np.isnan(e)), name
            assert_bits_equal(a, e, name)


@pytest.mark.parametrize("form", ["sat", "fv4", "fv31"])
def test_equals_k13_on_its_numbers(mx, form):
    """The network given a factory reverb's numbers, from the same uploaded random state, against reverb.hip."""
    V, N = 31, 200
    rng = np.random.default_rng({"sat": 1, "fv4": 2, "fv31": 3}[form])
    x = mx.DeviceBuffer.from_numpy(rng.uniform(-1, 1, (N, V)))
    if form == "sat":
        ref = mx.maxiSatReverbBank(V)
        net = mx.maxiReverbNetBank(V, rc.SAT["combs"], rc.SAT["aps"], None, 0.85, 0.2, 0.85)
    else:
        ref = mx.maxiFreeVerbBank(V)
        t = rc.FV if form == "fv4" else rc.FV31
        net = mx.maxiReverbNetBank(V, t["combs"], t["aps"], t["lowpass"], 0.84, 0.2, 0.85)
    assert (net.lengths, net.offsets, net.ring_doubles) == (ref.lengths[:len(net.lengths)], ref.offsets[:len(net.lengths)],
                                                            sum(net.lengths))
    F, S = len(net.lengths), net.ring_doubles
    rings = rng.uniform(-1, 1, (V, ref.ring_doubles))
    idx = (rng.integers(0, 1 << 30, (V, len(ref.lengths))) % np.array(ref.lengths)).astype(np.int32)
    ref.rings.upload(rings)
    ref.idx.upload(idx)
    net.rings.upload(rings[:, :S])
    net.idx.upload(idx[:, :F])
    if form != "sat":
        lp = rng.uniform(-1, 1, (V, 8))
        ref.lp.upload(lp)
        net.lp.upload(lp)
    if form == "fv31":
        room, absorb = rng.uniform(-6.0, 1.5, V), rng.uniform(0.0, 1.0, V)   # held for the whole block
        exp = ref.play(x, room, absorb).numpy()
        wc = ref.wc.numpy()
        assert_bits_equal(wc[:, 0], np.clip(room * 0.10 + 0.84, 0.0, 1.0), "w")
        net.set_comb_fb(np.repeat(wc[:, :1], 8, axis=1))
        net.set_comb_cut(np.repeat(wc[:, 1:], 8, axis=1))
    else:
        exp = ref.play(x).numpy()
    got = net.play(x).numpy()
    assert_bits_equal(got, exp, form + ": output")
    assert_bits_equal(net.rings.numpy(), ref.rings.numpy()[:, :S], form + ": rings")
    assert np.array_equal(net.idx.numpy(), ref.idx.numpy()[:, :F]), form + ": ring indices"
    if form != "sat":
        assert_bits_equal(net.lp.numpy(), ref.lp.numpy(), form + ": low-pass states")


def test_larger_bank(mx, host):
    V, N = 1000, 512
    rng = np.random.default_rng(1000)
    net = rh.Net(V, rc.FV_COMBS, rc.FV_APS + [13, 64], [1, 1, 0, 1, 1, 0, 1, 1], rng.uniform(0.7, 0.9, (V, 8)), rng.uniform(0, 0.5, (V, 8)),
                 rng.uniform(0.3, 0.9, (V, 6)))
    net.rings = np.ascontiguousarray(np.resize(rng.uniform(-1, 1, 1000003), (V, net.S)))
    net.idx = (rng.integers(0, 1 << 30, (V, 14)) % np.array(net.lengths)).astype(np.int32)
    net.lp = rng.uniform(-1, 1, (V, 8)) * np.array(net.lowpass, np.float64)
    b = make_bank(mx, net)
    both(mx, host, b, net, rng.uniform(-1, 1, (N, V)), "V=%d N=%d" % (V, N))
    rh.assert_state_equal(bank_parts(b), net.parts(), "V=%d" % V)


def test_facade_revnet_smoke_prints_the_python_banks_checksum(mx):
    exe = os.path.join(ROOT, "host", "facade_revnet_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_revnet_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "facade_revnet_smoke OK" in r.stdout, r.stdout + r.stderr
    # the fixed case of host/facade_revnet_smoke.cpp: every value exact in binary
    V, N = 21, 700
    n, v = np.arange(N)[:, None], np.arange(V)[None, :]
    x = np.where(v == 3, 0.0, ((n * (7 + v)) % 200) / 128.0 - 0.75)
    vv = np.arange(V)[:, None]
    cfb = 0.5 + vv / 64.0 - np.arange(3)[None, :] / 8.0
    cut = np.repeat((vv % 8) / 8.0, 3, axis=1)
    afb = 0.25 + vv / 32.0 - np.arange(2)[None, :] / 2.0
    b = mx.maxiReverbNetBank(V, [778, 64, 7], [125, 12], [0, 1, 0], cfb, cut, afb)
    out = b.play(mx.DeviceBuffer.from_numpy(np.ascontiguousarray(x))).numpy()
    h = 1469598103934665603
    for w in out.reshape(-1).view(np.uint64).tolist():
        h = ((h * 1099511628211) & 0xffffffffffffffff) ^ w
    assert re.search(r"checksum ([0-9a-f]{16})", r.stdout).group(1) == "%016x" % h
