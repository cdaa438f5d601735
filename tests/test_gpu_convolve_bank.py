"""GPU (-m gpu): maxiConvolveBank (mxg_convolve_bank_*, kernel K24).  Every stream of a bank is, bit for bit, a maxiConvolve of its
own: against the plain-C port per stream (both modes, the samples split into calls and in one call, the impulse spectra too), against
mx.maxiConvolve objects on the same device (carried state included: one more block after the split), against the fixtures dumped from
the compiled reference with an unrelated stream beside the golden one (no cross-talk); play_nv equals play on the narrowed,
transposed block; reset returns a fresh object's output; host/facade_convolve_smoke exits 0.

Below "the ring wraps" the parts that exist only on the device -- the ring of R = max K - 1 + 16 rows, its head word and the kernel
that advances it, the chunk loop of bank_play(), the block decode -- always against the port fed the whole input per stream, never
against another GPU run: more blocks than the ring has rows, in splits that tests/convolve_host.py's model of the head shows to
straddle the ring's end, land on slot 0, read history across the end and span launches; every launch geometry from 2 live lanes to
8 workgroups a row; 193 streams on 7 impulses in an order that is a real permutation; play_nv against the port; play and play_nv
between guard bands; two banks of different fftsize sharing the scratch slot call by call."""
import functools
import os
import subprocess

import numpy as np
import pytest

import convolve_host as ch
from conftest import ROOT
from test_gpu_workgroups import Dev

pytestmark = pytest.mark.gpu

IMP_OF = [0, 1, 0]
NB = 11  # blocks per stream: 10 go through in the splits below, the 11th shows the state they left
SPLITS = ([2, 7, 1, 1], [1, 1, 1, 5, 2, 1], [11])
# name -> (fftsize, hopsize, impulse lengths): frames = (len + bins - len % bins) // fftsize
CASES = {
    "k5_k1": (64, 16, (300, 40)),
    "k0_k5": (64, 16, (20, 300)),
    "k1_k0": (64, 16, (40, 20)),
    "k3_k1": (1024, 256, (2600, 900)),
    "k1_k39": (1024, 512, (900, 40000)),
}
FRAMES = {"k5_k1": (5, 1), "k0_k5": (0, 5), "k1_k0": (1, 0), "k3_k1": (3, 1), "k1_k39": (1, 39)}


def f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    F, H, lens = CASES[name]
    rng = np.random.default_rng(sum(lens) + F)
    pcms = tuple((rng.uniform(-1, 1, L) * np.exp(-np.arange(L) / (L / 5.0)) * 25000).astype(np.int16) for L in lens)
    x = rng.uniform(-1, 1, (len(IMP_OF), NB * F)).astype(np.float32)
    x.setflags(write=False)
    return pcms, x


def make_bank(mx, name):
    F, H, _ = CASES[name]
    pcms, _ = inputs(name)
    return mx.maxiConvolveBank(len(IMP_OF), [p / 32767.0 for p in pcms], IMP_OF, F, H)


def play_split(bank, x, split, mode):
    F = bank.fftsize
    out, at = [], 0
    for nb in split:
        out.append(bank.play(np.ascontiguousarray(x[:, at * F:(at + nb) * F]), mode).numpy())
        at += nb
    return np.concatenate(out, axis=1)


_oracle = {}


def oracle(port, name, mode):
    """port.convolve per stream, computed once per (case, mode) and shared"""
    if (name, mode) not in _oracle:
        F, H, _ = CASES[name]
        pcms, x = inputs(name)
        _oracle[name, mode] = [port.convolve(pcms[i], x[v], F, H, mode) for v, i in enumerate(IMP_OF)]
    return _oracle[name, mode]


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", list(CASES))
def test_bank_vs_port(mx, port, name, mode):
    _, x = inputs(name)
    exp = oracle(port, name, mode)
    bank = make_bank(mx, name)
    assert tuple(bank.frames) == FRAMES[name]
    for v, i in enumerate(IMP_OF):
        assert exp[v][1].shape[0] == bank.frames[i]
        r, im = bank.impulse(i)
        assert np.array_equal(f32bits(r), f32bits(exp[v][1])) and np.array_equal(f32bits(im), f32bits(exp[v][2])), "impulse %d" % i
    e = np.stack([exp[v][0] for v in range(len(IMP_OF))])
    if mode == 1:
        assert np.abs(e).max() > 1e-3
    for split in SPLITS:
        bank.reset()
        o = play_split(bank, x, split, mode)
        for v in range(len(IMP_OF)):
            assert np.array_equal(f32bits(o[v]), f32bits(e[v])), "stream %d, calls %s" % (v, split)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", list(CASES))
def test_bank_vs_single_objects(mx, name, mode):
    """mx.maxiConvolve objects fed the whole input in one call; the bank in calls of 2, 7, 1 blocks and then one more block, whose
    output depends on everything the split left behind (ring, pending sums)."""
    F, H, _ = CASES[name]
    pcms, x = inputs(name)
    bank = make_bank(mx, name)
    o = play_split(bank, x, SPLITS[0], mode)
    for v, i in enumerate(IMP_OF):
        c = mx.maxiConvolve()
        c.setup(pcms[i] / 32767.0, F, H)
        assert c.frames == bank.frames[i]
        if c.frames:
            r, im = c.impulse()
            br, bi = bank.impulse(i)
            assert np.array_equal(f32bits(r), f32bits(br)) and np.array_equal(f32bits(im), f32bits(bi))
        e = c.play(x[v], mode).numpy()
        assert np.array_equal(f32bits(o[v]), f32bits(e)), "stream %d" % v


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_bank_golden_no_crosstalk(mx, golden, tag):
    g = golden("convolve.npz")
    F, H = (int(v) for v in g["cfg_" + tag])
    pcm, x = g["pcm_" + tag], g["x_" + tag]
    other = np.random.default_rng(F + H).uniform(-1, 1, x.size).astype(np.float32)
    xs = np.stack([np.ascontiguousarray(x, np.float32), other])
    bank = mx.maxiConvolveBank(2, [pcm / 32767.0], [0, 0], F, H)
    assert bank.frames[0] == g["impR_" + tag].shape[0]
    r, i = bank.impulse(0)
    assert np.array_equal(f32bits(r), f32bits(g["impR_" + tag])) and np.array_equal(f32bits(i), f32bits(g["impI_" + tag]))
    for mode in (0, 1):
        bank.reset()
        o = np.concatenate([bank.play(np.ascontiguousarray(xs[:, :4 * F]), mode).numpy(),
                            bank.play(np.ascontiguousarray(xs[:, 4 * F:]), mode).numpy()], axis=1)
        assert np.array_equal(f32bits(o[0]), f32bits(g["out%d_%s" % (mode, tag)])), "mode %d" % mode
        if mode == 1:
            assert not np.array_equal(o[0], o[1])


@pytest.mark.parametrize("V", [3, 70])
def test_play_nv_equals_play(mx, V):
    """doubles [N][V] against floats [V][N]: V = 3 and 70 are ragged against the 32 x 32 tiles of the transposes; the doubles carry
    digits a float does not, so the narrowing is a real rounding."""
    F, H, nb = 64, 16, 5
    rng = np.random.default_rng(V)
    imps = [rng.uniform(-1, 1, 300), rng.uniform(-1, 1, 100)]
    imp_of = [v % 2 for v in range(V)]
    x = rng.uniform(-1, 1, (nb * F, V))
    assert not np.array_equal(x.astype(np.float32).astype(np.float64), x)
    a = mx.maxiConvolveBank(V, imps, imp_of, F, H)
    b = mx.maxiConvolveBank(V, imps, imp_of, F, H)
    for lo, hi in ((0, 2 * F), (2 * F, nb * F)):  # two calls: the state is carried on this path too
        o_nv = a.play_nv(np.ascontiguousarray(x[lo:hi]), 1).numpy()
        o = b.play(np.ascontiguousarray(x[lo:hi].T.astype(np.float32)), 1).numpy()
        assert o_nv.shape == (hi - lo, V) and o_nv.dtype == np.float64
        assert np.abs(o).max() > 1e-3
        assert np.array_equal(o_nv.view(np.uint64), np.ascontiguousarray(o.T.astype(np.float64)).view(np.uint64))


def test_reset_returns_a_fresh_bank(mx):
    name = "k5_k1"
    _, x = inputs(name)
    bank = make_bank(mx, name)
    first = play_split(bank, x, [3, 2], 1)
    again = play_split(bank, x, [3, 2], 1)   # the state moved on: the first block now carries the previous input's tail
    assert not np.array_equal(first, again)
    bank.reset()
    fresh = play_split(bank, x, [5], 1)
    assert np.array_equal(f32bits(fresh), f32bits(first))


def test_play_rejects_bad_arguments(mx):
    L = mx.lib()
    bank = make_bank(mx, "k5_k1")
    b = mx.DeviceBuffer(3 * 64, np.float32)
    assert L.mxg_convolve_bank_play(bank.h, b.ptr, 1, b.ptr, 2, None) == -1      # unknown mode
    assert L.mxg_convolve_bank_play(bank.h, b.ptr, 0, b.ptr, 0, None) == 0       # empty call
    assert L.mxg_convolve_bank_play(bank.h, None, 1, b.ptr, 0, None) == -1
    assert L.mxg_convolve_bank_play_nv(bank.h, b.ptr, 1, None, 0, None) == -1
    assert L.mxg_convolve_bank_frames(bank.h, 7) == 0


def test_facade_convolve_smoke():
    exe = os.path.join(ROOT, "host", "facade_convolve_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "facade_convolve_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


# =====================================================================================================================
# The ring wraps, calls span launches, every launch geometry, many streams (shapes and the model of the head: convolve_host.py)
# =====================================================================================================================
def impulse_pcm(rng, L):
    return (rng.uniform(-1, 1, L) * np.exp(-np.arange(L) / (L / 5.0)) * 25000).astype(np.int16)


@functools.lru_cache(maxsize=None)
def wrap_inputs(name):
    F, H, lens, _ = ch.ALL_CASES[name]
    rng = np.random.default_rng(sum(lens) + F + H)
    pcms = tuple(impulse_pcm(rng, L) for L in lens)
    x = rng.uniform(-1, 1, (len(IMP_OF), ch.case_blocks(name) * F)).astype(np.float32)
    x.setflags(write=False)
    return pcms, x


def wrap_bank(mx, name):
    F, H, _, _ = ch.ALL_CASES[name]
    pcms, _ = wrap_inputs(name)
    bank = mx.maxiConvolveBank(len(IMP_OF), [p / 32767.0 for p in pcms], IMP_OF, F, H)
    assert tuple(bank.frames) == ch.case_frames(name)
    return bank


def wrap_oracle(port, name, mode, blocks=None, twice=False):
    """port.convolve per stream over the whole input (its first `blocks` blocks; or the input fed twice), once per key, shared"""
    key = ("wrap", name, mode, blocks, twice)
    if key not in _oracle:
        F, H, _, _ = ch.ALL_CASES[name]
        pcms, x = wrap_inputs(name)
        xs = x if blocks is None else x[:, :blocks * F]
        xs = np.concatenate([xs, xs], axis=1) if twice else xs
        _oracle[key] = [port.convolve(pcms[i], xs[v], F, H, mode) for v, i in enumerate(IMP_OF)]
    return _oracle[key]


def assert_evidence(e, frames, imp_of, F, mode):
    """On the REFERENCE's output: mode 0 is silence by construction and shows nothing; in mode 1 the last block -- the one that depends
    on everything the earlier calls left behind -- is live in every stream that has an impulse frame, and a stream without one is silent."""
    for v, i in enumerate(imp_of):
        if mode == 0 or frames[i] == 0:
            assert not e[v].any(), v
        else:
            assert np.abs(e[v][-F:]).max() > 1e-3, v


def assert_streams(o, e, what):
    for v in range(len(e)):
        assert np.array_equal(f32bits(o[v]), f32bits(e[v])), "stream %d, %s" % (v, what)


def check_impulses(bank, exp, imp_of):
    for i in range(bank.I):
        v = list(imp_of).index(i)
        r, im = bank.impulse(i)
        assert exp[v][1].shape[0] == bank.frames[i]
        assert np.array_equal(f32bits(r), f32bits(exp[v][1])) and np.array_equal(f32bits(im), f32bits(exp[v][2])), "impulse %d" % i


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", list(ch.WRAP_CASES))
def test_ring_wraps_and_calls_span_launches(mx, port, name, mode):
    F, H, _, splits = ch.WRAP_CASES[name]
    _, x = wrap_inputs(name)
    bank = wrap_bank(mx, name)
    R, Kmax = ch.ring_rows(bank.frames), max(bank.frames)
    assert ch.case_blocks(name) > R + Kmax
    assert set().union(*(ch.ring_events(R, Kmax, s) for s in splits)) == ch.EVENTS
    exp = wrap_oracle(port, name, mode)
    check_impulses(bank, exp, IMP_OF)
    e = [exp[v][0] for v in range(len(IMP_OF))]
    assert_evidence(e, bank.frames, IMP_OF, F, mode)
    for split in splits:
        bank.reset()
        assert_streams(play_split(bank, x, split, mode), e, "calls %s" % (split,))


def test_second_feed_starts_at_a_moved_head(mx, port):
    """No reset between two feeds of the same 45 blocks: the second long call starts at head 5 of 20, on a ring full of the first."""
    name = "k5_k1"
    F = ch.WRAP_CASES[name][0]
    _, x = wrap_inputs(name)
    bank = wrap_bank(mx, name)
    R, Kmax, nb = ch.ring_rows(bank.frames), max(bank.frames), ch.case_blocks(name)
    assert ch.ring_head(R, [nb]) != 0
    assert ch.ring_events(R, Kmax, [nb, nb]) >= {"later_chunk", "store_wrap", "read_wrap"}
    e = [s[0] for s in wrap_oracle(port, name, 1, twice=True)]
    assert_evidence(e, bank.frames, IMP_OF, F, 1)
    o = np.concatenate([play_split(bank, x, [nb], 1), play_split(bank, x, [nb], 1)], axis=1)
    assert_streams(o, e, "two feeds of %d blocks" % nb)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", list(ch.GEOMETRY_CASES))
def test_every_launch_geometry(mx, port, name, mode):
    F, H, _, (split,) = ch.GEOMETRY_CASES[name]
    _, x = wrap_inputs(name)
    bank = wrap_bank(mx, name)
    R, Kmax = ch.ring_rows(bank.frames), max(bank.frames)
    assert Kmax >= 2 and sum(split) > R + Kmax
    assert ch.ring_events(R, Kmax, split) == ch.EVENTS
    exp = wrap_oracle(port, name, mode)
    check_impulses(bank, exp, IMP_OF)
    e = [exp[v][0] for v in range(len(IMP_OF))]
    assert_evidence(e, bank.frames, IMP_OF, F, mode)
    assert_streams(play_split(bank, x, split, mode), e, "calls %s" % (split,))


MANY_V, MANY_LENS, MANY_SPLIT = 193, (300, 20, 100, 40, 170, 230, 60), [19, 1, 2, 23]   # frames 5, 0, 2, 1, 3, 4, 1


def test_many_streams_in_a_permuted_order(mx, port):
    """193 = 3 * 64 + 1 streams on 7 impulses, imp_of drawn from a seeded generator: `order`, the stable sort by impulse, is a real
    permutation, so a stream that got its neighbour's impulse rows, ring or pending row differs from its own maxiConvolve.  Every
    stream has its own input."""
    F, H, V, nb = 64, 64, MANY_V, sum(MANY_SPLIT)
    rng = np.random.default_rng(193)
    pcms = [impulse_pcm(rng, L) for L in MANY_LENS]
    imp_of = rng.integers(0, len(pcms), V)
    x = rng.uniform(-1, 1, (V, nb * F)).astype(np.float32)
    assert set(imp_of.tolist()) == set(range(len(pcms)))
    assert (np.diff(imp_of) < 0).any()                                                  # not sorted
    assert not any(np.array_equal(imp_of[p:], imp_of[:-p]) for p in range(1, V))        # not periodic
    order = np.argsort(imp_of, kind="stable")
    assert not any(np.array_equal(order, (np.arange(V) + r) % V) for r in range(V))     # neither the identity nor a rotation
    bank = mx.maxiConvolveBank(V, [p / 32767.0 for p in pcms], imp_of, F, H)
    assert tuple(bank.frames) == tuple(ch.frames_of(L, F) for L in MANY_LENS) == (5, 0, 2, 1, 3, 4, 1)
    R, Kmax = ch.ring_rows(bank.frames), max(bank.frames)
    assert ch.ring_events(R, Kmax, MANY_SPLIT) == ch.EVENTS
    exp = [port.convolve(pcms[i], x[v], F, H, 1) for v, i in enumerate(imp_of)]
    check_impulses(bank, exp, imp_of)
    e = [s[0] for s in exp]
    assert_evidence(e, bank.frames, imp_of, F, 1)
    assert_streams(play_split(bank, x, MANY_SPLIT, 1), e, "calls %s" % MANY_SPLIT)


def test_play_nv_vs_port(mx, port):
    """doubles [N][V], V = 70 (ragged against the 32 x 32 tiles of the transposes), two calls of 19 and 26 blocks; the expectation is
    the port fed the narrowed column, widened."""
    F, H, V, calls = 64, 16, 70, [19, 26]
    rng = np.random.default_rng(70)
    pcms = [impulse_pcm(rng, 300), impulse_pcm(rng, 100)]
    imp_of = [v % 2 for v in range(V)]
    x = rng.uniform(-1, 1, (sum(calls) * F, V))
    assert not np.array_equal(x.astype(np.float32).astype(np.float64), x)   # the narrowing is a real rounding
    bank = mx.maxiConvolveBank(V, [p / 32767.0 for p in pcms], imp_of, F, H)
    assert tuple(bank.frames) == (5, 2)
    assert ch.ring_events(ch.ring_rows(bank.frames), 5, calls) >= {"later_chunk", "store_wrap"}
    e = [port.convolve(pcms[i], x[:, v].astype(np.float32), F, H, 1)[0] for v, i in enumerate(imp_of)]
    assert_evidence(e, bank.frames, imp_of, F, 1)
    at, out = 0, []
    for nb in calls:
        o = bank.play_nv(np.ascontiguousarray(x[at * F:(at + nb) * F]), 1).numpy()
        assert o.shape == (nb * F, V) and o.dtype == np.float64
        out.append(o)
        at += nb
    o = np.concatenate(out)
    for v in range(V):
        assert np.array_equal(np.ascontiguousarray(o[:, v]).view(np.uint64), e[v].astype(np.float64).view(np.uint64)), "stream %d" % v


@pytest.mark.parametrize("nv", [False, True])
def test_nothing_written_outside_the_output(mx, port, nv):
    """play and play_nv through the C-ABI, the output between guard bands, the input compared with what was uploaded: fftsize 2048
    (two lane blocks a row), 17 blocks (the second chunk is one frame: a single ragged tile)."""
    name, nb = "f2048", 17
    F = ch.GEOMETRY_CASES[name][0]
    V, N = len(IMP_OF), nb * F
    x = wrap_inputs(name)[1][:, :N]
    bank = wrap_bank(mx, name)
    e = np.stack([s[0] for s in wrap_oracle(port, name, 1, blocks=nb)])
    assert_evidence(e, bank.frames, IMP_OF, F, 1)
    L, d = mx.lib(), Dev(mx)
    if nv:
        xin = np.ascontiguousarray(x.T, np.float64)
        d.inp(xin, np.float64)
        out = d.io(np.full((N, V), -7.5, np.float64))
        d.call(L.mxg_convolve_bank_play_nv, bank.h, d.keep[0].ptr, nb, out, 1, None)
        o = out.back("the output of play_nv").T
        assert o.dtype == np.float64 and np.array_equal(o.astype(np.float32).astype(np.float64), o)
    else:
        xin = np.ascontiguousarray(x, np.float32)
        d.inp(xin, np.float32)
        out = d.io(np.full((V, N), -7.5, np.float32))
        d.call(L.mxg_convolve_bank_play, bank.h, d.keep[0].ptr, nb, out, 1, None)
        o = out.back("the output of play")
    assert_streams(o, e, "guarded")
    assert np.array_equal(d.keep[0].numpy().view(np.uint8), xin.view(np.uint8)), "the input was written"


def test_two_banks_share_the_scratch_slot(mx, port):
    """Banks of fftsize 64 and 512 played alternately, call by call, on the default stream: the scratch slot they share changes size
    in both directions between calls, while each bank's ring and head live on."""
    names = ("k5_k1", "f512")
    banks = [wrap_bank(mx, n) for n in names]
    splits = [ch.WRAP_CASES["k5_k1"][3][3], ch.GEOMETRY_CASES["f512"][3][0]]
    assert len(splits[0]) == len(splits[1])
    sizes = [[nb * ch.ALL_CASES[n][0] for nb in s] for n, s in zip(names, splits)]
    seq = [sizes[k % 2][k // 2] for k in range(2 * len(splits[0]))]   # the scratch is a multiple of this: the call's samples
    assert any(a < b for a, b in zip(seq, seq[1:])) and any(a > b for a, b in zip(seq, seq[1:]))
    outs, at = [[], []], [0, 0]
    for k in range(len(splits[0])):
        for j, bank in enumerate(banks):
            F, nb = bank.fftsize, splits[j][k]
            outs[j].append(bank.play(np.ascontiguousarray(wrap_inputs(names[j])[1][:, at[j] * F:(at[j] + nb) * F]), 1).numpy())
            at[j] += nb
    for j, n in enumerate(names):
        e = [s[0] for s in wrap_oracle(port, n, 1)]
        assert_evidence(e, banks[j].frames, IMP_OF, banks[j].fftsize, 1)
        R, Kmax = ch.ring_rows(banks[j].frames), max(banks[j].frames)
        assert ch.ring_events(R, Kmax, splits[j]) == ch.EVENTS
        assert_streams(np.concatenate(outs[j], axis=1), e, "bank %s" % n)
