"""GPU (-m gpu): maxiConvolveBank (mxg_convolve_bank_*, kernel K24).  Every stream of a bank is, bit for bit, a maxiConvolve of its
own: against the plain-C port per stream (both modes, the samples split into calls and in one call, the impulse spectra too), against
mx.maxiConvolve objects on the same device (carried state included: one more block after the split), against the fixtures dumped from
the compiled reference with an unrelated stream beside the golden one (no cross-talk); play_nv equals play on the narrowed,
transposed block; reset returns a fresh object's output; host/facade_convolve_smoke exits 0."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

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
