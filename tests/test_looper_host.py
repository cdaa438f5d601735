"""CPU (-m "not gpu"): K25's arithmetic (maximilian_amd/csrc/mxg_looper.h) in its host build (tests/host_looper.cpp, g++ under
the oracle's FPFLAGS) and through the library's _host twins (mxg_looprec_host, mxg_sample_pool_normalise_host) against the
reference's own bits (tests/golden/looper.npz): outputs, recordPosition, the lag's val, position and the whole content of every
slot -- guards and tails included -- at every stored cut and at further ones.  A seeded fuzz of 200 small cases then compares a
block call with the same call made one sample at a time and with random splits.  Also: the restated players step as mxg_smp.h's
do; the entry points are declared, exported and bound; the classes are present; every bad argument is refused by name before a
device is touched; and the one departure (an index outside [0, len)) behaves as specified."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import looper_host as lh
from conftest import ROOT, assert_bits_equal

EXTRA = (7, 64, 777, 1500)
ENTRY = ["mxg_sample_pool_alloc", "mxg_sample_pool_free", "mxg_sample_pool_stride", "mxg_sample_pool_lengths", "mxg_looprec_render",
         "mxg_looprec_host", "mxg_looprec_piece", "mxg_looprec_tile", "mxg_sample_pool_normalise", "mxg_sample_pool_normalise_host"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return lh.HostBackend(lh.build(tmp_path_factory.mktemp("looper_host")))


@pytest.fixture(scope="module")
def twin():
    import maximilian_amd as m
    return lh.TwinBackend(m)


@pytest.fixture(scope="module")
def g(golden):
    return golden("looper.npz")


@pytest.fixture(params=["host", "twin"])
def be(request, host, twin):
    return host if request.param == "host" else twin


@pytest.mark.parametrize("key", ["loop", "play"])
def test_golden_record_and_play(be, g, key):
    lh.check_cuts(be, g, key)
    lh.check_cuts(be, g, key, EXTRA)


@pytest.mark.parametrize("piece,tile", [(128, 8), (1, 1), (5, 3), (64, 8), (2000, 8)])
@pytest.mark.parametrize("key", ["loop", "play"])
def test_golden_as_the_kernel_cuts_it(host, g, key, piece, tile):
    """The decomposition of K25 -- the plan of a piece, the walk over an element's visits, all loads before the stores -- run on the
    host over the golden cases, for the kernel's piece and tile and for others."""
    lh.check_cuts(lh.PiecesBackend(host.L, piece, tile), g, key)


def test_fuzz_pieces_against_single_samples(host):
    """Random cases, outside the domain among them (bounds beyond [0, 1], NaN, heads uploaded out of range), where the plan has to
    search: the pieces give what sample after sample gives."""
    rng = np.random.default_rng(2503)
    for rep in range(300):
        Rr, Nn = int(rng.integers(1, 12)), int(rng.integers(1, 400))
        b0, x, en = lh.random_case(rng, Rr, Nn, cap=int(rng.integers(2, 200)))
        if rep % 3 == 0:
            k = int(rng.integers(0, Rr))
            b0.start[k], b0.end[k] = rng.choice([-0.5, 0.3, 1.0, 1.5, lh.NAN]), rng.choice([-0.2, 0.0, 0.6, 2.0, lh.NAN])
            b0.recpos[k] = rng.choice([-3.0, 0.0, 7.5, 1e9])
            b0.position[k] = rng.choice([-7.0, 0.0, 1e12, lh.NAN])
        mode = int(rng.choice([lh.PLAY_NONE, lh.PLAY, lh.PLAYLOOP]))
        ref, got = b0.copy(), b0.copy()
        o = host.render(ref, x, en, mode)
        p = lh.PiecesBackend(host.L, int(rng.choice([1, 3, 16, 128])), int(rng.choice([1, 4, 8]))).render(got, x, en, mode)
        lh.same_bank(got, ref, "fuzz %d" % rep)
        if mode != lh.PLAY_NONE:
            assert_bits_equal(p, o, "fuzz %d: output" % rep)
        assert not got.outside().any()


def test_golden_normalise(be, g):
    lh.check_normalise(be, g)


def test_layout_constants(host, twin):
    lo, hi = ctypes.c_int(0), ctypes.c_int(0)
    host.L.lp_h_guards(ctypes.byref(lo), ctypes.byref(hi))
    assert (lo.value, hi.value) == (lh.GUARD_LO, lh.GUARD_HI)
    for cap in (1, 2, 6, 7, 300, 4096, 44100):
        assert twin.lib.mxg_sample_pool_stride(cap) == lh.stride_of(cap) >= cap + lh.GUARD_LO + lh.GUARD_HI


def test_players_step_as_mxg_smp(host):
    """lp_play_step (mxg_looper.h) against smp_gen<0> / smp_gen<2> (mxg_smp.h), call after call from the same head."""
    rng = np.random.default_rng(2501)
    for rep in range(300):
        n = int(rng.integers(1, 700))
        s, e = rng.uniform(0, 1), rng.uniform(0, 1)
        if rep % 3 == 0:
            s, e = 0.0, 1.0
        pa = ctypes.c_double(float(np.floor(rng.uniform(-1, n + 1))) if rep % 2 else float(rng.uniform(-1, n + 1)))
        pb = ctypes.c_double(pa.value)
        for mode in (lh.PLAY, lh.PLAYLOOP):
            for _ in range(40):
                ia = host.L.lp_h_play_step(mode, ctypes.byref(pa), s, e, n)
                ib = host.L.lp_h_smp_step(mode, ctypes.byref(pb), s, e, n)
                assert ia == ib and pa.value == pb.value, (rep, mode, n, s, e)


def test_fuzz_block_against_single_samples_and_splits(host, twin):
    rng = np.random.default_rng(2502)
    for rep in range(200):
        Rr, Nn = int(rng.integers(1, 6)), int(rng.integers(1, 701))
        b0, x, en = lh.random_case(rng, Rr, Nn)
        mode = int(rng.choice([lh.PLAY_NONE, lh.PLAY, lh.PLAYLOOP]))
        whole = b0.copy()
        be = twin if rep % 2 else host
        ow = be.render(whole, x, en, mode)
        one = b0.copy()
        sl = (lambda a, c: en[a:c]) if en.ndim == 2 else (lambda a, c: en)
        o1 = [host.render(one, x[n:n + 1], sl(n, n + 1), mode) for n in range(Nn)]
        lh.same_bank(whole, one, "fuzz %d: block against single samples" % rep)
        cuts = sorted(set(rng.integers(0, Nn + 1, 4).tolist()) | {0, Nn})
        part = b0.copy()
        op = [be.render(part, x[a:c], sl(a, c), mode) for a, c in zip(cuts[:-1], cuts[1:])]
        lh.same_bank(whole, part, "fuzz %d: block against splits" % rep)
        if mode != lh.PLAY_NONE:
            assert_bits_equal(np.concatenate(o1), ow, "fuzz %d: output, single samples" % rep)
            assert_bits_equal(np.concatenate(op), ow, "fuzz %d: output, splits" % rep)
        assert not whole.dropped.any() and not whole.outside().any(), "fuzz %d: inside the domain nothing is dropped" % rep


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in ENTRY:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    assert re.search(r"#define MXG_LOOPER_PLAY_NONE \(-1\)", hdr)
    assert m.lib().mxg_looprec_piece() >= 64 and m.lib().mxg_looprec_tile() >= 1


def test_classes_present():
    import maximilian_amd as m
    assert hasattr(m, "maxiLooperBank")
    assert re.search(r"\bclass maxiLooperBank\b", open(os.path.join(ROOT, "maximilian_amd", "banks.py")).read())
    assert re.search(r"\bclass maxiLooperBank\b", open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read())


def _args(b, n=4, mode=lh.PLAYLOOP):
    x, en, out = np.zeros((n, b.R)), np.ones((n, b.R)), np.zeros((n, b.R))
    keep = (x, en, out)
    a = dict(R=b.R, N=n, pool=b.pool_ptr, stride=b.stride, cap=b.cap, len=b.len.ctypes.data, inp=x.ctypes.data, enable=en.ctypes.data, eps=1,
             mix=b.mix.ctypes.data, start=b.start.ctypes.data, end=b.end.ctypes.data, recpos=b.recpos.ctypes.data, lagval=b.lag.ctypes.data,
             play_mode=mode, pstart=b.pstart.ctypes.data, pend=b.pend.ctypes.data, position=b.position.ctypes.data, out=out.ctypes.data,
             dropped=b.dropped.ctypes.data)
    return a, keep


@pytest.mark.parametrize("entry", ["mxg_looprec_host", "mxg_looprec_render"])
def test_bad_arguments_are_refused_by_name(entry):
    """Both forms run the same checks, the device form before it touches a device (this machine has none)."""
    import maximilian_amd as m
    lib = m.lib()
    fn = getattr(lib, entry)
    b = lh.Bank([50, 20, 7], 50)

    def call(**kw):
        a, keep = _args(b)
        a.update(kw)
        v = list(a.values()) + ([None] if entry.endswith("render") else [])
        st = fn(*v)
        return st, lib.mxg_last_error().decode()

    for name, word in (("pool", "pool"), ("len", "len"), ("inp", "in "), ("enable", "enable"), ("mix", "mix"), ("start", "start"), ("end", "end"),
                       ("recpos", "recpos"), ("lagval", "lagval"), ("position", "position"), ("out", "out"), ("pstart", "pstart"), ("pend", "pend")):
        st, msg = call(**{name: None})
        assert st < 0 and word in msg and entry in msg, (name, st, msg)
    st, msg = call(N=0)
    assert st < 0 and "N is 0" in msg
    st, msg = call(N=(1 << 24) + 1)
    assert st < 0 and "2^24" in msg
    for mode in (1, 3, -2, 14):
        st, msg = call(play_mode=mode)
        assert st < 0 and "play_mode" in msg, mode
    st, msg = call(play_mode=lh.PLAY_NONE)
    assert st < 0 and "out is given without a play mode" in msg
    st, msg = call(cap=b.stride)
    assert st < 0 and "cap" in msg
    if entry.endswith("host"):
        st, msg = call(play_mode=lh.PLAY_NONE, out=None)
        assert st == 0, msg
        for bad, word in ((np.array([50, 0, 7], np.uint64), "len[1] is 0"), (np.array([50, 20, 51], np.uint64), "len[2] = 51 is larger than cap")):
            st, msg = call(len=bad.ctypes.data)
            assert st < 0 and word in msg, msg
            st = lib.mxg_sample_pool_normalise_host(b.R, b.pool_ptr, b.stride, b.cap, bad.ctypes.data, b.mix.ctypes.data)
            assert st < 0 and word in lib.mxg_last_error().decode()
            st = lib.mxg_sample_pool_lengths(b.R, b.cap, bad.ctypes.data, 8)   # refused before the copy
            assert st < 0 and word in lib.mxg_last_error().decode()


def test_pool_and_normalise_arguments():
    import maximilian_amd as m
    lib = m.lib()
    st = ctypes.c_size_t(0)
    assert not lib.mxg_sample_pool_alloc(0, 10, ctypes.byref(st)) and "R is 0" in lib.mxg_last_error().decode()
    assert not lib.mxg_sample_pool_alloc(4, 0, ctypes.byref(st)) and "cap is 0" in lib.mxg_last_error().decode()
    assert not lib.mxg_sample_pool_alloc(4, 10, None) and "stride is null" in lib.mxg_last_error().decode()
    assert lib.mxg_sample_pool_free(None) == 0
    b = lh.Bank([5, 3])
    lv = np.ones(2)
    for args, word in (((2, None, b.stride, b.cap, b.len.ctypes.data, lv.ctypes.data), "pool"),
                       ((2, b.pool_ptr, b.stride, b.cap, None, lv.ctypes.data), "len"),
                       ((2, b.pool_ptr, b.stride, b.cap, b.len.ctypes.data, None), "maxLevel")):
        assert lib.mxg_sample_pool_normalise_host(*args) < 0 and word in lib.mxg_last_error().decode()
        assert lib.mxg_sample_pool_normalise(*args, None) < 0 and word in lib.mxg_last_error().decode()


@pytest.mark.parametrize("case", ["start1", "end2", "nan", "recpos", "negative"])
def test_outside_the_domain(be, case):
    """The departure: the read gives 0, nothing is stored, every enabled sample outside is counted, the guards stay zero."""
    b = lh.Bank([50, 50], 60)
    for r in range(2):
        b.set_sample(r, lh.ramp(50))
    b.trigger()
    n = 120
    x = np.full((n, 2), 0.5)
    en = np.ones((n, 2))
    en[1::3, 0] = 0.0
    if case == "start1":
        b.start[0] = 1.0            # the head sits on element len
        expect = int(en[:, 0].sum())
    elif case == "end2":
        b.end[0] = 2.0              # the head walks on to 2 * len: 50 samples inside, then outside
        expect = int(en[50:100, 0].sum())
    elif case == "nan":
        b.start[0] = lh.NAN         # no compare is ever true: the head only counts up
        expect = int(en[50:, 0].sum())
    elif case == "recpos":
        b.recpos[0] = 1e9           # an uploaded head far outside: it wraps after one sample
        expect = int(en[0, 0])
    else:
        b.start[0], b.end[0] = -0.5, 0.0    # sample 0 records on element 0, then the head wraps to -25 and never gets back to 0
        expect = int(en[1:, 0].sum())
    good = b.copy()
    good.start[0], good.end[0], good.recpos[0] = 0.0, 1.0, 0.0
    o = be.render(b, x, en, lh.PLAYLOOP)
    og = be.render(good, x, en, lh.PLAYLOOP)
    if expect is not None:
        assert b.dropped[0] == expect, (b.dropped, expect)
    assert b.dropped[0] > 0 and b.dropped[1] == 0
    assert not b.outside().any(), "a guard or a tail was written"
    assert_bits_equal(b.slot(1), good.slot(1), "the neighbour slot")
    assert_bits_equal(o[:, 1], og[:, 1], "the neighbour's output")
    if case == "start1":
        assert_bits_equal(b.slot(0), lh.ramp(50), "nothing is stored")
        assert_bits_equal(o[:, 0], lh.ramp(50)[(np.arange(n) + 1) % 50], "the play head reads the old content")
        assert_bits_equal(b.recpos[:1], [50.0])


def test_standalone_program_under_sanitizers(tmp_path):
    """tests/host_looper.cpp with its own main under AddressSanitizer + UndefinedBehaviorSanitizer, run once as its own process."""
    exe = str(tmp_path / "host_looper_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-DLOOPER_HOST_MAIN", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_looper.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_looper: ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
