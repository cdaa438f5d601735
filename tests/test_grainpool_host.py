"""CPU (-m "not gpu"): K27's arithmetic (maximilian_amd/csrc/mxg_grainpool.h) in its host build (tests/host_grainpool.cpp, g++ under
the oracle's FPFLAGS) and through the library's mxg_granular_pool_host against the reference's own bits (tests/golden/grainpool.npz,
tools/gen/gen_golden_grainpool.py): the output, position, looper, randomOffset and the live grains in creation order at every
stored cut and with further cuts.  Also: with one slot and the default loop the twin equals the oracle's granular port for modes
0-3; mxg_stretch_loop_host refuses what it must, by name; every bad argument is refused by name before a device is touched; the
entry points are declared, exported and bound; and the stand-alone program replays every call of the table under the sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import grainpool_host as gh
from conftest import ROOT, assert_bits_equal

EXTRA = (7, 64, 777, 1500)
ENTRY = ["mxg_granular_pool_render", "mxg_granular_pool_host", "mxg_stretch_loop_host"]


@pytest.fixture(scope="module")
def g(golden):
    return golden("grainpool.npz")


@pytest.fixture(scope="module")
def host(tmp_path_factory, g):
    return gh.HostBackend(gh.build(tmp_path_factory.mktemp("grainpool_host")), {k: g["window/" + k] for k in gh.WINDOWS})


@pytest.fixture(scope="module")
def twin():
    import maximilian_amd as m
    return gh.TwinBackend(m)


@pytest.fixture(params=["host", "twin"])
def be(request, host, twin):
    return host if request.param == "host" else twin


def test_inputs_are_the_stored_ones(g):
    assert_bits_equal(np.concatenate(gh.pool_content()), g["pool"], "the pool's content")
    assert list(g["lens"]) == gh.LENS and list(g["cuts"]) == gh.CUTS
    assert g["out"].shape == (gh.T, gh.NS)


def test_golden_table(be, g):
    gh.check_table(be, g)


def test_golden_table_with_further_cuts(be, g):
    gh.check_table(be, g, EXTRA)


def test_golden_table_one_sample_per_call(host, g):
    """Modes 2 and 4 are rendered one sample per launch by the drop-in classes: every mode, cut after every sample of the first 150."""
    gh.check_table(host, g, range(150))


def test_golden_table_as_the_tile_form_cuts_it(host, g):
    """K27's tile form on the host: the scheduler pass, then every sample computed on its own from the birth lists."""
    gh.check_table(gh.TilesBackend(host.L, host.windows), g)
    gh.check_table(gh.TilesBackend(host.L, host.windows), g, EXTRA)


def test_advance_is_the_plain_recurrence(host):
    """gp_advance -- where the tile form gets a grain's position at a tile's start: advance_until for a positive step, its mirror
    gp_retreat_until for a negative one -- against `pos += inc` with the wrap, step by step: steps of either sign from far under an
    ulp to the whole slot, short mantissas (exact sums, ties) and long ones, positions on 0, on len and on powers of two."""
    rng = np.random.default_rng(2702)
    for rep in range(6000):
        dlen = float(rng.choice([130, 300, 777, 2048, 4096, 44100, 60000]))
        kind = rep % 6
        if kind == 0:
            inc = float(rng.choice([-1.0, -0.5, -0.25, -1.5, -2.0, -0.75, 1.0, 0.5, -3.0, -0.125]))
        elif kind == 1:
            inc = -float(rng.uniform(0.01, 3.0))
        elif kind == 2:
            inc = -float(rng.uniform(0.0, 1.0)) * dlen
        elif kind == 3:
            inc = -float(2.0 ** rng.integers(-60, 2)) * float(rng.choice([1.0, 1.5, 1.0 + 2.0 ** -52]))
        elif kind == 4:
            inc = float(rng.uniform(-3.0, 3.0))
        else:
            inc = float(rng.choice([0.0, -0.0, -dlen, dlen, -5e-324, -1e-310]))
        pos = float(rng.choice([0.0, dlen, 1.0, 2.0, 64.0, 128.0, dlen / 2, float(rng.uniform(0, dlen)), float(np.floor(rng.uniform(0, dlen)))]))
        steps = int(rng.choice([0, 1, 2, 63, 64, 440, 2204, int(rng.integers(0, 5000))]))
        got, want = host.L.gp_h_advance(pos, inc, dlen, steps), host.L.gp_h_advance_plain(pos, inc, dlen, steps)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (rep, pos, inc, dlen, steps, got, want)


def test_window_tables_are_the_references(twin, g):
    for name in gh.WINDOWS:
        w = np.zeros(gh.SAMPLE_DUR)
        assert twin.lib.mxg_grain_plan_window(twin.plan(name), w.ctypes.data) == gh.SAMPLE_DUR
        assert_bits_equal(w, g["window/" + name], name)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_one_slot_default_loop_equals_the_oracle(twin, port, mode):
    """The equivalence anchor: a pool of one slot, d_loop = NULL, ps_flags = 0 is mxg_granular_render's contract, which the oracle's
    granular port states (oracle/pyoracle.py granular)."""
    rng = np.random.default_rng(2700 + mode)
    S, T, n = 7, 1500, 3000
    smp = rng.uniform(-1, 1, n)
    a = rng.uniform(0, 1, (T, S)) if mode == 2 else rng.uniform(0.3, 1.8, S) * np.where(np.arange(S) % 3 == 2, -1.0, 1.0)
    b = rng.uniform(0.2, 2.0, S) if mode == 1 else None
    pm = None if mode == 2 else rng.uniform(0, 0.2, S)
    rnd = rng.integers(0, 10, (S, 64)).astype(np.int32) if mode < 2 else None
    exp, est, egst, rc = port.granular(mode, 0, smp, T, a, b, pm, rnd, grainLength=gh.GRAIN_LENGTH, overlaps=3)
    assert rc == 0
    mem = np.zeros(n + 16)
    mem[8:8 + n] = smp
    lens, slot = np.array([n], np.uint64), np.zeros(S, np.uint32)
    st, gst, out = np.zeros((4, S)), np.zeros((4, 8, S)), np.zeros((T, S))
    cuts = [0, 1, 500, 501, T]
    for n0, n1 in zip(cuts[:-1], cuts[1:]):
        aa = np.ascontiguousarray(a[n0:n1]) if mode == 2 else a
        o = np.zeros((n1 - n0, S))
        rc = twin.lib.mxg_granular_pool_host(twin.plan("hann"), mode, S, n1 - n0, mem.ctypes.data + 64, 0, n, 1, lens.ctypes.data, slot.ctypes.data,
                                             None, 3, aa.ctypes.data, gh._p(b), gh._p(pm), 0, gh._p(rnd), 0 if rnd is None else 64,
                                             st.ctypes.data, gst.ctypes.data, o.ctypes.data)
        assert rc == 0, twin.lib.mxg_last_error().decode()
        out[n0:n1] = o
    assert_bits_equal(out, exp, "output")
    assert_bits_equal(st, est, "scheduler state")
    assert_bits_equal(gst, egst, "live grains")


def test_stretch_loop_refusals(host, twin):
    ls, le = ctypes.c_uint64(7), ctypes.c_uint64(7)
    for args, word in (((4096, gh.np.nan, 0.5), "NaN"), ((4096, 0.25, float("nan")), "NaN"), ((4096, -0.25, 0.5), "negative"),
                       ((4096, 0.25, -0.0001), "negative"), ((4096, 0.5, 0.5), "loopStart >= loopEnd"), ((4096, 0.5, 0.25), "loopStart >= loopEnd"),
                       ((777, 0.5, 0.5005), "loopStart >= loopEnd"), ((4096, 0.5, 1.001), "loopEnd is larger than len"),
                       ((4096, 0.5, 1e300), "loopEnd is larger than len"), ((4096, 0.5, float("inf")), "loopEnd is larger than len")):
        why = host.L.gp_h_loop(*args, ctypes.byref(ls), ctypes.byref(le))
        assert why is not None and word in why.decode(), (args, why)
        assert twin.lib.mxg_stretch_loop_host(*args, ctypes.byref(ls), ctypes.byref(le)) < 0
        msg = twin.lib.mxg_last_error().decode()
        assert word in msg and "mxg_stretch_loop_host" in msg, msg
        assert (ls.value, le.value) == (7, 7), "a refused call writes nothing"
    for n, s, e in ((4096, 0.25, 0.5), (777, 0.25, 1.0), (4096, 1000 / 4096.0, 1001 / 4096.0), (130, 0.0, 0.01)):
        assert host.L.gp_h_loop(n, s, e, ctypes.byref(ls), ctypes.byref(le)) is None
        assert (ls.value, le.value) == gh.loop_samples(n, s, e)
        assert twin.lib.mxg_stretch_loop_host(n, s, e, ctypes.byref(ls), ctypes.byref(le)) == 0
        assert (ls.value, le.value) == gh.loop_samples(n, s, e)
    assert twin.lib.mxg_stretch_loop_host(0, 0.0, 1.0, ctypes.byref(ls), ctypes.byref(le)) < 0
    assert twin.lib.mxg_stretch_loop_host(10, 0.0, 1.0, None, ctypes.byref(le)) < 0


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in ENTRY:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    for name, v in (("MXG_GPOOL_PS_A", 1), ("MXG_GPOOL_PS_B", 2), ("MXG_GPOOL_PS_POSMOD", 4)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr)
    assert hasattr(m, "maxiGrainPoolBank")
    assert re.search(r"\bclass maxiGrainPoolBank\b", open(os.path.join(ROOT, "maximilian_amd", "grains.py")).read())
    assert re.search(r"\bclass maxiGrainPoolBank\b", open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read())
    assert "facade_grainpool_smoke" in open(os.path.join(ROOT, "host", "Makefile")).read()


def _args(S=3, T=4, mode=1):
    mem, lens = gh.pool_array(), np.array(gh.LENS, np.uint64)
    keep = dict(mem=mem, lens=lens, slot=np.array([0, 4, 2], np.uint32)[:S], loop=np.array([[0, 0, 0], [130, 4096, 777]], np.uint64), a=np.ones(S),
                b=np.ones(S), st=np.zeros((4, S)), gst=np.zeros((4, 8, S)), out=np.zeros((T, S)))
    a = dict(plan=None, mode=mode, S=S, T=T, pool=mem.ctypes.data + 8 * gh.GUARD, stride=gh.STRIDE, cap=gh.CAP, R=gh.R, len=lens.ctypes.data,
             slot=keep["slot"].ctypes.data, loop=keep["loop"].ctypes.data, overlaps=2, a=keep["a"].ctypes.data, b=keep["b"].ctypes.data, posmod=None,
             ps=0, rnd=None, Rn=0, st=keep["st"].ctypes.data, gst=keep["gst"].ctypes.data, out=keep["out"].ctypes.data)
    return a, keep


@pytest.mark.parametrize("entry", ["mxg_granular_pool_host", "mxg_granular_pool_render"])
def test_bad_arguments_are_refused_by_name(twin, entry):
    """Both forms run the same checks, the device form before it touches a device (this machine has none)."""
    lib = twin.lib
    fn = getattr(lib, entry)

    def call(**kw):
        a, keep = _args()
        a["plan"] = twin.plan("hann")
        a.update(kw)
        v = list(a.values()) + ([None] if entry.endswith("render") else [])
        return fn(*v), lib.mxg_last_error().decode(), keep

    if entry.endswith("host"):
        st, msg, keep = call()
        assert st == 0, msg
    for name, word in (("plan", "plan"), ("pool", "pool"), ("len", "len"), ("a", "a is null"), ("b", "timestretch"), ("st", "st is null"),
                       ("gst", "gst is null"), ("out", "out is null")):
        if name == "plan" and entry.endswith("render"):
            continue
        st, msg, _ = call(**{name: None})
        assert st < 0 and word in msg and entry in msg, (name, st, msg)
    for mode in (-1, 5, 99):
        st, msg, _ = call(mode=mode)
        assert st < 0 and "mode must be" in msg
    st, msg, _ = call(mode=4, b=None)
    assert st < 0 and "position" in msg
    st, msg, _ = call(R=0)
    assert st < 0 and "R is 0" in msg
    st, msg, _ = call(cap=0)
    assert st < 0 and "cap" in msg
    st, msg, _ = call(stride=gh.CAP - 1)
    assert st < 0 and "stride" in msg
    st, msg, _ = call(overlaps=0)
    assert st < 0 and "overlaps" in msg
    st, msg, _ = call(ps=8)
    assert st < 0 and "ps_flags" in msg
    st, msg, _ = call(slot=None, S=3, R=2)
    assert st < 0 and "S is larger than R" in msg
    if entry.endswith("host"):   # (the device form reads d_slot back before it launches: tests/test_gpu_grainpool.py)
        bad = np.array([0, 5, 2], np.uint32)
        st, msg, keep = call(slot=bad.ctypes.data)
        assert st < 0 and "slot[1] = 5 is outside the pool of R = 5 slots" in msg, msg
        assert not keep["out"].any() and not keep["st"].any()


def test_fuzz_block_against_single_samples_and_splits(host, twin):
    """Random streams over the table's pool, every mode and every PS bit: one call, the same call one sample at a time, and random
    splits give the same bits, on the host build and on the library's twin."""
    rng = np.random.default_rng(2701)
    mem, lens = gh.pool_array(), np.array(gh.LENS, np.uint64)
    for rep in range(40):
        mode, S, T = int(rng.integers(0, 5)), int(rng.integers(1, 6)), int(rng.integers(1, 900))
        ov = int(rng.choice([1, 2, 3, 5]))
        ps, a, b, pm, slot, loop, rnd, st0 = gh.random_case(rng, mode, S, T)

        def run(be, cuts):
            st, gst, out = st0.copy(), np.zeros((4, 8, S)), []
            for n0, n1 in zip(cuts[:-1], cuts[1:]):
                sl = lambda x, per: None if x is None else (np.ascontiguousarray(x[n0:n1]) if per else x)
                o, rc = be.call(mode, ov, "hann", n1 - n0, mem, lens, slot, loop, sl(a, mode == 2 or ps & 1), sl(b, ps & 2), sl(pm, ps & 4), ps, rnd, st, gst)
                assert rc == 0, (rep, mode, rc)
                out.append(o)
            return np.concatenate(out), st, gst

        whole = run(twin if rep % 2 else host, [0, T])
        ones = run(host, list(range(T + 1)))
        cuts = sorted(set(rng.integers(0, T + 1, 4).tolist()) | {0, T})
        parts = run(host if rep % 2 else twin, cuts)
        tiles = run(gh.TilesBackend(host.L, host.windows), cuts if rep % 3 else [0, T])
        for other, what in ((ones, "single samples"), (parts, "splits"), (tiles, "the tile form")):
            for x, y, name in zip(whole, other, ("output", "state", "grains")):
                assert_bits_equal(y, x, "fuzz %d (mode %d): %s, %s" % (rep, mode, name, what))


def test_more_than_eight_live_grains_is_reported_and_the_others_are_untouched(twin):
    """overlaps 12 is a birth every 36.75 samples and twelve grains alive.  Stream 0 draws zeros and runs past eight; streams 1 and 2
    draw 40 (a birth every 76.75 samples, six alive) and must be what they are in a call without stream 0."""
    mem, lens = gh.pool_array(), np.array(gh.LENS, np.uint64)
    S, T = 3, 1200
    slot, a = np.array([3, 4, 2], np.uint32), np.array([1.0, 0.5, -1.0])
    rnd = np.zeros((S, 64), np.int32)
    rnd[1:] = 40
    st, gst = np.zeros((4, S)), np.zeros((4, 8, S))
    o, rc = twin.call(0, 12, "hann", T, mem, lens, slot, None, a, None, None, 0, rnd, st, gst)
    assert rc < 0 and "more than 8 grains" in twin.lib.mxg_last_error().decode()
    st2, gst2 = np.zeros((4, 2)), np.zeros((4, 8, 2))
    o2, rc = twin.call(0, 12, "hann", T, mem, lens, slot[1:], None, a[1:], None, None, 0, np.ascontiguousarray(rnd[1:]), st2, gst2)
    assert rc == 0 and o2.any()
    assert_bits_equal(o[:, 1:], o2, "the neighbours' output")
    assert_bits_equal(st[:, 1:], st2, "the neighbours' state")
    assert_bits_equal(gst[:, :, 1:], gst2, "the neighbours' grains")
    assert (gst[3, :, 0] == gh.SAMPLE_DUR).all(), "the crowded stream keeps running with eight grains"


def test_foreign_grain_and_exhausted_draws_are_reported(twin):
    mem, lens = gh.pool_array(), np.array(gh.LENS, np.uint64)
    slot, a = np.array([0, 4], np.uint32), np.array([1.0, 1.0])
    st, gst = np.zeros((4, 2)), np.zeros((4, 8, 2))
    gst[:, 0, 0] = (200.0, 1.0, 3.0, 441.0)      # a position that fits the 4096 slot, not the 130 one this stream reads
    o, rc = twin.call(0, 2, "hann", 50, mem, lens, slot, None, a, None, None, 0, None, st, gst)
    assert rc < 0 and "could not have made" in twin.lib.mxg_last_error().decode()
    gst[...] = 0
    gst[:, 0, 1] = (200.0, 1.0, 3.0, 441.0)      # the same grain where it fits
    st[...] = 0
    o, rc = twin.call(0, 2, "hann", 50, mem, lens, slot, None, a, None, None, 0, None, st, gst)
    assert rc == 0 and o[:, 1].any()
    st, gst = np.zeros((4, 2)), np.zeros((4, 8, 2))
    o, rc = twin.call(0, 2, "hann", 2000, mem, lens, slot, None, a, None, None, 0, np.zeros((2, 2), np.int32), st, gst)
    assert rc < 0 and "d_rnd exhausted" in twin.lib.mxg_last_error().decode()


def test_a_length_above_cap_is_read_as_cap_and_an_empty_slot_is_silent(host):
    mem = gh.pool_array()
    slot, a = np.array([2], np.uint32), np.array([1.0])
    outs = []
    for ln in (gh.CAP, gh.CAP + 1000, 1 << 40):
        lens = np.array(gh.LENS, np.uint64)
        lens[2] = ln
        st, gst = np.zeros((4, 1)), np.zeros((4, 8, 1))
        o, rc = host.call(0, 2, "hann", 600, mem, lens, slot, None, a, None, None, 0, None, st, gst)
        assert rc == 0
        outs.append((o, st, gst))
    for x in outs[1:]:
        for p, q in zip(x, outs[0]):
            assert_bits_equal(p, q, "a length above cap")
    lens = np.array(gh.LENS, np.uint64)
    lens[2] = 0
    st, gst = np.full((4, 1), 3.0), np.zeros((4, 8, 1))
    o, rc = host.call(0, 2, "hann", 10, mem, lens, slot, None, a, None, None, 0, None, st, gst)
    assert rc == 5 and not o.any() and (st == 3.0).all()


def test_standalone_program_under_sanitizers(tmp_path, host):
    """tests/host_grainpool.cpp with its own main under AddressSanitizer + UndefinedBehaviorSanitizer, run once as its own process
    over a file of every call the golden table makes.  The tails of the slots and the gaps between them are poisoned there: a read
    outside [0, len) of a stream's slot ends the program."""
    path = str(tmp_path / "calls.bin")
    mem, lens = gh.pool_array(), np.array(gh.LENS, np.uint64)

    class Recorder:
        name = "recorder"

        def __init__(self, f):
            self.f, self.calls = f, 0

        def call(self, mode, ov, win, n, mem, lens, slot, loop, a, b, pm, ps, rnd, st, gst):
            S = st.shape[1]
            w = np.ascontiguousarray(host.windows[win])
            cnt = lambda x: 0 if x is None else x.size
            hdr = np.array([mode, S, n, ov, ps, 0 if rnd is None else rnd.shape[1], w.size, cnt(a), cnt(b), cnt(pm), loop is not None, rnd is not None], np.int64)
            for x in (hdr, w, slot, loop, a, b, pm, rnd, st, gst):
                if x is not None:
                    self.f.write(np.ascontiguousarray(x).tobytes())
            self.calls += 1
            return host.call(mode, ov, win, n, mem, lens, slot, loop, a, b, pm, ps, rnd, st, gst)

    with open(path, "wb") as f:
        f.write(np.array([gh.R, gh.STRIDE, gh.CAP, gh.GUARD], np.int64).tobytes() + lens.tobytes() + mem.tobytes())
        rec = Recorder(f)
        gh.run_table(rec)
    exe = str(tmp_path / "host_grainpool_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-DGPOOL_HOST_MAIN", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_grainpool.cpp")])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_grainpool: ok calls=%d failed=0 refused=6" % rec.calls in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
