"""CPU (-m "not gpu"): mxg_seq.h -- the arithmetic seq.hip's kernels run -- compiled for the host with g++ under the oracle's
FPFLAGS (tests/host_seq.cpp) reproduces tests/golden/seq.npz BIT FOR BIT: triggers, values, gates, and every state array at
every stored cut, for every case, with the blocks cut as stored and at further uneven positions.  Everything is compares,
+ - / floor and indexing, so no tolerance applies anywhere.  Also: mxg_seq_ratio_host against a step-by-step restatement, and
the sequencing classes of the drop-in header (tests/patches/seq_host_patch.cpp, host value types: no device) against the stream
the same patch gives with the reference."""
import os
import subprocess

import numpy as np
import pytest

import seq_host
from conftest import ROOT, assert_bits_equal

EXTRA = (1, 7, 64, 777, 1501, 3999)


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    return seq_host.HostBackend(seq_host.build(tmp_path_factory.mktemp("seq")))


@pytest.fixture(scope="module")
def g(golden):
    return golden("seq.npz")


assert_same, check_fused = seq_host.assert_same, seq_host.check_fused


@pytest.mark.parametrize("extra", [(), EXTRA])
@pytest.mark.parametrize("name", seq_host.FUSED_CASES)
def test_host_reproduces_golden(be, g, name, extra):
    c = seq_host.load_case(g, name)
    assert (c["trig"].sum(axis=0) >= 3).all() and c["gate"].any() and len(np.unique(c["val_idx"])) >= 6  # not rows of zeros
    trig, val, gate, states = seq_host.play_fused(be, c, extra)
    check_fused(c, name, trig, val, gate, states)


@pytest.mark.parametrize("extra", [(), EXTRA])
@pytest.mark.parametrize("kind", sorted(seq_host.KIND_NAMES))
def test_host_signal_reproduces_golden(be, g, kind, extra):
    out, states = seq_host.play_signal(be, g, kind, extra)
    seq_host.check_signal(g, kind, out, states)


def test_golden_holds_the_quirks(g):
    """What the file must contain for the tests above to mean something."""
    c = seq_host.load_case(g, "values")
    t = c["trig"]
    assert (t[1:] & t[:-1]).any()                       # two boundaries in consecutive samples
    assert c["vlen0"].tolist() != c["vlen%d" % (len(c["cuts"]) - 2)].tolist()   # a value list changes its length between two blocks
    s = seq_host.load_case(g, "step")
    steps = s["step0"]
    assert {1.0, 2.0, -1.0, 0.5} <= set(steps.tolist()) and (steps > s["vlen0"][s["vpat"]]).any() and (steps == -s["vlen0"][s["vpat"]]).any()
    assert set(c["hold"].tolist()) == {0.0, 1.0, 2.5, 300.0}
    assert sorted(c["vlen0"].tolist()) == [1, 3, 6, 10]
    assert (g["sig/index/out_idx"] == 255).any()        # maxiIndex's initial 0.0 before the first trigger
    assert "sha256" in str(g["provenance"])


def test_held_index_where_the_reference_leaves_the_table(be):
    """The one departure: maxiStep with step < -len keeps a negative index; the value read is the table's first entry."""
    V, N = 1, 12
    trig = np.zeros((N, V))
    trig[::2] = 1.0
    vals, vlen = seq_host.table([[10.0, 20.0, 30.0]], 3)
    dst, ist = seq_host.fresh_sig(seq_host.STEP, V)
    out = be.signal(seq_host.STEP, V, N, trig, None, vals, vlen, None, np.array([-7.0]), dst, ist)
    assert out[0, 0] == 10.0 and dst[1, 0] < 0 and set(out[:, 0].tolist()) <= {10.0, 20.0, 30.0}


def test_ratio_host_matches_restatement(be):
    import maximilian_amd as mx
    rng = np.random.default_rng(15)
    for trial in range(300):
        Pn, L = int(rng.integers(1, 6)), int(rng.integers(1, 65))
        plen = rng.integers(1, L + 1, Pn).astype(np.int32)
        times = rng.choice([0.0, 1.0, 3.0, 0.001, 991.0], (Pn, L)) * rng.uniform(0.5, 2.0, (Pn, L))
        if trial % 7 == 0:
            times[0] = 0.0                               # sum 0
        if trial % 11 == 0:
            times[-1, :plen[-1]] = rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0], plen[-1])  # negative and zero sums
        exp = np.full((Pn, L), np.nan)
        for p in range(Pn):                              # the restatement, step by step
            s = np.float64(0.0)
            for i in range(plen[p]):
                s = s + times[p, i]
            acc = np.float64(0.0)
            for i in range(plen[p]):
                acc = acc + times[p, i]
                with np.errstate(divide="ignore", invalid="ignore"):
                    b = acc / s
                exp[p, i] = 0.0 if b == 1.0 else b
        got = seq_host.ratio_tables(times, plen)
        assert_same(got, exp, "library")
        host = np.zeros_like(times)
        be.L.seq_host_ratio(Pn, L, plen.ctypes.data, np.ascontiguousarray(times).ctypes.data, host.ctypes.data)
        assert_same(host, exp, "host build")
    # a zero or NaN sum never fires
    norm = seq_host.ratio_tables(np.zeros((1, 3)), np.array([3], np.int32))
    dst, ist = seq_host.fresh_seq(1)
    t, _, _ = be.render(1000, 1, 500, np.array([20.0]), np.zeros(1), None, norm, np.array([3], np.int32), None, 0, None, None, None, None,
                        None, dst, ist, (True, False, False))
    assert not t.any()


def _build_patch(tmp_path, patch, incdir, extra):
    exe = str(tmp_path / "patch")
    subprocess.check_call(["g++", "-std=c++17"] + seq_host.fpflags() + ["-w", "-I" + incdir, "-o", exe,
                           os.path.join(ROOT, "oracle", "example_host.cpp"), os.path.join(ROOT, "tests", "patches", patch)] + extra)
    return exe


def test_host_patch_against_dropin_header(g, tmp_path):
    """The drop-in maxiRatioSeq / maxiStep / maxiCounter / maxiIndex / maxiZXToPulse / maxiTrigger are host value types: the patch
    runs without a device and gives the reference's stream bit for bit."""
    import maximilian_amd as mx
    exp = g["host_patch"]
    exe = _build_patch(tmp_path, "seq_host_patch.cpp", os.path.join(ROOT, "include"),
                       ["-L" + os.path.dirname(mx.LIB_PATH), "-lmaxigpu", "-Wl,-rpath," + os.path.dirname(mx.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    raw = str(tmp_path / "o.f64")
    r = subprocess.run([exe, str(exp.shape[0]), raw], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(raw, np.float64).reshape(exp.shape)
    assert (exp[:, 0] != 0).any() and (exp[:, 1] != 0).any()
    assert_bits_equal(got, exp, "seq_host_patch through the drop-in header")


def test_patches_compile_against_dropin_header():
    for patch in ("seq_patch.cpp", "seq_host_patch.cpp"):
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "patches", patch)])
