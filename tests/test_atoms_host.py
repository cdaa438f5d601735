"""CPU (-m "not gpu"): the host forms of K22 -- mxg_atoms_gabor_host and the mxg_atoms_*_host twins, i.e. csrc/mxg_atoms.h compiled
for the host -- against tests/golden/atoms.npz under the numerics contract (tests/atoms_host.py): createGabor over the contract's
lengths by bound and cap; the accelerator with raw atoms over CHANGING buffer lengths that make entries stall, bits and state; the
sum's order; a live list at capacity and one past it; the player over two loops of a block-aligned book, sorted and unsorted, with the
buffer that schedules nothing, and 65 streams with 65 books; the player's overflow."""
import numpy as np
import pytest

import atoms_host as ah

MXG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def L():
    import maximilian_amd as m
    return m.lib()


@pytest.fixture(scope="module")
def g(golden):
    return golden("atoms.npz")


@pytest.fixture(scope="module")
def cases():
    return ah.cases()


def test_create_gabor_by_bound_and_cap(L, g):
    differ = total = 0
    worst = 0.0
    for i, (freq, sr, length, phase, amp) in enumerate(ah.GABOR_CASES):
        a = np.zeros(length, np.float32)
        assert L.mxg_atoms_gabor_host(freq, sr, length, phase, amp, a.ctypes.data) == 0, L.mxg_last_error()
        ref = g[ah.gabor_key(i)]
        err, bound = np.abs(a.astype(np.float64) - ref), ah.gabor_bound(length, amp)
        print("createGabor %d: length %5d  max error %.3g  (bound %.3g)" % (i, length, err.max(), bound.max()))
        assert (err <= bound).all(), (i, float((err - bound).max()))
        nz = ref != 0
        differ += int((ah.bits(a)[nz] != ah.bits(ref)[nz]).sum())
        total += int(nz.sum())
        worst = max(worst, float((err / bound).max()))
    print("createGabor: %d of %d non-zero samples differ from the record (%.2f %%); worst error %.3f of the bound" % (differ, total, 100.0 * differ / total, worst))
    assert differ <= ah.CAP * total


@pytest.mark.parametrize("name", ["accel", "order", "piece", "player", "player65"])
def test_case_against_the_record(L, g, cases, name):
    r = ah.Runner(L, cases[name], host=True)
    out, rows, queues = r.run()
    r.close()
    print("%s: worst error %.3f of the derived bound" % (name, ah.check_case(g, cases[name], out, rows, queues)))


def test_accumulate_off_starts_from_zero(L, g, cases):
    case = cases["accel"]
    r = ah.Runner(L, case, host=True)
    out, _, _ = r.run(accumulate=False)
    r.close()
    model = ah.run_model(case)
    exp = ah.overlap_add(case, model, lambda s, atom: case.streams[s].raws[atom[1]], accumulate=False)
    assert np.array_equal(ah.bits(out), ah.bits(exp))


def test_sample_onset_against_numpy(L, cases):
    case = cases["accel"]
    r = ah.Runner(L, case, host=True, onset=ah.ONSET_SAMPLE)
    out, rows, _ = r.run()
    r.close()
    model = ah.run_model(case, ah.ONSET_SAMPLE)
    exp = ah.overlap_add(case, model, lambda s, atom: case.streams[s].raws[atom[1]])
    assert np.array_equal(ah.bits(out), ah.bits(exp))
    for s in range(case.S):
        assert np.array_equal(rows[s], np.array(model[s][1], np.int64))
    assert not np.array_equal(ah.bits(out), ah.bits(ah.overlap_add(case, ah.run_model(case), lambda s, atom: case.streams[s].raws[atom[1]])))


def test_live_list_at_capacity_and_one_past(L, cases):
    case = cases["piece"]
    r = ah.Runner(L, case, host=True, Q=ah.PIECE)      # 65 adds into a list of 64
    assert r.add(0) == MXG_ERR_INVALID and b"more than Q" in L.mxg_last_error()
    rows, queues = r.state()
    assert rows.tolist() == [[0, 0, 0]] and queues == [[]], "nothing was added"
    r.close()


def test_player_overflow_leaves_the_stream_untouched(L):
    case = ah.overflow_case()
    r = ah.Runner(L, case, host=True)
    buf = np.ascontiguousarray(case.init[:, :64])
    assert r.step("play", 64, buf) == MXG_ERR_INVALID and b"more than Q" in L.mxg_last_error()
    rows, queues = r.state()
    assert np.array_equal(ah.bits(buf[0]), ah.bits(case.init[0, :64])) and rows[0].tolist() == [0, 0, 0] and queues[0] == []
    assert not np.array_equal(ah.bits(buf[1]), ah.bits(case.init[1, :64])) and rows[1].tolist() == [64, 2, 0]
    r.close()
    big = ah.Runner(L, case, host=True, Q=5)           # at capacity: five atoms in a list of five
    assert big.step("play", 64, buf) == 0
    assert big.state()[0][0].tolist() == [64, 5, 0]
    big.close()


def test_host_program_holds_the_sine_below_one_ulp(tmp_path):
    """tests/host_atoms.cpp as a program: atoms_sin against quad precision, and the seeded queue scripts."""
    import os
    import re
    import subprocess
    from conftest import ROOT
    exe = str(tmp_path / "host_atoms")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_atoms.cpp"), "-lquadmath", "-lm"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0 and "host_atoms: ok" in out
    assert float(re.search(r"max error ([0-9.]+) ULP", out).group(1)) < 1.0
