"""GPU: K22 (atoms.hip) through the C-ABI against tests/golden/atoms.npz under the numerics contract (tests/atoms_host.py), and
against the library's own host build bit for bit: the cases of test_atoms_host.py -- raw atoms over changing block lengths with
stalls, the sum's order, a segment list of one LDS piece plus one, the player on sorted, unsorted and empty books, 65 streams with
65 books --; five carried blocks of different N against one long block; SAMPLE onsets against a numpy overlap-add; accumulate on and
off; S in {1, 3, 65} x N in {1, 7, 64, 513} with Gabor atoms of every contract length; a live list at capacity and one past it, the
player's overflow through the asynchronous error word; the Python bank."""
import numpy as np
import pytest

import atoms_host as ah

pytestmark = pytest.mark.gpu
MXG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def L(mx):
    return mx.lib()


@pytest.fixture(scope="module")
def g(golden):
    return golden("atoms.npz")


@pytest.fixture(scope="module")
def cases():
    return ah.cases()


@pytest.fixture(scope="module")
def host_runs(L, cases):
    """Every case once through the host twins: the bits the device has to give."""
    res = {}
    for name, case in cases.items():
        r = ah.Runner(L, case, host=True)
        res[name] = r.run()
        r.close()
    return res


@pytest.mark.parametrize("name", ["accel", "order", "piece", "player", "player65"])
def test_case_against_the_record_and_the_host_build(L, mx, g, cases, host_runs, name):
    r = ah.Runner(L, cases[name], host=False, dev=mx)
    out, rows, queues = r.run()
    r.close()
    print("%s: worst error %.3f of the derived bound" % (name, ah.check_case(g, cases[name], out, rows, queues)))
    hout, hrows, hqueues = host_runs[name]
    assert np.array_equal(ah.bits(out), ah.bits(hout)), name + ": the device is not bit-identical to the host build"
    assert np.array_equal(rows, hrows) and queues == hqueues


def test_accumulate_off_starts_from_zero(L, mx, cases):
    case = cases["accel"]
    r = ah.Runner(L, case, host=False, dev=mx)
    out, _, _ = r.run(accumulate=False)
    r.close()
    exp = ah.overlap_add(case, ah.run_model(case), lambda s, atom: case.streams[s].raws[atom[1]], accumulate=False)
    assert np.array_equal(ah.bits(out), ah.bits(exp))


def test_sample_onset_against_numpy(L, mx, cases):
    case = cases["accel"]
    r = ah.Runner(L, case, host=False, dev=mx, onset=ah.ONSET_SAMPLE)
    out, rows, _ = r.run()
    r.close()
    model = ah.run_model(case, ah.ONSET_SAMPLE)
    exp = ah.overlap_add(case, model, lambda s, atom: case.streams[s].raws[atom[1]])
    assert np.array_equal(ah.bits(out), ah.bits(exp))
    for s in range(case.S):
        assert np.array_equal(rows[s], np.array(model[s][1], np.int64))


def _gabor_streams(S):
    """S streams, every one with other Gabor atoms of the contract's lengths queued at time 0."""
    return [[(20.0 + 613.0 * ((s * 6 + k) % 31), ah.LENGTHS[(s + k + 5) % 6], 0.3 + 0.1 * s + k, 0.5 + 0.01 * s) for k in range(1 + s % 6)] for s in range(S)]


def _run_gabor(mx, host, S, blocks, onset="block"):
    L = mx.lib()
    spec = _gabor_streams(S)
    make = L.mxg_atoms_bank_create_host if host else L.mxg_atoms_bank_create
    bank = make(S, 8, None, None, None, None, 0)
    assert bank, L.mxg_last_error()
    rows = [(s, f, n, p, a) for s, atoms in enumerate(spec) for (f, n, p, a) in atoms]
    stream, kind = np.array([r[0] for r in rows], np.int32), np.zeros(len(rows), np.int32)
    length, par = np.array([r[2] for r in rows], np.uint32), np.array([(r[1], 44100.0, r[3], r[4]) for r in rows], np.float32)
    add = L.mxg_atoms_add_host if host else L.mxg_atoms_add
    assert add(bank, len(rows), stream.ctypes.data, kind.ctypes.data, length.ctypes.data, None, par.ctypes.data, None) == 0, L.mxg_last_error()
    outs = []
    for n in blocks:
        if host:
            buf = np.zeros((S, n), np.float32)
            assert L.mxg_atoms_fill_host(bank, n, buf.ctypes.data, ah.ONSET_BLOCK, 0) == 0
        else:
            d = mx.DeviceBuffer((S, n), np.float32, zero=False)
            assert L.mxg_atoms_fill(bank, n, d.ptr, ah.ONSET_BLOCK, 0, None) == 0, L.mxg_last_error()
            buf = d.numpy()
            d.free()
        outs.append(buf)
    L.mxg_atoms_bank_destroy(bank)
    return np.concatenate(outs, axis=1)


@pytest.fixture(scope="module")
def gabor_long(mx):
    """One block of 650 samples per S on the host build: what every cut of it has to give."""
    return {S: _run_gabor(mx, True, S, [650]) for S in (1, 3, 65)}


@pytest.mark.parametrize("S", [1, 3, 65])
@pytest.mark.parametrize("N", [1, 7, 64, 513])
def test_shapes_bit_identical_to_the_host_build(mx, gabor_long, S, N):
    blocks = [N] * min(4, 650 // N)
    got = _run_gabor(mx, False, S, blocks)
    exp = gabor_long[S][:, :sum(blocks)]
    assert (exp != 0).any()
    assert np.array_equal(ah.bits(got), ah.bits(exp)), "S %d N %d" % (S, N)


def test_gabor_atoms_against_the_record(mx, g):
    """createGabor on the device (one atom per stream, one block) against the recorded reference: bound and cap."""
    L = mx.lib()
    cs = [c for c in ah.GABOR_CASES if c[2] <= 2048]
    S, N = len(cs), 2048
    bank = L.mxg_atoms_bank_create(S, 2, None, None, None, None, 0)
    stream, kind = np.arange(S, dtype=np.int32), np.zeros(S, np.int32)
    length, par = np.array([c[2] for c in cs], np.uint32), np.array([(c[0], c[1], c[3], c[4]) for c in cs], np.float32)
    assert L.mxg_atoms_add(bank, S, stream.ctypes.data, kind.ctypes.data, length.ctypes.data, None, par.ctypes.data, None) == 0, L.mxg_last_error()
    d = mx.DeviceBuffer((S, N), np.float32, zero=False)
    assert L.mxg_atoms_fill(bank, N, d.ptr, ah.ONSET_BLOCK, 0, None) == 0, L.mxg_last_error()
    out = d.numpy()
    L.mxg_atoms_bank_destroy(bank)
    differ = total = 0
    for i, (freq, sr, length, phase, amp) in enumerate(cs):
        ref = g[ah.gabor_key(i)]
        a = out[i, :length]
        assert (out[i, length:] == 0).all()
        err, bound = np.abs(a.astype(np.float64) - ref), ah.gabor_bound(length, amp)
        assert (err <= bound).all(), (i, float((err - bound).max()))
        host = np.zeros(length, np.float32)
        assert L.mxg_atoms_gabor_host(freq, sr, length, phase, amp, host.ctypes.data) == 0
        assert np.array_equal(ah.bits(a), ah.bits(host)), "atom %d: the device is not bit-identical to the host build" % i
        nz = ref != 0
        differ += int((ah.bits(a)[nz] != ah.bits(ref)[nz]).sum())
        total += int(nz.sum())
    print("createGabor on the device: %d of %d non-zero samples differ from the record (%.2f %%)" % (differ, total, 100.0 * differ / total))
    assert differ <= ah.CAP * total


def test_five_carried_blocks_equal_one_long_block(mx, gabor_long):
    """Atoms queued at time 0 with offset 0: the reference's quantisation puts them on sample 0 however the stream is cut."""
    got = _run_gabor(mx, False, 3, [7, 64, 1, 513, 65])
    assert np.array_equal(ah.bits(got), ah.bits(gabor_long[3]))


def test_live_list_at_capacity_and_one_past(L, mx, cases):
    case = cases["piece"]
    r = ah.Runner(L, case, host=False, dev=mx, Q=ah.PIECE)      # 65 adds into a list of 64
    assert r.add(0) == MXG_ERR_INVALID and b"more than Q" in L.mxg_last_error()
    rows, queues = r.state()
    assert rows.tolist() == [[0, 0, 0]] and queues == [[]], "nothing was added"
    r.close()


def test_player_overflow_is_reported_and_leaves_the_stream_untouched(L, mx):
    case = ah.overflow_case()
    r = ah.Runner(L, case, host=False, dev=mx)
    buf = np.ascontiguousarray(case.init[:, :64])
    d = mx.DeviceBuffer.from_numpy(buf)
    assert L.mxg_atoms_play(r.bank, 64, d.ptr, ah.ONSET_BLOCK, 1, None) == 0, "the launch itself succeeds: the overflow is found on the device"
    assert L.mxg_sync() == MXG_ERR_INVALID and b"more than Q" in L.mxg_last_error(), "the next call reports it, once"
    assert L.mxg_last_async_error() == 0
    buf = d.numpy()
    rows, queues = r.state()
    assert np.array_equal(ah.bits(buf[0]), ah.bits(case.init[0, :64])) and rows[0].tolist() == [0, 0, 0] and queues[0] == []
    assert not np.array_equal(ah.bits(buf[1]), ah.bits(case.init[1, :64])) and rows[1].tolist() == [64, 2, 0]
    r.close()
    big = ah.Runner(L, case, host=False, dev=mx, Q=5)           # at capacity: five atoms in a list of five
    assert big.step("play", 64, buf) == 0 and L.mxg_sync() == 0
    assert big.state()[0][0].tolist() == [64, 5, 0]
    big.close()


def test_python_bank(mx, cases, host_runs):
    case = cases["player"]
    bank = mx.maxiAtomBank(case.S, capacity=16, books=[st.book.T for st in case.streams], num_samples=[st.num_samples for st in case.streams])
    outs = [bank.play(n).numpy() for _, n in case.blocks]
    idx, ai, q = bank.state()
    hout, hrows, hq = host_runs["player"]
    assert np.array_equal(ah.bits(np.concatenate(outs, axis=1)), ah.bits(hout))
    assert np.array_equal(idx, hrows[:, -1, 0]) and np.array_equal(ai, hrows[:, -1, 1]) and q == [x[-1] for x in hq]
    raw = np.arange(1, 11, dtype=np.float32)
    rb = mx.maxiAtomBank(2, capacity=4)
    off = rb.appendRaw(raw)
    rb.addAtom([0, 1, 1], off, [10, 4, 3], offset=[0, 2, 0])
    out = rb.fillNextBuffer(8, onset="sample").numpy()
    exp = np.zeros((2, 8), np.float32)
    exp[0, :8] = raw[:8]
    exp[1, 2:6] = raw[:4]
    exp[1, :3] += raw[:3]
    assert np.array_equal(out, exp)
    rb.addGabor(0, 440.0, 64, amp=0.5)
    assert np.abs(rb.fillNextBuffer(64).numpy()[0]).max() > 0.1
    bank.free(), rb.free()
