"""The atoms case (K22): one place for tools/gen/gen_golden_atoms.py, which records the UNMODIFIED reference's output for it in
tests/golden/atoms.npz, and for the tests that hold the host forms and the kernels to that record.

A case is S streams that share one sequence of blocks -- ("fill" | "play", N) -- and, per stream, a book (rows position, length, amp,
frequency, phase, and numSamples), a list of raw atoms (float32 arrays) and the addAtom calls in front of each block: (block, atom,
offset).  `init` is what the buffers hold before the fills (the reference adds on top of it).

Also here, independent of the library: Model, the queue's integer rules restated in Python (which atom adds which samples where, in
which order -- it gives the tests the numpy overlap-add of SAMPLE mode and the error envelope of the Gabor contract), and the
contract's bounds.

The numerics contract:
  RAW atoms                bit for bit, in either onset mode; sampleIdx, atomIdx and every queue entry bit for bit after every block.
  Gabor atom sample        a = fl(fl(env_f * s) * amp).  Our s and glibc's sinf are both floats next to the true sine: at most 1 float
                           ULP apart, ulp(s) <= 2^-23 |s| <= 2^-23.  Through the two roundings behind it (RN(x) - RN(x') is at most
                           |x - x'| plus one ULP of the result):
                               |a - a_ref| <= |env_f amp| 2^-23 + |amp| ulp(env_f s) + ulp(a) <= 3 * 2^-23 * |env_f amp|   (+ denormals)
  Output sample            the float sum, in queue order, of the n atoms live there: the terms differ by the bound above and each of
                           the n additions rounds once more, a partial sum being at most P = |init| + sum |env_f amp|:
                               |y - y_ref| <= sum_a 3 * 2^-23 |env_f amp|_a + n * 2^-23 * P
  The cap                  at most 3 % of the non-zero atom samples differ from the record at all."""
import ctypes

import numpy as np

GABOR, RAW = 0, 1
ONSET_BLOCK, ONSET_SAMPLE = 0, 1
PIECE = 64          # MXG_ATOMS_PIECE
TILE = 256          # K22b's tile of output samples
LENGTHS = (1, 2, 63, 64, 65, 257)
EPS = 2.0 ** -23
TINY = 2.0 ** -149
CAP = 0.03

# createGabor: (freq, sampleRate, length, startPhase, amp).  The contract's lengths, and two long atoms at the top of the band, where
# the sine's argument reaches 5e3 and 4e4 rad.
GABOR_CASES = [(440.0, 44100.0, 1, 0.0, 1.0), (1234.5, 44100.0, 2, 0.5, 0.75), (20.0, 44100.0, 63, 1.0, 0.025), (9000.0, 44100.0, 64, -2.0, 1.5),
               (19999.0, 48000.0, 65, 3.0, 0.3), (3000.0, 44100.0, 257, 0.25, 0.9), (17000.0, 44100.0, 2048, 0.1, 0.5),
               (20000.0, 44100.0, 16384, 2.5, 0.025)]


def gabor_key(i):
    return "gabor/%d" % i


def window_f(length):
    """(float)env[i]: the gaussian window of maxiGrains.h:75-92 (numpy's exp is libm's here; the tests take env from the library's
    host call wherever bits matter -- this is for the error envelope only)."""
    i = np.arange(length, dtype=np.float64)
    ph = ((i / float(length)) - 0.5) * 2.0
    return np.exp((ph * ph) / (-2.0 * 0.3 * 0.3)).astype(np.float32)


def gabor_numpy(freq, sr, length, phase, amp):
    """createGabor's float operations in numpy with the DOUBLE sine rounded to float where the reference calls sinf: the model the
    generator holds the reference's own sinf against (below 2 % of samples differ), not a test reference."""
    f32 = np.float32
    cycle = f32(sr) / f32(freq)
    max_phase = f32(np.float64(f32(length) / cycle) * 6.283185307179586476925286766559)
    inc = f32(1.0 / length)
    x = inc * np.arange(length).astype(f32)
    arg = (x * max_phase) + f32(phase)
    s = np.sin(arg.astype(np.float64)).astype(f32)
    return (window_f(length) * s) * f32(amp)


def book_gabor_args(row):
    """What the player hands to createGabor for a book atom (maxiAtoms.cpp:211)."""
    pos, length, amp, freq, phase = [np.float32(x) for x in row]
    val = max(min(float(freq), 1.0), 0.0)
    return np.float32(((val - 0.0) / (1.0 - 0.0) * (20000.0 - 20.0)) + 20.0), np.float32(44100.0), int(length), phase, np.float32(float(amp) / 40.0)


class Stream:
    def __init__(self, book=None, num_samples=1, raws=(), adds=()):
        self.book = np.zeros((5, 0), np.float32) if book is None else np.ascontiguousarray(np.array(book, np.float32).T.reshape(5, -1))
        self.num_samples = int(num_samples)
        self.raws = [np.ascontiguousarray(r, np.float32) for r in raws]
        self.adds = list(adds)


class Case:
    def __init__(self, name, blocks, streams, init_seed=None, Q=None):
        self.name, self.blocks, self.streams = name, list(blocks), list(streams)
        self.S, self.T = len(streams), sum(n for _, n in blocks)
        self.init = np.zeros((self.S, self.T), np.float32)
        if init_seed is not None:
            self.init = np.random.default_rng(init_seed).uniform(-1, 1, (self.S, self.T)).astype(np.float32)
        self.Q = Q

    def ops(self, s, reverse_adds=False):
        """The stream's script for tools/gen/atoms_ref_dump.cpp: rows (0, atom, offset) | (1, n, 0) | (2, n, 0)."""
        out = []
        for j, (mode, n) in enumerate(self.blocks):
            a = [(0, atom, off) for (blk, atom, off) in self.streams[s].adds if blk == j]
            out += a[::-1] if reverse_adds else a
            out.append((2 if mode == "play" else 1, n, 0))
        return np.array(out, np.int64).reshape(-1, 3)


def _raw(rng, n, scale=1.0):
    return (rng.uniform(-1, 1, n) * scale).astype(np.float32)


def cases():
    rng = np.random.default_rng(2201)
    out = {}
    # -- the accelerator with raw atoms over CHANGING buffer lengths.  Stream 0: atoms of every length; one beginning on a block's last
    # sample (offset 63 in a block of 64), one ending on a block's first (65 samples from a block's start), one spanning three blocks
    # (130), one straddling the tile edge inside the block of 513 (257); offsets 10 and 5 in front of blocks of 7 and 1, so that
    # startTime + pos falls behind the block's end and the entries STALL (the generator asserts it).  Stream 1: other atoms, other
    # offsets.  Stream 2: nothing, ever.
    blocks = [("fill", n) for n in (64, 64, 7, 7, 64, 513, 1, 1, 64, 7, 513, 64)]
    lens0 = [1, 2, 63, 64, 65, 257, 130, 300]
    s0 = Stream(raws=[_raw(rng, n) for n in lens0],
                adds=[(0, 0, 0), (0, 3, 63), (0, 4, 0), (0, 6, 10), (1, 1, 5), (2, 2, 3), (4, 5, 0), (5, 5, 0), (5, 7, 100), (6, 0, 0), (8, 6, 5), (9, 3, 0),
                      (10, 7, 512)])
    lens1 = [65, 257, 7, 1]
    s1 = Stream(raws=[_raw(rng, n) for n in lens1], adds=[(0, 1, 1), (1, 0, 63), (2, 2, 6), (3, 3, 6), (5, 1, 256), (7, 0, 0), (9, 2, 9)])
    out["accel"] = Case("accel", blocks, [s0, s1, Stream()], init_seed=7)
    # -- the sum's order: three atoms of one onset, a large one and two whose samples are 2^-22 of it
    big, small1, small2 = _raw(rng, 33) + np.float32(2.0), _raw(rng, 33, 2.0 ** -22), _raw(rng, 33, 2.0 ** -22)
    out["order"] = Case("order", [("fill", 64)], [Stream(raws=[big, small1, small2], adds=[(0, 0, 0), (0, 1, 0), (0, 2, 0)])])
    # -- a live list of one LDS piece plus one: 65 atoms of 10 samples due in one block of 7 and ending in the next
    out["piece"] = Case("piece", [("fill", 7), ("fill", 7)], [Stream(raws=[_raw(rng, 10) for _ in range(PIECE + 1)], adds=[(0, k, k % 7) for k in range(PIECE + 1)])], Q=PIECE + 1)
    # -- the player over two full loops of a block-aligned book (8 buffers of 64 per loop, and one more).  Rows: position, length, amp,
    # frequency, phase.  Stream 0 sorted, with two atoms of one position, one of 257 samples across blocks, and one at 448 -- in its
    # buffer (idx + 64) % 512 is 0 and NOTHING is scheduled.  Stream 1 unsorted: the walk stops at 128 in the first two buffers and takes
    # 128, 64 (late: offset +64) and 0 (later still) in the third.  Stream 2: an empty book.
    play = [("play", 64)] * 17
    sorted_book = [(0, 63, 20.0, 0.02, 0.0), (0, 257, 12.0, 0.3, 1.0), (64, 1, 40.0, 0.5, 0.5), (128, 2, 30.0, 0.9, -1.0), (192, 64, 25.0, 0.11, 2.0),
                   (256, 65, 35.0, 0.05, 0.3), (448, 64, 40.0, 0.2, 0.0)]
    unsorted_book = [(0, 65, 30.0, 0.07, 0.2), (128, 63, 22.0, 0.4, 0.0), (64, 257, 18.0, 0.015, 1.5), (0, 2, 40.0, 0.6, 0.1), (320, 64, 28.0, 0.25, 0.0)]
    out["player"] = Case("player", play, [Stream(sorted_book, 512), Stream(unsorted_book, 512), Stream(None, 512)])
    # -- 65 streams, every one with another book (two loops of 256 samples)
    books = []
    for s in range(65):
        rows = [(64 * ((s + k) % 3), LENGTHS[(s + 2 * k) % 6], 10.0 + s + k, ((7 * s + 13 * k) % 50) / 50.0, 0.3 + 0.1 * k) for k in range(1 + s % 3)]
        books.append(Stream(sorted(rows), 256))
    out["player65"] = Case("player65", [("play", 64)] * 8, books)
    return out


# ---- the queue's rules, in Python ----------------------------------------------------------------------------------------------------
def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


class Model:
    """One stream.  An entry: [startTime, pos, size, atom] with atom = ("raw", index) or ("gabor", book index).  step() returns the
    block's segments in queue order: (atom, src_pos, dst_off, count)."""

    def __init__(self, stream):
        self.st, self.idx, self.atom_idx, self.q = stream, 0, 0, []

    def add(self, atom, size, offset):
        self.q.append([self.idx + offset, 0, size, atom])

    def play(self, n):
        bk, ns = self.st.book, self.st.num_samples
        looped = self.idx % ns
        if looped < n:
            self.atom_idx = 0
        limit = np.float32((self.idx + n) % ns)
        while self.atom_idx < bk.shape[1] and bk[0, self.atom_idx] < limit:
            d = abs(np.float32(looped) - bk[0, self.atom_idx])      # |looped - position|: INTEGRATION.md section 4
            self.add(("gabor", self.atom_idx), int(bk[1, self.atom_idx]), int(d))
            self.atom_idx += 1

    def fill(self, n, onset=ONSET_BLOCK):
        segs, keep = [], []
        for e in self.q:
            start = _i32(e[0] + e[1])
            if self.idx <= start < self.idx + n:
                dst = start - self.idx if onset == ONSET_SAMPLE else 0
                cnt = max(0, min(n - dst, e[2] - e[1]))
                if cnt:
                    segs.append((e[3], e[1], dst, cnt))
                e[1] += cnt
            if e[1] != e[2]:
                keep.append(e)
        self.q = keep
        self.idx += n
        return segs


def run_model(case, onset=ONSET_BLOCK):
    """Per stream: the segments of every block, and the state rows (sampleIdx, atomIdx, queue length) and queues after every block."""
    res = []
    for st in case.streams:
        m, blocks, rows, queues = Model(st), [], [], []
        for j, (mode, n) in enumerate(case.blocks):
            for (blk, atom, off) in st.adds:
                if blk == j:
                    m.add(("raw", atom), len(st.raws[atom]), off)
            if mode == "play":
                m.play(n)
            blocks.append(m.fill(n, onset))
            rows.append((m.idx, m.atom_idx, len(m.q)))
            queues.append([(e[0], e[1], e[2]) for e in m.q])
        res.append((blocks, rows, queues))
    return res


def overlap_add(case, model, atoms, accumulate=True):
    """The float32 sum in queue order, sample after sample: numpy only.  atoms(s, atom) -> the atom's float32 samples."""
    out = case.init.copy() if accumulate else np.zeros_like(case.init)
    for s, (blocks, _, _) in enumerate(model):
        t0 = 0
        for (mode, n), segs in zip(case.blocks, blocks):
            for atom, src, dst, cnt in segs:
                a = atoms(s, atom)
                out[s, t0 + dst:t0 + dst + cnt] = out[s, t0 + dst:t0 + dst + cnt] + a[src:src + cnt]     # (float32 + float32, rounded once)
            t0 += n
    return out


def envelope(case, model, accumulate=True):
    """The contract's bound on every output sample (module docstring): raw atoms add nothing to it."""
    tol = np.zeros((case.S, case.T))
    for s, (blocks, _, _) in enumerate(model):
        t0 = 0
        for (mode, n), segs in zip(case.blocks, blocks):
            terms, count, mag = np.zeros(n), np.zeros(n), np.abs(case.init[s, t0:t0 + n]).astype(np.float64) if accumulate else np.zeros(n)
            for atom, src, dst, cnt in segs:
                if atom[0] == "raw":
                    mag[dst:dst + cnt] += np.abs(case.streams[s].raws[atom[1]][src:src + cnt])
                    continue
                _, _, length, _, amp = book_gabor_args(case.streams[s].book[:, atom[1]])
                e = np.abs(window_f(length).astype(np.float64) * float(amp))[src:src + cnt]
                terms[dst:dst + cnt] += 3 * EPS * e + 4 * TINY
                count[dst:dst + cnt] += 1
                mag[dst:dst + cnt] += e
            tol[s, t0:t0 + n] = terms + count * EPS * mag
            t0 += n
    return tol


def gabor_bound(length, amp):
    """The contract's bound on one atom sample."""
    return 3 * EPS * np.abs(window_f(length).astype(np.float64) * float(amp)) + 4 * TINY


# ---- a case through the C-ABI ----------------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data


class Runner:
    """A case on a bank of the library: host=True the _host twins (numpy arrays), host=False the device calls (`dev`: the package, for
    its DeviceBuffer)."""

    def __init__(self, L, case, host, dev=None, Q=None, onset=ONSET_BLOCK):
        self.L, self.case, self.host, self.dev, self.onset = L, case, host, dev, onset
        S = case.S
        starts = np.zeros(S + 1, np.int64)
        for s, st in enumerate(case.streams):
            starts[s + 1] = starts[s] + st.book.shape[1]
        book = np.ascontiguousarray(np.concatenate([st.book for st in case.streams], axis=1), np.float32)
        ns = np.array([st.num_samples for st in case.streams], np.uint32)
        self.raw_off, pool, at = [], [], 0
        for st in case.streams:
            offs = []
            for r in st.raws:
                offs.append(at)
                pool.append(r)
                at += len(r)
            self.raw_off.append(offs)
        pool = np.concatenate(pool).astype(np.float32) if pool else np.zeros(0, np.float32)
        self.Q = Q or case.Q or 96
        make = L.mxg_atoms_bank_create_host if host else L.mxg_atoms_bank_create
        self.bank = make(S, self.Q, _p(starts), _p(book), _p(ns), _p(pool), len(pool))
        assert self.bank, L.mxg_last_error()

    def close(self):
        if self.bank:
            self.L.mxg_atoms_bank_destroy(self.bank)
            self.bank = None

    def add(self, j):
        rows = [(s, atom, off) for s, st in enumerate(self.case.streams) for (blk, atom, off) in st.adds if blk == j]
        if not rows:
            return 0
        stream = np.array([r[0] for r in rows], np.int32)
        kind = np.full(len(rows), RAW, np.int32)
        length = np.array([len(self.case.streams[s].raws[a]) for s, a, _ in rows], np.uint32)
        offset = np.array([r[2] for r in rows], np.uint32)
        raw_off = np.array([self.raw_off[s][a] for s, a, _ in rows], np.uint32)
        fn = self.L.mxg_atoms_add_host if self.host else self.L.mxg_atoms_add
        return fn(self.bank, len(rows), _p(stream), _p(kind), _p(length), _p(offset), None, _p(raw_off))

    def step(self, mode, n, buf, accumulate=True):
        """buf: float32 [S][n] (numpy) -- the block's initial content in, the sums out."""
        L = self.L
        if self.host:
            fn = L.mxg_atoms_play_host if mode == "play" else L.mxg_atoms_fill_host
            return fn(self.bank, n, _p(buf), self.onset, int(accumulate))
        d = self.dev.banks.DeviceBuffer.from_numpy(buf)
        fn = L.mxg_atoms_play if mode == "play" else L.mxg_atoms_fill
        st = fn(self.bank, n, d.ptr, self.onset, int(accumulate), None)
        if st == 0:
            buf[...] = d.numpy()
        d.free()
        return st

    def state(self):
        S, Q = self.case.S, self.Q
        idx, ai, nl = np.zeros(S, np.int64), np.zeros(S, np.uint32), np.zeros(S, np.int32)
        start, pos, size = np.zeros((S, Q), np.int64), np.zeros((S, Q), np.uint32), np.zeros((S, Q), np.uint32)
        assert self.L.mxg_atoms_state(self.bank, _p(idx), _p(ai), _p(nl), _p(start), _p(pos), _p(size)) == 0, self.L.mxg_last_error()
        rows = np.stack([idx, ai.astype(np.int64), nl.astype(np.int64)], axis=1)
        queues = [[(int(start[s, k]), int(pos[s, k]), int(size[s, k])) for k in range(nl[s])] for s in range(S)]
        return rows, queues

    def run(self, accumulate=True, blocks=None):
        """The whole case: out float32 [S][T], rows [S][blocks][3], queues [S][blocks] lists."""
        case = self.case
        out = case.init.copy()
        rows, queues, t0 = [], [], 0
        for j, (mode, n) in enumerate(blocks or case.blocks):
            assert self.add(j) == 0, self.L.mxg_last_error()
            buf = np.ascontiguousarray(out[:, t0:t0 + n])
            assert self.step(mode, n, buf, accumulate) == 0, self.L.mxg_last_error()
            out[:, t0:t0 + n] = buf
            r, q = self.state()
            rows.append(r)
            queues.append(q)
            t0 += n
        return out, np.stack(rows, axis=1), [[queues[j][s] for j in range(len(queues))] for s in range(case.S)]


def golden_queues(g, case, maxq):
    """The recorded queues of a case as Runner.run returns them."""
    q = g["queue/" + case.name]
    return [[[tuple(int(x) for x in e) for e in q[s, j] if e[2] >= 0] for j in range(q.shape[1])] for s in range(case.S)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_case(g, case, out, rows, queues):
    """A run of `case` (Runner.run) against the record under the contract: state and queues bit for bit; streams without a book bit
    for bit, the others inside the derived envelope.  Returns the largest error over its bound."""
    name = case.name
    assert np.array_equal(rows, g["rows/" + name]), name + ": sampleIdx / atomIdx / queue length"
    assert queues == golden_queues(g, case, None), name + ": the queue's entries or their order"
    ref = g["out/" + name]
    tol = envelope(case, run_model(case))
    worst = 0.0
    for s, st in enumerate(case.streams):
        if st.book.shape[1] == 0:
            assert np.array_equal(bits(out[s]), bits(ref[s])), "%s: stream %d (raw atoms) is not bit-identical" % (name, s)
            continue
        err = np.abs(out[s].astype(np.float64) - ref[s])
        assert (err <= tol[s]).all(), "%s: stream %d: %.3g over the bound at %d" % (name, s, (err - tol[s]).max(), int(np.argmax(err - tol[s])))
        assert ((ref[s] == 0) == (out[s] == 0)).all() or (tol[s][(ref[s] == 0) != (out[s] == 0)] > 0).all()
        live = tol[s] > 0
        worst = max(worst, float((err[live] / tol[s][live]).max()) if live.any() else 0.0)
    return worst


def overflow_case():
    """Stream 0: a book of five atoms at position 0 (a live list of 4 overflows in the first block); stream 1: two atoms (it does not)."""
    rows = [(0, 64, 20.0 + k, 0.1 * (k + 1), 0.3) for k in range(5)]
    return Case("overflow", [("play", 64)] * 2, [Stream(rows, 512), Stream(rows[:2], 512)], init_seed=11, Q=4)
