"""A model of maxiConvolveBank's ring head (kernel K24, csrc/convolve_bank.hip), for the tests on both sides: which of the paths that
depend on the head a given split of the blocks into calls takes.  Pure Python, the library is not imported: it restates the two lines
of bank_play() -- a call of nb blocks goes through in chunks of c = min(kChunk, nb - b0) frames, and behind each chunk the head moves to
(head + c) % R -- so that a test can assert that ITS inputs wrap the ring, whatever kChunk or the impulse lengths become later.
Also the shapes that the GPU tests run and tests/test_spectral_cpu.py pins the port at (one table, so that the two cannot drift)."""

KCHUNK = 16  # kChunk of csrc/convolve_bank.hip (tests/test_convolve_bank_cabi.py checks the source for it)
EVENTS = frozenset(["later_chunk", "store_wrap", "lands_on_0", "read_wrap"])


def frames_of(length, fftsize):
    """impulse frames of maxiConvolve::setup: the impulse padded by bins - length % bins zeros, in whole fftsize frames"""
    bins = fftsize // 2
    return (length + bins - length % bins) // fftsize


def ring_rows(frames):
    """R of a bank whose impulses have these frame counts"""
    return max(max(frames), 1) - 1 + KCHUNK


def ring_events(R, Kmax, split):
    """The events of a fresh (or reset) bank fed the calls of `split`, as a set of names:
      later_chunk  a chunk with b0 > 0: a call's second or later launch
      store_wrap   head + c > R: the chunk's new rows straddle the end of the ring
      lands_on_0   head + c == R: the advance lands exactly on slot 0
      read_wrap    a chunk that starts at head < Kmax - 1 after the ring has wrapped: some of the Kmax - 1 rows of history it reads
                   sit at the top of the ring, and they are frames that were stored there, not the zeros of reset()"""
    head, wrapped, ev = 0, False, set()
    for nb in split:
        b0 = 0
        while b0 < nb:
            c = min(KCHUNK, nb - b0)
            if b0 > 0:
                ev.add("later_chunk")
            if wrapped and head < Kmax - 1:
                ev.add("read_wrap")
            if head + c > R:
                ev.add("store_wrap")
            if head + c == R:
                ev.add("lands_on_0")
            wrapped = wrapped or head + c >= R
            head = (head + c) % R
            b0 += c
    return ev


def ring_head(R, split):
    """the head after the calls of `split`"""
    head = 0
    for nb in split:
        for b0 in range(0, nb, KCHUNK):
            head = (head + min(KCHUNK, nb - b0)) % R
    return head


# name -> (fftsize, hopsize, impulse lengths of impulses 0 and 1, splits); every split of a case feeds the same number of blocks
SPLITS_R20 = ([45], [17, 16, 12], [3, 16, 1, 20, 5], [19, 1, 2, 23], [1] * 45)
WRAP_CASES = {
    "k5_k1": (64, 16, (300, 40), SPLITS_R20),                                    # R = 20: 45 blocks wrap it twice
    "k0_k5": (64, 16, (20, 300), SPLITS_R20),                                    # streams 0 and 2 have no impulse frame at all
    "k1_k39": (1024, 512, (900, 40000), ([112], [54, 33, 25], [38, 16, 58])),    # R = 54: the history spans most of the ring
    "k5_k1_hop64": (64, 64, (300, 40), SPLITS_R20),                              # the window covers the whole block
}
# one per launch geometry of bank_play(): pairs = fftsize / 4 lanes a row, threads = 64 up to 64 pairs, then pairs up to 256, then 256
# in laneBlocks = pairs / 256 workgroups a row.  One split each, which has to produce all four events alone.
GEOMETRY_CASES = {
    "f8": (8, 8, (30, 5), ([18, 1, 2, 22],)),                 # K = 4, 1: R = 19; 2 live lanes of 64
    "f16": (16, 4, (50, 10), ([17, 1, 3, 21],)),              # K = 3, 1: R = 18; 4 live lanes
    "f256": (256, 256, (700, 150), ([17, 1, 3, 21],)),        # K = 3, 1: 64 pairs, the edge of `pairs > 64`
    "f512": (512, 128, (1300, 300), ([17, 1, 3, 21],)),       # K = 3, 1: 128 lanes
    "f1024": (1024, 1024, (2600, 600), ([17, 1, 3, 21],)),    # K = 3, 1: 256 lanes, one lane block
    "f2048": (2048, 2048, (6000, 1200), ([17, 1, 3, 21],)),   # K = 3, 1: two lane blocks
    "f4096": (4096, 1024, (11000, 2400), ([17, 1, 3, 21],)),  # K = 3, 1: four
    "f8192": (8192, 8192, (20000, 4800), ([1, 16, 20],)),     # K = 2, 1: R = 17; eight
}
ALL_CASES = dict(WRAP_CASES, **GEOMETRY_CASES)


def case_frames(name):
    F, _, lens, _ = ALL_CASES[name]
    return tuple(frames_of(L, F) for L in lens)


def case_blocks(name):
    totals = {sum(s) for s in ALL_CASES[name][3]}
    assert len(totals) == 1, name
    return totals.pop()
