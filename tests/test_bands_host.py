"""CPU (-m "not gpu"): mxg_bands.h -- the arithmetic bands.hip's kernels run -- compiled for the host with g++ under the oracle's
FPFLAGS (tests/host_bands.cpp) against the numpy model of tests/bands_host.py: Bark limits, octave maps, band sums, averages,
peaks and hold counters BIT FOR BIT; specific / relative / total within the bounds of bands_host.py (the host build calls glibc's
pow, numpy its own).  The table shapes the reference is known to give are pinned as numbers.  (tests/host_bands.cpp with
-DBND_HOST_MAIN is the stand-alone program for a run under -fsanitize=address,undefined.)"""
import numpy as np
import pytest

import bands_host as bh


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    return bh.HostBackend(bh.build(tmp_path_factory.mktemp("bands")))


def test_bark_limits_host_model_and_known_shapes(be):
    m = bh.ModelBackend()
    for sR, bS in bh.BARK_CONFIGS + [(44100, 2), (44100, 3), (44100, 64), (48000, 4096), (11025, 256)]:
        lim = be.bark_limits(sR, bS)
        assert lim.tolist() == m.bark_limits(sR, bS).tolist(), (sR, bS)
        assert lim[0] == 0 and lim[24] == bS // 2 - 1 and (np.diff(lim) >= 0).all(), (sR, bS)
    lim = be.bark_limits(44100, 16)   # empty bands: limits 0 1 1 1 ... 7
    assert lim[:4].tolist() == [0, 1, 1, 1] and lim[24] == 7
    assert (np.diff(be.bark_limits(22050, 1024)) == 0).any() and 252 in be.bark_limits(22050, 1024).tolist()
    assert be.bark_limits(44100, 1024)[23] == 511 - 245   # band 23 alone is 245 of 512 bins


def test_octave_map_host_model_and_known_shapes(be):
    m = bh.ModelBackend()
    for sr in (44100.0, 48000.0, 8000.0):
        for n in (8, 16, 256, 512, 2048):
            for per in (0, 1, 3, 12, 24):
                a, na = be.octave_map(sr, n, per)
                b, nb = m.octave_map(sr, n, per)
                assert na == nb and a.tolist() == b.tolist(), (sr, n, per)
    a, na = be.octave_map(44100.0, 512, 12)
    assert na == 104 and len(set(a.tolist())) == 76
    a, na = be.octave_map(44100.0, 8, 1)
    assert a.tolist() == [6, 7, 8, 8, 8, 9, 9, 9] and na == 9
    a, na = be.octave_map(44100.0, 2048, 1)
    assert na == 9 and a[0] == 0
    assert be.octave_map(100.0, 8, 1)[1] == 0


@pytest.mark.parametrize("sR,bS", bh.BARK_CONFIGS)
def test_bark_host_against_model(be, sR, bS):
    lim = be.bark_limits(sR, bS)
    x = bh.bark_spectra(9, bS // 2, 19)
    hs, *hl = be.bark(lim, x)
    ms, *ml = bh.ModelBackend().bark(lim, x)
    bh.bits_equal(hs, ms, "band sums")
    assert (hs[1] == 0).all() and np.isnan(hl[1][1]).all() and hl[2][1] == 0   # the silent frame: 24 NaNs in relative
    assert np.isnan(hs[2]).sum() == 1 and np.isinf(hs[4]).sum() == 1 and (hs[3] < 0).any() and np.isnan(hl[0][3]).any()
    empty = np.diff(lim) == 0
    assert (hs[:, empty] == 0).all() and (hl[0][:, empty] == 0).all()   # pow(0, 0.23) = 0 exactly
    print("bark %s: host against the model %s" % ((sR, bS), bh.check_loudness(hl, ml, str((sR, bS)))))
    # the sequential order matters on this input: summed in ascending order of magnitude, some band gets other bits
    fin = [f for f in range(9) if np.isfinite(x[f]).all()]
    resorted = np.array([[np.add.accumulate(np.sort(x[f, lim[b]:lim[b + 1]].astype(np.float64)))[-1] if lim[b + 1] > lim[b] else 0.0
                          for b in range(24)] for f in fin])
    if bS >= 512:
        assert (resorted != hs[fin]).any()


@pytest.mark.parametrize("sr,n,per", bh.OCTAVE_CONFIGS)
def test_octave_host_against_model_with_state_over_uneven_calls(be, sr, n, per):
    model = bh.ModelBackend()
    m, nA = be.octave_map(sr, n, per)
    x = bh.octave_spectra(44, n, 7)
    for hold, decay, slope in ((0, 0.9, 0.0), (2, 0.9, 0.01), (2, 0.0, 0.0), (0, 1.0, -0.001)):
        ps, hs = np.zeros((1, nA), np.float32), np.zeros((1, nA), np.int32)
        pm, hm = ps.copy(), hs.copy()
        seen_hold = seen_decay = False
        for a, b in zip((0, 1, 8, 20, 27), (1, 8, 20, 27, 44)):   # calls of 1, 7, 12, 7, 17 frames
            ha, hp = be.octave(m, nA, x[a:b], 1, b - a, 1.0, slope, hold, decay, ps, hs)
            ma, mp = model.octave(m, nA, x[a:b], 1, b - a, 1.0, slope, hold, decay, pm, hm)
            bh.bits_equal(ha, ma, "averages %d..%d" % (a, b))
            bh.bits_equal(hp, mp, "peaks %d..%d" % (a, b))
            bh.bits_equal(ps, pm, "peak state at %d" % b)
            assert hs.tolist() == hm.tolist()
            seen_hold |= bool((hs > 0).any())
            seen_decay |= bool((hp < np.maximum.accumulate(hp, axis=0)).any())
        assert seen_hold == (hold > 0) and (seen_decay or decay == 1.0)
    full, _ = be.octave(m, nA, x, 1, 44, 1.0, 0.0, 0, 0.9)
    assert np.isnan(full[9]).any() and np.isfinite(full[:9]).all()
    if (sr, n, per) == (44100.0, 8, 1):   # averages[0 .. 6) all equal bin 0's value, the last three bins are dropped
        assert (full[:9, :6] == x[:9, :1]).all()


@pytest.fixture(scope="module")
def g(golden):
    return golden("bands.npz")


def test_host_build_reproduces_the_reference(be, g):
    """Limits, maps, averages, peaks and hold counters bit for bit; specific / relative / total too: the host build calls the
    glibc pow the reference was recorded with."""
    print("host build against the reference:", bh.play_bark_cases(be, g, exact=True))
    bh.play_octave_cases(be, g)
    bh.play_octave_cases(be, g, (0, 44))


def test_model_reproduces_the_reference(g):
    """The numpy model: tables and every octave output bit for bit, the loudness within the bounds (numpy's pow)."""
    print("model against the reference:", bh.play_bark_cases(bh.ModelBackend(), g, exact=False))
    bh.play_octave_cases(bh.ModelBackend(), g)


def test_golden_holds_the_cases(g):
    """What the file must contain for the tests above to mean something."""
    assert {1, 7} <= set(np.diff(bh.OCTAVE_CUTS).tolist()) and bh.OCTAVE_FRAMES >= 40
    assert {h for h, _, _ in bh.OCTAVE_RUNS} == {0, 2} and {d for _, d, _ in bh.OCTAVE_RUNS} == {0.9, 0.0, 1.0}
    assert any(s != 0 for _, _, s in bh.OCTAVE_RUNS)
    for i, (sR, bS) in enumerate(bh.BARK_CONFIGS):
        sp, rl = g["bark/%d/specific" % i], g["bark/%d/relative" % i]
        assert g["bark/%d/limits" % i][24] == bS // 2 - 1
        assert np.isnan(rl[1]).all() and np.isnan(sp[2]).sum() == 1 and np.isnan(sp[3]).any() and np.isinf(sp[4]).sum() == 1
    for i in range(len(bh.OCTAVE_CONFIGS)):
        assert np.isnan(g["oct/%d/0/averages" % i][9]).any() and (g["oct/%d/1/holds" % i] > 0).any()
    assert "sha256" in str(g["provenance"])
