"""GPU: mxg_bark_batch / mxg_octave_batch (K19, bands.hip) against the numpy model of tests/bands_host.py (pinned to the host build
of the same arithmetic by test_bands_host.py) on the smallest shapes at which the tiling can go wrong: frame counts around the
64-frame wave, bin counts below, at and above the 32-bin chunk, rows with an unaligned stride and base pointer, several streams,
state carried over three calls.  Band sums, averages, peaks and hold counters are compared bit for bit; specific / relative / total
within the bounds of bands_host.py (the measured maxima are printed).  Every output is followed by canary values that must
survive, every NULL-output combination leaves the arrays not asked for untouched, NaN positions coincide with the model's."""
import itertools

import numpy as np
import pytest

import bands_host as bh

pytestmark = pytest.mark.gpu
NFRAMES = (1, 63, 64, 65, 130)
CANARY = 8


def dev_rows(mx, x, stride, offset):
    """x [nframes][bins] float32 as rows of `stride` floats starting `offset` floats into a device block (the gaps hold NaN)."""
    nf, bins = x.shape
    host = np.full(offset + nf * stride + 4, np.nan, np.float32)
    for f in range(nf):
        host[offset + f * stride: offset + f * stride + bins] = x[f]
    buf = mx.DeviceBuffer.from_numpy(host)
    return buf, buf.ptr + 4 * offset


def out_buf(mx, n, dtype, fill):
    return mx.DeviceBuffer.from_numpy(np.full(n + CANARY, fill, dtype))


def take(buf, n, fill, what):
    a = buf.numpy()
    assert (a[n:] == fill).all(), "%s: the canary after the output is gone" % what
    return a[:n]


def test_golden_cases_through_the_cabi(mx, golden):
    """tests/golden/bands.npz, recorded from the compiled reference: limits, maps, averages, peaks and hold counters bit for bit
    (the octave frames cut into calls of uneven length, state carried on the device), the loudness within the bounds."""
    g = golden("bands.npz")
    be = bh.GpuBackend(mx)
    print("device against the reference: measured maxima %s" % bh.play_bark_cases(be, g, exact=False))
    bh.play_octave_cases(be, g)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("bS", [16, 64, 1024, 4096])
def test_bark_against_model(mx, bS, aligned):
    lib, model = mx.lib(), bh.ModelBackend()
    bark = mx.maxiBarkBatch()
    bark.setup(44100, bS)
    lim = bark.limits()
    assert lim.tolist() == model.bark_limits(44100, bS).tolist()
    bins = bS // 2
    stride, offset = (bins, 0) if aligned else (bins + 3, 1)
    worst = {}
    for nf in NFRAMES:
        x = bh.bark_spectra(nf, bins, 100 + nf)
        ref = model.bark(lim, x)
        src, ptr = dev_rows(mx, x, stride, offset)
        outs = [out_buf(mx, nf * 24, np.float64, -7.0) for _ in range(3)] + [out_buf(mx, nf, np.float64, -7.0)]
        mx._lib.check(lib.mxg_bark_batch(bark.plan, ptr, stride, nf, *[o.ptr for o in outs], None), "mxg_bark_batch")
        got = [take(o, nf * 24, -7.0, "bark").reshape(nf, 24) for o in outs[:3]] + [take(outs[3], nf, -7.0, "bark total")]
        bh.bits_equal(got[0], ref[0], "band sums, bufferSize %d, %d frames" % (bS, nf))
        w = bh.check_loudness(got[1:], ref[1:], "bufferSize %d, %d frames" % (bS, nf))
        worst = {k: max(v, worst.get(k, 0)) for k, v in w.items()}
        if nf > 4:
            assert np.isnan(got[2][1]).all() and got[3][1] == 0   # the silent frame
    print("bark bufferSize %d aligned %s: measured maxima %s" % (bS, aligned, worst))


def test_bark_null_outputs_leave_the_others_untouched(mx):
    lib, model = mx.lib(), bh.ModelBackend()
    bark = mx.maxiBarkBatch()
    bark.setup(22050, 1024)
    lim = bark.limits()
    nf = 65
    x = bh.bark_spectra(nf, 512, 5)
    ref = model.bark(lim, x)
    src, ptr = dev_rows(mx, x, 512, 0)
    sizes = [nf * 24, nf * 24, nf * 24, nf]
    for want in itertools.product((False, True), repeat=4):
        outs = [out_buf(mx, n, np.float64, -7.0) for n in sizes]
        args = [o.ptr if w else None for o, w in zip(outs, want)]
        mx._lib.check(lib.mxg_bark_batch(bark.plan, ptr, 512, nf, *args, None), "mxg_bark_batch")
        for i, (o, w, n) in enumerate(zip(outs, want, sizes)):
            a = o.numpy()
            if not w:
                assert (a == -7.0).all(), (want, i)
                continue
            assert (a[n:] == -7.0).all(), (want, i)
            r = ref[i]
            got = a[:n].reshape(r.shape)
            if i == 0:
                bh.bits_equal(got, r, "band sums %s" % (want,))
                continue
            assert np.array_equal(np.isnan(got), np.isnan(r)) and np.array_equal(np.isinf(got), np.isinf(r)), (want, i)
            fin = np.isfinite(r)
            if i == 1:
                assert bh.ulp64(got[fin], r[fin]).max() <= bh.ULP_SPECIFIC, (want, i)
            else:
                assert (np.abs(got[fin] - r[fin]) <= (bh.REL_RELATIVE if i == 2 else bh.REL_TOTAL) * np.abs(r[fin])).all(), (want, i)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("sr,n,per", [(44100.0, 8, 1), (44100.0, 512, 12), (44100.0, 2048, 1), (44100.0, 512, 0)])
def test_octave_averages_against_model(mx, sr, n, per, aligned):
    lib, model = mx.lib(), bh.ModelBackend()
    oc = mx.maxiOctaveBatch()
    oc.setup(sr, n, per)
    m, nA = model.octave_map(sr, n, per)
    assert oc.nAverages == nA and oc.spe2avg.tolist() == m.tolist()
    stride, offset = (n, 0) if aligned else (n + 3, 1)
    for nf in NFRAMES:
        x = bh.octave_spectra(nf, n, 200 + nf)
        ref, _ = model.octave(m, nA, x, 1, nf, 1.0, 0.01, 0, 0.9)
        src, ptr = dev_rows(mx, x, stride, offset)
        avg = out_buf(mx, nf * nA, np.float32, -7.0)
        mx._lib.check(lib.mxg_octave_batch(oc.plan, ptr, stride, nf, 1, 1.0, 0.01, 0, 0.9, avg.ptr, None, None, None, None), "mxg_octave_batch")
        bh.bits_equal(take(avg, nf * nA, -7.0, "averages").reshape(nf, nA), ref, "averages, %d bins, %d frames" % (n, nf))


@pytest.mark.parametrize("S,fps", list(itertools.product((1, 3, 65), (1, 2, 7))))
def test_octave_peaks_carry_state_over_three_calls(mx, S, fps):
    lib, model = mx.lib(), bh.ModelBackend()
    oc = mx.maxiOctaveBatch(S)
    oc.setup(44100.0, 512, 3)
    m, nA = oc.spe2avg, oc.nAverages
    ps, hs = np.zeros((S, nA), np.float32), np.zeros((S, nA), np.int32)
    d_ps, d_hs = out_buf(mx, S * nA, np.float32, 0.0), out_buf(mx, S * nA, np.int32, 0)
    for call, (hold, decay) in enumerate(((2, 0.9), (0, 0.0), (2, 1.0))):
        x = bh.octave_spectra(S * fps, 512, 300 + call)
        if call == 1:
            x *= np.float32(0.25)   # below the peaks of the first call: they hold, count down and decay
        ra, rp = model.octave(m, nA, x, S, fps, 1.0, 0.0, hold, decay, ps, hs)
        src, ptr = dev_rows(mx, x, 512, 0)
        avg, pk = out_buf(mx, S * fps * nA, np.float32, -7.0), out_buf(mx, S * fps * nA, np.float32, -7.0)
        mx._lib.check(lib.mxg_octave_batch(oc.plan, ptr, 512, S, fps, 1.0, 0.0, hold, decay, avg.ptr, pk.ptr, d_ps.ptr, d_hs.ptr, None),
                      "mxg_octave_batch")
        bh.bits_equal(take(avg, S * fps * nA, -7.0, "averages").reshape(-1, nA), ra, "averages, call %d" % call)
        bh.bits_equal(take(pk, S * fps * nA, -7.0, "peaks").reshape(-1, nA), rp, "peaks, call %d" % call)
        bh.bits_equal(take(d_ps, S * nA, 0.0, "peak state").reshape(S, nA), ps, "peak state, call %d" % call)
        assert take(d_hs, S * nA, 0, "hold state").reshape(S, nA).tolist() == hs.tolist()
    # the peak pass without a peaks array: the state moves on as the model's
    ra, _ = model.octave(m, nA, x, S, fps, 1.0, 0.0, 1, 0.9, ps, hs)
    avg = out_buf(mx, S * fps * nA, np.float32, -7.0)
    mx._lib.check(lib.mxg_octave_batch(oc.plan, ptr, 512, S, fps, 1.0, 0.0, 1, 0.9, avg.ptr, None, d_ps.ptr, d_hs.ptr, None), "mxg_octave_batch")
    bh.bits_equal(take(avg, S * fps * nA, -7.0, "averages").reshape(-1, nA), ra, "averages, no peaks array")
    bh.bits_equal(take(d_ps, S * nA, 0.0, "peak state").reshape(S, nA), ps, "peak state, no peaks array")
    assert take(d_hs, S * nA, 0, "hold state").reshape(S, nA).tolist() == hs.tolist()
    # no peak pass: the state and a peaks array are not touched
    avg = out_buf(mx, S * fps * nA, np.float32, -7.0)
    mx._lib.check(lib.mxg_octave_batch(oc.plan, ptr, 512, S, fps, 1.0, 0.0, 0, 0.9, avg.ptr, None, None, None, None), "mxg_octave_batch")
    bh.bits_equal(take(d_ps, S * nA, 0.0, "peak state").reshape(S, nA), ps, "peak state after a call without the peak pass")


def test_python_classes(mx):
    bark = mx.maxiBarkBatch()
    bark.setup(44100, 1024)
    x = bh.bark_spectra(70, 512, 3)
    d = mx.DeviceBuffer.from_numpy(x)
    ref = bh.ModelBackend().bark(bark.limits(), x)
    out = bark.analyse(d, bandsum=True, specific=True, relative=True, total=True)
    bh.bits_equal(out["bandsum"].numpy(), ref[0], "maxiBarkBatch band sums")
    bh.check_loudness([out[k].numpy() for k in ("specific", "relative", "total")], ref[1:], "maxiBarkBatch")
    oc = mx.maxiOctaveBatch(2)
    oc.setup(44100.0, 512, 12)
    oc.peakHoldTime = 2
    y = bh.octave_spectra(2 * 35, 512, 4)
    ps, hs = np.zeros((2, oc.nAverages), np.float32), np.zeros((2, oc.nAverages), np.int32)
    ra, rp = bh.ModelBackend().octave(oc.spe2avg, oc.nAverages, y, 2, 35, 1.0, 0.0, 2, 0.9, ps, hs)
    avg, pk = oc.calculate(mx.DeviceBuffer.from_numpy(y))
    bh.bits_equal(avg.numpy(), ra, "maxiOctaveBatch averages")
    bh.bits_equal(pk.numpy(), rp, "maxiOctaveBatch peaks")
    assert oc.peakHoldTimes.numpy().tolist() == hs.tolist()
