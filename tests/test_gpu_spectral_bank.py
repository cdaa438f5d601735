"""GPU parity (-m gpu): maxiFFTBank / maxiIFFTBank (kernel K29) against the oracle per stream, against the single-stream entry
points on the same device (bit for bit: the same arithmetic), across the splits of tests/test_spectral_bank_cabi.py, in both row
layouts; ffttest.cpp's chain over 65 streams; the FFT bank's rows into the maxiMFCC mirror; the launch count.
Every case feeds one block of ntot(hop) samples per stream, as long as the longest split: a split that sums to fewer samples uses
its head, and what the bank returns is then the head of the one reference computed for the block (frames and overlap-add are
causal)."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_spectral import PHASE_ATOL
from test_spectral_bank_cabi import splits

pytestmark = pytest.mark.gpu

NTOT = 2000
FFT_CASES = ([(V, fs, hop) for (fs, hop) in [(64, 16), (64, 24), (8, 8), (1024, 256), (2048, 512)] for V in (1, 3, 65, 130)]
             + [(3, 8192, 2048)])
IFFT_CASES = [(65, 64, 16, 0), (65, 64, 24, 0), (65, 8, 8, 0), (65, 64, 16, 48), (65, 1024, 256, 0), (3, 2048, 512, 0), (3, 8192, 2048, 0)]
KEYS = ("real", "imag", "mags", "phases")


def ntot(hop):
    return max(sum(c) for c in splits(hop))


def same_f32(a, b):
    """bit equality of float32 arrays, NaN == NaN whatever its sign and payload (conftest.assert_bits_equal says why)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def special_streams(V):
    """(stream of the +Inf, stream of the NaN)"""
    return (1, V - 1) if V >= 3 else (0, 0)


@functools.lru_cache(maxsize=None)
def block(V, n=NTOT, seed=0):
    """double [n][V], none of it representable as float; one +Inf and one NaN in known streams"""
    rng = np.random.default_rng(1000 * V + seed)
    x = rng.uniform(-1, 1, (n, V))
    assert (x.astype(np.float32).astype(np.float64) != x).all()
    si, sn = special_streams(V)
    x[700, si] = np.inf
    x[1300, sn] = np.nan
    x.setflags(write=False)
    return x


def rows_of(buf, V, F, bins, layout):
    """a bank's [V * F][bins] block as [V][F][bins]"""
    a = buf.numpy()
    return a.reshape(F, V, bins).transpose(1, 0, 2) if layout == 0 else a.reshape(V, F, bins)


def run_fft_bank(bank, x, calls, layout, want=KEYS):
    got = {k: [] for k in want}
    off = 0
    for N in calls:
        F = bank.frames(N)
        out = bank.process(x[off:off + N], N=N, want=want, layout=layout)
        for k in want:
            got[k].append(rows_of(out[k], bank.V, F, bank.bins, layout))
        off += N
    return {k: np.concatenate(got[k], axis=1) for k in want}


@functools.lru_cache(maxsize=None)
def fft_expected(port, V, fs, hop):
    """the oracle on every stream of block(V, ntot(hop)): {key: [V][ntot(hop) // hop][bins]}"""
    x = block(V, ntot(hop))
    per = [port.fft_stream(x[:, v].astype(np.float32), fs, hop, 0) for v in range(V)]
    return {k: np.stack([p[k] for p in per]) for k in KEYS}


def fft_single(mx, V, fs, hop):
    """mxg_fft_batch on every stream alone, same device: {key: [V][ntot(hop) // hop][bins]}"""
    x = block(V, ntot(hop))
    got = {k: [] for k in KEYS}
    for v in range(V):
        f = mx.maxiFFT()
        f.setup(fs, hop, 0)
        assert f.process_signal(x[:, v].astype(np.float32), want_complex=True) == x.shape[0] // hop
        for k, b in zip(KEYS, (f.getReal(), f.getImag(), f.getMagnitudes(), f.getPhases())):
            got[k].append(b.numpy())
    return {k: np.stack(got[k]) for k in KEYS}


def phase_close(a, b):
    nan = np.isnan(b)
    if not np.array_equal(np.isnan(a), nan):
        return False
    d = np.abs(np.where(nan, 0, a) - np.where(nan, 0, b))
    d = np.minimum(d, 2 * np.pi - d)
    return float(d.max(initial=0)) <= PHASE_ATOL


@pytest.mark.parametrize("V,fs,hop", FFT_CASES)
def test_fft_bank_against_oracle_and_single_stream(mx, port, V, fs, hop):
    x = block(V, ntot(hop))
    e = fft_expected(port, V, fs, hop)
    s = fft_single(mx, V, fs, hop)
    si, sn = special_streams(V)
    clean = [v for v in range(V) if v not in (si, sn)]
    assert np.isnan(e["mags"][si]).any() and np.isnan(e["mags"][sn]).any()   # the Inf and the NaN reached their streams' frames
    bank = mx.maxiFFTBank(V, fs, hop)
    for calls in splits(hop):
        F = sum(calls) // hop
        for layout in ((0, 1) if len(calls) == 1 else (len(calls) % 2,)):
            bank.reset()
            g = run_fft_bank(bank, x, calls, layout)
            tag = (calls, layout)
            assert g["mags"].shape == (V, F, fs // 2), tag
            assert bank.pos == sum(calls) % hop, tag
            for k in ("real", "imag", "mags"):
                assert same_f32(g[k], e[k][:, :F]), (tag, k, "oracle")
            assert phase_close(g["phases"], e["phases"][:, :F]), tag
            for k in KEYS:
                assert same_f32(g[k], s[k][:, :F]), (tag, k, "mxg_fft_batch on the stream alone")
            assert all(np.isfinite(g[k][clean]).all() for k in KEYS), tag       # the neighbours of the Inf and NaN streams


def test_fft_bank_optional_outputs_state_and_two_streams(mx, port):
    """mags alone and real + imag alone take other instantiations of the 1024-point kernel; a second bank on a second stream runs
    between the calls of the first without disturbing it; reset() reproduces the first run."""
    V, fs, hop = 65, 1024, 256
    x, y = block(V), block(V, seed=1)
    assert ntot(hop) == NTOT
    e = fft_expected(port, V, fs, hop)
    calls = splits(hop)[0]
    F = sum(calls) // hop
    L = mx.lib()
    st = ctypes.c_void_p(L.mxg_stream_create())
    try:
        a = mx.maxiFFTBank(V, fs, hop)
        b = mx.maxiFFTBank(V, fs, hop, stream=st)
        got_a, got_b, off = [], [], 0
        for N in calls:
            oa = a.process(x[off:off + N], N=N, want=("mags",))
            ob = b.process(y[off:off + N], N=N, want=("real", "imag"))
            got_a.append(rows_of(oa["mags"], V, oa["mags"].shape[0] // V, fs // 2, 0))
            got_b.append(rows_of(ob["real"], V, ob["real"].shape[0] // V, fs // 2, 0))
            off += N
        ga, gb = np.concatenate(got_a, axis=1), np.concatenate(got_b, axis=1)
        assert same_f32(ga, e["mags"][:, :F])
        ey = np.stack([port.fft_stream(y[:, v].astype(np.float32), fs, hop, 0, want=("real",))["real"] for v in range(V)])
        assert same_f32(gb, ey[:, :F])
        a.reset()
        again = run_fft_bank(a, x, calls, 0, want=("mags",))["mags"]
        assert same_f32(again, ga)
    finally:
        L.mxg_sync()
        L.mxg_stream_destroy(st)


def run_ifft_bank(bank, A, B, calls, form, layout):
    """A, B [V][C][bins]: row c of stream v is consumed at the bank's c-th point -> (out [sum(calls)][V], rows used)"""
    outs, c0 = [], 0
    for N in calls:
        C = bank.rows(N)
        a, b = A[:, c0:c0 + C], B[:, c0:c0 + C]
        if layout == 0:
            a, b = a.transpose(1, 0, 2), b.transpose(1, 0, 2)
        outs.append(bank.process(np.ascontiguousarray(a), np.ascontiguousarray(b), N, form=form, layout=layout).numpy())
        c0 += C
    return np.concatenate(outs, axis=0), c0


def spectra(V, fs, hop, seed, zero_phase):
    rng = np.random.default_rng(fs + 7 * hop + seed)
    C = -(-ntot(hop) // hop)
    m = np.abs(rng.normal(0, 3, (V, C, fs // 2))).astype(np.float32)
    ph = np.zeros_like(m) if zero_phase else rng.uniform(-np.pi, np.pi, m.shape).astype(np.float32)
    return m, ph


@pytest.mark.parametrize("V,fs,hop,win", IFFT_CASES)
def test_ifft_bank_zero_phase_bit_exact(mx, port, V, fs, hop, win):
    """Phases 0: cos = 1 and sin = 0 on every libm, so outputs and carried buffers are the oracle's bits per stream, for calls
    that start and end in the middle of a hop."""
    m, ph = spectra(V, fs, hop, 0, True)
    full = [port.ifft_stream(m[v], ph[v], fs, hop, win)[0] for v in range(V)]
    bank = mx.maxiIFFTBank(V, fs, hop, win)
    for calls in splits(hop):
        n = sum(calls)
        layout = len(calls) % 2
        bank.reset()
        out, used = run_ifft_bank(bank, m, ph, calls, 0, layout)
        assert used == -(-n // hop) and bank.pos == n % hop, calls
        exp = np.stack([f[:n] for f in full], axis=1).astype(np.float64)
        assert same_f64(out, exp), calls
        bufs = bank.buffers()
        for v in range(V):
            assert same_f32(bufs[v], port.ifft_stream(m[v, :used], ph[v, :used], fs, hop, win)[2]), (calls, v)


@pytest.mark.parametrize("V,fs,hop,win", [(65, 64, 16, 48), (65, 1024, 256, 0)])
def test_ifft_bank_random_phase_and_cartesian(mx, port, V, fs, hop, win):
    """Random phases: the bits of mxg_ifft_batch per stream with a carried buffer (the device's own cosf / sinf on both sides), and
    within test_ifft_random_phase's bound of the oracle: 4e-7 * (sum of a frame's magnitudes) / n * overlap.  Cartesian rows: the
    bits of mxg_ifft_batch_complex(as_reference = 0) per stream."""
    L = mx.lib()
    m, ph = spectra(V, fs, hop, 1, False)
    re, im = spectra(V, fs, hop, 2, False)
    re = re * np.sign(im)                                             # signed real parts
    C = m.shape[1]
    single, single_buf, cart, cart_buf = [], [], [], []
    for v in range(V):
        f = mx.maxiIFFT()
        f.setup(fs, hop, win)
        single.append(f.process_frames(m[v], ph[v]).numpy())
        single_buf.append(f.buffer.numpy())
        g = mx.maxiIFFT()
        g.setup(fs, hop, win)
        dr, di = mx.DeviceBuffer.from_numpy(re[v]), mx.DeviceBuffer.from_numpy(im[v])
        o = mx.DeviceBuffer(C * hop, np.float32, zero=False)
        mx._lib.check(L.mxg_ifft_batch_complex(g.plan, dr.ptr, di.ptr, C, 0, g.buffer.ptr, o.ptr, None, None), "mxg_ifft_batch_complex")
        cart.append(o.numpy())
        cart_buf.append(g.buffer.numpy())
    bank = mx.maxiIFFTBank(V, fs, hop, win)
    for calls in splits(hop):
        n = sum(calls)
        layout = (len(calls) + 1) % 2
        for form, A, B, ref, ref_buf in ((0, m, ph, single, single_buf), (1, re, im, cart, cart_buf)):
            bank.reset()
            out, used = run_ifft_bank(bank, A, B, calls, form, layout)
            assert same_f64(out, np.stack([r[:n] for r in ref], axis=1).astype(np.float64)), (calls, form)
            if used == C:
                assert same_f32(bank.buffers(), np.stack(ref_buf)), (calls, form)
            if form == 0:
                for v in range(V):
                    e = port.ifft_stream(m[v, :used], ph[v, :used], fs, hop, win)[0][:n]
                    tol = 4e-7 * m[v].sum(axis=1).max() / fs * (fs // hop)
                    assert np.abs(out[:, v] - e).max() <= tol and np.abs(e).max() > 100 * tol, (calls, v)


@pytest.mark.parametrize("zero_phase", [True, False])
@pytest.mark.parametrize("fs,hop", [(64, 16), (1024, 256)])
def test_chain_fft_bank_to_ifft_bank(mx, port, fs, hop, zero_phase):
    """ffttest.cpp over 65 streams: maxiFFTBank -> the magnitudes moved up three bins by a torch op on the device rows -> maxiIFFTBank
    in after-FFT mode, across an unaligned split.  Judged in two steps: the FFT rows against the oracle (as above), then the IFFT
    output against the oracle fed THE DEVICE'S OWN rows in the order the held-first rule names -- bit for bit with zeroed phases,
    within the random-phase bound with the real ones."""
    import torch
    V, bins, L = 65, fs // 2, mx.lib()
    x = block(V)[:, :].copy()
    x[~np.isfinite(x)] = 0.25                                        # a finite block: the chain's second step compares sums
    calls = [100, 411, 1, 0, hop, 2 * hop - 1, NTOT - 512 - 3 * hop + 1]
    assert sum(calls) == NTOT
    dev = torch.device("cuda")
    fb, ib = mx.maxiFFTBank(V, fs, hop), mx.maxiIFFTBank(V, fs, hop)
    rows_m, rows_p, outs, off = [], [], [], 0
    for N in calls:
        F = fb.frames(N)
        assert ib.rows(N, ib.AFTER_FFT) == F
        dx = torch.from_numpy(np.ascontiguousarray(x[off:off + N])).to(dev)
        mbuf = torch.empty((max(F * V, 1), bins), dtype=torch.float32, device=dev)   # (a call without a frame still names its outputs)
        pbuf = torch.empty((max(F * V, 1), bins), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        mx._lib.check(L.mxg_fft_bank_process(fb.h, dx.data_ptr(), N, 0, None, None, mbuf.data_ptr(), pbuf.data_ptr(), None), "fft bank")
        mx._lib.check(L.mxg_sync(), "mxg_sync")
        mags, phases = mbuf[:F * V], pbuf[:F * V]
        raw_p = phases.cpu().numpy().reshape(F, V, bins)
        moved = torch.roll(mags, 3, dims=1)
        moved[:, :3] = 0
        if zero_phase:
            phases.zero_()
        torch.cuda.synchronize()
        out = ib.process(moved, phases, N, rows=ib.AFTER_FFT, layout=0).numpy()
        outs.append(out)
        rows_m.append(moved.cpu().numpy().reshape(F, V, bins))
        rows_p.append(phases.cpu().numpy().reshape(F, V, bins))
        raw = mags.cpu().numpy().reshape(F, V, bins)
        e = fft_expected_finite(port, V, fs, hop, x)
        f0 = sum(r.shape[0] for r in rows_m) - F
        assert same_f32(raw.transpose(1, 0, 2), e["mags"][:, f0:f0 + F]), ("fft rows", N)
        assert phase_close(raw_p.transpose(1, 0, 2), e["phases"][:, f0:f0 + F]), ("fft rows, phases", N)
        off += N
    out = np.concatenate(outs, axis=0)
    M, P = np.concatenate(rows_m, axis=0), np.concatenate(rows_p, axis=0)          # [frames][V][bins]
    C = -(-NTOT // hop)
    zero = np.zeros((1, bins), np.float32)
    for v in range(V):
        seq_m = np.concatenate([zero, M[:C - 1, v]])                               # point k takes frame k - 1; point 0 the zeros of setup
        seq_p = np.concatenate([zero, P[:C - 1, v]])
        e = port.ifft_stream(seq_m, seq_p, fs, hop, 0)[0][:NTOT].astype(np.float64)
        if zero_phase:
            assert same_f64(out[:, v], e), v
        else:
            tol = 4e-7 * seq_m.sum(axis=1).max() / fs * (fs // hop)
            assert np.abs(out[:, v] - e).max() <= tol and np.abs(e).max() > 100 * tol, v


_finite_cache = {}


def fft_expected_finite(port, V, fs, hop, x):
    key = (V, fs, hop)
    if key not in _finite_cache:
        per = [port.fft_stream(x[:, v].astype(np.float32), fs, hop, 0, want=("mags", "phases")) for v in range(V)]
        _finite_cache[key] = {k: np.stack([p[k] for p in per]) for k in ("mags", "phases")}
    return _finite_cache[key]


def test_fft_bank_rows_into_mfcc_mirror(mx):
    """Composition: the bank's frame-major magnitudes go straight into maxiMFCC.mfcc; the result is the bits the mirror gives on
    the per-stream mxg_fft_batch magnitudes laid out the same way."""
    V, fs, hop = 65, 1024, 256
    x = block(V).copy()
    x[~np.isfinite(x)] = 0.25
    F = NTOT // hop
    bank = mx.maxiFFTBank(V, fs, hop)
    mags = bank.process(x, want=("mags",))["mags"]
    mf = mx.maxiMFCC()
    mf.setup(fs // 2, 42, 13, 20.0, 20000.0)
    got = mf.mfcc(mags).numpy()
    per = []
    for v in range(V):
        f = mx.maxiFFT()
        f.setup(fs, hop, 0)
        assert f.process_signal(x[:, v].astype(np.float32)) == F
        per.append(f.getMagnitudes().numpy())
    single = np.ascontiguousarray(np.stack(per).transpose(1, 0, 2).reshape(F * V, fs // 2))
    assert same_f32(mags.numpy(), single)
    exp = mf.mfcc(mx.DeviceBuffer.from_numpy(single)).numpy()
    assert got.shape == (F * V, 13) and same_f64(got, exp)


def kernels_launched(mx, fn):
    L = mx.lib()
    prev = L.mxg_prof_enable(1)
    try:
        L.mxg_prof_reset()
        fn()
        L.mxg_sync()
        total = 0
        for i in range(L.mxg_prof_count()):
            label, ms, n = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_size_t()
            assert L.mxg_prof_read(i, ctypes.byref(label), ctypes.byref(ms), ctypes.byref(n)) == 0
            total += n.value
        return total
    finally:
        L.mxg_prof_enable(prev)
        L.mxg_prof_reset()


def test_launch_count_does_not_depend_on_V(mx):
    counts = {}
    for V in (3, 130):
        x = mx.DeviceBuffer.from_numpy(block(V)[:777])
        fb, ib = mx.maxiFFTBank(V, 64, 16), mx.maxiIFFTBank(V, 64, 16)
        fb.process(x, N=5, want=("mags",))                                                  # both banks now stand inside a hop
        ib.process(np.zeros((V, 64 // 2), np.float32), np.zeros((V, 64 // 2), np.float32), 5)
        F = fb.frames(772)
        rows = {}
        nf = kernels_launched(mx, lambda: rows.update(fb.process(mx.DeviceBuffer.from_numpy(block(V)[5:777]), N=772)))
        ni = kernels_launched(mx, lambda: ib.process(rows["mags"], rows["phases"], 772, rows=ib.AFTER_FFT))
        assert F == 48 and rows["mags"].shape[0] == V * F
        counts[V] = (nf, ni)
    assert counts[3] == counts[130] == (2, 2), counts


def test_process_refuses_null_pointers_on_a_live_bank(mx):
    """Each refusal names the argument, launches nothing and leaves the bank where it stood."""
    L = mx.lib()
    V, fs, hop, bins = 3, 64, 16, 32
    fb, ib = mx.maxiFFTBank(V, fs, hop), mx.maxiIFFTBank(V, fs, hop)
    x = mx.DeviceBuffer.from_numpy(block(V)[:40])
    o = mx.DeviceBuffer((V * 2, bins), np.float32)
    y = mx.DeviceBuffer((40, V), np.float64)
    rows = mx.DeviceBuffer((V * 3, bins), np.float32)

    def refused(status, fn, word):
        msg = L.mxg_last_error().decode()
        assert status < 0 and fn in msg and word in msg, (status, msg)

    refused(L.mxg_fft_bank_process(fb.h, None, 40, 0, None, None, o.ptr, None, None), "mxg_fft_bank_process", "d_in")
    refused(L.mxg_fft_bank_process(fb.h, x.ptr, 40, 0, None, None, None, None, None), "mxg_fft_bank_process", "d_mags")
    refused(L.mxg_fft_bank_process(fb.h, x.ptr, 40, 2, None, None, o.ptr, None, None), "mxg_fft_bank_process", "layout")
    assert L.mxg_fft_bank_process(fb.h, None, 0, 0, None, None, o.ptr, None, None) == 0        # N = 0 does nothing
    assert fb.pos == 0 and fb.frames(40) == 2
    assert ib.rows(40) == 3
    refused(L.mxg_ifft_bank_process(ib.h, 0, 0, 0, rows.ptr, rows.ptr, 3, 40, None, None), "mxg_ifft_bank_process", "d_out")
    refused(L.mxg_ifft_bank_process(ib.h, 0, 0, 0, None, rows.ptr, 3, 40, y.ptr, None), "mxg_ifft_bank_process", "d_a")
    refused(L.mxg_ifft_bank_process(ib.h, 0, 0, 0, rows.ptr, None, 3, 40, y.ptr, None), "mxg_ifft_bank_process", "d_b")
    refused(L.mxg_ifft_bank_process(ib.h, 0, 0, 0, rows.ptr, rows.ptr, 2, 40, y.ptr, None), "mxg_ifft_bank_process", "nrows = 2")
    refused(L.mxg_ifft_bank_process(ib.h, 2, 0, 0, rows.ptr, rows.ptr, 3, 40, y.ptr, None), "mxg_ifft_bank_process", "input")
    refused(L.mxg_ifft_bank_process(ib.h, 0, 2, 0, rows.ptr, rows.ptr, 3, 40, y.ptr, None), "mxg_ifft_bank_process", "row_mode")
    assert ib.pos == 0
    mx._lib.check(L.mxg_fft_bank_process(fb.h, x.ptr, 40, 0, None, None, o.ptr, None, None), "fft bank")   # both still work
    mx._lib.check(L.mxg_ifft_bank_process(ib.h, 0, 0, 0, rows.ptr, rows.ptr, 3, 40, y.ptr, None), "ifft bank")
    assert fb.pos == 8 and ib.pos == 8 and not y.numpy().any()
