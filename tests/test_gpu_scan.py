"""GPU (-m gpu): the TIME-PARALLEL tolerance mode for small banks of linear filters (knob "time_parallel", csrc/scan.hip): a
wavefront takes one voice, its 64 lanes take consecutive time segments, the segment states are joined by a Kogge-Stone scan over
wavefront shuffles (north_star: "wavefront shuffles for the biquad recurrence").  The arithmetic is reordered, so the mode is not
bit-exact: stated tolerance |error| <= SCAN_RTOL (1e-10) x the voice's peak over the carried blocks, against the oracle's sequential
recurrence, for stable settings and finite input over the whole domain the classes accept.  With the knob off (the default) the
same calls are bit-exact -- asserted here too, so the knob cannot leak.  The scan's arithmetic (csrc/mxg_scan.h) is + - * in a fixed
order with contraction off, so the device is also held to the 64-lane host build of that header (tests/host_scan.cpp) BIT FOR BIT:
a differing bit is a bug, whatever the tolerance says."""
import numpy as np
import pytest

import scan_host as sh
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SCAN_RTOL = 1e-10  # x per-voice peak of |reference output| (measured, host build = device bits: <= 6.3e-11, a 10 Hz biquad over 2048-sample blocks; <= 8e-14 for the other kinds)


def _scaled_err(got, exp):
    peak = np.maximum(np.abs(exp).max(axis=0), 1e-300)
    return float((np.abs(got - exp) / peak).max())


@pytest.fixture
def scan_on(mx):
    prev = mx.lib().mxg_tune(b"time_parallel", 1)
    yield
    mx.lib().mxg_tune(b"time_parallel", prev)


@pytest.mark.parametrize("V,N", [(1, 64), (6, 512), (70, 2048), (6, 128), (3, 1024)])
@pytest.mark.parametrize("kind", ["dc", "svf", "biquad"])
def test_filter2_time_parallel_within_tolerance(mx, port, scan_on, kind, V, N):
    rng = np.random.default_rng(V * 1000 + N)
    blocks = 3
    x = rng.uniform(-1, 1, (blocks * N, V))
    v = np.arange(V)
    if kind == "dc":
        R = 0.99 + 0.009 * rng.uniform(0, 1, V)
        bank = mx.maxiDCBlockerBank(V)
        run = lambda xb: bank.play(mx.DeviceBuffer.from_numpy(xb), R).numpy()
        exp, est, _ = port.filter2(0, x, R[None, :])
    elif kind == "svf":
        cut, q = 80.0 + 900.0 * rng.uniform(0, 1, V), 0.5 + 4.0 * rng.uniform(0, 1, V)
        bank = mx.maxiSVFBank(V)
        bank.setCutoff(cut); bank.setResonance(q)
        run = lambda xb: bank.play(mx.DeviceBuffer.from_numpy(xb), 0.5, 0.25, 0.125, 0.6).numpy()
        exp, est, _ = port.filter2(1, x, np.stack([cut, q, np.full(V, 0.5), np.full(V, 0.25), np.full(V, 0.125), np.full(V, 0.6)]))
    else:
        typ = (v % 7).astype(np.float64)
        cut, q, gain = 100.0 + 3000.0 * rng.uniform(0, 1, V), 0.4 + 3.0 * rng.uniform(0, 1, V), -9.0 + 18.0 * rng.uniform(0, 1, V)
        bank = mx.maxiBiquadBank(V)
        bank.set(typ.astype(np.int32), cut, q, gain)
        run = lambda xb: bank.play(mx.DeviceBuffer.from_numpy(xb)).numpy()
        exp, est, _ = port.filter2(2, x, np.stack([typ, cut, q, gain]))
    got = np.concatenate([run(x[b * N:(b + 1) * N]) for b in range(blocks)])   # state carried from block to block
    err = _scaled_err(got, exp)
    print("%s V=%d N=%d: max |err| / peak = %.3e (tolerance %.0e)" % (kind, V, N, err, SCAN_RTOL))
    assert err <= SCAN_RTOL
    assert np.abs(bank.state.numpy()[:est.shape[0]] - est).max() <= SCAN_RTOL * max(1.0, np.abs(est).max())


@pytest.mark.parametrize("kind", ["lores", "hires"])
@pytest.mark.parametrize("V,N", [(6, 512), (33, 256)])
def test_lores_time_parallel_within_tolerance(mx, port, scan_on, kind, V, N):
    rng = np.random.default_rng(V + N)
    x = rng.uniform(-1, 1, (3 * N, V))
    cut, res = 200.0 + 5000.0 * rng.uniform(0, 1, V), 1.0 + 12.0 * rng.uniform(0, 1, V)
    bank = mx.maxiFilterBank(V)
    got = np.concatenate([bank.render(kind, mx.DeviceBuffer.from_numpy(x[b * N:(b + 1) * N]), cut, res).numpy() for b in range(3)])
    exp, est = port.filter(0 if kind == "lores" else 1, x, cut, res)
    err = _scaled_err(got, exp)
    print("%s V=%d N=%d: max |err| / peak = %.3e" % (kind, V, N, err))
    assert err <= SCAN_RTOL
    st = bank.state.numpy()
    serr = sh.state_err(port, kind, np.stack([cut, res]), st[:2], est[:2], exp).max()
    print("    final state (x, y), continued from it: max |err| / peak = %.3e" % serr)
    assert serr <= SCAN_RTOL
    assert_bits_equal(st[2:], est[2:], "outputs[0..2]: not lores's / hires's to touch")


def test_knob_off_is_bit_exact_and_odd_shapes_fall_back(mx, port):
    """Default knob: the exact kernels.  With the knob on, shapes the scan does not take (N not a multiple of 64) still go through the
    exact kernels and stay bit-exact."""
    rng = np.random.default_rng(7)
    V, N = 6, 512
    x = rng.uniform(-1, 1, (N, V))
    typ, cut, q, gain = np.zeros(V), np.full(V, 1200.0), np.full(V, 0.7), np.zeros(V)
    exp, _, _ = port.filter2(2, x, np.stack([typ, cut, q, gain]))
    bank = mx.maxiBiquadBank(V)
    bank.set(typ.astype(np.int32), cut, q, gain)
    assert_bits_equal(bank.play(mx.DeviceBuffer.from_numpy(x)).numpy(), exp, "knob off")
    prev = mx.lib().mxg_tune(b"time_parallel", 1)
    try:
        bank = mx.maxiBiquadBank(V)
        bank.set(typ.astype(np.int32), cut, q, gain)
        assert_bits_equal(bank.play(mx.DeviceBuffer.from_numpy(x[:500])).numpy(), exp[:500], "N = 500 falls back to the exact kernel")
    finally:
        mx.lib().mxg_tune(b"time_parallel", prev)


# ---- the device against the host build of mxg_scan.h, and the scan over its whole domain -----------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("scan"))


class _knob:
    def __init__(self, mx, value):
        self.mx, self.value = mx, value

    def __enter__(self):
        self.prev = self.mx.lib().mxg_tune(b"time_parallel", self.value)

    def __exit__(self, *a):
        self.mx.lib().mxg_tune(b"time_parallel", self.prev)


class _Dev:
    """A bank of `kind` on the device set from parameter rows par [P][V] (tests/scan_host.py), from the state st0 [rows][V] (the
    bank's remaining rows zero, or `full` = all its rows).  run(x) plays one block, state() downloads every row."""

    def __init__(self, mx, kind, par, st0=None, full=None):
        self.mx, self.kind, self.par = mx, kind, np.ascontiguousarray(par, np.float64)
        V = self.par.shape[1]
        if kind == "dc":
            self.bank = mx.maxiDCBlockerBank(V)
            self.coef = self.par[:1].copy()
        elif kind == "svf":
            self.bank = mx.maxiSVFBank(V)
            self.bank.setCutoff(self.par[0]); self.bank.setResonance(self.par[1])
            self.coef = np.concatenate([self.bank.coefficients(), self.par[2:6]])
        elif kind == "biquad":
            self.bank = mx.maxiBiquadBank(V)
            self.bank.set(self.par[0].astype(np.int32), self.par[1], self.par[2], self.par[3])
            self.coef = self.bank.host_coef
        else:
            from maximilian_amd.banks import filter_coeffs
            self.bank = mx.maxiFilterBank(V)
            self.coef = np.ascontiguousarray(filter_coeffs(0, self.par[0], self.par[1])[:2])
        st = np.zeros(self.bank.state.shape) if full is None else np.array(full, np.float64)
        if st0 is not None:
            st[:st0.shape[0]] = st0
        self.bank.state.upload(st)

    def run(self, x, kind=None, **kw):
        xb = self.mx.DeviceBuffer.from_numpy(np.ascontiguousarray(x))
        if self.kind == "dc":
            return self.bank.play(xb, self.par[0]).numpy()
        if self.kind == "svf":
            return self.bank.play(xb, *self.par[2:6]).numpy()
        if self.kind == "biquad":
            return self.bank.play(xb).numpy()
        return self.bank.render(kind or self.kind, xb, self.par[0], self.par[1], **kw).numpy()

    def stream(self, x, sizes):
        out, at = [], 0
        for n in sizes:
            out.append(self.run(x[at:at + n]))
            at += n
        assert at == x.shape[0]
        return np.concatenate(out)

    def state(self):
        return self.bank.state.numpy()


def _box(kind, V, rng):
    """The ordinary settings of the tolerance tests above, as parameter rows."""
    u = lambda: rng.uniform(0, 1, V)
    if kind == "dc":
        return (0.99 + 0.009 * u())[None, :]
    if kind == "svf":
        return np.stack([80.0 + 900.0 * u(), 0.5 + 4.0 * u()] + [np.full(V, m) for m in sh.SVF_MIX])
    if kind == "biquad":
        return np.stack([(np.arange(V) % 7).astype(np.float64), 100.0 + 3000.0 * u(), 0.4 + 3.0 * u(), -9.0 + 18.0 * u()])
    return np.stack([200.0 + 5000.0 * u(), 1.0 + 12.0 * u()])


@pytest.mark.parametrize("L", sh.ALL_L)
@pytest.mark.parametrize("kind", sh.KINDS)
def test_device_equals_host_model_bit_for_bit(mx, host, scan_on, kind, L):
    """The scan's reordered arithmetic is still + - * in a fixed order with contraction off: the wavefront must give the bits of the
    64-lane host build of the same header.  A wrong shuffle distance, `lane >= d` guard, squaring count or state row differs here
    however benign the settings."""
    N = 64 * L
    full = sh.sweep_params(kind)
    for V in (1, 3, 70):
        rng = np.random.default_rng(1000 * L + V)
        par = np.ascontiguousarray(full[:, rng.choice(full.shape[1], V, replace=V > full.shape[1])])
        x = rng.uniform(-1, 1, (2 * N, V))
        dev = _Dev(mx, kind, par, full=rng.uniform(-1, 1, (5 if kind in ("lores", "hires") else 3, V)))
        st0 = dev.state()
        got = dev.stream(x, [N, N])
        exp, est = sh.host_scan(host, kind, x, dev.coef, st0[:sh.NSTATE[kind]], 2)
        what = "%s L=%d V=%d" % (kind, L, V)
        assert_bits_equal(got, exp, what + ": output")
        st = dev.state()
        assert_bits_equal(st[:sh.NSTATE[kind]], est, what + ": carried state")
        assert_bits_equal(st[sh.NSTATE[kind]:], st0[sh.NSTATE[kind]:], what + ": rows the scan does not own")


@pytest.mark.parametrize("N", [2048, 512])
@pytest.mark.parametrize("kind", sh.KINDS)
def test_full_domain_on_device(mx, port, host, scan_on, kind, N):
    """The sweep of tests/test_scan_host.py as one bank per kind, one voice per setting: within SCAN_RTOL of the oracle's
    sequential recurrence, three carried blocks from random states -- and the host model's bits."""
    par, x, st0 = sh.sweep_case(kind, N)
    dev = _Dev(mx, kind, par, st0)
    got = dev.stream(x, [N] * 3)
    gst = dev.state()[:sh.NSTATE[kind]]
    exp, est = sh.oracle_seq(port, kind, x, par, st0)
    err = sh.scaled_err(got, exp)
    serr = sh.state_err(port, kind, par, gst, est, exp)
    w = int(err.argmax())
    print("%s N=%d, %d settings: max |err| / peak = %.3e at %s; continued from the final state %.3e (tolerance %.0e)"
          % (kind, N, par.shape[1], err.max(), par[:, w].tolist(), serr.max(), SCAN_RTOL))
    assert err.max() <= SCAN_RTOL and serr.max() <= SCAN_RTOL
    hexp, hst = sh.host_scan(host, kind, x, dev.coef, st0, 3)
    assert_bits_equal(got, hexp, "%s N=%d: output against the host model" % (kind, N))
    assert_bits_equal(gst, hst, "%s N=%d: state against the host model" % (kind, N))


@pytest.mark.parametrize("kind", sh.KINDS)
def test_the_scan_is_still_taken(mx, kind):
    """No voice of the ordinary boxes is rendered by anything but the scan: with the knob on every voice differs from the exact
    kernel's output in at least one bit (a voice that fell back to the sequential step would be bit-identical).  There is no
    per-voice fallback in mxg_scan.h; this keeps it so."""
    V, N = 70, 512
    rng = np.random.default_rng(31)
    par, x = _box(kind, V, rng), rng.uniform(-1, 1, (N, V))
    exact = _Dev(mx, kind, par).run(x)
    with _knob(mx, 1):
        scanned = _Dev(mx, kind, par).run(x)
    same = (scanned.view(np.uint64) == exact.view(np.uint64)).all(axis=0)
    print("%s: %d of %d voices bit-identical to the exact kernel" % (kind, int(same.sum()), V))
    assert not same.any()
    assert sh.scaled_err(scanned, exact).max() <= SCAN_RTOL


def test_dispatch_edge_voices(mx, port):
    """Knob on: 4096 voices are scanned (within tolerance, not the exact bits), 4097 are not (the oracle's bits)."""
    N = 128
    for V in (4096, 4097):
        rng = np.random.default_rng(V)
        par, x = _box("biquad", V, rng), rng.uniform(-1, 1, (N, V))
        exp, est = sh.oracle_seq(port, "biquad", x, par, np.zeros((3, V)))
        with _knob(mx, 1):
            dev = _Dev(mx, "biquad", par)
            got = dev.run(x)
        if V == 4096:
            assert sh.scaled_err(got, exp).max() <= SCAN_RTOL
            assert not np.array_equal(got.view(np.uint64), exp.view(np.uint64)), "V = 4096 is meant to take the scan"
        else:
            assert_bits_equal(got, exp, "V = 4097: the exact kernel")
            assert_bits_equal(dev.state(), est, "V = 4097: state")


@pytest.mark.parametrize("kind", sh.KINDS)
def test_dispatch_edge_block_sizes(mx, port, kind):
    """Knob on: blocks the scan does not take -- 64 x 3, no multiple of 64, 64 x 33, 64 x 64 -- are the exact kernels' bits."""
    V = 6
    with _knob(mx, 1):
        for N in (192, 500, 2112, 4096):
            rng = np.random.default_rng(N)
            par, x, st0 = _box(kind, V, rng), rng.uniform(-1, 1, (N, V)), rng.uniform(-1, 1, (sh.NSTATE[kind], V))
            dev = _Dev(mx, kind, par, st0)
            exp, est = sh.oracle_seq(port, kind, x, par, st0)
            assert_bits_equal(dev.run(x), exp, "%s N=%d" % (kind, N))
            assert_bits_equal(dev.state()[:sh.NSTATE[kind]], est, "%s N=%d: state" % (kind, N))


@pytest.mark.parametrize("which", ["cutoff", "resonance"])
def test_modulated_lores_is_not_scanned(mx, which):
    """Knob on: a per-sample cutoff or resonance keeps the modulated kernel -- the same bits as with the knob off."""
    V, N = 6, 512
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (N, V))
    cut = 300.0 + 2000.0 * rng.uniform(0, 1, (N, V)) if which == "cutoff" else 300.0 + 2000.0 * rng.uniform(0, 1, V)
    res = 1.0 + 8.0 * rng.uniform(0, 1, (N, V)) if which == "resonance" else 1.0 + 8.0 * rng.uniform(0, 1, V)
    kw = dict(cutoff_per_sample=which == "cutoff", res_per_sample=which == "resonance")
    outs, states = [], []
    for knob in (0, 1):
        with _knob(mx, knob):
            bank = mx.maxiFilterBank(V)
            outs.append(bank.render("lores", mx.DeviceBuffer.from_numpy(x), cut, res, **kw).numpy())
            states.append(bank.state.numpy())
    assert_bits_equal(outs[1], outs[0], "per-sample %s: output" % which)
    assert_bits_equal(states[1], states[0], "per-sample %s: state" % which)


MIXED = [512, 500, 64, 7, 2048, 192, 128]  # scanned, exact, scanned, exact, scanned, exact, scanned


@pytest.mark.parametrize("kind", sh.KINDS)
def test_mixed_sequence_on_one_bank(mx, port, scan_on, kind):
    """Scanned and exact kernels alternate on one bank, the state handed from one to the other: the whole stream is within tolerance."""
    V = 6
    rng = np.random.default_rng(17)
    par, x, st0 = _box(kind, V, rng), rng.uniform(-1, 1, (sum(MIXED), V)), rng.uniform(-1, 1, (sh.NSTATE[kind], V))
    dev = _Dev(mx, kind, par, st0)
    got = dev.stream(x, MIXED)
    exp, est = sh.oracle_seq(port, kind, x, par, st0)
    err = sh.scaled_err(got, exp).max()
    serr = sh.state_err(port, kind, par, dev.state()[:sh.NSTATE[kind]], est, exp).max()
    print("%s, blocks %s: max |err| / peak = %.3e, continued from the final state %.3e" % (kind, MIXED, err, serr))
    assert err <= SCAN_RTOL and serr <= SCAN_RTOL


def test_filter_bank_rows_between_scanned_blocks(mx, port, scan_on):
    """maxiFilterBank: lopass / hipass (outputs[0], state row 2) and bandpass (outputs[1..2], rows 3-4) blocks between scanned lores
    blocks.  A scanned block leaves rows 2-4 bit-identical; the exact blocks are fed what lores just produced, so from the device's
    own input and rows they are the oracle's bits, and against the oracle's own chain they differ only by what lores handed them."""
    V = 6
    rng = np.random.default_rng(23)
    par = _box("lores", V, rng)
    dev = _Dev(mx, "lores", par, full=rng.uniform(-1, 1, (5, V)))
    ost = dev.state()                                     # the oracle's chain
    kinds = {"lores": 0, "bandpass": 2, "lopass": 3, "hipass": 4}
    y_dev = y_or = None
    for kind, n in [("lores", 512), ("lopass", 512), ("lores", 256), ("hipass", 100), ("lores", 128), ("bandpass", 128), ("lores", 1024),
                    ("lopass", 64)]:
        before = dev.state()
        if kind == "lores":
            xin_dev = xin_or = rng.uniform(-1, 1, (n, V))
        else:
            xin_dev, xin_or = np.ascontiguousarray(y_dev[:n]), np.ascontiguousarray(y_or[:n])
        cut = par[0] if kind in ("lores", "bandpass") else np.full(V, 0.25)
        res = par[1] if kind == "lores" else (np.full(V, 0.6) if kind == "bandpass" else None)
        xb = mx.DeviceBuffer.from_numpy(xin_dev)
        got = dev.bank.render(kind, xb, cut, res).numpy()
        after = dev.state()
        exp, ost = port.filter(kinds[kind], xin_or, cut, res, state=ost)
        what = "%s block of %d" % (kind, n)
        if kind == "lores":
            assert_bits_equal(after[2:], before[2:], what + ": rows 2-4 across a scanned block")
            y_dev, y_or = got, exp
        else:
            same, sst = port.filter(kinds[kind], xin_dev, cut, res, state=before)
            assert_bits_equal(got, same, what + ": the exact kernel from the device's own input and rows")
            assert_bits_equal(after, sst, what + ": its state")
        assert sh.scaled_err(got, exp, peak_of=np.concatenate([exp, y_or])).max() <= SCAN_RTOL, what


# ---- non-finite samples, unstable settings: the voice itself follows the host model, its neighbours do not notice -----------------
@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("setting", range(len(sh.NONFINITE_SETTINGS)), ids=["%s%d" % (k, i) for i, (k, _) in enumerate(sh.NONFINITE_SETTINGS)])
def test_nonfinite_sample_and_its_neighbours(mx, host, scan_on, setting, L):
    kind, p = sh.NONFINITE_SETTINGS[setting]
    V, N, bad_v = 31, 64 * L, 13
    rng = np.random.default_rng(setting * 10 + L)
    par = np.tile(np.array(p, np.float64)[:, None], (1, V))
    clean = rng.uniform(-1, 1, (2 * N, V))
    st0 = rng.uniform(-1, 1, (sh.NSTATE[kind], V))
    ref = _Dev(mx, kind, par, st0)
    good, good_st = ref.stream(clean, [N, N]), ref.state()
    keep = np.arange(V) != bad_v
    for name, value in sh.BAD_SAMPLES:
        for at in sorted({N // 2 + 3 * L // 8, N // 2 + L - 1, N - 1}):
            x = clean.copy()
            x[at, bad_v] = value
            dev = _Dev(mx, kind, par, st0)
            got, st = dev.stream(x, [N, N]), dev.state()
            exp, est = sh.host_scan(host, kind, x, dev.coef, st0, 2)
            what = "%s %s at %d, L=%d" % (kind, name, at, L)
            assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(np.isfinite(got), np.isfinite(exp)), what + ": masks"
            assert_bits_equal(got, exp, what + ": output against the host model")
            assert_bits_equal(st[:sh.NSTATE[kind]], est, what + ": state against the host model")
            assert not np.isfinite(got[at:, bad_v]).all(), what
            assert_bits_equal(got[:, keep], good[:, keep], what + ": the other voices")
            assert_bits_equal(st[:, keep], good_st[:, keep], what + ": the other voices' states")


@pytest.mark.parametrize("kind", ["lores", "hires"])
def test_unstable_voice_and_its_neighbours(mx, host, scan_on, kind):
    """10 kHz with res = 1 diverges in the reference too; the bound does not cover that voice.  It follows the host model bit for
    bit and no other voice notices."""
    V, N, bad_v = 31, 512, 13
    rng = np.random.default_rng(41)
    par = _box(kind, V, rng)
    par_bad = par.copy()
    par_bad[:, bad_v] = [10000.0, 1.0]
    x, st0 = rng.uniform(-1, 1, (2 * N, V)), rng.uniform(-1, 1, (2, V))
    ref, dev = _Dev(mx, kind, par, st0), _Dev(mx, kind, par_bad, st0)
    good, got = ref.stream(x, [N, N]), dev.stream(x, [N, N])
    exp, est = sh.host_scan(host, kind, x, dev.coef, st0, 2)
    assert np.abs(exp[:, bad_v]).max() > 1e100 or not np.isfinite(exp[:, bad_v]).all(), "the setting is meant to diverge"
    assert_bits_equal(got, exp, kind + ": output against the host model")
    assert_bits_equal(dev.state()[:2], est, kind + ": state against the host model")
    keep = np.arange(V) != bad_v
    assert_bits_equal(got[:, keep], good[:, keep], kind + ": the other voices")
    assert_bits_equal(dev.state()[:, keep], ref.state()[:, keep], kind + ": the other voices' states")
