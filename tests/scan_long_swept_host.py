"""Helpers of the swept long scan's tests (tests/test_scan_long_swept_host.py, tests/test_gpu_scan_long_swept.py; K31,
mxg_scan_long_render_swept): the sweep set, the sequential yardsticks (the oracle's filter(..., cps=True, rps=True) for lores /
hires, the library's bit-exact mxg_lag_host with alpha_per_sample = 1 for the lag), the long-double recurrences
(tests/host_scan_long_swept.cpp), the per-kind bounds and the host twin mxg_scan_long_swept_host as a renderer with carried state.

A `kind` is one of KINDS.  A case's parameters are par = (cutoff, res) or (alpha, alphaReciprocal), each [N][V], one voice per
setting of the sweep set; coef_ps() turns them into the [N][rows][V] array the entry points take."""
import ctypes
import os
import subprocess

import numpy as np

import scan_host as sh
from conftest import HOST_OPT, ROOT

KINDS = ["lores", "hires", "lag"]
KIND_ID = {"lores": 3, "hires": 4, "lag": 5}
NSTATE = {"lores": 2, "hires": 2, "lag": 1}   # state rows the scan reads and writes
NROWS = {"lores": 5, "hires": 5, "lag": 1}    # state rows of the sequential entry point's array
TS = 1024                                     # the swept chunk length
RAGGED = 3 * TS + 5 * 64 + 7                  # three chunks, blocks of 256 and 64, seven plain steps
SR = 44100.0
# chunks per call: a chunk boundary; phase B with runs of two chunks per lane and its Kogge-Stone; the ragged N; a long stream
SWEEP_N = {"2": 2 * TS, "66": 66 * TS, "ragged": RAGGED, "4097": 4097 * TS}

# The bound per kind, x the voice's peak of the sequential output, for a stream of up to 3 x 4097 chunks (1.26e7 samples) carried
# from a state: the worst |twin - sequential| / peak over the sweep set below at 2, 66 and 4097 chunks and the ragged N, and over
# const_case's settings (coefficients that stand still, the constant long scan's whole domain) at 66 and 4097 chunks, three carried
# calls, on this module's streams and on other noise (tools/measure_longsweep_tolerance.py, profiles/longsweep_tolerance.json) -- x 2,
# rounded up to one significant digit.  tests/test_scan_long_swept_host.py's docstring has the figures.
SWEPT_RTOL = {"lores": 6e-12, "hires": 6e-12, "lag": 5e-12}


def lib():
    import maximilian_amd
    return maximilian_amd.lib()


def build(tmp):
    """tests/host_scan_long_swept.cpp: the swept recurrences in long double."""
    so = str(tmp / "libscan_long_swept_host.so")
    subprocess.check_call(["g++", "-std=c++17"] + HOST_OPT + ["-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "host_scan_long_swept.cpp")])
    L = ctypes.CDLL(so)
    L.scan_long_swept_ld.restype = ctypes.c_int
    L.scan_long_swept_ld.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.c_void_p, ctypes.c_void_p]
    return L


# ---- the sweep set ---------------------------------------------------------------------------------------------------------------
def _lfo(n, hz, lo, hi, phase=0.0):
    return lo + (hi - lo) * (0.5 + 0.5 * np.sin(2.0 * np.pi * hz * n / SR + phase))


CUTOFFS = ["slow-lfo", "audio-lfo", "ramp", "low-lfo", "steps"]   # all inside 10 Hz ... 8 kHz
RESONANCES = ["res1", "res30", "res1000", "res-lfo"]
ALPHAS = ["log-sweep", "walk", "steps"]
RECIPS = ["one-minus", "independent"]
# A cutoff that jumps to a random value in 10 Hz ... 8 kHz every 37 samples pumps a high-Q resonator: at resonance 1000 and under the
# resonance LFO (up to 100) the reference's own float64 recurrence leaves the condition below (peak <= 1e6) -- peaks of 5e9 ... 3e33
# after 2 chunks x 3 calls, overflow to NaN at 66 (lores and hires alike; at resonance 30 the peak stays near 1e5).  These two are
# therefore not in the set; the stepped cutoff runs at resonance 1 and 30.  tests/test_scan_long_swept_host.py checks that they do diverge.
DIVERGING = ["steps/res1000", "steps/res-lfo"]


def settings(kind):
    """The names of the sweep set's settings, one voice each."""
    if kind == "lag":
        return ["%s/%s" % (a, r) for a in ALPHAS for r in RECIPS]
    return [s for s in ("%s/%s" % (c, r) for c in CUTOFFS for r in RESONANCES) if s not in DIVERGING]


def barely_damped(kind):
    """The settings the 4097-chunk case runs: res 1000 at the low LFO; alpha near 1e-6."""
    return ["log-sweep/one-minus", "steps/one-minus"] if kind == "lag" else ["low-lfo/res1000"]


def _cutoff(name, N, calls, rng):
    n = np.arange(calls * N, dtype=np.float64)
    if name == "slow-lfo":
        return _lfo(n, 2.0, 200.0, 8000.0)
    if name == "audio-lfo":
        return _lfo(n, 200.0, 100.0, 8000.0)
    if name == "ramp":                                  # 10 Hz -> 8 kHz over every call
        return np.tile(np.linspace(10.0, 8000.0, N), calls)
    if name == "low-lfo":
        return _lfo(n, 2.0, 10.0, 60.0)                # (at 2 Hz; a 5 Hz LFO over 10 ... 60 Hz pumps res 1000 without bound: 4e46 after 1.26e7 samples)
    hold = rng.uniform(10.0, 8000.0, (calls * N + 36) // 37)   # a new value every 37 samples
    return np.repeat(hold, 37)[:calls * N]


def _res(name, N, calls):
    if name == "res-lfo":
        return _lfo(np.arange(calls * N, dtype=np.float64), 3.0, 1.0, 100.0)
    return np.full(calls * N, float(name[3:]))


def _alpha(name, N, calls, rng):
    NN = calls * N
    if name == "log-sweep":                             # 1e-6 ... 1 over every call
        return np.tile(np.exp(np.linspace(np.log(1e-6), 0.0, N)), calls)
    if name == "walk":                                  # a random walk reflected into [0, 1]
        w = np.cumsum(rng.normal(0.0, 0.01, NN)) + 0.5
        w = np.abs(np.mod(w, 2.0))
        return np.where(w > 1.0, 2.0 - w, w)
    return np.where((np.arange(NN) // 53) % 2 == 0, 1e-6, 1.0)   # stepping between 1e-6 and 1 every 53 samples


def sweep_case(kind, N, calls=3, seed=2031, only=None):
    """(names, par, x [calls * N][V] uniform noise in [-1, 1], st0 [NSTATE][V] random and non-zero); par = two arrays [calls * N][V].
    only: a list of setting names instead of the whole set."""
    names = settings(kind) if only is None else list(only)
    rng = np.random.default_rng(seed * 7 + KIND_ID[kind] * 100003 + N)
    NN, V = calls * N, len(names)
    a, b = np.empty((NN, V)), np.empty((NN, V))
    for v, name in enumerate(names):
        first, second = name.split("/")
        if kind == "lag":
            a[:, v] = _alpha(first, N, calls, rng)
            b[:, v] = 1.0 - a[:, v] if second == "one-minus" else _lfo(np.arange(NN, dtype=np.float64), 7.0, 0.5, 0.999)
        else:
            a[:, v] = _cutoff(first, N, calls, rng)
            b[:, v] = _res(second, N, calls)
    x = rng.uniform(-1, 1, (NN, V))
    st0 = rng.uniform(-1, 1, (NSTATE[kind], V))
    st0[np.abs(st0) < 1e-3] = 0.5
    return names, (a, b), x, st0


def const_case(kind, N, calls=3, seed=2031, long=False):
    """sweep_case's shape for coefficients that do NOT move: the full-domain settings of the constant long scan (tests/scan_long_host.py's
    sweep_params: 10 Hz ... 8 kHz x res 1 ... 1000, alpha 1e-6 ... 1; long: its long_params, the barely-damped ones and three more), held
    for the whole stream.  The bound covers them too: a sweep may well stand still."""
    import scan_long_host as sl
    p = sl.long_params(kind) if long else sl.sweep_params(kind)
    names = ["const " + "/".join("%g" % v for v in p[:, i]) for i in range(p.shape[1])]
    NN, V = calls * N, p.shape[1]
    a = np.ascontiguousarray(np.broadcast_to(p[0], (NN, V)))
    b = 1.0 - a if kind == "lag" else np.ascontiguousarray(np.broadcast_to(p[1], (NN, V)))
    rng = np.random.default_rng(seed * 11 + KIND_ID[kind] * 100003 + N)
    x = rng.uniform(-1, 1, (NN, V))
    st0 = rng.uniform(-1, 1, (NSTATE[kind], V))
    st0[np.abs(st0) < 1e-3] = 0.5
    return names, (a, b), x, st0


def coef_ps(kind, par, rows=None):
    """[N][rows][V]: sweep_lores / sweep_hires give rows = 3 (mxg_filter_render_coefs' array), sweep_lag rows = 2; another `rows`
    (>= 2) repacks rows 0-1 and fills the others with a value nobody may read."""
    import maximilian_amd as mx
    c = mx.sweep_lag(par[0], par[1]) if kind == "lag" else (mx.sweep_lores if kind == "lores" else mx.sweep_hires)(par[0], par[1])
    if rows is None or rows == c.shape[1]:
        return c
    out = np.full((c.shape[0], rows, c.shape[2]), np.nan)
    out[:, :2] = c[:, :2]
    return np.ascontiguousarray(out)


# ---- the sequential yardsticks -----------------------------------------------------------------------------------------------------
def oracle_seq(port, kind, x, par, st0):
    """The sequential per-sample recurrence over the whole stream: (out, final state [NSTATE][V])."""
    x = np.ascontiguousarray(x, np.float64)
    N, V = x.shape
    if kind == "lag":
        a, r = np.ascontiguousarray(par[0], np.float64), np.ascontiguousarray(par[1], np.float64)
        val, out = np.ascontiguousarray(st0[0], np.float64).copy(), np.empty_like(x)
        assert lib().mxg_lag_host(V, N, x.ctypes.data, a.ctypes.data, r.ctypes.data, 1, val.ctypes.data, out.ctypes.data) == 0
        return out, val[None, :].copy()
    st = np.zeros((5, V))
    st[:2] = st0
    out, st = port.filter(0 if kind == "lores" else 1, x, par[0], par[1], state=st, cps=True, rps=True)
    return out, st[:2].copy()


def assert_stable(exp, names, what):
    """The condition on the sweep set: the float64 sequential output of every setting is finite with peak <= 1e6."""
    peak = np.abs(exp).max(axis=0)
    bad = [names[v] for v in range(len(names)) if not (np.isfinite(exp[:, v]).all() and peak[v] <= 1e6)]
    assert not bad, "%s: settings outside the stable set: %s" % (what, bad)


def seq_long_double(L, kind, x, coef, st0):
    """The recurrence in long double over the whole stream, from the same float64 coefficients: (out, final state)."""
    x, coef = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(coef, np.float64)
    st, out = np.ascontiguousarray(st0, np.float64).copy(), np.empty_like(x)
    assert L.scan_long_swept_ld(KIND_ID[kind], x.shape[1], x.shape[0], x.ctypes.data, coef.ctypes.data, coef.shape[1], st.ctypes.data, out.ctypes.data) == 0
    return out, st


def state_err(port, kind, par, got_st, exp_st, exp_out, n=256):
    """A carried state is worth what the stream does from it (tests/scan_host.py's state_err): the sequential recurrence runs n more
    samples of noise from the state under test and from the sequential recurrence's own, the parameters held at the stream's last."""
    V = exp_out.shape[1]
    x = np.random.default_rng(99).uniform(-1, 1, (n, V))
    hold = tuple(np.repeat(p[-1:], n, axis=0) for p in par)
    a, _ = oracle_seq(port, kind, x, hold, got_st)
    b, _ = oracle_seq(port, kind, x, hold, exp_st)
    return sh.scaled_err(a, b, peak_of=np.concatenate([exp_out, b]))


def full_state(kind, st0, fill=None):
    """The state array of the sequential entry point ([5][V] / [1][V]) holding the scan's rows; the other rows `fill`."""
    st0 = np.asarray(st0, np.float64)
    st = np.zeros((NROWS[kind], st0.shape[1])) if fill is None else np.full((NROWS[kind], st0.shape[1]), fill, np.float64)
    st[:NSTATE[kind]] = st0
    return st


def host_swept(kind, x, coef, st, calls=1, inplace=False):
    """mxg_scan_long_swept_host over `calls` equal pieces of x [N][V] and coef [N][rows][V], the state array st (full_state) carried:
    (out, final state array)."""
    L = lib()
    x = np.ascontiguousarray(x, np.float64)
    coef = np.ascontiguousarray(coef, np.float64)
    N, V = x.shape
    assert N % calls == 0 and coef.shape[0] == N and coef.shape[2] == V
    n, rows = N // calls, coef.shape[1]
    st = np.ascontiguousarray(st, np.float64).copy()
    assert st.shape == (NROWS[kind], V)
    out = x.copy() if inplace else np.empty((N, V))
    for b in range(calls):
        ob = out[b * n:(b + 1) * n]
        xb = ob if inplace else x[b * n:(b + 1) * n]
        rc = L.mxg_scan_long_swept_host(KIND_ID[kind], V, n, xb.ctypes.data, coef[b * n:(b + 1) * n].ctypes.data, rows, st.ctypes.data, ob.ctypes.data)
        assert rc == 0, L.mxg_last_error().decode()
    return out, st
