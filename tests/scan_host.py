"""Helpers of the time-parallel scan tests (tests/test_scan_host.py, tests/test_gpu_scan.py): the host build of
maximilian_amd/csrc/mxg_scan.h (tests/host_scan.cpp) as a bank renderer over the layouts of scan_filter_launch, the coefficient rows
and the sequential recurrences through the oracle, the long-double sequential recurrence, and the parameter sets of the full-domain
sweep.  A `kind` is one of KINDS; its parameters are rows par [P][V] as the oracle takes them (dc: R; svf: cutoff, res, lp, bp, hp,
notch; biquad: type, cutoff, Q, gain; lores / hires: cutoff, res)."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import HOST_OPT, ROOT

P = ctypes.c_void_p
KINDS = ["dc", "svf", "biquad", "lores", "hires"]
KIND_ID = {k: i for i, k in enumerate(KINDS)}
NSTATE = {"dc": 2, "svf": 3, "biquad": 3, "lores": 2, "hires": 2}   # state rows a bank of the kind carries through the scan
ALL_L = [1, 2, 4, 8, 16, 32]
SCAN_RTOL = 1e-10  # x the voice's peak of the sequential output over the carried blocks: the published bound of the mode
SVF_MIX = (0.5, 0.25, 0.125, 0.6)


def build(tmp):
    so = str(tmp / "libscan_host.so")
    subprocess.check_call(["g++", "-std=c++17"] + HOST_OPT + ["-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "host_scan.cpp")])
    L = ctypes.CDLL(so)
    for fn in (L.scan_host_render, L.scan_host_seq_ld):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, P, P, P, P]
    return L


def coef_rows(port, kind, par):
    """The coefficient rows [NC][V] the kernels get, from the oracle's restatement of the reference's setters."""
    par = np.ascontiguousarray(par, np.float64)
    V = par.shape[1]
    if kind == "dc":
        return par[:1].copy()
    if kind == "svf":
        return np.ascontiguousarray(np.concatenate([port.filter2(1, np.zeros((1, V)), par)[2], par[2:6]]))
    if kind == "biquad":
        return port.filter2(2, np.zeros((1, V)), par)[2]
    return np.ascontiguousarray(port.filter_coeffs(0, par[0], par[1])[:2])


def oracle_seq(port, kind, x, par, st0):
    """The oracle's sequential recurrence over the whole stream x [N][V] from the state st0 [NSTATE][V]: (out, final state)."""
    V = x.shape[1]
    if kind in ("lores", "hires"):
        st = np.zeros((5, V))
        st[:2] = st0
        out, st = port.filter(0 if kind == "lores" else 1, x, par[0], par[1], state=st)
        return out, st[:2].copy()
    st = np.zeros((3, V))
    st[:NSTATE[kind]] = st0
    out, st, _ = port.filter2(KIND_ID[kind], x, par, st=st)
    return out, st[:NSTATE[kind]].copy()


def _run(fn, kind, x, coef, st0, blocks):
    x = np.ascontiguousarray(x, np.float64)
    coef = np.ascontiguousarray(coef, np.float64)
    N, V = x.shape
    assert N % blocks == 0 and coef.shape[1] == V
    n = N // blocks
    st = np.ascontiguousarray(st0, np.float64).copy()
    assert st.shape == (NSTATE[kind], V)
    out = np.empty((N, V))
    for b in range(blocks):
        xb, ob = np.ascontiguousarray(x[b * n:(b + 1) * n]), np.empty((n, V))
        assert fn(KIND_ID[kind], V, n, xb.ctypes.data, coef.ctypes.data, st.ctypes.data, ob.ctypes.data) == 0
        out[b * n:(b + 1) * n] = ob
    return out, st


def host_scan(L, kind, x, coef, st0, blocks=1):
    """The 64-lane host model over `blocks` equal blocks of x [N][V], the state carried: (out, final state)."""
    return _run(L.scan_host_render, kind, x, coef, st0, blocks)


def seq_long_double(L, kind, x, coef, st0):
    """The sequential recurrence in long double over the whole stream: (out, final state), rounded to double at the end."""
    return _run(L.scan_host_seq_ld, kind, x, coef, st0, 1)


def scaled_err(got, exp, peak_of=None):
    peak = np.maximum(np.abs(exp if peak_of is None else peak_of).max(axis=0), 1e-300)
    return np.abs(got - exp).max(axis=0) / peak


def state_err(port, kind, par, got_st, exp_st, exp_out, n=256):
    """A carried state is worth what the stream does from it: the sequential recurrence runs n more samples (noise in [-1, 1]) from
    the state under test and from the sequential recurrence's own; the two outputs on the same scale as the stream's error, the
    voice's peak of the sequential output.  (A state's own magnitude is no scale: a direct-form-II state at 20 Hz is 1e5 x the
    output, and any one component passes through zero.)"""
    x = np.random.default_rng(99).uniform(-1, 1, (n, exp_out.shape[1]))
    a, _ = oracle_seq(port, kind, x, par, got_st)
    b, _ = oracle_seq(port, kind, x, par, exp_st)
    return scaled_err(a, b, peak_of=np.concatenate([exp_out, b]))


# ---- the full domain the classes accept: a fixed grid with the corners + a seeded log-uniform part ------------------------------
def _loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def sweep_params(kind, seed=2024):
    rng = np.random.default_rng(seed + KIND_ID[kind])
    if kind == "dc":  # R 0 ... 1.0 (1.0: a pure integrator of the differences)
        grid = [0.0, 0.5, 0.9, 0.95, 0.99, 0.995, 0.999, 0.9999, 0.999999, 1.0]
        return np.concatenate([grid, 1.0 - _loguniform(rng, 1e-7, 0.1, 22)])[None, :]
    if kind == "svf":  # 20 Hz ... 22 kHz, res 0 (the damping = 0 branch) ... 1000
        g = [(c, r) for c in (20.0, 100.0, 1000.0, 5000.0, 15000.0, 22000.0) for r in (0.0, 0.5, 2.0, 30.0, 1000.0)]
        cut = np.concatenate([[c for c, _ in g], _loguniform(rng, 20.0, 22000.0, 34)])
        res = np.concatenate([[r for _, r in g], _loguniform(rng, 0.05, 1000.0, 34)])
        return np.stack([cut, res] + [np.full(cut.size, m) for m in SVF_MIX])
    if kind == "biquad":  # all seven types, 10 Hz ... 21.5 kHz, Q 0.1 ... 50, gain -18 ... +18 dB (types 4-6 use it)
        g = [(t, c, q, gn) for t in range(7) for c in (10.0, 20.0, 60.0, 1000.0, 10000.0, 21500.0) for q in (0.1, 0.7, 8.0, 50.0)
             for gn in ((-18.0, 18.0) if t >= 4 else (0.0,))]
        n = 200
        typ = np.concatenate([[t for t, _, _, _ in g], rng.integers(0, 7, n)]).astype(np.float64)
        cut = np.concatenate([[c for _, c, _, _ in g], _loguniform(rng, 10.0, 21500.0, n)])
        q = np.concatenate([[q for _, _, q, _ in g], _loguniform(rng, 0.1, 50.0, n)])
        gain = np.concatenate([[gn for _, _, _, gn in g], rng.uniform(-18.0, 18.0, n)])
        return np.stack([typ, cut, q, gain])
    # lores / hires: 10 Hz ... 8 kHz, res 1 ... 1000
    g = [(c, r) for c in (10.0, 100.0, 1000.0, 4000.0, 8000.0) for r in (1.0, 2.0, 30.0, 1000.0)]
    cut = np.concatenate([[c for c, _ in g], _loguniform(rng, 10.0, 8000.0, 30)])
    res = np.concatenate([[r for _, r in g], _loguniform(rng, 1.0, 1000.0, 30)])
    return np.stack([cut, res])


def sweep_case(kind, N, blocks=3, seed=2024):
    """(par [P][V], x [blocks * N][V] uniform noise in [-1, 1], st0 [NSTATE][V] random and non-zero) of the sweep at block size N."""
    par = sweep_params(kind, seed)
    V = par.shape[1]
    rng = np.random.default_rng(seed * 7 + KIND_ID[kind] * 100003 + N)
    x = rng.uniform(-1, 1, (blocks * N, V))
    st0 = rng.uniform(-1, 1, (NSTATE[kind], V))
    st0[np.abs(st0) < 1e-3] = 0.5
    return par, x, st0


# ---- the named settings of the non-finite-input tests (all stable) ----------------------------------------------------------------
NONFINITE_SETTINGS = [
    ("dc", [0.995]),
    ("svf", [700.0, 2.0] + list(SVF_MIX)),
    ("biquad", [0.0, 1200.0, 0.7, 0.0]),    # low-pass 1200 Hz, Q 0.7
    ("biquad", [6.0, 3000.0, 0.7, 6.0]),    # high-shelf 3 kHz
    ("lores", [800.0, 3.0]),
    ("hires", [800.0, 3.0]),
]
BAD_SAMPLES = [("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)]
