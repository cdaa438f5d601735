"""Helpers of the long time-parallel scan's tests (tests/test_scan_long_host.py, tests/test_gpu_scan_long.py): the host twin
mxg_scan_long_host as a bank renderer with carried state, the sequential recurrences it is measured against (the oracle's for
kinds 0-4 through tests/scan_host.py; for the lag the library's bit-exact mxg_lag_host), the long-double recurrences, the
per-kind bounds and the shapes of the sweep.  A `kind` is one of KINDS; parameters are rows par [P][V] as in tests/scan_host.py,
the lag's is one row alpha (alphaReciprocal = 1 - alpha, as maxiLagExp::init sets it)."""
import ctypes
import os
import subprocess

import numpy as np

import scan_host as sh
from conftest import HOST_OPT, ROOT

KINDS = sh.KINDS + ["lag"]
KIND_ID = {k: i for i, k in enumerate(KINDS)}
NSTATE = dict(sh.NSTATE, lag=1)                                          # state rows the scan reads and writes
NROWS = {"dc": 3, "svf": 3, "biquad": 3, "lores": 5, "hires": 5, "lag": 1}  # state rows of the sequential entry point's array
T = 2048
RAGGED = 3 * T + 5 * 64 + 7
# chunks per call of the sweep: a chunk boundary; one lane run of phase B plus one; a run of 64 plus one (the Kogge-Stone of phase
# B with runs longer than one chunk); and the ragged N (three chunks, K10 blocks of 256 and 64, seven plain steps)
SWEEP_N = {"2": 2 * T, "65": 65 * T, "4097": (64 * 64 + 1) * T, "ragged": RAGGED}

# The bound per kind, x the voice's peak of the sequential output, for a stream of up to 3 x 4097 chunks (2.5e7 samples) carried from
# a state: the worst of the WHOLE sweep -- at 2, 65 and 4097 chunks and the ragged N on this module's streams
# (tests/test_scan_long_host.py, its docstring has the figures) and every setting at 4097 chunks on other noise
# (tools/measure_longscan_tolerance.py, profiles/longscan_tolerance.json) -- x 2, rounded up to one significant digit.
SCAN_LONG_RTOL = {"dc": 5e-12, "svf": 8e-10, "biquad": 4e-10, "lores": 2e-12, "hires": 2e-12, "lag": 9e-12}


def lib():
    import maximilian_amd
    return maximilian_amd.lib()


def build(tmp):
    """tests/host_scan_long.cpp: the lag's recurrence in long double."""
    so = str(tmp / "libscan_long_host.so")
    subprocess.check_call(["g++", "-std=c++17"] + HOST_OPT + ["-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                           os.path.join(ROOT, "tests", "host_scan_long.cpp")])
    L = ctypes.CDLL(so)
    L.scan_long_lag_ld.restype = ctypes.c_int
    L.scan_long_lag_ld.argtypes = [ctypes.c_size_t, ctypes.c_size_t] + [ctypes.c_void_p] * 4
    return L


def lag_alphas(seed=2024):
    """The lag's sweep: alpha from 1e-6 to 1, the corners and a seeded log-uniform part."""
    rng = np.random.default_rng(seed + 5)
    grid = [1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 0.5, 0.9, 0.999, 1.0]
    return np.concatenate([grid, np.exp(rng.uniform(np.log(1e-6), 0.0, 22))])[None, :]


def sweep_params(kind, seed=2024):
    return lag_alphas(seed) if kind == "lag" else sh.sweep_params(kind, seed)


def _long_memory(kind, p):
    """Whether a setting of the sweep barely decays or does not decay at all: where the whole sweep at 4097 chunks
    (tools/measure_longscan_tolerance.py, profiles/longscan_tolerance.json) has its worst figures, every one of them."""
    if kind == "dc":
        return p[0] >= 0.999999                                  # an integrator of the differences, or nearly one
    if kind == "svf":
        return p[1] == 0.0 or (p[0] == 20.0 and p[1] == 1000.0)  # res 0: |pole| = 1 at EVERY cutoff; the highest resonance at the lowest
    if kind == "biquad":
        return p[1] == 10.0 and ((p[0] <= 3 and p[2] == 50.0) or (p[0] == 6 and p[3] == -18.0))   # poles nearest z = 1
    if kind == "lag":
        return p[0] < 2e-6
    return p[1] == 1000.0 and p[0] <= 100.0                      # lores / hires


def long_params(kind, n=3):
    """The settings the TEST runs at 4097 chunks a call (8.4 M samples per voice and call, 2.5 s of CPU per setting): every
    _long_memory setting of the sweep and n spread evenly over it.  The whole sweep at that length is
    tools/measure_longscan_tolerance.py's; SCAN_LONG_RTOL is built on it."""
    par = sweep_params(kind)
    V = par.shape[1]
    idx = set(np.linspace(0, V - 1, n).astype(int).tolist()) | {i for i in range(V) if _long_memory(kind, par[:, i].tolist())}
    return np.ascontiguousarray(par[:, sorted(idx)])


def sweep_case(kind, N, calls=3, seed=2024, par=None):
    """(par, x [calls * N][V] uniform noise in [-1, 1], st0 random and non-zero): tests/scan_host.py's sweep_case for kinds 0-4
    (the same streams), the alpha sweep for the lag; with `par` given, those settings instead of the whole sweep."""
    if kind != "lag" and par is None:
        return sh.sweep_case(kind, N, calls, seed)
    par = lag_alphas(seed) if par is None else par
    V = par.shape[1]
    rng = np.random.default_rng(seed * 7 + KIND_ID[kind] * 100003 + N)
    x = rng.uniform(-1, 1, (calls * N, V))
    st0 = rng.uniform(-1, 1, (NSTATE[kind], V))
    st0[np.abs(st0) < 1e-3] = 0.5
    return par, x, st0


def coef_rows(port, kind, par):
    if kind == "lag":
        a = np.ascontiguousarray(par[0], np.float64)
        return np.stack([a, 1.0 - a])
    return sh.coef_rows(port, kind, par)


def oracle_seq(port, kind, x, par, st0):
    """The sequential recurrence over the whole stream: (out, final state [NSTATE][V])."""
    if kind != "lag":
        return sh.oracle_seq(port, kind, x, par, st0)
    x = np.ascontiguousarray(x, np.float64)
    coef = coef_rows(port, kind, par)
    val, out = np.ascontiguousarray(st0[0], np.float64).copy(), np.empty_like(x)
    N, V = x.shape
    assert lib().mxg_lag_host(V, N, x.ctypes.data, coef[0].ctypes.data, coef[1].ctypes.data, 0, val.ctypes.data, out.ctypes.data) == 0
    return out, val[None, :].copy()


def seq_long_double(hosts, kind, x, coef, st0):
    """hosts = (tests/scan_host.py's build, this module's build)."""
    if kind != "lag":
        return sh.seq_long_double(hosts[0], kind, x, coef, st0)
    x, coef = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(coef, np.float64)
    st, out = np.ascontiguousarray(st0, np.float64).copy(), np.empty_like(x)
    assert hosts[1].scan_long_lag_ld(x.shape[1], x.shape[0], x.ctypes.data, coef.ctypes.data, st.ctypes.data, out.ctypes.data) == 0
    return out, st


def state_err(port, kind, par, got_st, exp_st, exp_out, n=256):
    """tests/scan_host.py's state_err: a carried state is worth what the sequential recurrence does from it."""
    x = np.random.default_rng(99).uniform(-1, 1, (n, exp_out.shape[1]))
    a, _ = oracle_seq(port, kind, x, par, got_st)
    b, _ = oracle_seq(port, kind, x, par, exp_st)
    return sh.scaled_err(a, b, peak_of=np.concatenate([exp_out, b]))


def full_state(kind, st0, fill=None):
    """The state array of the sequential entry point ([3][V] / [5][V] / [1][V]) holding the scan's rows; the other rows `fill`."""
    st0 = np.asarray(st0, np.float64)
    st = np.zeros((NROWS[kind], st0.shape[1])) if fill is None else np.full((NROWS[kind], st0.shape[1]), fill, np.float64)
    st[:NSTATE[kind]] = st0
    return st


def host_long(kind, x, coef, st, calls=1, inplace=False):
    """mxg_scan_long_host over `calls` equal pieces of x [N][V], the state array st (full_state) carried: (out, final state array)."""
    L = lib()
    x = np.ascontiguousarray(x, np.float64)
    coef = np.ascontiguousarray(coef, np.float64)
    N, V = x.shape
    assert N % calls == 0 and coef.shape[1] == V
    n = N // calls
    st = np.ascontiguousarray(st, np.float64).copy()
    assert st.shape == (NROWS[kind], V)
    out = x.copy() if inplace else np.empty((N, V))
    for b in range(calls):
        ob = out[b * n:(b + 1) * n]
        xb = ob if inplace else x[b * n:(b + 1) * n]
        rc = L.mxg_scan_long_host(KIND_ID[kind], V, n, xb.ctypes.data, coef.ctypes.data, st.ctypes.data, ob.ctypes.data)
        assert rc == 0, L.mxg_last_error().decode()
    return out, st
