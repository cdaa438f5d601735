"""CPU (-m "not gpu"): mxg_fx.h -- the arithmetic fx.hip's flanger / chorus kernels run -- compiled for the host.
The tile machinery (trajectory, classification, two-run touched set, staging) is fuzzed against the step-by-step
recurrence of maxiDelayline::dl over random sizes including <= 0, NaN, 1, shorter than the tile and above cap
(tests/host_fx.cpp); the per-sample effect arithmetic is compared with the numpy checker tests/fx_port.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fx_port
from conftest import HOST_OPT, ROOT
from test_fx_cpu import bits_equal

P = ctypes.c_void_p


@pytest.fixture(scope="module")
def fx_host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fx") / "libfx_host.so")
    subprocess.check_call(["g++", "-std=c++17"] + HOST_OPT + ["-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "maximilian_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "host_fx.cpp")])
    lib = ctypes.CDLL(so)
    lib.fx_tile_fuzz.restype = ctypes.c_int
    lib.fx_tile_fuzz.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, P, ctypes.c_int, P, ctypes.c_double, P]
    lib.fx_flanger_host.argtypes = [ctypes.c_int, P, ctypes.c_uint32] + [ctypes.c_double] * 4 + [ctypes.c_int, P]
    lib.fx_chorus_host.argtypes = [ctypes.c_int, P, ctypes.c_uint32] + [ctypes.c_double] * 4 + [P, ctypes.c_int, P]
    return lib


def size_stream(rng, n, cap, T, regime):
    if regime == "mixed":
        pool = np.array([np.nan, -3.0, -1e12, 0.0, 0.5, 1.0, 2.0, T - 1.0, T, T + 1.0, cap - 1.0, cap, cap + 5.0,
                         3e9, -2147483649.0])
        s = rng.choice(pool, n)
        m = rng.random(n) < 0.5
        s[m] = rng.uniform(-10, 2.5 * cap, m.sum())
        return s
    if regime == "long":     # an LFO-like drift around a large size: mostly conflict-free tiles
        base = rng.uniform(T + 5, max(cap, T + 6))
        return base + 0.3 * base * np.sin(np.arange(n) * rng.uniform(1e-3, 0.1)) + 1.0
    return rng.uniform(-2, 1.5 * T, n)  # short: sizes around the tile


@pytest.mark.parametrize("regime", ["mixed", "long", "short"])
def test_tile_machinery_matches_recurrence(fx_host, regime):
    rng = np.random.default_rng({"mixed": 1, "long": 2, "short": 3}[regime])
    conflicted = 0
    for trial in range(300):
        T = int(rng.choice([8, 64]))
        cap = int(rng.choice([1, 3, 50, 200, 1000]))
        n = int(rng.integers(1, 700))
        sizes = np.ascontiguousarray(size_stream(rng, n, cap, T, regime))
        ph0 = int(rng.choice([0, 0, 5, cap - 1, cap + 7, -3]))
        x = np.ascontiguousarray(rng.uniform(-1, 1, n))
        nc = ctypes.c_int(0)
        bad = fx_host.fx_tile_fuzz(T, cap, n, sizes.ctypes.data, ph0, x.ctypes.data, float(rng.choice([0.0, 0.7, 1.2])),
                                   ctypes.byref(nc))
        assert bad == 0, (trial, T, cap, n, ph0)
        conflicted += nc.value
    if regime != "long":
        assert conflicted > 0  # both kinds of tile were exercised


def test_effect_arithmetic_matches_port(fx_host):
    rng = np.random.default_rng(9)
    N, cap = 3000, 2048
    for delay, fb, speed, depth in [(800, 0.5, 1.0, 0.5), (20, 0.99, 7.0, 1.0), (0, 1.2, 3.0, 1.5), (300, 0.2, 0.3, np.nan)]:
        x = np.ascontiguousarray(rng.uniform(-1, 1, N))
        got = np.zeros(N)
        fx_host.fx_flanger_host(N, x.ctypes.data, delay, fb, speed, depth, 44100.0, cap, got.ctypes.data)
        assert bits_equal(got, fx_port.Flanger(1, cap).flange(x[:, None], delay, fb, speed, depth)[:, 0])
        from maximilian_amd.banks import chorus_coeffs
        c, r = chorus_coeffs(np.array([speed * 3]))[:, 0]
        rd = np.ascontiguousarray(rng.integers(0, 2 ** 31 - 1, N, dtype=np.int32))
        fx_host.fx_chorus_host(N, x.ctypes.data, delay, fb, c, r, depth, rd.ctypes.data, cap, got.ctypes.data)
        exp = fx_port.Chorus(1, cap).chorus(x[:, None], delay, fb, np.array([[c], [r]]), depth, rd[:, None])[:, 0]
        assert bits_equal(got, exp)
