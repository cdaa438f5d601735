"""CPU (-m "not gpu"): the numpy checker of the flanger / chorus banks (tests/fx_port.py) against the reference's own
output (tests/golden/fx.npz, tools/gen/gen_golden_fx.py), bit for bit, every case and every final state."""
import os
import subprocess

import numpy as np
import pytest

import fx_port
from conftest import GOLDEN, ROOT

FX = os.path.join(GOLDEN, "fx.npz")


def bits_equal(a, b):
    """bit for bit, all NaNs one class (x86 and the device spell a produced NaN differently)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def cases(kind):
    z = np.load(FX)
    return [str(c) for c in z["cases"] if str(c).startswith(kind)]


def load(name):
    z = np.load(FX)
    return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


def chorus_coef(speed):
    from maximilian_amd.banks import chorus_coeffs
    return chorus_coeffs(speed)


def test_golden_covers_the_contract():
    z = np.load(FX)
    assert os.path.getsize(FX) <= 1.5 * 2 ** 20
    assert "sha256" in str(z["provenance"]) and "ffp-contract=off" in str(z["provenance"])
    names = [str(c) for c in z["cases"]]
    assert any(n.startswith("fl_") for n in names) and any(n.startswith("ch_") for n in names)
    allp = {k: np.concatenate([np.ravel(load(n)[k]) for n in names]) for k in ("feedback", "depth", "speed")}
    for fb in (0.0, 0.99, 1.2):
        assert fb in allp["feedback"]
    for dp in (0.0, 1.0, 1.5):
        assert dp in allp["depth"]
    assert np.isnan(allp["depth"]).any()
    sp = allp["speed"]
    assert (sp < 10).any() and (sp == 10).any() and (sp > 10).any()
    assert any(load(n)["ps"].any() for n in names) and any(not load(n)["ps"].any() for n in names)


@pytest.mark.parametrize("name", cases("fl"))
def test_flanger_port_matches_reference(name):
    c = load(name)
    N, V = c["in"].shape
    f = fx_port.Flanger(V, 705600)  # the reference's own ring: nothing is clamped
    y = f.flange(c["in"], c["delay"], c["feedback"], c["speed"], c["depth"])
    assert bits_equal(y, c["out"])
    assert np.array_equal(f.ring.phase, c["phase"].astype(np.int64))
    assert bits_equal(f.lfo_phase, c["lfo_phase"])
    assert not f.overflow.any()


@pytest.mark.parametrize("name", cases("ch"))
def test_chorus_port_matches_reference(name):
    c = load(name)
    N, V = c["in"].shape
    ch = fx_port.Chorus(V, 705600)
    y = ch.chorus(c["in"], c["delay"], c["feedback"], chorus_coef(c["speed"]), c["depth"], c["rand"])
    assert bits_equal(y, c["out"])
    assert np.array_equal(np.stack([r.phase for r in ch.rings]), c["phase"].astype(np.int64))
    assert bits_equal(ch.lx, c["lp"][0]) and bits_equal(ch.ly, c["lp"][1])


def test_port_edge_sizes():
    # sizes <= 0, NaN and beyond 2^31 all reset the phase every sample (x86's INT_MIN); above cap is held and counted
    d = np.array([np.nan, -5.0, 0.0, 0.9, 1.0, 2147483647.9, 2147483648.0, -2147483648.9, -2147483649.0, 1e300])
    assert fx_port.cvt_i32(d).tolist() == [-2 ** 31, -5, 0, 0, 1, 2147483647, -2 ** 31, -2147483648, -2 ** 31, -2 ** 31]
    f = fx_port.Flanger(3, 16)
    x = np.ones((40, 3))
    f.flange(x, [0, 10, 40], 0.5, 1.0, 0.0)
    assert f.overflow.tolist() == [0, 0, 40]
    assert f.ring.phase.tolist() == [1, 40 % 11, 40 % 16]  # sizes delay + 1: 1, 11, 41 -> 16



EX = "/root/reference/cpp/commandline/maximilian_examples"


@pytest.mark.parametrize("example", ["23.Chorus", "24.Flanger"])
def test_effect_examples_compile_against_dropin(example, tmp_path):
    """The reference's two effect examples compile verbatim against include/maximilian.h (where the reference exists)."""
    src = os.path.join(EX, example, "main.cpp")
    if not os.path.exists(src):
        pytest.skip("the reference's examples are not present")
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I" + os.path.join(ROOT, "include"), src,
                           "-o", str(tmp_path / "main.o")], cwd=str(tmp_path))


def test_fx_patch_compiles_against_dropin(tmp_path):
    """tests/patches/fx_patch.cpp (value semantics: maxiFlanger in a std::vector, its public dl / lfo) builds here too."""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "patches", "fx_patch.cpp"), "-o", str(tmp_path / "p.o")])
    src = tmp_path / "members.cpp"
    src.write_text('#include "maximilian.h"\n#include <vector>\n'
                   'double f(maxiFlanger &fl) { std::vector<maxiFlanger> v(2, fl); v.push_back(fl);\n'
                   '  return v[1].dl.dl(0.5, 10, 0.5) + fl.lfo.triangle(1.0); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(tmp_path / "m.o")])


def test_facade_banks_compile(tmp_path):
    src = tmp_path / "facade.cpp"
    src.write_text('#include "maximilian_bank.hpp"\n'
                   'void f(const double *in, const int32_t *rnd, double *out) {\n'
                   '  maxiFlangerBank fl(64, 2048); fl.setParams(std::vector<uint32_t>(64, 800), std::vector<double>(64, 0.5),\n'
                   '      std::vector<double>(64, 1.0), std::vector<double>(64, 0.5)); fl.flange(512, in, out);\n'
                   '  maxiChorusBank ch(64, 2048); ch.setParams(std::vector<uint32_t>(64, 800), std::vector<double>(64, 0.5),\n'
                   '      std::vector<double>(64, 1.0), std::vector<double>(64, 0.5)); ch.chorus(512, in, rnd, out); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(tmp_path / "f.o")])
