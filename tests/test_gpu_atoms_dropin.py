"""GPU: the drop-in atoms classes in a running program, and the C++ facade.  tests/patches/atoms_patch.cpp (host/dropin_at) -- a book,
its player, and an accelerator with raw atoms added by hand, filled with buffers of 64 and of 16 samples so that an entry stalls -- is
run, and its stream is checked against tests/golden/atoms.npz, which tools/gen/gen_golden_atoms.py recorded from the same source
compiled against the reference: BIT FOR BIT where only raw atoms and the initial ramp sound, and within the derived bound of the
Gabor contract elsewhere (tests/atoms_host.py: per live Gabor atom 3 * 2^-23 |env_f amp| and one rounding of the partial sum).
host/facade_atoms_smoke: maxiAtomBank of include/maximilian_bank.hpp against the host arithmetic."""
import os
import subprocess

import numpy as np
import pytest

import atoms_host as ah
from conftest import ROOT

pytestmark = pytest.mark.gpu

# the patch's book (rows position, length, amp, frequency, phase), its loop and its buffer: tests/patches/atoms_patch.cpp
BOOK = [(0, 63, 20, 0.02, 0), (0, 257, 12, 0.3, 1), (64, 2, 30, 0.9, -1), (192, 64, 25, 0.11, 2), (256, 65, 35, 0.05, 0.3), (512, 1, 40, 0.5, 0.5),
        (576, 300, 18, 0.15, 0), (960, 64, 40, 0.2, 0)]
BLOCKS, B, LOOP = 40, 64, 1024


def run(exe, *args):
    path = os.path.join(ROOT, exe)
    if not os.path.exists(path):
        pytest.fail("%s is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)" % exe)
    r = subprocess.run([path] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert b"ERROR" not in r.stderr, r.stderr.decode()
    return r.stdout.decode()


def test_atoms_patch_against_reference(golden, tmp_path):
    exp = golden("atoms.npz")["patch"]
    out = str(tmp_path / "o.f32")
    run("host/dropin_at", out)
    got = np.fromfile(out, np.float32)
    assert got.shape == exp.shape == (BLOCKS * B,)
    # where Gabor atoms are live, and how large: every book atom starts on its position in every loop (block-aligned, sorted), except
    # the one at 960, in whose buffer nothing is scheduled
    tol = np.zeros(len(exp))
    count = np.zeros(len(exp))
    mag = np.abs(0.001 * (np.arange(len(exp)) % B)) + 1.0      # the ramp, and the raw atoms (|click| <= 0.5, |ramp| < 1)
    for loop0 in range(0, len(exp), LOOP):
        for row in BOOK:
            if (row[0] + B) % LOOP == 0:
                continue
            _, _, length, _, amp = ah.book_gabor_args(row)
            e = np.abs(ah.window_f(length).astype(np.float64) * float(amp))
            t0 = loop0 + int(row[0])
            n = min(length, len(exp) - t0)
            if n <= 0:
                continue
            tol[t0:t0 + n] += 3 * ah.EPS * e[:n] + 4 * ah.TINY
            count[t0:t0 + n] += 1
            mag[t0:t0 + n] += e[:n]
    tol += count * ah.EPS * mag
    raw_only = count == 0
    assert raw_only.sum() > 300 and (exp[raw_only] != np.float32(0.001) * (np.arange(len(exp)) % B).astype(np.float32)[raw_only]).sum() > 100, \
        "raw atoms sound where no Gabor atom does"
    assert np.array_equal(ah.bits(got[raw_only]), ah.bits(exp[raw_only])), "raw atoms and the initial ramp: bit for bit"
    err = np.abs(got.astype(np.float64) - exp)
    print("atoms patch: max |difference| %.3e, worst %.3f of the derived bound; %d of %d samples differ"
          % (err.max(), (err[~raw_only] / tol[~raw_only]).max(), int((ah.bits(got) != ah.bits(exp)).sum()), len(exp)))
    assert (err <= tol).all()


def test_facade_atoms_smoke():
    assert "facade_atoms_smoke: ok" in run("host/facade_atoms_smoke")
