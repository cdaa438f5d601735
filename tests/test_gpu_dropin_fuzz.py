"""GPU (-m gpu): DIFFERENTIAL FUZZ of the drop-in boundary.  tests/patches/fuzz_patch.cpp -- a seeded random graph of the drop-in
classes with rare random events (changed literals, other methods, setters, public state members, copies, vectors that grow, objects
destroyed and constructed again, skipped and doubled calls, delay sizes changed on the block edges) -- is built against
include/maximilian.h (host/dropin_fz) and run once per (profile, seed); the expected samples are what the SAME file computes when
linked with the unmodified reference (tests/golden/dropin_fuzz.npz, tools/gen/gen_golden_fuzz.py).  Everything is bit for bit: no
tolerance, no excluded frames (sinewave / coswave, the one <= 1 ULP pair, stay out of the generator by construction).

Every child is a subprocess with its own time limit.  MEASURED on an MI355X: host/dropin_p5 (public_members_patch.cpp) renders 6000
frames in 4.115 s = 0.686 ms per frame (the header of this commit differs from its parent's by four counters only); the limit of a
child is 4 x that x its frame count (16.5 s for 6000 frames).
A child that faults, aborts or runs into its limit ends the SESSION (pytest.exit): nothing more is started on a device that has just
faulted.  Measured wall time of this file: 94 children in 82-87 s, the slowest 2.8 s (tests/test_gpu_dropin.py on the same machine: 36-38 s).
No seed has differed on the unmodified engine so far; one that does gets a named regression here (seed + frame count, one line on what
it hit) next to the fix."""
import importlib.util
import os
import re
import subprocess
import time

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("gen_golden_fuzz", os.path.join(ROOT, "tools", "gen", "gen_golden_fuzz.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

P5_MS_PER_FRAME = 0.686      # measured, see the docstring
MECH_OFF_FRAMES = 2000       # the mechanism-off variants render this prefix of the golden stream (never below 2000 frames)
_G = np.load(os.path.join(ROOT, "tests", "golden", "dropin_fuzz.npz"))
CORE = [tuple(int(v) for v in x) for x in _G["core_pairs"]]
DIGEST = [tuple(int(v) for v in x) for x in _G["digest_pairs"]]
_cache = {}
walls = []


def child_limit(frames):
    return 4 * P5_MS_PER_FRAME * 1e-3 * frames


def run_fz(profile, seed, frames, tmp, total=None, **env_extra):
    """One child.  `total` is the length the patch is told (profile 3 places its last events by it): the golden run's, also where
    only a prefix is rendered."""
    exe = os.path.join(ROOT, "host", "dropin_fz")
    if not os.path.exists(exe):
        pytest.fail("host/dropin_fz is not built (python -c 'import __graft_entry__ as g; g.build()' builds it)")
    out = os.path.join(str(tmp), "fz_%d_%d_%s.f64" % (profile, seed, "_".join(sorted(env_extra)) or "on"))
    env = dict(os.environ, MXG_FUZZ_SEED=str(seed), MXG_FUZZ_PROFILE=str(profile), MXG_FUZZ_FRAMES=str(total or frames))
    for k in ("MXG_FUZZ_LOG", "MXG_FUZZ_MAXOBJ", "MXG_PS_DERIVE", "MXG_PS_ZEROCOPY"):
        env.pop(k, None)
    env.update(env_extra)
    t0 = time.time()
    try:
        r = subprocess.run([exe, str(frames), out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                           timeout=child_limit(frames), env=env)
    except subprocess.TimeoutExpired:
        pytest.exit("dropin_fz profile %d seed %d %r ran into its limit of %.1f s: nothing more is started" % (
            profile, seed, env_extra, child_limit(frames)), returncode=3)
    wall = time.time() - t0
    walls.append((wall, profile, seed, tuple(sorted(env_extra))))
    if r.returncode in (134, 139, 124, 137, -6, -11, -9):
        pytest.exit("dropin_fz profile %d seed %d %r ended with status %d: nothing more is started\n%s" % (
            profile, seed, env_extra, r.returncode, r.stderr[-2000:]), returncode=3)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ERROR" not in r.stderr, r.stderr[-2000:]    # (a device failure or a refused argument would print one line and play silence)
    return np.fromfile(out, np.float64).reshape(frames, 2), r.stderr, wall


def run_pair(profile, seed, frames, tmp):
    key = (profile, seed, frames)
    if key not in _cache:
        got, log, wall = run_fz(profile, seed, frames, tmp)
        _cache[key] = (got, stats(log), gen.parse_counts(log))
        print("profile %d seed %d: %.2f s" % (profile, seed, wall))
    return _cache[key]


def stats(log):
    """The drop-in host's statistics lines -> {"launches": {pool: n}, "async": {...}, "rewinds": {...}, "derived": {...}, "undos": n, "forms": {1..9: n}}."""
    m = re.search(r"launches: osc (\d+) \(async blocks (\d+)\), env (\d+) \((\d+)\), filter (\d+)", log)
    p = re.search(r"pools: sample (\d+) \(async blocks (\d+)\), delay (\d+) \((\d+)\), filter2 (\d+) \((\d+)\), envgen (\d+) \((\d+)\), "
                  r"filter async (\d+); rewinds: osc (\d+) env (\d+) filter (\d+) sample (\d+) delay (\d+) filter2 (\d+) envgen (\d+); "
                  r"derived blocks: osc (\d+) env (\d+) filter (\d+) sample (\d+) delay (\d+) filter2 (\d+) envgen (\d+); delay undos (\d+)", log)
    f = re.search(r"derived forms 1-9: " + " ".join([r"(\d+)"] * 9), log)
    assert m and p and f, log
    a = [int(x) for x in m.groups()]
    b = [int(x) for x in p.groups()]
    pools = ["osc", "env", "filter", "sample", "delay", "filter2", "envgen"]
    return {
        "launches": dict(zip(pools, [a[0], a[2], a[4], b[0], b[2], b[4], b[6]])),
        "async": dict(zip(pools, [a[1], a[3], b[8], b[1], b[3], b[5], b[7]])),
        "rewinds": dict(zip(pools, b[9:16])),
        "derived": dict(zip(pools, b[16:23])),
        "undos": b[23],
        "forms": {k + 1: int(x) for k, x in enumerate(f.groups())},
    }


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fuzz")


@pytest.mark.parametrize("profile,seed", CORE)
def test_core_seed_stream_is_the_references(profile, seed, tmp):
    """The full stereo stream, both channels, all frames."""
    exp = _G["core_%d_%d" % (profile, seed)]
    got, _, counts = run_pair(profile, seed, gen.FRAMES[profile], tmp)
    assert_bits_equal(got, exp, "fuzz profile %d seed %d (channel 1 = object frame %% %d)" % (profile, seed, counts["objects"]))


def _explain(profile, seed, got, block, nobj):
    """Where the reference build is at hand: the first differing frame of the block and the object tapped there."""
    lo, hi = block * gen.BLOCK, min((block + 1) * gen.BLOCK, got.shape[0])
    msg = "fuzz profile %d seed %d: block %d (frames %d..%d) differs; channel 1 taps object frame %% %d there (all of 0..%d)" % (
        profile, seed, block, lo, hi - 1, nobj, nobj - 1)
    if os.path.exists(gen.EXE):
        ref, _ = gen.run_reference(profile, seed, got.shape[0])
        neq = (ref.view(np.uint64) != got.view(np.uint64)) & ~(np.isnan(ref) & np.isnan(got))
        f1 = np.flatnonzero(neq[:, 1])
        f0 = np.flatnonzero(neq[:, 0])
        if len(f0):
            msg += "; channel 0 first differs at frame %d: %r, reference %r" % (f0[0], got[f0[0], 0], ref[f0[0], 0])
        if len(f1):
            msg += "; channel 1 first differs at frame %d = object %d: %r, reference %r" % (f1[0], f1[0] % nobj, got[f1[0], 1], ref[f1[0], 1])
    return msg


@pytest.mark.parametrize("profile,seed", DIGEST)
def test_digest_seed_every_block_is_the_references(profile, seed, tmp):
    i = DIGEST.index((profile, seed))
    got, _, counts = run_pair(profile, seed, gen.DIGEST_FRAMES[profile], tmp)
    assert got.shape[0] == int(_G["digest_frames"][i])
    d = gen.block_digests(got)
    exp = _G["digests"][i, :len(d)]
    if not np.array_equal(d, exp):
        pytest.fail(_explain(profile, seed, got, int(np.argmax(d != exp)), counts["objects"]))
    names = list(_G["count_names"])
    assert [counts.get(n, 0) for n in names] == _G["counts"][i].tolist(), "the patch drew other events than in the reference build"


@pytest.mark.parametrize("switch", ["MXG_PS_DERIVE", "MXG_PS_ZEROCOPY"])
@pytest.mark.parametrize("profile,seed", CORE)
def test_core_seed_same_bits_with_the_mechanism_off(profile, seed, switch, tmp):
    """Derived arguments off (one launch per call wherever an argument is a signal), and separately zero-copy renders off (short
    blocks through device memory and copy commands): the reference's bits either way."""
    frames = min(MECH_OFF_FRAMES, gen.FRAMES[profile])
    assert frames >= 2000
    exp = _G["core_%d_%d" % (profile, seed)][:frames]
    got, log, wall = run_fz(profile, seed, frames, tmp, total=gen.FRAMES[profile], **{switch: "0"})
    print("profile %d seed %d %s=0: %.2f s" % (profile, seed, switch, wall))
    assert_bits_equal(got, exp, "fuzz profile %d seed %d with %s=0" % (profile, seed, switch))
    if switch == "MXG_PS_DERIVE":
        assert sum(stats(log)["derived"].values()) == 0


def test_fuzz_reaches_the_machinery(tmp):
    """The seed lists enter the states they were written for (read-only counters of the engine, printed by host/dropin_main.cpp):
    asynchronous next blocks served, derived-argument blocks used, rewinds in EVERY pool class, the delay ring's undo."""
    total = None
    for p, s, frames in [(p, s, gen.FRAMES[p]) for p, s in CORE] + [(p, s, gen.DIGEST_FRAMES[p]) for p, s in DIGEST]:
        st = run_pair(p, s, frames, tmp)[1]
        if total is None:
            total = {k: (dict(v) if isinstance(v, dict) else v) for k, v in st.items()}
            continue
        for k, v in st.items():
            if isinstance(v, dict):
                for q in v:
                    total[k][q] += v[q]
            else:
                total[k] += v
    print("over %d runs: %r" % (len(CORE + DIGEST), total))
    slowest = max(walls)
    print("children so far: %d, %.1f s in all, slowest %.2f s (profile %d seed %d %r)" % ((len(walls), sum(w[0] for w in walls)) + slowest))
    for pool in ("osc", "env", "filter", "sample", "filter2", "envgen"):
        assert total["async"][pool] > 0, "no asynchronous block served in the %s pool" % pool
    assert total["async"]["delay"] == 0                      # (a delay line never renders ahead: its ring could not be rewound)
    for pool in ("osc", "env", "filter", "delay", "filter2"):
        assert total["derived"][pool] > 0, "no derived-argument block in the %s pool" % pool
    for pool in ("osc", "env", "filter", "sample", "delay", "filter2", "envgen"):
        assert total["rewinds"][pool] > 0, "no rewind in the %s pool" % pool
        assert total["launches"][pool] > 0
    assert total["undos"] > 0, "the delay pool's undo path never ran"
    for form in range(1, 10):     # x | x*a | x+b | x*a+b | (x+b)*a | x1+x2 | (x1+x2)*a | x1*x2 | ((x+b)*a)+c
        assert total["forms"][form] > 0, "no block was filled from derived-argument form %d" % form
