"""CPU: the seeded random patch tests/patches/fuzz_patch.cpp and its expected streams tests/golden/dropin_fuzz.npz (written by
tools/gen/gen_golden_fuzz.py from oracle/_ref/example_fz, the patch linked with the UNMODIFIED reference).  Where oracle/_ref/ is
present the reference build must reproduce every stored stream and digest bit for bit; the conditions the generator chose the seed
lists under are recomputed from the stored file either way, so a regenerated file cannot quietly drop them.  (That the patch compiles
against include/maximilian.h in the three failure modes is tests/test_dropin_cpu.py::test_header_builds_in_every_failure_mode.)"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("gen_golden_fuzz", os.path.join(ROOT, "tools", "gen", "gen_golden_fuzz.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def _exe():
    if not os.path.exists(gen.EXE):
        pytest.skip("oracle/_ref/example_fz not built (needs the reference sources at build time)")
    return gen.EXE


def test_reference_reproduces_core_streams(golden):
    _exe()
    g = golden("dropin_fuzz.npz")
    assert len(g["core_pairs"]) >= 10
    for p, s in g["core_pairs"]:
        exp = g["core_%d_%d" % (p, s)]
        got, _ = gen.run_reference(int(p), int(s), exp.shape[0])
        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), "profile %d seed %d" % (p, s)


def test_reference_reproduces_digests_and_counts(golden):
    _exe()
    g = golden("dropin_fuzz.npz")
    names = list(g["count_names"])
    for i, (p, s) in enumerate(g["digest_pairs"]):
        frames = int(g["digest_frames"][i])
        got, counts = gen.run_reference(int(p), int(s), frames)
        d = gen.block_digests(got)
        assert np.array_equal(d, g["digests"][i, :len(d)]), "profile %d seed %d: first differing block %d" % (
            p, s, int(np.argmax(d != g["digests"][i, :len(d)])))
        assert [counts.get(n, 0) for n in names] == g["counts"][i].tolist(), "profile %d seed %d: the patch's counts" % (p, s)


def test_same_seed_same_bytes_other_seed_other_bytes():
    _exe()
    a, _ = gen.run_reference(0, 7, 3000)
    b, _ = gen.run_reference(0, 7, 3000)
    c, _ = gen.run_reference(0, 8, 3000)
    d, _ = gen.run_reference(1, 7, 3000)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != c.tobytes() and a.tobytes() != d.tobytes()


def test_event_log_does_not_change_the_stream():
    """MXG_FUZZ_LOG=1 (one line per event, for minimising a failing seed) only prints."""
    _exe()
    a, _ = gen.run_reference(2, 5, 2000)
    b, _ = gen.run_reference(2, 5, 2000, extra_env={"MXG_FUZZ_LOG": "1"})
    assert a.tobytes() == b.tobytes()


def test_golden_file_meets_the_generators_conditions(golden):
    g = golden("dropin_fuzz.npz")
    core, dig = g["core_pairs"], g["digest_pairs"]
    assert len(core) >= 10 and len(dig) >= 64
    assert set(dig[:, 0].tolist()) == {0, 1, 2, 3} and set(core[:, 0].tolist()) == {0, 1, 2, 3}
    assert len({tuple(x) for x in dig.tolist()}) == len(dig) and len({tuple(x) for x in core.tolist()}) == len(core)
    for p, s in core:
        st = g["core_%d_%d" % (p, s)]
        assert st.shape == (gen.FRAMES[int(p)], 2) and st.dtype == np.float64
        ok, why = gen.stream_ok(st)
        assert ok, "core profile %d seed %d: %s" % (p, s, why)
    assert (g["digest_finite"] >= gen.MIN_FINITE).all()
    assert (g["digest_peak"] >= gen.PEAK_LO).all() and (g["digest_peak"] <= gen.PEAK_HI).all()
    assert g["digest_frames"].tolist() == [gen.DIGEST_FRAMES[int(p)] for p, _ in dig]
    assert gen.FRAMES[2] % 1024 != 0 and gen.DIGEST_FRAMES[2] % 1024 != 0  # profile 2: no multiple of its bufferSize
    assert gen.DIGEST_FRAMES[3] - 500 - 1000 >= 1500 and min(gen.DIGEST_FRAMES.values()) >= 2000
    nblocks = (g["digest_frames"] + gen.BLOCK - 1) // gen.BLOCK
    for i, n in enumerate(nblocks):
        assert (g["digests"][i, :n] != 0).all()
    # no more than one drawn seed in four skipped, and the skipped ones are on record
    drawn, skipped = int(g["drawn"]), g["skipped"]
    assert drawn == len(core) + len(dig) + len(skipped) and len(skipped) <= gen.MAX_SKIPPED * drawn
    assert ("skipped %d" % len(skipped)) in str(g["provenance"]) and "sha256" in str(g["provenance"])
    # every event kind >= 20 times, every class / method / operator in >= 3 seeds
    assert gen.coverage_problems(g["count_names"], g["counts"]) == []
    names = list(g["count_names"])
    for need in gen.EVENT_NAMES + ["phasor", "saw", "triangle", "square", "pulse", "impulse", "phasorBetween", "sinebuf", "sinebuf4", "sawn",
                                   "noise", "phaseReset", "lores", "hires", "bandpass", "lopass", "hipass", "adsr", "adsr2", "ar",
                                   "setAttack", "setDecay", "setSustain", "setRelease", "setCutoff", "setResonance", "envMember", "dl",
                                   "dlFromPosition", "play", "playOnce", "playAtSpeed", "playAtSpeedBetweenPoints", "play4", "trigger",
                                   "setPosition", "svf", "svfSet", "biquad", "biquadSet", "dcblocker", "envgen", "flange", "chorus",
                                   "copyAssign", "copyTemp", "vecGrow", "vecShrink", "reconstruct", "skip", "twice", "groups"] + [
                                       "op%d" % k for k in range(9)]:
        assert need in names, need
    # the fx classes in one profile only
    fx = g["counts"][:, names.index("flange")] + g["counts"][:, names.index("chorus")]
    assert (fx[dig[:, 0] != 2] == 0).all() and (fx[dig[:, 0] == 2] > 0).any()
