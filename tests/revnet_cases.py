"""The cases of tests/golden/revnet.npz, shared by tools/gen/gen_golden_revnet.py (which runs the reference's maxiReverbFilters
objects over them) and the tests (which regenerate the same inputs and parameters and check their digest against the file).
A case is a network -- parallel combs summed in order into serial allpasses -- with per-voice feedbacks and cutoffs that hold
for the whole case."""
import hashlib

import numpy as np

TILE = 64
RING = 44100
MAX_STAGES = 32
PATCH_FRAMES, PATCH_CHANNELS = 2500, 16

SAT = dict(combs=[778, 901, 1011, 1123], lowpass=[0, 0, 0, 0], aps=[125, 42, 12])
FV_COMBS = [1557, 1617, 1491, 1422, 1277, 1356, 1188, 1116]
FV_APS = [225, 556, 441, 341]
FV = dict(combs=FV_COMBS, lowpass=[1] * 8, aps=FV_APS)
FV31 = dict(combs=FV_COMBS, lowpass=[1] * 8, aps=FV_APS + [13 * (j + 1) for j in range(4, 31)])
WIDE = dict(combs=[64 + 3 * c if c % 4 == 1 else 1 + (7 * c) % 61 for c in range(32)], lowpass=[int(c % 4 == 1) for c in range(32)],
            aps=[1 + (11 * a) % 67 for a in range(32)])

# fb / cut: "fixed" = the constructor values (0.85 / 0.2 / 0.85, FreeVerb's 0.84), or (lo, hi) drawn per voice and stage
CASES = [
    dict(name="sat_like", V=2, N=3000, noise=1800, amp=1.0, seed=31, fb="fixed", keep_rings=False, **SAT),
    dict(name="fv_like", V=1, N=3000, noise=1800, amp=1.0, seed=32, fb="fixed", comb_fb=0.84, keep_rings=False, **FV),
    dict(name="mixed", V=3, N=2000, noise=1400, amp=1.0, seed=33, fb=(-0.7, 0.7), keep_rings=True,
         combs=[1, 64, 63, 65, 2], lowpass=[0, 1, 0, 1, 0], aps=[1, 2, 63, 64, 65, 300]),
    dict(name="ap_only", V=2, N=1500, noise=1000, amp=1.0, seed=34, fb=(-0.9, 0.9), keep_rings=True, combs=[], lowpass=[],
         aps=[7, 129, 64, 1, 30]),
    dict(name="comb_only", V=2, N=1500, noise=1000, amp=1.0, seed=35, fb=(-0.9, 0.9), keep_rings=True, combs=[90, 33, 2],
         lowpass=[1, 0, 0], aps=[]),
    dict(name="wide", V=1, N=1000, noise=700, amp=1.0, seed=36, fb=(-0.3, 0.3), keep_rings=True, **WIDE),
    dict(name="sat_sub", V=1, N=2000, noise=1500, amp=1e-307, seed=37, fb="fixed", keep_rings=False, subnormal=True, **SAT),
]


def topology(case):
    return list(case["combs"]), list(case["aps"]), list(case["lowpass"])


def layout(combs, aps):
    """offsets [P + A] and the ring doubles per voice, written out here independently of mxg_revfilt.h."""
    lens = list(combs) + list(aps)
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(lens)[:-1]])] if lens else []
    return offs, int(sum(lens))


def inputs(case):
    """x [N][V], comb_fb [V][P], comb_cut [V][P], ap_fb [V][A]."""
    N, V, P, A = case["N"], case["V"], len(case["combs"]), len(case["aps"])
    rng = np.random.default_rng(case["seed"])
    x = rng.uniform(-1.0, 1.0, (N, V)) * case["amp"]
    x[case["noise"]:] = 0.0   # the tail
    x[500:650] = 0.0          # a silent stretch inside the noise
    if case["fb"] == "fixed":
        comb_fb = np.full((V, P), case.get("comb_fb", 0.85))
        comb_cut = np.full((V, P), 0.2)
        ap_fb = np.full((V, A), 0.85)
    else:
        lo, hi = case["fb"]
        comb_fb = rng.uniform(lo, hi, (V, P))
        comb_cut = rng.uniform(0.0, 1.0, (V, P))
        ap_fb = rng.uniform(lo, hi, (V, A))
    return np.ascontiguousarray(x), comb_fb, comb_cut, ap_fb


def inputs_digest(case, x, comb_fb, comb_cut, ap_fb):
    h = hashlib.sha256()
    combs, aps, lowp = topology(case)
    for a in (np.asarray(combs, np.int64), np.asarray(aps, np.int64), np.asarray(lowp, np.int64), x, comb_fb, comb_cut, ap_fb):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
