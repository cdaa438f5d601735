"""The cases of tests/golden/reverb.npz, shared by tools/gen/gen_golden_reverb.py (which runs the reference over them) and the
tests (which regenerate the same inputs and check their digest against the file).  Also the topology of the three classes,
written out here a second time -- independent of maximilian_amd/csrc/mxg_reverb.h, which the tests compare with it."""
import hashlib

import numpy as np

SAT, FREEVERB, STEREO = 0, 1, 2
NCOMB = {SAT: 4, FREEVERB: 8, STEREO: 8}
CHANNELS = {SAT: 1, FREEVERB: 1, STEREO: 2}
_FV_COMBS = [1557, 1617, 1491, 1422, 1277, 1356, 1188, 1116]
_FV_AP = [225, 556, 441, 341]
LENGTHS = {
    SAT: [778, 901, 1011, 1123] + [125, 42, 12],
    FREEVERB: _FV_COMBS + _FV_AP + [13 * (j + 1) for j in range(4, 31)],
    STEREO: _FV_COMBS + _FV_AP,
}
RING_DOUBLES = {SAT: 3992, FREEVERB: 18905, STEREO: 12587}
PATCH_FRAMES = 6000


def layout(kind):
    lens = LENGTHS[kind]
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    assert sum(lens) == RING_DOUBLES[kind]
    return lens, offs, sum(lens)


# params: "none" (play(x) only), "block" (one value per voice), "ps" (one per sample, beyond both clamps);
# modes: "play", "params", or "alt" (the two overloads alternating on one object in runs of 1 .. 200 samples)
CASES = [
    dict(name="sat", kind=SAT, V=2, N=6000, noise=3600, amp=1.0, params="none", modes="play", seed=11, keep_rings=True),
    dict(name="fv_play", kind=FREEVERB, V=1, N=6500, noise=4000, amp=1.0, params="none", modes="play", seed=12),
    dict(name="fv_params", kind=FREEVERB, V=2, N=6500, noise=4000, amp=1.0, params="block", modes="params", seed=13),
    dict(name="fv_alt", kind=FREEVERB, V=2, N=6500, noise=4000, amp=1.0, params="ps", modes="alt", seed=14, clamps=True),
    dict(name="fv_ps", kind=FREEVERB, V=1, N=6000, noise=4000, amp=1.0, params="ps", modes="params", seed=15, clamps=True),
    dict(name="stereo", kind=STEREO, V=1, N=6000, noise=3600, amp=1.0, params="block", modes="play", seed=16),
    dict(name="sat_sub", kind=SAT, V=1, N=6000, noise=4000, amp=1e-307, params="none", modes="play", seed=17, subnormal=True),
    dict(name="fv_sub", kind=FREEVERB, V=1, N=6000, noise=4000, amp=1e-307, params="block", modes="alt", seed=18, subnormal=True),
    dict(name="stereo_sub", kind=STEREO, V=1, N=6000, noise=4000, amp=1e-307, params="none", modes="play", seed=19, subnormal=True),
]


def inputs(case):
    """x [N][V], mode int32 [N], room [N][V], absorb [N][V] (block-rate parameters: every row the same)."""
    N, V = case["N"], case["V"]
    rng = np.random.default_rng(case["seed"])
    x = rng.uniform(-1.0, 1.0, (N, V)) * case["amp"]
    x[case["noise"]:] = 0.0                       # the tail
    x[1000:1300] = 0.0                            # a silent stretch inside the noise
    if case["params"] == "ps":
        room = rng.uniform(-21.0, 3.0, (N, V))
        absorb = rng.uniform(-1.5, 1.5, (N, V))
    elif case["params"] == "block":
        room = np.broadcast_to(rng.uniform(-6.0, 1.5, V), (N, V)).copy()
        absorb = np.broadcast_to(rng.uniform(0.05, 0.9, V), (N, V)).copy()
    else:
        room, absorb = np.zeros((N, V)), np.zeros((N, V))
    if case["modes"] == "alt":
        mode = np.zeros(N, np.int32)
        n, m = 0, 0
        while n < N:
            run = int(rng.choice([1, 1, 2, 7, 63, 64, 65, 200]))
            mode[n:n + run] = m
            n, m = n + run, 1 - m
    else:
        mode = np.full(N, 1 if case["modes"] == "params" else 0, np.int32)
    return np.ascontiguousarray(x), mode, np.ascontiguousarray(room), np.ascontiguousarray(absorb)


def inputs_digest(x, mode, room, absorb):
    h = hashlib.sha256()
    for a in (x, mode, room, absorb):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def runs(mode):
    """[(start, stop, mode)] for the runs of equal mode."""
    edges = np.flatnonzero(np.diff(mode)) + 1
    starts = np.concatenate([[0], edges])
    stops = np.concatenate([edges, [len(mode)]])
    return [(int(a), int(b), int(mode[a])) for a, b in zip(starts, stops)]
