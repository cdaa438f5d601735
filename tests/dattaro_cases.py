"""The cases of tests/golden/dattaro.npz, shared by tools/gen/gen_golden_dattaro.py (which runs the reference over them) and
the tests (which regenerate the same inputs and check their digest against the file).  Also the length rule of
maxiDattaroReverb, written out here a second time in numpy -- independent of maximilian_amd/csrc/mxg_dattaro.h, which the
tests compare with it."""
import hashlib

import numpy as np

RINGS, TAPS, STATE = 10, 14, 5
# ring order of a voice: AP0 AP1 | AP4 AP5 AP6 AP7 | D0 D1 D2 D3, lengths at 29.8 kHz
ORIG_LEN = [142, 107, 908, 2656, 672, 1800, 4217, 3163, 4453, 3720]
ORIG_TAP = [266, 2974, 1913, 1996, 1990, 187, 1066, 353, 3627, 1228, 2673, 2111, 335, 121]
TAP_RING = [6, 6, 3, 7, 8, 5, 9, 8, 8, 5, 9, 6, 3, 7]
MAX_LEN = 44100
TILE = 64
RATES = [8000, 22050, 44100, 48000, 96000]
# the issue's check values (compiled from the unmodified reference): D0..D3, fbap[0..7] and the tap positions at 44 100 Hz,
# D and fbap at 48 000 Hz
CHECK_44100 = dict(D=[6240, 4680, 6589, 5505], fbap=[210, 158, 560, 409, 1343, 3930, 994, 2663],
                   taps=[393, 4401, 2830, 2953, 2944, 276, 1577, 522, 5367, 1817, 3955, 3123, 495, 179])
CHECK_48000 = dict(D=[6792, 5094, 7172, 5991], fbap=[228, 172, 610, 446, 1462, 4278, 1082, 2899])
PATCH_FRAMES = 5000


def scale(orig, sample_rate):
    """floor(((float)orig / 29.8f) * ((float)sampleRate / 1000.0f)) in float32, for an array of rates."""
    sr = np.asarray(sample_rate, np.float32)
    return np.floor((np.float32(orig) / np.float32(29.8)) * (sr / np.float32(1000.0))).astype(np.int64)


def lengths(sample_rate):
    return [int(scale(o, sample_rate)) for o in ORIG_LEN]


def taps(sample_rate):
    return [int(scale(o, sample_rate)) for o in ORIG_TAP]


def layout(sample_rate):
    lens = lengths(sample_rate)
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    return lens, offs, sum(lens)


def accepted(rates):
    """The acceptance rule over an array of integer rates: every length in [2, 44100], a 64-sample tile legal on the eight
    tank rings (64 <= D) and on all taps (D - 1 - p is 0 or >= 64)."""
    rates = np.asarray(rates)
    L = np.stack([scale(o, rates) for o in ORIG_LEN])
    T = np.stack([scale(o, rates) for o in ORIG_TAP])
    ok = ((L >= 2) & (L <= MAX_LEN)).all(axis=0) & (L[2:] >= TILE).all(axis=0)
    for j in range(TAPS):
        dist = L[TAP_RING[j]] - 1 - T[j]
        ok &= (dist == 0) | (dist >= TILE)
    return ok


def accepted_ends():
    """(lowest, highest) accepted rate among 1 .. 400 000."""
    r = np.arange(1, 400001)
    a = r[accepted(r)]
    return int(a.min()), int(a.max())


# signal: "impulse" (one sample per voice, the rest silence), "noise" (uniform noise throughout), "tail" (noise, then
# silence for more than twice the longest ring).  blocks: the lengths a bank replays the case in, repeated to the end.
CASES = [
    dict(name="r8000", rate=8000, V=2, N=3500, signal="tail", noise=1000, seed=21, blocks=[1, 63, 64, 65, 512], keep_rings=True),
    dict(name="r22050", rate=22050, V=1, N=8200, signal="tail", noise=1500, seed=22, blocks=[4096, 7, 300]),
    dict(name="r44100", rate=44100, V=1, N=15300, signal="tail", noise=2000, seed=23, blocks=[1, 63, 64, 65, 2, 512, 4096, 7, 1700]),
    dict(name="r48000_impulse", rate=48000, V=1, N=6000, signal="impulse", noise=1, seed=24, blocks=[6000]),
    dict(name="r96000", rate=96000, V=1, N=5000, signal="noise", noise=5000, seed=25, blocks=[777, 64]),
    dict(name="low_end", rate=None, end=0, V=1, N=1500, signal="impulse", noise=1, seed=26, blocks=[1500]),
    # (at the high end the first taps answer after some 8 200 samples on the right and 12 300 on the left)
    dict(name="high_end", rate=None, end=1, V=1, N=13000, signal="noise", noise=13000, seed=27, blocks=[100, 1400]),
]


def case_rate(case):
    return case["rate"] if case["rate"] is not None else accepted_ends()[case["end"]]


def inputs(case):
    """x [N][V]"""
    N, V = case["N"], case["V"]
    rng = np.random.default_rng(case["seed"])
    x = rng.uniform(-1.0, 1.0, (N, V))
    if case["signal"] == "impulse":
        x[1:] = 0.0
    else:
        x[case["noise"]:] = 0.0
    return np.ascontiguousarray(x)


def inputs_digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def block_edges(case):
    """[(start, stop)] of the blocks a bank replays the case in."""
    out, n, k = [], 0, 0
    while n < case["N"]:
        ln = case["blocks"][k % len(case["blocks"])]
        out.append((n, min(n + ln, case["N"])))
        n, k = out[-1][1], k + 1
    return out
