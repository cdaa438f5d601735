"""CPU (-m "not gpu"): the host build of maximilian_amd/csrc/mxg_revfilt.h (tests/host_revnet.cpp).
Its step-by-step walk of a network reproduces every network case of tests/golden/revnet.npz (arrays of the unmodified reference's
maxiReverbFilters objects) -- output, ring contents, indices, low-pass states -- bit for bit; block boundaries do not matter; and
the tile replay the kernel is built on (sub-tiles on short rings, the wrap, the index advance, the low-pass walk over a tile's
reads) equals the walk over random topologies whose lengths include 1, 2, 63, 64 and 65."""
import numpy as np
import pytest

import revnet_cases as rc
import revnet_host as rh
from conftest import assert_bits_equal


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return rh.build(tmp_path_factory.mktemp("revnet"))


@pytest.fixture(scope="module")
def g():
    return rh.load_golden()


def test_golden_file_holds_every_case(g):
    assert [str(n) for n in g["cases"]] == [c["name"] for c in rc.CASES]
    assert "maxiReverb.cpp" in str(g["provenance"]) and "sha256" in str(g["provenance"])
    assert g["patch"].shape == (rc.PATCH_FRAMES, rc.PATCH_CHANNELS)
    assert int(g["sat_sub/n_subnormal"]) >= 100


@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_walk_reproduces_the_reference(host, g, case):
    net, x = rh.case_net(case, g)
    got = rh.host_render(host, net, x)
    assert_bits_equal(got, g[case["name"] + "/out"], case["name"] + ": output")
    rh.check_case_state(case, g, net.rings, net.idx, net.lp, case["name"])


def test_block_boundaries_do_not_matter(host, g):
    case = next(c for c in rc.CASES if c["name"] == "mixed")
    net, x = rh.case_net(case, g)
    got, n = [], 0
    for size in (1, 63, 64, 65, 512, len(x)):
        blk = np.ascontiguousarray(x[n:n + size])
        got.append(rh.host_render(host, net, blk))
        n += len(blk)
    assert n == len(x)
    assert_bits_equal(np.concatenate(got), g["mixed/out"], "mixed, in blocks: output")
    rh.check_case_state(case, g, net.rings, net.idx, net.lp, "mixed, in blocks")


def random_topology(rng):
    special = [1, 2, 63, 64, 65]
    P, A = int(rng.integers(0, 7)), int(rng.integers(0, 7))
    if P + A == 0:
        A = 1
    combs = [int(rng.choice(special)) if rng.random() < 0.6 else int(rng.integers(1, 200)) for _ in range(P)]
    aps = [int(rng.choice(special)) if rng.random() < 0.6 else int(rng.integers(1, 200)) for _ in range(A)]
    lowp = [int(d >= rc.TILE and rng.random() < 0.6) for d in combs]
    return combs, aps, lowp


def test_tile_replay_equals_the_walk(host):
    rng = np.random.default_rng(2030)
    seen = set()
    for trial in range(60):
        combs, aps, lowp = random_topology(rng)
        if trial == 0:   # every special length as a comb, as a low-pass comb where it may be one, and as an allpass
            combs, lowp, aps = [1, 2, 63, 64, 65, 64, 65], [0, 0, 0, 0, 0, 1, 1], [1, 2, 63, 64, 65]
        seen.update(combs + aps)
        V = 2
        N = int(rng.choice([1, 63, 64, 65, 130, 200]))
        fb = rng.uniform(-1.2, 1.2, (V, len(combs)))
        cut = rng.uniform(-0.3, 1.3, (V, len(combs)))
        apf = rng.uniform(-1.2, 1.2, (V, len(aps)))
        a = rh.Net(V, combs, aps, lowp, fb, cut, apf).randomise(rng)
        if trial % 5 == 1:
            a.idx[0, :] = -3          # stored indices outside their rings restart at 0
            a.idx[1, :] = 1 << 20
        b = rh.Net(V, combs, aps, lowp, fb, cut, apf)
        b.rings, b.idx, b.lp = a.rings.copy(), a.idx.copy(), a.lp.copy()
        x = rng.uniform(-1, 1, (N, V))
        what = "combs %s low-pass %s allpasses %s N=%d" % (combs, lowp, aps, N)
        for blk in (x, np.ascontiguousarray(x[:37])):   # a second block continues from where the first one stopped
            exp = rh.host_render(host, a, blk)
            got, collisions = rh.host_tiled(host, b, blk)
            assert collisions == 0, what
            assert_bits_equal(got, exp, what + ": output")
            rh.assert_state_equal(b.parts(), a.parts(), what)
    assert {1, 2, 63, 64, 65} <= seen
