"""The inputs of tests/test_gpu_phase.py can tell implementations apart (CPU,
the oracle alone).

A phase (i, j) of an ss x ss grid is S[j::ss, i::ss] of the oracle's (ss W) x
(ss H) sample frame S. For every cell of the GPU tests and ss 2 .. 4, any two
distinct phases of S differ on at least 50 % of the pixels: an implementation
that ignores or swaps (i, j) cannot pass there. (A phase need not differ from
the plain frame: at 17x11 the centre phase (1, 1) of ss 3 is the plain frame,
byte for byte, on all five cells.)
"""
import itertools

import pytest

from test_gpu_launch_matrix import World
from test_gpu_supersample import CELL_IDS, CELLS, H, STEPS, W

MIN_DIFFERENT = 0.5


@pytest.fixture(scope="module")
def wd(pkg, oracle, textures):
    return World(pkg, oracle, textures)


def check_phases_differ(S, ss, label):
    phases = {(i, j): S[j::ss, i::ss] for j in range(ss) for i in range(ss)}
    worst = min((float((phases[a] != phases[b]).any(-1).mean()), a, b)
                for a, b in itertools.combinations(sorted(phases), 2))
    print(f"{label}: the closest two phases {worst[1]}, {worst[2]} differ on {worst[0]:.1%} of the pixels")
    assert worst[0] >= MIN_DIFFERENT, (label, worst)


@pytest.mark.parametrize("ss", [2, 3, 4])
@pytest.mark.parametrize("key,overlay", CELLS, ids=CELL_IDS)
def test_phases_of_a_cell_differ(wd, key, overlay, ss):
    S = wd.ref(key, overlay, "view", ss * W, ss * H, STEPS)[0]
    assert S.shape == (ss * H, ss * W, 4)
    check_phases_differ(S, ss, f"{key}, overlay {overlay}, ss {ss}")


def test_phases_of_the_larger_cell_differ(wd):
    S = wd.ref("small", False, "view", 2 * 68, 2 * 44, 400)[0]
    check_phases_differ(S, 2, "small, 68x44, ss 2")
