"""The premise of the shutter-frame tests, held with the CPU oracle alone.

tests/test_gpu_shutter.py compares every frame of a shutter call with
shutter_cases' reference. That catches a wrong kernel only if the wrong frames
it could produce differ from the right one: for every case, at 68x44 and 400
steps, each output frame differs on at least 10 % of the pixels from the same
group shifted by one sub-frame, from each of its own sub-frames alone, from the
still frame (every sub-frame the group's first scene and camera) and from the
next output frame.
"""
import numpy as np
import pytest

from shutter_cases import PREMISE, Shutter
from test_gpu_launch_matrix import H, W

CASES = ("view_k4_ss2", "view_k3_ss1", "flyby_k4_ss2", "own_k4_ss2", "mix_k2_ss1")


@pytest.fixture(scope="module")
def sh(pkg, oracle, textures):
    return Shutter(pkg, oracle, textures)


@pytest.mark.parametrize("name", CASES)
def test_premise(sh, name):
    case = sh.case(name)
    rows = sh.premise(case, W, H)
    assert len(rows) == case.M
    for m, (shifted, own, still, nxt) in enumerate(rows):
        print(f"{name} frame {m}: shifted {shifted:.3f} own sub-frame {own:.3f} still {still:.3f} next "
              f"{'-' if nxt is None else format(nxt, '.3f')}")
        assert shifted >= PREMISE, f"{name} frame {m}: the group shifted by one sub-frame differs on {shifted:.1%} only"
        assert own >= PREMISE, f"{name} frame {m}: one of its sub-frames alone differs on {own:.1%} only"
        assert still >= PREMISE, f"{name} frame {m}: the still frame differs on {still:.1%} only"
        assert nxt is not None and nxt >= PREMISE, f"{name} frame {m}: the next frame differs on {nxt} only"


def test_reference_is_the_rule(sh):
    """The reference's own arithmetic: K equal sub-frames resolve to themselves,
    and the rounding is half up."""
    a = np.arange(256, dtype=np.uint8).reshape(8, 8, 4)
    for k in (1, 2, 3, 32):
        assert np.array_equal(sh.resolve([a] * k), a)
    lo, hi = np.zeros((1, 1, 4), np.uint8), np.full((1, 1, 4), 1, np.uint8)
    assert sh.resolve([lo, hi]).max() == 1 and sh.resolve([lo, lo, hi]).max() == 0
    assert sh.resolve([np.full((1, 1, 4), 255, np.uint8)] * 32).min() == 255


def test_default_phases_are_the_progressive_order(sh, pkg):
    case = sh.case("view_k4_ss2")
    order = pkg.abi.phase_order(2)
    ph = sh.phases(case)
    assert ph.shape == (16, 2)
    for j in range(16):
        assert tuple(ph[j]) == order[j % 4]
