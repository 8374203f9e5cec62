"""The sequences of tests/sequence_cases.py tell their frames apart (oracle alone).

tests/test_gpu_sequence.py compares every frame of a sequence launch with the
oracle's frame of that frame's own scene. That comparison catches a kernel
which read a neighbouring frame's scene only if the neighbours' frames
differ, so for the camera "view" any two frames of a sequence must differ on
at least 1 % of the pixels at every size the GPU tests render it at.

The minima over all pairs, at 400 steps:

  MIX      68x44 100 of 2992 (3.3 %)   33x17 25 (4.5 %)   17x11 6 (3.2 %)
  GEO8     68x44 120 (4.0 %)           17x11 7 (3.7 %)
  SHADE8   68x44 411 (13.7 %)          17x11 27 (14.4 %)
  ORBIT40  68x44 385 (12.9 %)          17x11 23 (12.3 %)
"""
import pytest

from sequence_cases import MIX, NAMES, SIZES, Sequences, min_pair_difference


@pytest.fixture(scope="module")
def sq(pkg, oracle, textures):
    return Sequences(pkg, oracle, textures)


def test_lengths(sq, pkg):
    assert [len(sq.scenes(n)) for n in NAMES] == [len(MIX), 8, 8, 40]
    assert len(sq.scenes("ORBIT40")) > pkg.abi.MAX_BATCH  # a window of it fills a launch, one more is refused


@pytest.mark.parametrize("name,size", [(n, s) for n in NAMES for s in SIZES[n]],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_any_two_frames_differ(sq, name, size):
    w, h = size
    d, pair = min_pair_difference(sq, name, w, h)
    print(f"{name} {w}x{h}: frames {pair} differ on {d} of {w * h} pixels ({100.0 * d / (w * h):.1f} %)")
    assert 100 * d >= w * h, f"{name} {w}x{h}: frames {pair} differ on {d} of {w * h} pixels only"


def test_geo8_and_shade8_change_what_they_say(sq, pkg):
    """GEO8 moves spheres[0] alone (geometry); SHADE8 changes shading-only fields alone."""
    abi = pkg.abi
    geo, shade = sq.scenes("GEO8"), sq.scenes("SHADE8")
    assert all(not abi.scene_shading_only(geo[0], s) for s in geo[1:])
    assert all(abi.scene_shading_only(shade[0], s) for s in shade[1:])
