"""The pairs of tests/reshade_cases.py on the oracle alone: are they what the
GPU test needs them to be?

- B differs from A in shading-only fields at most (sr_scene_shading_only) and
  the two scenes are not equal;
- the oracle's frames of A (its own background) and of B (background B)
  differ on more than 10 % of the pixels, for every camera and every sample
  grid the GPU test launches (on the box-resolved frame for ss > 1): a
  reshade that wrote the retained frame's old colours, or nothing, cannot
  equal the oracle's frame of B.
"""
import numpy as np
import pytest

import reshade_cases as R
import shading_cases as S


@pytest.fixture(scope="module")
def pairs(pkg, oracle, textures):
    return R.Pairs(pkg, oracle, textures)


@pytest.mark.parametrize("pair", R.PAIRS, ids=[p["id"] for p in R.PAIRS])
def test_pair_changes_the_frame(pkg, pairs, pair):
    a, b = pairs.scene("A", pair["key"]), pairs.scene("B", pair["key"])
    assert pkg.abi.scene_shading_only(a, b)
    assert not np.array_equal(pkg.scenes.struct_bytes(a), pkg.scenes.struct_bytes(b))
    assert pairs.bg_b.shape != pairs.bg_a.shape
    for cam in pair["cams"]:
        for ss in pair["ss"]:
            share = R.changed_share(pairs.resolved("A", pair, cam, ss), pairs.resolved("B", pair, cam, ss))
            print(f"MEASURED {pair['id']} {cam} ss {ss}: {share:.1%} of the pixels differ")
            assert share > R.MIN_CHANGED, (pair["id"], cam, ss, share)


def test_phase_images_change(pairs):
    """sr_render_phase's images of the kinds pair (ss 2): each of the four
    phases differs between A and B as the whole frame does."""
    pair = R.KIND_PAIR
    sa, sb = pairs.frame("A", pair, "view", 2)[0], pairs.frame("B", pair, "view", 2)[0]
    for j in range(2):
        for i in range(2):
            assert R.changed_share(sa[j::2, i::2], sb[j::2, i::2]) > R.MIN_CHANGED, (i, j)


@pytest.mark.parametrize("names", R.SHADING_PAIRS, ids=[f"{a}->{b}" for a, b in R.SHADING_PAIRS])
def test_shading_pair(pkg, pairs, names):
    a, b = (S.BY_NAME[n] for n in names)
    sa, sb = S.build(pkg, a), S.build(pkg, b)
    assert pkg.abi.scene_shading_only(sa, sb), "the two cases differ in a geometry field"
    assert not np.array_equal(pkg.scenes.struct_bytes(sa), pkg.scenes.struct_bytes(sb))
    for x, y in ((a, b),):
        assert (x.camera, x.params, x.textures, x.specs) == (y.camera, y.params, y.textures, y.specs)
    share = R.changed_share(pairs.shading_frame("A", names[0])[0], pairs.shading_frame("B", names[1])[0])
    print(f"MEASURED {names[0]} -> {names[1]}: {share:.1%} of the pixels differ")
    assert share > R.MIN_CHANGED, share
