"""The table of tests/extreme_cases.py is what it says, on the CPU oracle alone.

tests/test_gpu_scene_extremes.py compares the kernel with the oracle on
these scenes; a case whose primitive is off screen, hidden or too small for
a 64x40 frame would pass there whatever the culling did. So for every case,
host and step schedule the oracle renders the scene and the same scene
without the primitive, and the primitive must change a minimum share of the
pixels (extreme_cases.MIN_SHARE: 2 % of 2560 pixels, 1 % for the thin
group). These are conditions on the inputs: a case that falls short gets a
closer camera, never a lower share.

The zero-size and non-finite groups, and the primitives whose exact test
accepts nothing by construction (an empty range, an all-zero frame), have no
minimum: there the host scene (scenes.scene_default(False) plus the
primitive, or the 21-object scene) must differ from the frame of the hole
alone, and a primitive that accepts nothing must leave its own frame empty.
"""
import numpy as np
import pytest

import extreme_cases as X


@pytest.fixture(scope="module")
def tex(pkg, oracle):
    sc = pkg.scenes
    return oracle.TextureSet(sc.skybox(256, 128), sc.default_texture_array()[0])


def test_table_shape():
    """Every group and every primitive type is in the table; names are unique."""
    assert {c.group for c in X.CASES} == set(X.MIN_SHARE)
    assert {c.spec["type"] for c in X.CASES} == set(X.TYPE_OF)
    assert len({c.name for c in X.CASES}) == len(X.CASES)
    for group in ("signed", "horizon", "enclosing", "far", "frames"):
        assert any(c.group == group and c.min_share == 0.02 for c in X.CASES)
    assert all(c.min_share == 0.01 for c in X.CASES if c.group == "thin")
    assert all(set(c.schedules) == {"600x2"} for c in X.CASES if c.group == "far")


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_primitive_is_on_screen(pkg, oracle, tex, case):
    cam = X.camera_of(pkg, case)
    for host in case.hosts:
        for schedule in case.schedules:
            params = X.params_of(pkg, case, schedule)
            scene = X.build(pkg, case, host)
            bare = X.without_primitive(pkg, case, host)
            assert bare.num_objects == scene.num_objects - 1
            with_p = oracle.render(scene, cam, params, X.W, X.H, tex)
            without = oracle.render(bare, cam, params, X.W, X.H, tex)
            share = X.changed_share(with_p, without)
            label = f"{case.name} / {host} / {schedule}: the primitive changes {share:.4f} of the frame"
            if case.min_share > 0.0:
                assert share >= case.min_share, label
            else:
                hole = oracle.render(pkg.scenes.scene_black_hole_only(), cam, params, X.W, X.H, tex)
                if host != "alone":
                    assert X.changed_share(with_p, hole) > 0.0, label
                elif case.group != "zero":  # an empty range or a zero frame: the test accepts nothing
                    assert share == 0.0, label


@pytest.mark.parametrize("case", [c for c in X.CASES if c.group == "far"], ids=lambda c: c.name)
def test_far_cases_take_the_reseed_branch(pkg, oracle, tex, case):
    """u_f enters the shader only through the reseed branch (frag:891-912:
    u < u_f, a new orbital frame from the r = 1 / u_f sphere or the flat
    continuation beyond it). With u_f = 1e-6 no ray of these frames takes it
    before it leaves by u < 0, so a pixel whose step count differs between
    the two renders took the branch - among them, where the primitive lies
    beyond r = 1 / u_f, the pixels that show it."""
    cam = X.camera_of(pkg, case)
    cam_r = float(np.linalg.norm(np.array(cam.transform.pos[:3], dtype=np.float64)))
    assert cam_r < 1.0 / case.u_f  # the rays start inside the sphere: the branch is not the start's
    for host in case.hosts:
        for schedule in case.schedules:
            params = X.params_of(pkg, case, schedule)
            never = X.params_of(pkg, case, schedule)
            never.u_f = 1.0e-6
            scene = X.build(pkg, case, host)
            a = oracle.render(scene, cam, params, X.W, X.H, tex)
            b = oracle.render(scene, cam, never, X.W, X.H, tex)
            bare = oracle.render(X.without_primitive(pkg, case, host), cam, params, X.W, X.H, tex)
            took = a[2] != b[2]
            shows = (a[1].view(np.uint32) != bare[1].view(np.uint32)).any(-1)
            assert took.mean() >= 0.02, (case.name, host, took.mean())
            if case.beyond_uf:
                assert (took & shows).mean() >= 0.02, (case.name, host, (took & shows).mean())


def texel_cells():
    import test_gpu_texel_edges as T

    return T.non_vacuous_cells()


@pytest.mark.parametrize("cell", texel_cells(), ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}")
def test_texel_patterns_stop_and_pass_rays(pkg, oracle, cell):
    """tests/test_gpu_texel_edges.py's arrays, on the oracle alone: with the
    pinhole, islands and seam patterns at 7x5 texels and above, at least 2 %
    of a frame's rays stop at the textured rectangle or sphere (alpha exactly
    1) and at least 2 % pass through it, so a wrong opacity classification
    in either direction changes pixels there."""
    import test_gpu_texel_edges as T

    pattern, size, obj = cell
    stop, went = T.stop_pass_shares(pkg, oracle, pkg.scenes.skybox(256, 128), pattern, size, obj, 0, (0, 0, 0))
    assert stop >= 0.02 and went >= 0.02, (cell, stop, went)
