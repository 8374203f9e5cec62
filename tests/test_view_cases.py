"""The table of tests/view_cases.py is what it says, on the CPU oracle alone.

tests/test_gpu_view_extremes.py compares the kernel with the oracle at these
cameras and parameters; a case whose frame is one colour, or the default
frame over again, would pass there whatever the kernel's shortcuts did with
the parameter. So for every case and both host scenes the oracle's frame must
be of the case's class (view_cases.Case.expect): a `rich` frame has at least
50 distinct RGBA8 colours and differs from the default-parameter frame in at
least 2 % of its pixels (bytes, float bits or step count); the other classes
are exactly the property they name. These are conditions on the inputs: a case
that falls short gets a different camera, never a lower bar.
"""
import numpy as np
import pytest

import view_cases as V


@pytest.fixture(scope="module")
def tex(pkg, oracle):
    sc = pkg.scenes
    return oracle.TextureSet(sc.skybox(256, 128), sc.default_texture_array()[0])


@pytest.fixture(scope="module")
def defaults(pkg, oracle, tex):
    """The default frame by (host, size), read-only."""
    cache = {}

    def get(host, size):
        if (host, size) not in cache:
            out = oracle.render(V.host_scene(pkg, host), V.default_camera(pkg), V.default_params(pkg), *size, tex)
            for a in out:
                a.setflags(write=False)
            cache[(host, size)] = out
        return cache[(host, size)]

    return get


def params_value(case, key):
    return {**V.PARAMS, **case.params}.get(key)


def test_table_shape():
    """Every group, every class and every listed value is in the table; names are unique."""
    assert {c.group for c in V.CASES} == set(V.GROUPS)
    assert {c.expect for c in V.CASES} == set(V.EXPECT)
    assert len({c.name for c in V.CASES}) == len(V.CASES)
    assert all(any(c.group == g and c.finite for c in V.CASES) for g in V.GROUPS)

    def values(group, key):
        return [params_value(c, key) for c in V.CASES if c.group == group]

    def has(vals, want):
        vals, want = [float(np.float32(v)) for v in vals], [float(np.float32(w)) for w in want]  # as the struct holds them
        return all(any((v != v and w != w) or (v == w and np.signbit(v) == np.signbit(w)) for v in vals) for w in want)

    assert has(values("u_f", "u_f"), [0.0, -0.0, -0.01, 1e-40, 0.3, 0.5, 0.6, 0.66, 2.0 / 3.0, 1.0, 2.0, V.INF, V.NAN,
                                      0.01])
    assert has(values("revolutions", "max_revolutions"), [-2, -1, 0, 1, 3, 8, 50])
    assert any(params_value(c, "max_revolutions") == 50 and params_value(c, "max_steps") == 7 for c in V.CASES)
    assert any(params_value(c, "max_revolutions") == -1 and c.params.get("u_f") == 0.2 for c in V.CASES)
    assert has([c.fov for c in V.CASES if c.group == "fov"], [0.0, 1.0, 179.0, 180.0, 181.0, 270.0, 360.0, -90.0,
                                                              V.NAN])
    for t in (2, 3):
        assert has([params_value(c, "curved_percentage") for c in V.CASES
                    if c.group == "split" and params_value(c, "raytrace_type") == t], [-0.5, 0.0, 1.0, 1.5, V.NAN])
    assert has(values("noise", "percent_black"), [0.0, 0.5, 1.0, 2.0, V.NAN])
    assert any(params_value(c, "max_steps") == 65536 and c.size == (16, 8) for c in V.CASES)
    # the cameras at r = 100: the host's own sum (precompute.cpp derive_frame: doubles, <= 1e4)
    r2 = {n: sum(float(np.float32(v)) ** 2 for v in V.BY_NAME[n].pos)
          for n in ("uf_0p01_r100", "uf_0p01_r100_up", "uf_0p01_r100_down")}
    assert r2["uf_0p01_r100_down"] < r2["uf_0p01_r100"] == 1.0e4 < r2["uf_0p01_r100_up"]
    assert float(np.float32(1.0) / np.float32(0.01)) == 100.0  # uf_radius, the other half of win_ok
    assert V.BY_NAME["pos_r1"].pos == (0.0, 0.0, 1.0) and V.BY_NAME["pos_origin"].pos == (0.0, 0.0, 0.0)
    for name, r in (("pos_r1e5_fov2", 1e5), ("pos_r1e15_fov2", 1e15), ("pos_r1e25_fov2", 1e25)):
        c = V.BY_NAME[name]
        assert c.fov == 2.0 and abs(np.linalg.norm(np.array(c.pos, dtype=np.float64)) / r - 1.0) < 1e-6


@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.name)
def test_case_is_of_its_class(pkg, oracle, tex, defaults, case):
    cam, params = V.camera_of(pkg, case), V.params_of(pkg, case)
    for host in V.HOSTS:
        frame = oracle.render(V.host_scene(pkg, host), cam, params, *case.size, tex)
        V.check_expectation(case, frame, defaults(host, case.size), f"{case.name} / {host}")


def test_nonpositive_u_f_is_one_frame_and_not_the_default_u_f(pkg, oracle, tex):
    """u_f in {0, -0, -0.01, 1e-40, NaN}: u < u_f is never true before u < 0
    ends the ray, so the five give one frame - and not the frame u_f = 0.01
    gives from the same camera, which differs in at least 2 % of the pixels
    on both hosts (the rays that reach r = 100)."""
    names = ("uf_0", "uf_m0", "uf_m0p01", "uf_denormal", "uf_nan")
    cam = V.camera_of(pkg, V.BY_NAME[names[0]])
    for host in V.HOSTS:
        scene = V.host_scene(pkg, host)
        frames = [oracle.render(scene, V.camera_of(pkg, V.BY_NAME[n]), V.params_of(pkg, V.BY_NAME[n]), V.W, V.H, tex)
                  for n in names]
        for n, f in zip(names[1:], frames[1:]):
            assert not V.changed(frames[0], f).any(), (host, n)
        ref = oracle.render(scene, cam, V.default_params(pkg), V.W, V.H, tex)
        assert V.changed(frames[0], ref).mean() >= 0.02, (host, float(V.changed(frames[0], ref).mean()))


def test_overshoot_cases_show_the_scene(pkg, oracle, tex):
    """50 revolutions in 7 steps give at most three colours from any camera
    (view_cases.Case.expect), so the class alone says little. The two cases
    together must, on each host, show two step counts on at least 2 % of the
    pixels each and differ from the frame of the hole alone in at least 2 %:
    rays end at different steps and the scene's objects decide where."""
    hole = pkg.scenes.scene_black_hole_only()
    cases = [c for c in V.CASES if c.expect == "overshoot"]
    assert len(cases) == 2
    for host in V.HOSTS:
        ok = []
        for case in cases:
            cam, params = V.camera_of(pkg, case), V.params_of(pkg, case)
            frame = oracle.render(V.host_scene(pkg, host), cam, params, V.W, V.H, tex)
            bare = oracle.render(hole, cam, params, V.W, V.H, tex)
            counts = np.bincount(frame[2].ravel())
            ok.append(int((counts >= 0.02 * frame[2].size).sum()) >= 2 and V.changed(frame, bare).mean() >= 0.02)
        assert any(ok), (host, ok)


def test_negative_revolutions_trace_inward_falling_rays(pkg, oracle, tex):
    """max_revolutions < 0: every step angle is negative, so a lane with
    du < 0 (the kernel's `outward`) moves toward larger u. The frames are
    pictures of the scene: at least 2 % of the pixels of rev_m1 and rev_m2
    differ from the frame of the hole alone."""
    hole = pkg.scenes.scene_black_hole_only()
    for name in ("rev_m1", "rev_m2", "rev_m1_uf0p2"):
        case = V.BY_NAME[name]
        cam, params = V.camera_of(pkg, case), V.params_of(pkg, case)
        bare = oracle.render(hole, cam, params, V.W, V.H, tex)
        for host in V.HOSTS:
            frame = oracle.render(V.host_scene(pkg, host), cam, params, V.W, V.H, tex)
            assert V.changed(frame, bare).mean() >= 0.02, (name, host, float(V.changed(frame, bare).mean()))
