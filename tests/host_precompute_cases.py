"""The inputs of tests/test_host_precompute.py and of the script that recorded
its digests (tests/golden/make_host_precompute_digests.py): every scene the
generators and the case tables of this suite yield, three test rays, the
camera / params rows of view_cases on two scenes, and the texture arrays of
test_gpu_texel_edges. Host only."""
import hashlib

import numpy as np

import extreme_cases as X
import pick_cases as P
import shading_cases as S
import test_gpu_texel_edges as T
import view_cases as V


def scenes(pkg):
    """[(id, Scene)]"""
    sc = pkg.scenes
    out = [
        ("gen/default-textured", sc.scene_default(True)),
        ("gen/default", sc.scene_default(False)),
        ("gen/black-hole-only", sc.scene_black_hole_only()),
        ("gen/stress", sc.scene_stress()),
        ("gen/features", sc.scene_features()),
        ("gen/random-7-8", sc.scene_random(7, n_objects=8, translucent=False, planes=False)),
        ("gen/random-11-21", sc.scene_random(11, n_objects=21, translucent=True, planes=True)),
        ("gen/random-11-21-opaque", sc.scene_random(11, n_objects=21, translucent=False)),
    ]
    out += [(f"gen/random-{seed}", sc.scene_random(seed)) for seed in range(6)]
    for c in X.CASES:
        out += [(f"extreme/{c.name}/{h}", X.build(pkg, c, h)) for h in c.hosts]
    out += [(f"texel/{k}", X.scene_alone(pkg, spec)) for k, spec in X.TEXEL_OBJECTS.items()]
    for c in S.CASES:
        out += [(f"shading/{c.name}/{h}", S.build(pkg, c, h)) for h in c.hosts]
    for c in P.cases(pkg):
        out.append((f"pick/{c['id']}", c["scene"]))
        out += [(f"pick/{c['id']}/pass{k}", s) for k, s in enumerate(P.recoloured(pkg, c["scene"], c["flags"]))]
    assert len({k for k, _ in out}) == len(out)
    return out


def press_r_test_ray(pkg):
    """The press-R polyline of the launch matrix (tests/test_gpu_launch_matrix.py World)."""
    sc, abi = pkg.scenes, pkg.abi
    cam0 = sc.camera_look((1.0, 3.0, 16.0), (0.18, -0.1, -1.0))
    fwd = list(cam0.transform.axes[6:9])
    pts = abi.test_ray_points(list(cam0.transform.pos), fwd, 600, 2)[:abi.MAX_POINTS]
    tr = abi.default_test_ray()
    tr.visible = 1
    tr.num_curved_points = len(pts)
    for i, p in enumerate(pts):
        tr.curved_points[i][0], tr.curved_points[i][1], tr.curved_points[i][2] = p
    for k in range(3):
        tr.flat_origin[k] = cam0.transform.pos[k] + fwd[k]
        tr.flat_dir[k] = fwd[k]
    return tr


def test_rays(pkg):
    """[(id, TestRay)]: the default ray, the launch matrix's press-R polyline,
    the same one hidden, and the bench's 1000-point overlay."""
    hidden = press_r_test_ray(pkg)
    hidden.visible = 0
    return [("default", pkg.abi.default_test_ray()), ("press-r", press_r_test_ray(pkg)), ("press-r-hidden", hidden),
            ("overlay-1000", pkg.scenes.test_ray_overlay())]


def frames(pkg):
    """[(id, host, Camera, Params, width, height, cull, projection)]: every
    view_cases row on the default and the max-capacity scene, and the default
    row with culling off and under the angular projections."""
    abi = pkg.abi
    out = []
    for host in V.HOSTS:
        for c in V.CASES:
            w, h = c.size
            out.append((f"{host}/{c.name}", host, V.camera_of(pkg, c), V.params_of(pkg, c), w, h, True,
                        abi.PROJECTION_RECTILINEAR))
        cam, prm = V.default_camera(pkg), V.default_params(pkg)
        out.append((f"{host}/default/cull-off", host, cam, prm, V.W, V.H, False, abi.PROJECTION_RECTILINEAR))
        out.append((f"{host}/default/equirect", host, cam, prm, V.W, V.H, True, abi.PROJECTION_EQUIRECT))
        out.append((f"{host}/default/fisheye", host, cam, prm, V.W, V.H, True, abi.PROJECTION_FISHEYE))
    assert len({r[0] for r in out}) == len(out)
    return out


def arrays():
    """[(id, texture array)]"""
    return [(name, arr) for name, arr, _, _ in T.ARRAY_CASES]


def digest(status, *buffers) -> str:
    """SHA-256 over the status and, when it is 0, the buffers' bytes."""
    h = hashlib.sha256(np.int32(status).tobytes())
    for b in buffers:
        if b is not None:
            h.update(np.ascontiguousarray(b).tobytes())
    return h.hexdigest()


def compute(pkg) -> dict:
    """{"scenes" | "test_rays" | "frames" | "opacity": {id: digest}} from the loaded library."""
    abi = pkg.abi
    out = {"scenes": {}, "test_rays": {}, "frames": {}, "opacity": {}}
    for name, scene in scenes(pkg):
        out["scenes"][name] = digest(*abi.debug_pack_scene(scene))
    default = pkg.scenes.scene_default(True)
    for name, tr in test_rays(pkg):
        out["test_rays"][name] = digest(*abi.debug_pack_scene(default, tr))
    hosts = {h: V.host_scene(pkg, h) for h in V.HOSTS}
    for name, host, cam, prm, w, h, cull, proj in frames(pkg):
        out["frames"][name] = digest(*abi.debug_frame(hosts[host], None, cam, prm, w, h, cull, proj))
    for name, arr in arrays():
        out["opacity"][name] = digest(0, abi.debug_opacity_bits(arr))
    return out
