"""ctypes mirror of include/sr/sr.h and the loader for libsr.so.

The structs are field-for-field copies of the C-ABI (which itself mirrors the
GLSL uniform block of the reference's assets/shaders/black_hole.frag:15-192);
`check_layout()` compares every size against the compiled library.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "lib" / "libsr.so"

MAX_LIGHTS = 4
MAX_TEXTURES = 10
MAX_MATERIALS = 10
MAX_SPHERES = 3
MAX_PLANES = 3
MAX_DISKS = 3
MAX_HOLLOW_DISKS = 3
MAX_CYLINDERS = 3
MAX_RECTANGLES = 3
MAX_BOXES = 3
MAX_OBJECTS = 21
MAX_POINTS = 1000
# floats per pixel of the integrate -> shade hand-off (csrc/device_scene.h SR_PS_FIELDS)
PS_FIELDS = 4 + 8 * 4 + 16

OBJECT_SPHERE, OBJECT_PLANE, OBJECT_DISK, OBJECT_HOLLOW_DISK = 0, 1, 2, 3
OBJECT_CYLINDER, OBJECT_RECTANGLE, OBJECT_BOX = 4, 5, 6
RAYTRACE_CURVED, RAYTRACE_FLAT, RAYTRACE_HALF_WIDTH, RAYTRACE_HALF_HEIGHT = 0, 1, 2, 3
FILTER_LERP, FILTER_WEIGHTED = 0, 1

SR_OK = 0
SR_E_INVALID = -1
SR_E_CAPACITY = -2
SR_E_HIP = -3
SR_E_NOMEM = -4
SR_E_NOT_READY = -5
SR_E_NO_DEVICE = -6
SR_E_IO = -7

F3 = C.c_float * 3
F9 = C.c_float * 9


class Transform(C.Structure):
    _fields_ = [("pos", F3), ("axes", F9)]


class Camera(C.Structure):
    _fields_ = [("transform", Transform), ("fov", C.c_float)]


class Light(C.Structure):
    _fields_ = [
        ("transform", Transform),
        ("color", F3),
        ("intensity", C.c_float),
        ("attenuation_constant", C.c_float),
        ("attenuation_linear", C.c_float),
        ("attenuation_quadratic", C.c_float),
    ]


class Material(C.Structure):
    _fields_ = [
        ("color", C.c_float * 4),
        ("ambient", C.c_float),
        ("diffuse", C.c_float),
        ("specular", C.c_float),
        ("shininess", C.c_float),
        ("texture_index", C.c_int32),
        ("normal_map_index", C.c_int32),
        ("invert_uv_x", C.c_int32),
        ("invert_uv_y", C.c_int32),
        ("swap_uvs", C.c_int32),
        ("double_sided_normals", C.c_int32),
        ("flip_normals", C.c_int32),
    ]


class Sphere(C.Structure):
    _fields_ = [("transform", Transform), ("radius", C.c_float)]


class Plane(C.Structure):
    _fields_ = [
        ("transform", Transform),
        ("texture_offset", C.c_float * 2),
        ("repeat_texture", C.c_int32),
        ("texture_size", C.c_float * 2),
    ]


class Disk(C.Structure):
    _fields_ = [("plane", Plane), ("radius", C.c_float)]


class HollowDisk(C.Structure):
    _fields_ = [("plane", Plane), ("inner_radius", C.c_float), ("outer_radius", C.c_float)]


class Cylinder(C.Structure):
    _fields_ = [("transform", Transform), ("height", C.c_float), ("radius", C.c_float)]


class Rectangle(C.Structure):
    _fields_ = [("plane", Plane), ("width", C.c_float), ("height", C.c_float)]


class Box(C.Structure):
    _fields_ = [("transform", Transform), ("width", C.c_float), ("depth", C.c_float), ("height", C.c_float)]


class Object(C.Structure):
    _fields_ = [("type", C.c_int32), ("index", C.c_int32), ("material_index", C.c_int32)]


class Scene(C.Structure):
    _fields_ = [
        ("num_objects", C.c_int32),
        ("objects", Object * MAX_OBJECTS),
        ("spheres", Sphere * MAX_SPHERES),
        ("planes", Plane * MAX_PLANES),
        ("disks", Disk * MAX_DISKS),
        ("hollow_disks", HollowDisk * MAX_HOLLOW_DISKS),
        ("cylinders", Cylinder * MAX_CYLINDERS),
        ("rectangles", Rectangle * MAX_RECTANGLES),
        ("boxes", Box * MAX_BOXES),
        ("materials", Material * MAX_MATERIALS),
        ("num_lights", C.c_int32),
        ("lights", Light * MAX_LIGHTS),
        ("texture_sizes", (C.c_float * 2) * MAX_TEXTURES),
        ("max_texture_size", C.c_float * 2),
    ]


class Params(C.Structure):
    _fields_ = [
        ("max_steps", C.c_int32),
        ("max_revolutions", C.c_int32),
        ("u_f", C.c_float),
        ("crosshair", C.c_int32),
        ("raytrace_type", C.c_int32),
        ("curved_percentage", C.c_float),
        ("percent_black", C.c_float),
        ("time", C.c_float),
        ("filter_mode", C.c_int32),
    ]


class TestRay(C.Structure):
    _fields_ = [
        ("visible", C.c_int32),
        ("radius", C.c_float),
        ("extended_length", C.c_float),
        ("curved_color", C.c_float * 4),
        ("flat_color", C.c_float * 4),
        ("flat_origin", F3),
        ("flat_dir", F3),
        ("num_curved_points", C.c_int32),
        ("curved_points", F3 * MAX_POINTS),
    ]


# sr_ray_map_ptrs (sr.h "Ray maps"): device pointers, any of them null; the
# components per pixel and the element type of each map
RAY_MAPS = {"end": (1, "int32"), "id": (1, "int32"), "sky_dir": (3, "float32"), "sky_uv": (2, "float32"),
            "hit_point": (3, "float32"), "hit_normal": (3, "float32"), "hit_view": (3, "float32"),
            "hit_base": (4, "float32"), "hit_step": (1, "int32")}


class RayMapPtrs(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in RAY_MAPS]


# Functions declared in include/sr/sr.h: name -> (restype, argtypes)
_p = C.c_void_p
_i = C.c_int
SIGNATURES = {
    "sr_version": (C.c_char_p, []),
    "sr_status_string": (C.c_char_p, [_i]),
    "sr_params_default": (None, [C.POINTER(Params)]),
    "sr_test_ray_default": (None, [C.POINTER(TestRay)]),
    "sr_scene_clear": (None, [C.POINTER(Scene)]),
    "sr_default_scene": (None, [C.POINTER(Scene)]),
    "sr_default_camera": (None, [C.POINTER(Camera)]),
    "sr_camera_hyperbolic_trajectory": (C.c_int, [C.POINTER(Camera), C.c_float, C.c_float, C.c_float]),
    "sr_create": (_i, [C.POINTER(_p), _i]),
    "sr_destroy": (None, [_p]),
    "sr_set_background": (_i, [_p, _p, _i, _i, _i]),
    "sr_set_texture_array": (_i, [_p, _p, _i, _i, _i, _i]),
    "sr_set_scene": (_i, [_p, C.POINTER(Scene)]),
    "sr_set_test_ray": (_i, [_p, C.POINTER(TestRay)]),
    "sr_render": (_i, [_p, C.POINTER(Camera), C.POINTER(Params), _i, _i, _i, _i, _p, C.c_size_t, _p]),
    "sr_render_blocks": (_i, [_p, C.POINTER(Camera), C.POINTER(Params), _i, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    "sr_render_debug": (_i, [_p, C.POINTER(Camera), C.POINTER(Params), _i, _i, _i, _i, _p, _p, _p, _p]),
    "sr_blocks_row_count": (_i, [_i, _i, _i, _i]),
    "sr_set_split": (_i, [_p, _i, _i, _i]),
    "sr_set_latency_mode": (_i, [_p, _i]),
    "sr_write_png": (_i, [C.c_char_p, _p, _i, _i, C.c_size_t, _i]),
    "sr_render_blocks_batch": (_i, [_p, C.POINTER(Camera), _i, C.POINTER(Params), _i, _i, _i, _i, _i, _p,
                                    C.c_size_t, C.c_size_t, _p]),
    "sr_wave_costs": (_i, [_p, C.POINTER(Camera), C.POINTER(Params), _i, _i, _p, _p]),
    "sr_render_block_list": (_i, [_p, C.POINTER(Camera), _i, C.POINTER(Params), _i, _i, _i, C.POINTER(_i), _i, _p,
                                  C.c_size_t, C.c_size_t, _p]),
    "sr_abi_struct_sizes": (_i, [C.POINTER(C.c_size_t), _i]),
    "sr_diag_counters": (_i, [_p, C.POINTER(C.c_int64), _i]),
    "sr_test_ray_points": (_i, [C.POINTER(C.c_float), C.POINTER(C.c_float), _i, _i, C.POINTER(C.c_float), _i, C.POINTER(_i)]),
    "sr_block_costs": (_i, [_p, _i, _i, C.c_double, _p]),
    "sr_balanced_blocks": (_i, [_p, _i, _i, _p, _i, C.POINTER(_i)]),
    "sr_assemble_blocks": (_i, [_p, C.c_size_t, C.c_size_t, _p, _i, _i, _i, _i, C.c_size_t, _p, C.c_size_t, _i, _i,
                                _p]),
    "sr_render_ss": (_i, [_p, C.POINTER(Camera), C.POINTER(Params), _i, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    "sr_render_block_list_ss": (_i, [_p, C.POINTER(Camera), _i, C.POINTER(Params), _i, _i, _i, C.POINTER(_i), _i, _i,
                                     _p, C.c_size_t, C.c_size_t, _p]),
    "sr_resolve_box": (_i, [_p, C.c_size_t, C.c_size_t, _i, _i, _i, _p, C.c_size_t, C.c_size_t, _i, _i, _p]),
    "sr_render_adaptive": (_i, [_p, C.POINTER(Camera), C.POINTER(Params), _i, _i, _i, _i, _i, _p, C.c_size_t, _p, _p]),
    "sr_edge_tiles": (_i, [_p, C.c_size_t, _i, _i, _i, _i, _p, _i, _p]),
    "sr_render_phase": (_i, [_p, C.POINTER(Camera), C.POINTER(Params), _i, _i, _i, _i, _i, _i, _i, _p, C.c_size_t, _p]),
    "sr_render_accumulate": (_i, [_p, C.POINTER(Camera), C.POINTER(Params), _i, _i, _i, _i, _i, _p, _i, _i, _p,
                                  C.c_size_t, _p]),
    "sr_accum_add": (_i, [_p, C.c_size_t, C.c_size_t, _i, _i, _i, _i, _p, C.c_size_t, _i, _p]),
    "sr_accum_resolve": (_i, [_p, C.c_size_t, _i, _i, _i, _p, C.c_size_t, _i, _p]),
    "sr_phase_order": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "sr_scene_shading_only": (_i, [C.POINTER(Scene), C.POINTER(Scene)]),
    "sr_can_reshade": (_i, [_p]),
    "sr_reshade": (_i, [_p, _p, C.c_size_t, C.c_size_t, _p]),
    "sr_reshade_debug": (_i, [_p, _p, _p, _p, _p]),
    "sr_pick_map": (_i, [_p, _p, C.c_size_t, C.c_size_t, _p]),
    "sr_set_projection": (_i, [_p, _i]),
    "sr_get_projection": (_i, [_p]),
    "sr_projection_dir": (_i, [_i, C.c_float, _i, _i, _i, _i, C.POINTER(C.c_float)]),
    "sr_set_scene_sequence": (_i, [_p, C.POINTER(Scene), _i]),
    "sr_scene_sequence_length": (_i, [_p]),
    "sr_render_sequence": (_i, [_p, _i, C.POINTER(Camera), _i, C.POINTER(Params), _i, _i, _i, _i, _i, _p, C.c_size_t,
                                C.c_size_t, _p]),
    "sr_render_sequence_block_list": (_i, [_p, _i, C.POINTER(Camera), _i, C.POINTER(Params), _i, _i, _i, C.POINTER(_i),
                                           _i, _i, _p, C.c_size_t, C.c_size_t, _p]),
    "sr_render_sequence_debug": (_i, [_p, _i, C.POINTER(Camera), C.POINTER(Params), _i, _i, _i, _i, _p, _p, _p, _p]),
    "sr_trace_rays": (_i, [_p, _p, _p, _i, C.POINTER(Params), _p, _p, _p, _p, _p]),
    "sr_camera_rays": (_i, [C.POINTER(Camera), _i, _i, _i, _i, _i, _p, _p]),
    "sr_render_shutter": (_i, [_p, _i, C.POINTER(Camera), _p, _i, _i, C.POINTER(Params), _i, _i, _i, _i, _i, _p,
                               C.c_size_t, C.c_size_t, _p]),
    "sr_render_shutter_block_list": (_i, [_p, _i, C.POINTER(Camera), _p, _i, _i, C.POINTER(Params), _i, _i, _i,
                                          C.POINTER(_i), _i, _i, _p, C.c_size_t, C.c_size_t, _p]),
    "sr_render_accumulate_shutter": (_i, [_p, _i, C.POINTER(Camera), _p, _i, C.POINTER(Params), _i, _i, _i, _i, _i, _i,
                                          _p, C.c_size_t, _p]),
    "sr_shutter_resolve": (_i, [_p, C.c_size_t, C.c_size_t, _i, _i, _i, _i, _p, C.c_size_t, C.c_size_t, _i, _p]),
    "sr_shutter_phases": (_i, [_i, _i, _p]),
    "sr_ray_maps": (_i, [_p, C.POINTER(RayMapPtrs), C.c_size_t, C.c_size_t, _p]),
    "sr_sky_uv": (_i, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sr_trace_ray_maps": (_i, [_p, _p, _p, _i, C.POINTER(Params), C.POINTER(RayMapPtrs), _p]),
}
# sr_set_projection's values (sr.h "Projections")
PROJECTION_RECTILINEAR, PROJECTION_EQUIRECT, PROJECTION_FISHEYE = 0, 1, 2
PROJECTIONS = {"rectilinear": PROJECTION_RECTILINEAR, "equirect": PROJECTION_EQUIRECT, "fisheye": PROJECTION_FISHEYE}
# header functions a library built from an earlier revision lacks (the parent
# build of an A/B timing, tools/bench_ab.sh): such a library still loads
SINCE_PROJECTIONS = ("sr_set_projection", "sr_get_projection", "sr_projection_dir")
SINCE_SEQUENCES = ("sr_set_scene_sequence", "sr_scene_sequence_length", "sr_render_sequence",
                   "sr_render_sequence_block_list", "sr_render_sequence_debug")
SINCE_TRACE = ("sr_trace_rays", "sr_camera_rays")
SINCE_SHUTTER = ("sr_render_shutter", "sr_render_shutter_block_list", "sr_render_accumulate_shutter",
                 "sr_shutter_resolve", "sr_shutter_phases")
SINCE_RAY_MAPS = ("sr_ray_maps", "sr_sky_uv")
SINCE_TRACE_MAPS = ("sr_trace_ray_maps",)
# sr_ray_maps' `end` codes (sr.h "Ray maps")
RAY_END_NONE, RAY_END_SKY, RAY_END_OPAQUE = 0, 1, 2
SHUTTER_OWN_SCENE = -1 # sr_render_shutter's first_scene for the context's own scene (sr.h "Shutter frames")
TRACE_MAX_RAYS = 1 << 28  # rays of one trace launch (sr.h "Ray queries")
MAX_SEQUENCE = 256  # scenes of a sequence (sr.h "Scene sequences")
# sr_pick_map's codes below the indices into scene.objects[]
PICK_SKY, PICK_HOLE, PICK_TEST_RAY_FLAT, PICK_TEST_RAY_CURVED, PICK_NONE = -1, -2, -3, -4, -5
MAX_SUPERSAMPLE = 4
MAX_BATCH = 32  # frames (cameras or phases) of one launch
MAX_ACCUM_PASSES = 256
# exported beside the header set (parity tooling)
EXTRA_SIGNATURES = {
    "sr_debug_set_culling": (_i, [_p, _i]),
    "sr_debug_set_timing": (_i, [_p, _i]),
    "sr_debug_kernel_times": (_i, [_p, C.POINTER(C.c_float), _i, C.POINTER(_i)]),
    "sr_debug_last_order": (_i, [_p, C.POINTER(_i), _i, C.POINTER(_i)]),
    "sr_debug_pixel_state": (_i, [_p, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_size_t)]),
    "sr_debug_retained_shape": (_i, [_p, C.POINTER(_i)]),
    # the host precomputation (csrc/host/precompute.cpp) without a device or a context
    "sr_debug_precompute_sizes": (_i, [C.POINTER(C.c_size_t), _i]),
    "sr_debug_pack_scene": (_i, [C.POINTER(Scene), C.POINTER(TestRay), _p, _p]),
    "sr_debug_frame": (_i, [C.POINTER(Scene), C.POINTER(TestRay), C.POINTER(Camera), C.POINTER(Params), _i, _i, _i,
                            _i, _p]),
    "sr_debug_step_table": (_i, [_i, _i, _p, C.c_size_t]),
    "sr_debug_opacity_bits": (_i, [_p, _i, _i, _i, _i, _p, C.c_size_t]),
    "sr_debug_shutter_div": (_i, [_i, _i]),
}

_lib = None


class SRError(RuntimeError):
    def __init__(self, status: int, what: str):
        super().__init__(f"{what}: {status_string(status)} ({status})")
        self.status = status


def load(path: str | os.PathLike | None = None) -> C.CDLL:
    """Load libsr.so (built in-tree by `make -C schwarzschild-raytracer_amd`).

    Raises FileNotFoundError when the library has not been built: there is no
    fallback implementation.
    """
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else Path(os.environ.get("SR_LIB", LIB_PATH))
    if not p.exists():
        raise FileNotFoundError(f"{p} not built; run __graft_entry__.build() or make -C schwarzschild-raytracer_amd")
    lib = C.CDLL(str(p), mode=C.RTLD_GLOBAL)
    for name, (res, args) in {**SIGNATURES, **EXTRA_SIGNATURES}.items():
        if (name in EXTRA_SIGNATURES or name in SINCE_PROJECTIONS or name in SINCE_SEQUENCES or
                name in SINCE_TRACE or name in SINCE_SHUTTER or name in SINCE_RAY_MAPS or
                name in SINCE_TRACE_MAPS) and not hasattr(lib, name):
            continue  # debug tooling and newer calls an older library (a bisection build) may lack
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def status_string(status: int) -> str:
    try:
        return load().sr_status_string(status).decode()
    except Exception:  # noqa: BLE001 - best effort in error paths
        return "status"


def check(status: int, what: str) -> None:
    if status != SR_OK:
        raise SRError(status, what)


def projection_dir(projection: int, fov: float, uv_width: int, uv_height: int, px: int, py: int):
    """sr_projection_dir: the local direction L (float32 [3]) of pixel (px, py)
    of a uv_width x uv_height frame under `projection`, or None when the pixel
    has no ray. Host only."""
    import numpy as np

    out = np.zeros(3, dtype=np.float32)
    rc = load().sr_projection_dir(int(projection), float(fov), int(uv_width), int(uv_height), int(px), int(py),
                                  out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc < 0:
        raise SRError(rc, "sr_projection_dir")
    return out if rc == 1 else None


def sky_uv(direction):
    """sr_sky_uv: get_bg's (u, v) (float32 [2]) of a direction (3 floats, taken
    as it is, not normalised), the code the ray-map kernels run. Host only."""
    import numpy as np

    d = np.ascontiguousarray(direction, dtype=np.float32).reshape(3)
    out = np.zeros(2, dtype=np.float32)
    check(load().sr_sky_uv(d.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float))),
          "sr_sky_uv")
    return out


def camera_rays(cam: Camera, projection, width: int, height: int, row_begin: int = 0, row_end: int | None = None):
    """sr_camera_rays: the rays the frame kernels start with for rows
    [row_begin, row_end) of a width x height frame under `projection`
    (PROJECTION_* or its name) -> (origins, dirs), float32 [rows, width, 3]
    host arrays; a pixel without a ray has a NaN direction. Host only."""
    import numpy as np

    if isinstance(projection, str):
        projection = PROJECTIONS[projection]
    row_end = height if row_end is None else row_end
    rows = max(int(row_end) - int(row_begin), 0)
    o = np.empty((rows, int(width), 3), dtype=np.float32)
    d = np.empty((rows, int(width), 3), dtype=np.float32)
    check(load().sr_camera_rays(C.byref(cam), int(projection), int(width), int(height), int(row_begin), int(row_end),
                                o.ctypes.data, d.ctypes.data), "sr_camera_rays")
    return o, d


def write_png(path, frame, flip_rows: bool = True) -> None:
    """sr_write_png: an [H, W, 4] uint8 frame (host array; rows bottom-up as
    sr_render leaves them when flip_rows) as an RGBA8 PNG."""
    import numpy as np

    a = np.ascontiguousarray(frame, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"expected an [H, W, 4] frame, got {a.shape}")
    h, w, _ = a.shape
    check(load().sr_write_png(str(path).encode(), a.ctypes.data, w, h, w * 4, 1 if flip_rows else 0), "sr_write_png")


def resolve_box(samples, ss: int):
    """sr_resolve_box's host form: uint8 sample frames [..., ss * rows, ss * W, 4]
    (host array) -> their box-resolved [..., rows, W, 4]."""
    import numpy as np

    a = np.ascontiguousarray(samples, dtype=np.uint8)
    if a.ndim < 3 or a.shape[-1] != 4 or ss < 1 or a.shape[-3] % ss or a.shape[-2] % ss:
        raise ValueError(f"expected [..., {ss} * rows, {ss} * W, 4] samples, got {a.shape}")
    lead, rows, w = a.shape[:-3], a.shape[-3] // ss, a.shape[-2] // ss
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    out = np.empty(lead + (rows, w, 4), dtype=np.uint8)
    if n and rows and w:
        check(load().sr_resolve_box(a.ctypes.data, 4 * ss * w, 4 * ss * w * ss * rows, w, rows, ss, out.ctypes.data,
                                    4 * w, 4 * w * rows, n, 0, None), "sr_resolve_box")
    return out


def edge_tiles(frame, threshold: int, grow: int = 0):
    """sr_edge_tiles' host form: an [H, W, 4] uint8 frame (host array, rows may
    be strided) -> its flagged 16x16 tiles, uint8 [ceil(H / 16), ceil(W / 16)]."""
    import numpy as np

    a = np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.strides[1:] != (4, 1) or a.strides[0] < 0:
        a = np.ascontiguousarray(frame, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"expected an [H, W, 4] frame, got {a.shape}")
    h, w, _ = a.shape
    out = np.empty(((h + 15) // 16, (w + 15) // 16), dtype=np.uint8)
    check(load().sr_edge_tiles(a.ctypes.data, a.strides[0], w, h, int(threshold), int(grow), out.ctypes.data, 0, None),
          "sr_edge_tiles")
    return out


def phase_order(ss: int):
    """sr_phase_order: the ss * ss phases (x, y) of an ss x ss grid in
    progressive order."""
    lib = load()
    out = []
    x, y = C.c_int(), C.c_int()
    for k in range(ss * ss if 1 <= ss <= MAX_SUPERSAMPLE else 1):
        check(lib.sr_phase_order(int(ss), k, C.byref(x), C.byref(y)), "sr_phase_order")
        out.append((x.value, y.value))
    return out


def _aligned_rows(rows: int, pitch: int, align: int = 8):
    """A zeroed host buffer of rows x pitch bytes whose base is a multiple of `align`."""
    import numpy as np

    raw = np.zeros(rows * pitch + align, dtype=np.uint8)
    o = (-raw.ctypes.data) % align
    return raw[o:o + rows * pitch]


def accum_add(images, accum=None, reset: bool = False):
    """sr_accum_add's host form: uint8 images [n, rows, W, 4] (or one [rows, W,
    4]) added to the uint16 accumulator [rows, W, 4] (host arrays; a new zero
    accumulator when None) -> the accumulator."""
    import numpy as np

    a = np.ascontiguousarray(images, dtype=np.uint8)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[-1] != 4:
        raise ValueError(f"expected [n, rows, W, 4] images, got {a.shape}")
    n, rows, w, _ = a.shape
    if accum is None:
        accum = _aligned_rows(rows, 8 * w).view(np.uint16).reshape(rows, w, 4)
    if accum.dtype != np.uint16 or accum.shape != (rows, w, 4) or accum.strides[1:] != (8, 2):
        raise ValueError(f"expected a uint16 [{rows}, {w}, 4] accumulator with dense pixels")
    if rows and w:
        check(load().sr_accum_add(a.ctypes.data, 4 * w, 4 * w * rows, n, w, rows, 1 if reset else 0, accum.ctypes.data,
                                  accum.strides[0], 0, None), "sr_accum_add")
    return accum


def accum_resolve(accum, n: int):
    """sr_accum_resolve's host form: a uint16 accumulator [rows, W, 4] of n
    images (host array) -> the uint8 frame [rows, W, 4]."""
    import numpy as np

    a = np.asarray(accum)
    if a.dtype != np.uint16 or a.ndim != 3 or a.shape[2] != 4 or a.strides[1:] != (8, 2):
        raise ValueError(f"expected a uint16 [rows, W, 4] accumulator with dense pixels, got {a.dtype} {a.shape}")
    rows, w, _ = a.shape
    out = np.empty((rows, w, 4), dtype=np.uint8)
    if rows and w:
        check(load().sr_accum_resolve(a.ctypes.data, a.strides[0], w, rows, int(n), out.ctypes.data, 4 * w, 0, None),
              "sr_accum_resolve")
    return out


def shutter_phases(ss: int, sub_frames: int):
    """sr_shutter_phases: the default phase pairs of a shutter frame's
    sub_frames sub-frames, uint8 [sub_frames, 2] {x, y}: sr_phase_order(ss, k
    mod ss * ss)."""
    import numpy as np

    out = np.zeros((max(int(sub_frames), 0), 2), dtype=np.uint8)
    check(load().sr_shutter_phases(int(ss), int(sub_frames), out.ctypes.data), "sr_shutter_phases")
    return out


def shutter_resolve(images, sub_frames: int):
    """sr_shutter_resolve's host form: uint8 sub-frame images [M * sub_frames,
    rows, W, 4] (host array) -> the M shutter frames [M, rows, W, 4], frame m
    the rounded mean of images m * sub_frames .. (m + 1) * sub_frames - 1."""
    import numpy as np

    a = np.ascontiguousarray(images, dtype=np.uint8)
    k = int(sub_frames)
    if a.ndim != 4 or a.shape[-1] != 4 or k < 1 or a.shape[0] % k or a.shape[0] == 0:
        raise ValueError(f"expected [M * {k}, rows, W, 4] images, got {a.shape}")
    n, rows, w, _ = a.shape
    out = np.empty((n // k, rows, w, 4), dtype=np.uint8)
    if rows and w:
        check(load().sr_shutter_resolve(a.ctypes.data, 4 * w, 4 * w * rows, k, n // k, w, rows, out.ctypes.data, 4 * w,
                                        4 * w * rows, 0, None), "sr_shutter_resolve")
    return out


def scene_shading_only(a: Scene, b: Scene) -> bool:
    """sr_scene_shading_only: b differs from a in lights and the materials'
    rgb, Phong terms and normal maps at most (a retained frame outlives it)."""
    return bool(load().sr_scene_shading_only(C.byref(a), C.byref(b)))


def _precompute_sizes():
    out = (C.c_size_t * 3)()
    check(load().sr_debug_precompute_sizes(out, 3), "sr_debug_precompute_sizes")
    return tuple(int(v) for v in out)


def debug_pack_scene(scene: Scene | None, test_ray: TestRay | None = None):
    """sr_debug_pack_scene: (status, scene image bytes, segment buffer bytes)
    that sr_set_scene(scene) and sr_set_test_ray(test_ray) would upload on a
    fresh context (None: no scene / the default test ray). Host only; the
    buffers are None unless the status is SR_OK."""
    import numpy as np

    n_scene, n_segs, _ = _precompute_sizes()
    img, segs = np.zeros(n_scene, dtype=np.uint8), np.zeros(n_segs, dtype=np.uint8)
    rc = load().sr_debug_pack_scene(C.byref(scene) if scene is not None else None,
                                    C.byref(test_ray) if test_ray is not None else None, img.ctypes.data,
                                    segs.ctypes.data)
    return (rc, img, segs) if rc == SR_OK else (rc, None, None)


def debug_frame(scene: Scene | None, test_ray: TestRay | None, cam: Camera, params: Params, width: int, height: int,
                cull: bool = True, projection: int = PROJECTION_RECTILINEAR):
    """sr_debug_frame: (status, frame struct bytes) of a whole-frame sr_render
    on that fresh context. Host only; None unless the status is SR_OK."""
    import numpy as np

    out = np.zeros(_precompute_sizes()[2], dtype=np.uint8)
    rc = load().sr_debug_frame(C.byref(scene) if scene is not None else None,
                               C.byref(test_ray) if test_ray is not None else None, C.byref(cam), C.byref(params),
                               int(width), int(height), 1 if cull else 0, int(projection), out.ctypes.data)
    return (rc, out) if rc == SR_OK else (rc, None)


def debug_step_table(max_steps: int, max_revolutions: int):
    """sr_debug_step_table: float32 [max_steps + 4, 4] rows {step, step / 6,
    cos phi, sin phi} of the schedule, the last four rows zero padding."""
    import numpy as np

    out = np.empty((int(max_steps) + 4, 4), dtype=np.float32)
    check(load().sr_debug_step_table(int(max_steps), int(max_revolutions), out.ctypes.data, out.size),
          "sr_debug_step_table")
    return out


def debug_opacity_bits(arr):
    """sr_debug_opacity_bits: the opacity bitmap of a [layers, h, w, 3 or 4]
    uint8 texture array, uint8 [layers, h, ceil(w / 8)]."""
    import numpy as np

    a = np.ascontiguousarray(arr, dtype=np.uint8)
    layers, h, w, ch = a.shape
    out = np.empty((layers, h, (w + 7) // 8), dtype=np.uint8)
    check(load().sr_debug_opacity_bits(a.ctypes.data, w, h, layers, ch, out.ctypes.data, out.size),
          "sr_debug_opacity_bits")
    return out


def check_layout() -> dict:
    lib = load()
    out = (C.c_size_t * 6)()
    check(lib.sr_abi_struct_sizes(out, 6), "sr_abi_struct_sizes")
    got = dict(zip(["camera", "params", "scene", "test_ray", "material", "light"], list(out)))
    want = {
        "camera": C.sizeof(Camera),
        "params": C.sizeof(Params),
        "scene": C.sizeof(Scene),
        "test_ray": C.sizeof(TestRay),
        "material": C.sizeof(Material),
        "light": C.sizeof(Light),
    }
    if got != want:
        raise AssertionError(f"ctypes layout mismatch: C {got} vs ctypes {want}")
    return got


def default_params(**overrides) -> Params:
    p = Params()
    load().sr_params_default(C.byref(p))
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def default_test_ray() -> TestRay:
    t = TestRay()
    load().sr_test_ray_default(C.byref(t))
    return t


def default_scene() -> Scene:
    s = Scene()
    load().sr_default_scene(C.byref(s))
    return s


def default_camera() -> Camera:
    c = Camera()
    load().sr_default_camera(C.byref(c))
    return c


def camera_flyby(t: float, initial_distance: float = 30.0, closest_distance: float = 10.0,
                 cam: Camera | None = None) -> Camera:
    """The app's H-key flyby camera at eased time t in [0, 1] (src/main.cpp:404-410:
    Camera::hyperbolicTrajectory(30, 10, t), camera.cpp:20-39)."""
    src = cam if cam is not None else default_camera()
    c = Camera()
    C.memmove(C.addressof(c), C.addressof(src), C.sizeof(Camera))
    check(load().sr_camera_hyperbolic_trajectory(C.byref(c), initial_distance, closest_distance, t),
          "sr_camera_hyperbolic_trajectory")
    return c


def test_ray_points(pos, forward, max_steps: int, max_revolutions: int = 2):
    """Host press-R geodesic (src/main.cpp:94-124) -> list of (x, y, z)."""
    lib = load()
    cap = max_steps + 2
    buf = (C.c_float * (3 * cap))()
    n = C.c_int()
    check(
        lib.sr_test_ray_points((C.c_float * 3)(*pos), (C.c_float * 3)(*forward), max_steps, max_revolutions, buf, cap, C.byref(n)),
        "sr_test_ray_points",
    )
    return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(min(n.value, cap))]
