"""Materials, lights, texture mappings and skyboxes no generator of scenes.py
draws (a helper, not a test module).

CASES is a table of named cases for tests/test_shading_cases.py (the oracle
alone: is the case what it says?), tests/test_gpu_shading_extremes.py (the
kernel against the oracle, culling on against off) and, for the cases that fit
the reference shader's "features" capacity profile, tests/golden/make_golden.py
--set r5 (the oracle against the reference shader). tests/extreme_cases.py
varies the primitives and tests/view_cases.py the cameras and the frame
parameters; both keep plain_material and one_light. Here the geometry is
plain and the shading side of the scene is at or past an edge:

    Case.group     specular | light | alpha | mapping | normalmap | seams | skybox
    Case.specs     the primitives (extreme_cases specs; "material": 0, the
                   default, or 2); () is the hole alone
    Case.material  overrides of plain_material's fields on material 0
                   ("color": four floats); Case.material2: on material 2
    Case.lights    the scene's lights (light(), below); num_lights overrides
                   their count
    Case.scene     further mutations of the built scene (texture sizes), a
                   function of the scene
    Case.camera    (pos, target, fov)
    Case.params    overrides of PARAMS
    Case.textures  the key of a texture set (textures_of): (skybox, texture
                   array, the (w, h) of its layers); None in either place is
                   a context without that upload
    Case.visible   the minimum share of pixels in which the frame differs from
                   the baseline's: the same primitives, camera and params
                   with plain_material, one_light and the "std" textures
                   (MIN_SHARE; 0: no minimum, the reason is beside the entry)
    Case.hosts     "alone": the primitives, one material, the lights.
                   "stacked": the same in front of BACK, an opaque blue
                   rectangle with a material of its own: whether the ray goes
                   on past the case's primitive changes the colour as well as
                   the step count
    Case.flat      the case also runs with raytrace_type 1
    Case.nonfinite the oracle's float frame holds a NaN or an infinity (in
                   every mode and on every host of the case)
    Case.aim       the centre pixel's expected value (the 65x41 frame has its
                   centre pixel at uv = (0, 0): the centre ray is the camera's
                   forward axis, radial for CAM, so it is traced flat in both
                   modes): "nan_rgb" (NaN, NaN, NaN, 1) or ("texel", u, v):
                   the rgb of layer 0 sampled at (u, v), bit for bit (the
                   aimed materials are ambient 1, diffuse 0, specular 0)
    Case.pin       None: not in golden_r5.npz (more capacity than the
                   "features" profile has, a context without an upload, or a
                   filter the shader has not, or left out for the fixture's
                   size); "pin": the shader's frame pins the oracle's;
                   "undefined": the shader's result rests on an operation
                   GLSL leaves undefined and is far from the oracle's
                   (tests/test_oracle_golden_shading.py EXCLUDED)
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import extreme_cases as X

OBJECTS = X.TEXEL_OBJECTS

W, H = 65, 41  # odd: the centre pixel is at uv = (0, 0); 5 x 3 tiles of 16 x 16, partial waves on two edges
STEPS, REVOLUTIONS = 100, 2
PARAMS = {"max_steps": STEPS, "max_revolutions": REVOLUTIONS, "percent_black": -1.0, "crosshair": 0}
MIN_SHARE = 0.02
GROUPS = ("specular", "light", "alpha", "mapping", "normalmap", "seams", "skybox")
PS_HITS = 4  # csrc/device_scene.h SR_PS_HITS: the hit log's length

NAN, INF = float("nan"), float("inf")
F32 = np.float32
BELOW_1 = float(np.nextafter(F32(1.0), F32(0.0)))
ABOVE_1 = float(np.nextafter(F32(1.0), F32(2.0)))

CAM = ((0.0, 0.0, 12.0), (0.0, 0.0, 0.0), 60.0)  # tests/test_gpu_texel_edges.py's camera
FACING = X.axes_up((0.0, 0.0, 1.0))   # normal +z (towards CAM), columns x and -y
AWAY = X.axes_up((0.0, 0.0, -1.0))    # normal -z, columns x and +y
RECT = {"type": "rectangle", "pos": (-3.0, 1.75, 6.0), "axes": FACING, "width": 6.0, "height": 3.5}
RECT_AWAY = {"type": "rectangle", "pos": (-3.0, -1.75, 6.0), "axes": AWAY, "width": 6.0, "height": 3.5}
BACK = {"type": "rectangle", "pos": (-5.0, 3.0, 3.0), "axes": FACING, "width": 10.0, "height": 6.0}
BACK_COLOR = (0.2, 0.4, 0.9, 1.0)
HIT = (0.0, 0.0, 6.0)  # where CAM's centre ray meets RECT


def light(pos=(5.0, 12.0, 14.0), color=(1.0, 1.0, 1.0), intensity=6.0, att=(1.0, 0.05, 0.01)):
    """extreme_cases.one_light's values unless given."""
    return {"pos": pos, "color": color, "intensity": intensity, "att": att}


@dataclass
class Case:
    name: str
    group: str
    specs: tuple = (RECT,)
    material: dict = field(default_factory=dict)
    material2: dict = field(default_factory=dict)
    lights: tuple = (light(),)
    num_lights: int | None = None
    scene: object = None
    camera: tuple = CAM
    params: dict = field(default_factory=dict)
    textures: str = "std"
    visible: float = MIN_SHARE
    hosts: tuple = ("alone",)
    flat: bool = False
    nonfinite: bool = False
    aim: object = None
    pin: str | None = "pin"

    @property
    def modes(self) -> tuple:
        return ("curved", "flat") if self.flat else ("curved",)


# ---- textures --------------------------------------------------------------------
def _random(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def random_array(w, h, seed=0):
    """[2, h, w, 4]: random texels; alpha 255 on layer 0, random on layer 1."""
    arr = _random(100 * w + h + seed, (2, h, w, 4))
    arr[0, :, :, 3] = 255
    return arr


def normal_array(kind, w, h):
    """Layer 0 random colours (alpha 255), layer 1 the normal map."""
    arr = random_array(w, h, seed=7)
    if kind == "zero":  # nrm(0) = 0 * (1 / sqrt(0)) = 0 * inf
        arr[1] = 0
    elif kind == "blue":  # ordinary tangent-space normals: a gentle tilt around (0, 0, 1), never zero
        x = np.arange(w)[None, :] + 0 * np.arange(h)[:, None]
        y = 0 * np.arange(w)[None, :] + np.arange(h)[:, None]
        arr[1] = np.stack([100 + (56 * x) // max(w - 1, 1), 100 + (56 * y) // max(h - 1, 1), 230 + 0 * x, 255 + 0 * x],
                          axis=-1).astype(np.uint8)
    return arr


def skybox(w, h, channels):
    bg = _random(7 * w + h + channels, (h, w, channels))
    if channels == 4:
        bg[:, :, 3] = np.minimum(bg[:, :, 3], 254)  # alpha < 255 everywhere
    return bg


SKY_SIZES = ((1, 1), (2, 1), (1, 2), (3, 2), (5, 7))  # (w, h)
_TEXTURE_MAKERS = {
    "std": lambda sc: (sc.skybox(256, 128), random_array(7, 5), (7, 5)),
    "no_array": lambda sc: (sc.skybox(256, 128), None, (7, 5)),
    "no_bg": lambda sc: (None, random_array(7, 5), (7, 5)),
    "logged13x9": lambda sc: (sc.skybox(256, 128), random_array(13, 9, seed=3), (13, 9)),
    "nm_rand7x5": lambda sc: (sc.skybox(256, 128), random_array(7, 5, seed=7), (7, 5)),
    "nm_rand3x2": lambda sc: (sc.skybox(256, 128), random_array(3, 2, seed=7), (3, 2)),
    "nm_zero": lambda sc: (sc.skybox(256, 128), normal_array("zero", 7, 5), (7, 5)),
    "nm_blue": lambda sc: (sc.skybox(256, 128), normal_array("blue", 7, 5), (7, 5)),
    **{f"sky{w}x{h}x{ch}": (lambda sc, w=w, h=h, ch=ch: (skybox(w, h, ch), random_array(7, 5), (7, 5)))
       for w, h in SKY_SIZES for ch in (3, 4)},
}
_textures = {}


def textures_of(pkg, key):
    """(skybox or None, texture array or None, (w, h) of the array's layers), read-only."""
    if key not in _textures:
        bg, arr, size = _TEXTURE_MAKERS[key](pkg.scenes)
        for a in (bg, arr):
            if a is not None:
                a.setflags(write=False)
        _textures[key] = (bg, arr, size)
    return _textures[key]


# ---- scene building --------------------------------------------------------------
def _set_light(L, d):
    for i in range(3):
        L.transform.pos[i] = d["pos"][i]
        L.color[i] = d["color"][i]
    for i in range(9):
        L.transform.axes[i] = X.IDENT[i]
    L.intensity = d["intensity"]
    L.attenuation_constant, L.attenuation_linear, L.attenuation_quadratic = d["att"]


def build(pkg, case, host="alone", plain=False):
    """The case's scene on a host; plain: with plain_material and one_light
    (the baseline of the case)."""
    s = X.empty_scene(pkg)
    for spec in case.specs:
        X.append_primitive(s, spec, spec.get("material", 0))
    if host == "stacked":
        X.plain_material(s.materials[1], BACK_COLOR)
        X.append_primitive(s, BACK, 1)
    size = textures_of(pkg, "std" if plain else case.textures)[2]
    pkg.scenes.set_scene_texture_sizes(s, [size] * pkg.abi.MAX_TEXTURES, size)
    if plain:
        return s
    for index, overrides in ((0, case.material), (2, case.material2)):
        m = s.materials[index]
        X.plain_material(m)
        for k, v in overrides.items():
            if k == "color":
                for i in range(4):
                    m.color[i] = v[i]
            else:
                setattr(m, k, v)
    for i, d in enumerate(case.lights):
        _set_light(s.lights[i], d)
    s.num_lights = len(case.lights) if case.num_lights is None else case.num_lights
    if case.scene is not None:
        case.scene(s)
    return s


def camera_of(pkg, case):
    pos, target, fov = case.camera
    return pkg.scenes.camera_look(pos, tuple(float(t) - float(p) for p, t in zip(pos, target)), fov=fov)


def params_of(pkg, case, mode="curved"):
    return pkg.abi.default_params(**{**PARAMS, **case.params, **({"raytrace_type": 1} if mode == "flat" else {})})


def samples_own_textures(case) -> bool:
    m = {**case.material, **case.material2}
    return m.get("texture_index", -1) >= 0 or m.get("normal_map_index", -1) >= 0 or case.group == "skybox"


def oracle_params_for_shader(pkg, case, params):
    """The params with which the oracle is held against the reference shader
    on SwiftShader (golden_r5.npz): SwiftShader's own texture filter
    (oracle.FILTER_SWIFTSHADER, tests/test_oracle_golden.py) where the case
    samples a texture or a skybox of its own, the case's params elsewhere."""
    if not samples_own_textures(case):
        return params
    p = pkg.scenes.struct_from_bytes(pkg.abi.Params, pkg.scenes.struct_bytes(params))
    p.filter_mode = 2  # oracle.FILTER_SWIFTSHADER
    return p


def encode_frames(rgba8):
    """[n, H, W, 4] uint8 frames as golden_r5.npz stores them: [n, 4, H, W]
    channel planes of differences along x, modulo 256."""
    planes = np.moveaxis(np.asarray(rgba8, dtype=np.uint8), -1, 1).copy()
    planes[..., 1:] = planes[..., 1:] - planes[..., :-1]
    return planes


def decode_frames(planes_dx):
    return np.ascontiguousarray(np.moveaxis(np.cumsum(planes_dx, axis=-1, dtype=np.uint8), 1, -1))


def cells():
    """(case, host, mode) of the GPU matrix and of the oracle's check."""
    return [(c, h, m) for c in CASES for h in c.hosts for m in c.modes]


def cell_id(cell):
    c, host, mode = cell
    return f"{c.name}-{host}-{mode}"


def changed(a, b):
    """The pixels in which two (rgba8, rgba32, steps) frames differ (NaN = NaN)."""
    fa, fb = a[1].view(np.uint32), b[1].view(np.uint32)
    both_nan = np.isnan(a[1]) & np.isnan(b[1])
    return (a[0] != b[0]).any(-1) | ((fa != fb) & ~both_nan).any(-1) | (a[2] != b[2])


def distinct_colours(frame) -> int:
    """The distinct float colours of an oracle frame (by their bits)."""
    return len(np.unique(np.ascontiguousarray(frame[1]).view(np.uint32).reshape(-1, 4), axis=0))


# ---- the table -------------------------------------------------------------------
def _name(x) -> str:
    return repr(x).replace("-", "m").replace(".", "p").replace("+", "")


BOTH = ("alone", "stacked")
# the highlight of this light lies inside RECT's image (the mirror point of CAM and the light is near (0.7, 0.5, 6))
SPEC_LIGHT = (light(pos=(1.5, 1.0, 13.0)),)
# half a unit in front of RECT's plane, beyond its right edge: reflected off the left part, it leaves away from CAM
GRAZING_LIGHT = (light(pos=(8.0, 0.5, 6.5)),)


def _spec(name, material, **kw):
    return Case("spec_" + name, "specular", material=material, lights=SPEC_LIGHT, **kw)


def _light(name, *lights, **kw):
    return Case("light_" + name, "light", lights=lights, **kw)


def _sizes(which, v):
    """texture_sizes (every layer) or max_texture_size set to (v, v)."""
    def mutate(s):
        if which == "texture_sizes":
            for i in range(len(s.texture_sizes)):
                s.texture_sizes[i][0] = s.texture_sizes[i][1] = v
        else:
            s.max_texture_size[0] = s.max_texture_size[1] = v
    return mutate


def _twice_max(s):  # texture_sizes > max_texture_size: uv runs to 2, the sampler wraps
    for i in range(len(s.texture_sizes)):
        s.texture_sizes[i][0], s.texture_sizes[i][1] = 2.0 * s.max_texture_size[0], 2.0 * s.max_texture_size[1]


TEXTURED = {"texture_index": 0}
PLANE = OBJECTS["plane_patch"]  # facing CAM at z = 6: texture_offset (-2, -1.5), texture_size (4, 3), no repeat
# lighting off: the pixel is the texel (ambient 1), for the aimed cases
TEXEL_ONLY = {"texture_index": 0, "ambient": 1.0, "diffuse": 0.0, "specular": 0.0}
NORMAL_MAPPED = {"normal_map_index": 1}

# a box of 3 centred at (5, 0, 5), slightly tilted, and the six cameras that face its faces from 6 units
BOX = {"type": "box", "pos": (3.5, -1.5, 3.5), "axes": X.axes_up((0.1, 1.0, 0.05)), "width": 3.0, "depth": 3.0,
       "height": 3.0}
BOX_CENTRE = (5.0, 0.0, 5.0)
BOX_VIEWS = {"px": (6.0, 0.0, 0.0), "mx": (-6.0, 0.0, 0.0), "py": (0.0, 6.0, 0.0), "my": (0.0, -6.0, 0.0),
             "pz": (0.0, 0.0, 6.0), "mz": (0.0, 0.0, -6.0)}

# the pole (local y) of this sphere points at CAM: the centre ray meets it at (0, 0, 8.5), local.y / r = 1
POLE_SPHERE = {"type": "sphere", "pos": (0.0, 0.0, 6.0), "axes": FACING, "radius": 2.5}
CENTRE_DISK = {"type": "disk", "pos": HIT, "axes": FACING, "radius": 3.0}
CENTRE_ANNULUS = {"type": "annulus", "pos": HIT, "axes": FACING, "inner": 0.0, "outer": 3.0}
# identity axes: phi = atan2(local.x, local.z) is 0 / 2 pi where x = 0 and z > 0, CAM's centre column
SEAM_CYLINDER = {"type": "cylinder", "pos": (0.0, -2.5, 6.0), "axes": X.IDENT, "height": 5.0, "radius": 2.0}

# Eight textured layers across the view of SIDEWAYS (CAM's position, looking along +x) under the weighted filter,
# where no textured hit is classified opaque in the step loop (a plane's never is): every hit is logged as "maybe
# translucent". A step tests one chord and takes its nearest hit; these rays run across the radial direction, so a
# step advances them r * 0.126 along x, 1.5 at the camera and 2.4 at x = 15: the layers lie 2 to 3.5 apart, one to a
# chord. Material 0 samples the all-opaque layer 0 (alpha exactly 1 or 0.99999994, the weighted sum of four 1.0),
# material 2 the random-alpha layer 1. By distance from the camera:
#   A (plane, m2) | D1 (disk, m0) the middle | B, C (rectangles, m2) | R1 (m2) a 7 x 4 patch | R2 (disk, m2) |
#   P1, P2 (planes, m0)
# In the middle the log holds A, D1, B, C when the ray stops: D1's shaded alpha is 1, so B and C are dropped and D1's
# step count is the pixel's. Inside R1 and outside D1 five translucent hits come first: the log fills with four and
# the resume kernel shades the fifth, then P1.
SIDEWAYS = ((0.0, 0.0, 12.0), (1.0, 0.0, 12.0), 60.0)
FACING_MX = X.axes_up((-1.0, 0.0, 0.0), ref=(0.0, 0.0, 1.0))  # normal -x, columns z and -y


def _layer(kind, x, material, **kw):
    """A layer at x facing SIDEWAYS; a rectangle of w x h is centred on the view's axis."""
    spec = {"type": kind, "pos": (x, 0.0, 12.0), "axes": FACING_MX, "material": material, **kw}
    if kind == "rectangle":
        spec["pos"] = (x, spec["height"] / 2.0, 12.0 - spec["width"] / 2.0)
    return spec


LAYERS = (
    _layer("plane", 1.5, 2, texture_offset=(-0.5, 0.25), texture_size=(3.0, 2.0), repeat_texture=1),
    _layer("disk", 3.5, 0, radius=0.4),
    _layer("rectangle", 5.5, 2, width=8.0, height=6.0),
    _layer("rectangle", 7.5, 2, width=11.0, height=8.0),
    _layer("rectangle", 9.5, 2, width=7.0, height=4.0),
    _layer("disk", 12.0, 2, radius=13.0),
    _layer("plane", 15.0, 0, texture_offset=(0.3, -0.7), texture_size=(2.0, 3.0), repeat_texture=1),
    _layer("plane", 18.5, 0, texture_offset=(1.1, 0.4), texture_size=(2.5, 1.5), repeat_texture=1),
)

UP = ((0.0, 0.0, 12.0), (0.0, 1.0, 12.0), 60.0)     # v = asin(dir.y) / pi + 0.5 reaches 1 in the centre pixel
DOWN = ((0.0, 0.0, 12.0), (0.0, -1.0, 12.0), 60.0)  # v = 0
# u = atan2(dir.z, dir.x) / (2 pi): the wrap 0 / 1 is where dir.z = 0 and dir.x > 0, the centre column of the camera
# that looks along +x; along -x the centre column's u is 1/2. Both are pitched up a little and the camera at the hole
# looks down on it: from a level camera u is one value per column, and a skybox one texel high gives at most W colours.
ALONG_PX = ((0.0, 0.0, 12.0), (1.0, 0.3, 12.0), 60.0)
ALONG_MX = ((0.0, 0.0, 12.0), (-1.0, 0.3, 12.0), 60.0)
AT_HOLE = ((0.0, 4.0, 11.0), (0.0, 0.0, 0.0), 60.0)
SKY_CAMERAS = {"hole": AT_HOLE, "up": UP, "down": DOWN, "px": ALONG_PX, "mx": ALONG_MX}
HOLE_IN_VIEW = ("hole",)
# The skybox cells golden_r5.npz holds (the fixture may not outgrow golden_r4.npz, and these frames of random texels
# compress worst): looking up from every skybox, every view of the 5x7x4 one and the u wrap of two small ones. The
# shader has one filter, so none of the weighted-filter cells.
SKY_PINNED = ({(0, "up", w, h, ch) for w, h in SKY_SIZES for ch in (3, 4)} | {(0, v, 5, 7, 4) for v in SKY_CAMERAS}
              | {(0, "px", 2, 1, 3), (0, "px", 1, 2, 4)})

CASES = [
    # -- specular: t_pow(max(dot(view, reflect), 0), shininess), binary64 pow rounded to binary32
    _spec("shin_0", {"shininess": 0.0}, flat=True),  # pow(0, 0) = 1 where the reflection misses
    *[_spec("shin_" + _name(v), {"shininess": v}) for v in (1.0, 2.0, 3.0, 0.5, 1e4)],
    _spec("shin_inf", {"shininess": INF}),
    # pow(0, -2) = inf where the reflection misses: the left part of RECT under GRAZING_LIGHT (nowhere under SPEC_LIGHT)
    Case("spec_shin_m2", "specular", material={"shininess": -2.0}, lights=GRAZING_LIGHT, nonfinite=True),
    _spec("shin_minf", {"shininess": -INF}, nonfinite=True),
    _spec("shin_nan", {"shininess": NAN}, nonfinite=True, pin="undefined"),
    Case("spec_shin_m2_spec0", "specular", material={"shininess": -2.0, "specular": 0.0}, lights=GRAZING_LIGHT,
         nonfinite=True),  # 0 * inf
    *[_spec(f"{f}_{_name(v)}", {f: v}, nonfinite=v != v or v == INF)
      for f in ("ambient", "diffuse", "specular") for v in (-0.5, 2.0, INF, NAN)],
    # every infinity above is positive: these give -inf pixels (unorm8 stores them as 0, +inf as 255)
    _spec("ambient_minf", {"ambient": -INF}, nonfinite=True),
    _spec("specular_minf", {"specular": -INF}, nonfinite=True),
    # -- lights
    _light("none", num_lights=0),
    _light("four", light(), light((-6.0, 2.0, 9.0), (1.0, 0.3, 0.2), 4.0, (1.0, 0.09, 0.032)),
           light((2.0, -5.0, 10.0), (0.2, 0.9, 0.4), 8.0, (0.5, 0.1, 0.02)),
           light((0.5, 0.5, 7.0), (0.3, 0.4, 1.0), 2.0, (1.0, 0.0, 0.05))),
    _light("att_000", light(att=(0.0, 0.0, 0.0)), nonfinite=True),  # 1 / 0
    # 0.1 d^2 - 1 with the light 2 in front of RECT's centre: d runs from 2 to 3.9, the denominator changes sign at 3.16
    _light("att_const_neg", light(pos=(0.0, 0.0, 8.0), att=(-1.0, 0.0, 0.1))),
    _light("att_quad_neg", light(att=(1.0, 0.05, -0.01))),
    _light("intensity_0", light(intensity=0.0)),
    _light("intensity_m3", light(intensity=-3.0)),
    _light("intensity_inf", light(intensity=INF), nonfinite=True),
    _light("intensity_minf", light(intensity=-INF), nonfinite=True),
    _light("intensity_nan", light(intensity=NAN), nonfinite=True),
    _light("color_neg", light(color=(-0.5, 1.0, 1.0))),
    _light("color_2", light(color=(2.0, 2.0, 2.0))),
    _light("color_nan", light(color=(NAN, 1.0, 1.0)), nonfinite=True),
    _light("color_neg_att_000", light(color=(-0.5, 1.0, -1.0), att=(0.0, 0.0, 0.0)), nonfinite=True),  # -x / 0
    # the light on the surface where the centre ray meets it: nrm(0) = 0 * inf
    _light("at_hit", light(pos=HIT), nonfinite=True, aim="nan_rgb", flat=True),
    _light("behind", light(pos=(1.0, 1.0, 3.0))),
    _light("at_origin", light(pos=(0.0, 0.0, 0.0))),
    _light("at_1e30", light(pos=(1e30, 1e30, 1e30))),  # dist^2 = inf: ldir = 0, att = 0
    _light("pos_nan", light(pos=(NAN, 12.0, 14.0)), nonfinite=True),
    _light("pos_inf", light(pos=(INF, 12.0, 14.0)), nonfinite=True, pin="undefined"),
    # -- alpha: color[3] == 1 ends the ray, in hit_opacity and again in the shade kernel
    *[Case("alpha_" + label, "alpha", material={"color": (0.9, 0.5, 0.2, v)}, hosts=BOTH, nonfinite=v != v or v == INF)
      for label, v in (("0", 0.0), ("0p5", 0.5), ("below_1", BELOW_1), ("above_1", ABOVE_1), ("2", 2.0), ("m1", -1.0),
                       ("nan", NAN), ("inf", INF))],
    # single-sided surfaces seen from behind give vec4(0) and the ray goes on: frag starts at 0.5 under the crosshair
    Case("single_sided_behind", "alpha", specs=(RECT_AWAY,), material={"double_sided_normals": 0},
         params={"crosshair": 1}, hosts=BOTH),
    Case("single_sided_flipped", "alpha", material={"double_sided_normals": 0, "flip_normals": 1},
         params={"crosshair": 1}, hosts=BOTH),
    Case("single_sided_behind_flipped_half", "alpha", specs=(RECT_AWAY,),  # seen again, and translucent
         material={"double_sided_normals": 0, "flip_normals": 1, "color": (0.9, 0.5, 0.2, 0.5)},
         params={"crosshair": 1}, hosts=BOTH),
    Case("hit_log_weighted", "alpha", specs=LAYERS, material=TEXTURED, material2={"texture_index": 1},
         textures="logged13x9", camera=SIDEWAYS, params={"filter_mode": 1}, pin=None),
    # -- mapping: uv * texture_sizes / max_texture_size, the planes' offset, size, repeat and inversion
    *[Case(f"map_{which}_{_name(v)}", "mapping", material=TEXTURED, scene=_sizes(which, v))
      for which in ("texture_sizes", "max_texture_size") for v in (0.0, -3.0, NAN, INF, 1e30)],
    Case("map_sizes_twice_max", "mapping", material=TEXTURED, scene=_twice_max),
    # Without repeat the texture shows where 0 <= puv <= 1, puv = (uv - offset) / size: nowhere for a size of 0 (x / 0),
    # NaN and 1e-30 and for offsets of 1e30, and for the negative size except with the inversion (uv = size - uv). The
    # frame is then the untextured one, the baseline itself: no minimum for these (a kernel that textured a pixel would
    # still differ from the oracle).
    *[Case(f"map_plane_{label}_rep{rep}_inv{inv}", "mapping", specs=({**PLANE, **over, "repeat_texture": rep},),
           material={"texture_index": 0, "invert_uv_x": inv, "invert_uv_y": inv},
           visible=0.0 if rep == 0 and (label, inv) != ("size_neg", 1) else MIN_SHARE)
      for label, over in (("size_0", {"texture_size": (0.0, 0.0)}), ("size_neg", {"texture_size": (-4.0, -3.0)}),
                          ("size_nan", {"texture_size": (NAN, NAN)}), ("size_1em30", {"texture_size": (1e-30, 1e-30)}),
                          ("offset_1e30", {"texture_offset": (1e30, 1e30)}),
                          ("offset_m1e30", {"texture_offset": (-1e30, -1e30)}))
      for rep in (0, 1) for inv in (0, 1)],
    *[Case(f"map_normal_map_index_{i}", "mapping", material={"normal_map_index": i}, textures="nm_rand7x5",
           pin="pin" if i < 2 else None)  # (the shader's profile holds two texture_sizes)
      for i in (0, 1, 2, 11)],
    Case("map_no_array", "mapping", material=TEXTURED, textures="no_array", pin=None),
    # -- normal maps: surface_frame of every type, nrm(frame * texel)
    # (the disk's centre lies on the centre ray: its tangent is nrm(0))
    *[Case("nm_" + kind, "normalmap", specs=(spec,), material=NORMAL_MAPPED, textures="nm_rand7x5",
           nonfinite=kind == "disk", aim="nan_rgb" if kind == "disk" else None)
      for kind, spec in OBJECTS.items()],
    *[Case("nm_box_" + view, "normalmap", specs=(BOX,), material={**NORMAL_MAPPED, "texture_index": 0},
           textures="nm_rand7x5",
           camera=(tuple(c + d for c, d in zip(BOX_CENTRE, off)), BOX_CENTRE, 50.0))
      for view, off in BOX_VIEWS.items()],
    Case("nm_rect_tilted", "normalmap", specs=({**RECT, "axes": X.axes_up((0.2, 0.3, 1.0))},), material=NORMAL_MAPPED,
         textures="nm_rand7x5"),
    Case("nm_rect_sheared", "normalmap", specs=({**RECT, "axes": X.sheared(FACING)},), material=NORMAL_MAPPED,
         textures="nm_rand7x5"),
    Case("nm_sphere_sheared", "normalmap", specs=({**OBJECTS["sphere"], "axes": X.sheared(OBJECTS["sphere"]["axes"])},),
         material=NORMAL_MAPPED, textures="nm_rand7x5"),
    Case("nm_flipped", "normalmap", material={**NORMAL_MAPPED, "flip_normals": 1}, textures="nm_rand7x5"),
    Case("nm_textured", "normalmap", material={**NORMAL_MAPPED, "texture_index": 0}, textures="nm_rand7x5"),
    Case("nm_3x2", "normalmap", material=NORMAL_MAPPED, textures="nm_rand3x2"),
    Case("nm_zero", "normalmap", material=NORMAL_MAPPED, textures="nm_zero", nonfinite=True, pin="undefined"),
    Case("nm_blue", "normalmap", material=NORMAL_MAPPED, textures="nm_blue"),
    # -- seams of the uv maps, the special point on the centre ray
    Case("seam_sphere_pole", "seams", specs=(POLE_SPHERE,), material=TEXEL_ONLY, aim=("texel", 0.0, 1.0), flat=True),
    Case("seam_disk_centre", "seams", specs=(CENTRE_DISK,), material=TEXEL_ONLY, aim=("texel", 0.0, 0.0), flat=True),
    Case("seam_annulus_centre", "seams", specs=(CENTRE_ANNULUS,), material=TEXEL_ONLY, aim=("texel", 0.0, 0.0),
         flat=True),
    Case("seam_cylinder_phi0", "seams", specs=(SEAM_CYLINDER,), material=TEXEL_ONLY, flat=True),
    # inner == outer accepts no point (extreme_cases' zero group); one float below, the ring is 2.4e-7 wide and no
    # chord of these frames lands in it: no minimum for either
    Case("seam_annulus_inner_eq_outer", "seams", specs=({**CENTRE_ANNULUS, "inner": 3.0},), material=TEXEL_ONLY,
         visible=0.0),
    Case("seam_annulus_inner_below_outer", "seams",
         specs=({**CENTRE_ANNULUS, "inner": float(np.nextafter(F32(3.0), F32(0.0)))},), material=TEXEL_ONLY,
         visible=0.0),
    # -- skyboxes: get_bg's atan2 / asin and bilinear at sizes where every lookup wraps; the hole alone
    *[Case(f"sky_{w}x{h}x{ch}_{view}_f{f}", "skybox", specs=(), camera=cam, params={"filter_mode": f},
           textures=f"sky{w}x{h}x{ch}", flat=True, pin="pin" if (f, view, w, h, ch) in SKY_PINNED else None)
      for w, h in SKY_SIZES for ch in (3, 4) for view, cam in SKY_CAMERAS.items() for f in (0, 1)
      if f == 0 or (w, h) in ((2, 1), (5, 7))],
    Case("sky_5x7x4_behind_half_alpha", "skybox", material={"color": (0.9, 0.5, 0.2, 0.5)}, textures="sky5x7x4",
         flat=True),
    Case("sky_none", "skybox", specs=(), textures="no_bg", flat=True, pin=None),
]

BY_NAME = {c.name: c for c in CASES}
