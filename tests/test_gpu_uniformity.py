"""The wave-uniformity the integrate and shade kernels assert, checked at run time.

geodesic.hip says "this value is the same in every active lane" at 62 places
the compiler does not verify: SGPR constraints of asm statements (SR_PIN on a
budget slot's record, a frame's start record and its header, the texture
sizes of hit_opacity_uniform, the fast loops' "; keep" statements) and
readfirstlane used as an assertion (the budget event's `spent`, (slot, face)
under the two waterfalls, the recording step index, the sequence resume's
frame). Given a per-lane operand the compiler takes the first active lane's
value and nothing faults. `make` also builds lib/libsr_chk.so, the same
kernel source with -DSR_CHECK_UNIFORM (csrc/kernels/uniform.h): every such
site first compares its operand's bits with the first active lane's, over the
active lanes, and counts the waves that reached it (seen) and the waves whose
lanes disagreed (bad); the kernel goes on as the shipping one does.

Every group below runs its launches on libsr.so and on libsr_chk.so and
asserts
- bad == 0 at every site, offenders named by site, source line and group;
- every output of the checked launch (RGBA8, float FragColor, steps, costs,
  pick maps) equal to the shipping library's, bit for bit: checking does not
  alter the frame, and the checked build is a third register allocation
  (tests/test_gpu_allocation.py).
The shipping library's frames of these same cases are held to the oracle by
the modules the cases come from. The last test asserts seen > 0 at every site
over the whole module (it needs the tests before it: run the module whole).
"""
import contextlib
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import extreme_cases as X
import shading_cases as S
import view_cases as V
from sequence_cases import MIX, Sequences
from test_gpu_launch_matrix import LIST, NB8, H, W
from test_gpu_view_extremes import BATCHES

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LIBCHK = ROOT / "schwarzschild-raytracer_amd" / "lib" / "libsr_chk.so"
SELF_SITES = ("SELF_LANE", "SELF_CONST", "SELF_NAN", "SELF_BRANCH")
# sites of code the build compiles out: {name: reason} (none: with
# SR_NC_KERNEL = 0 the dead cylinder-plane code holds no asserted site)
EXEMPT = {}


class Uniform:
    """The two libraries, a renderer on each, and the checked build's counters."""

    def __init__(self, pkg, textures):
        assert LIBCHK.exists(), "lib/libsr_chk.so not built (make -C schwarzschild-raytracer_amd)"
        self.pkg = pkg
        self.lib = lib = pkg.abi.load(LIBCHK)
        lib.sr_debug_uniform_sites.restype = C.c_int
        lib.sr_debug_uniform_site_name.restype = C.c_char_p
        lib.sr_debug_uniform_site_name.argtypes = [C.c_int]
        self.n = int(lib.sr_debug_uniform_sites())
        self.names = [lib.sr_debug_uniform_site_name(i).decode() for i in range(self.n)]
        self.bg, self.arr = textures
        self.ship, self.chk = pkg.Renderer(0), pkg.Renderer(0, lib=lib)
        self.textures(self.bg, self.arr)
        self.total_seen = np.zeros(self.n, dtype=np.int64)
        self.groups = 0

    @property
    def both(self):
        return (self.ship, self.chk)

    def textures(self, bg, arr):
        for r in self.both:
            r.set_background(bg)
            r.set_texture_array(arr)

    def reset_counters(self):
        assert self.lib.sr_debug_uniform_reset() == 0

    def counters(self):
        seen, bad = (C.c_uint * self.n)(), (C.c_uint * self.n)()
        assert self.lib.sr_debug_uniform_read(seen, bad, self.n) == 0
        return np.array(seen, dtype=np.int64), np.array(bad, dtype=np.int64)

    def lines(self):
        out = (C.c_int * self.n)()
        assert self.lib.sr_debug_uniform_lines(out, self.n) == 0
        return list(out)

    def reset_state(self, test_ray):
        for r in self.both:
            r.set_split(0)
            r.set_latency_mode(False)
            r.set_culling(True)
            r.set_projection("rectilinear")
            r.set_test_ray(test_ray)

    def close(self):
        for r in self.both:
            r.close()


@pytest.fixture(scope="module")
def u(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    un = Uniform(pkg, textures)
    yield un
    un.close()


@pytest.fixture(scope="module")
def sq(pkg, oracle, textures):
    return Sequences(pkg, oracle, textures)  # (its World: the scenes, cameras and the press-R polyline; no oracle frame)


@contextlib.contextmanager
def group(u, sq, label):
    """The launches of one group: counters reset before, read after; the
    context state is put back; bad == 0 at every site. A group whose frames
    differ between the libraries still reports its counters: the line whose
    lanes disagree is the likelier cause."""
    u.reset_state(sq.wd.test_rays[False])
    u.reset_counters()
    differs = None
    try:
        yield
    except pytest.fail.Exception as e:  # pair(): an output differs
        differs = e
    finally:
        u.reset_state(sq.wd.test_rays[False])
        u.textures(u.bg, u.arr)
    seen, bad = u.counters()
    u.total_seen += seen
    u.groups += 1
    if bad.any():
        lines = u.lines()
        pytest.fail(f"{label}: lanes of one wave disagree at " + "; ".join(
            f"{u.names[i]} (line {lines[i]}): {bad[i]} of {seen[i]} waves" for i in np.flatnonzero(bad))
            + (f"; and {differs.msg}" if differs else ""))
    if differs:
        raise differs
    assert seen.sum() > 0, f"{label}: the checked library counted nothing"


def host(tensors):
    import torch

    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def pair(u, label, fn):
    """fn(renderer) -> [(what, tensor)] on both libraries: every output equal, bit for bit."""
    outs = []
    for r in u.both:
        named = fn(r)
        outs.append(([n for n, _ in named], host([t for _, t in named])))
    (names, a), (_, b) = outs
    assert len(a) == len(b) and len(a) > 0
    for what, x, y in zip(names, a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, (label, what)
        if x.tobytes() != y.tobytes():
            n = int((np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8)).sum())
            pytest.fail(f"{label}, {what}: the checked library's output differs from libsr.so's in {n} bytes")


def debug(r, cam, prm, w, h, y0=0, y1=None, what="debug", launches=1):
    for _ in range(launches):
        f, b, s = r.render_debug(cam, prm, w, h, y0, y1)
    return [(what + " FragColor", f), (what + " RGBA8", b), (what + " steps", s)]


def filled(shape):
    import torch

    return torch.full(shape, 77, dtype=torch.uint8, device="cuda")


def test_checked_library_shares_the_abi(pkg, u):
    """The checked library differs from libsr.so only in the kernels' checks: same ABI (struct sizes)."""
    n = 6
    a, b = (C.c_size_t * n)(), (C.c_size_t * n)()
    pkg.abi.load().sr_abi_struct_sizes(a, n)
    u.lib.sr_abi_struct_sizes(b, n)
    assert list(a) == list(b)
    assert len(set(u.names)) == u.n and set(SELF_SITES) <= set(u.names) and set(EXEMPT) <= set(u.names)


def test_selftest(u):
    """One 64-lane wave through the kernels' own macros: the lane index is
    reported, a constant and a NaN constant are not (bits are compared), nor is
    a value equal among the odd lanes inside `if (lane & 1)` that the even
    lanes never evaluate (the exec mask is honoured). One wave each: the check
    is not compiled away and counts once per wave."""
    u.reset_counters()
    assert u.lib.sr_debug_uniform_selftest() == 0
    seen, bad = u.counters()
    u.total_seen += seen
    got = {n: (int(seen[u.names.index(n)]), int(bad[u.names.index(n)])) for n in SELF_SITES}
    assert got == {"SELF_LANE": (1, 1), "SELF_CONST": (1, 0), "SELF_NAN": (1, 0), "SELF_BRANCH": (1, 0)}
    others = [i for i, n in enumerate(u.names) if n not in SELF_SITES]
    assert not seen[others].any() and not bad[others].any()
    lines = u.lines()
    assert all(lines[u.names.index(n)] > 0 for n in SELF_SITES)


# ---- the launch matrix at 68x44 ---------------------------------------------------------
CONFIGS = {"plain": (False, True), "overlay": (True, True), "cull_off": (False, False), "overlay_cull_off": (True, False)}


def matrix_launches(r, wd, key, overlay, cull):
    prm, cam, cams = wd.params(), wd.cams["view"], wd.cam_array(wd.batch)
    r.set_scene(wd.scene(key))
    r.set_test_ray(wd.test_rays[overlay])
    r.set_culling(cull)
    out = debug(r, cam, prm, W, H)
    out += debug(r, cam, prm, W, H, 7, 25, "row band")
    out.append(("rows [40, H)", r.render(cam, prm, W, H, 40, H)))
    for first, step in ((0, 1), (1, 2)):
        buf = filled((len(range(first, NB8, step)) * 8, W, 4))
        r.render_blocks(cam, prm, W, H, 8, first, step, out=buf)
        out.append((f"blocks ({first}, {step})", buf))

    def batch_and_list(what):
        res = []
        buf = filled((3, len(range(1, NB8, 2)) * 8, W, 4))
        lst = filled((3, len(LIST) * 8, W, 4))
        for _ in range(2):  # the second launch runs the learned order (and the split tiles)
            r.render_blocks_batch(cams, prm, W, H, 8, 1, 2, out=buf)
            r.render_block_list(cams, prm, W, H, 8, LIST, out=lst)
        return res + [(what + "batch (1, 2)", buf), (what + "padded block list", lst)]

    out += batch_and_list("")
    for lanes in (16, 4, 1):
        r.set_split(4, lanes, 1)
        out += debug(r, cam, prm, W, H, what=f"split {lanes}", launches=2)
        out += batch_and_list(f"split {lanes} ")
    r.set_split(0)
    r.set_latency_mode(True)
    out += debug(r, cam, prm, W, H, what="latency")
    out += batch_and_list("latency ")
    r.set_latency_mode(False)
    out.append(("wave costs", r.wave_costs(cam, prm, W, H)))
    return out


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("key", ["small", "general", "large", "stacked"])
def test_launch_matrix(u, sq, key, config):
    """Small, general and large scenes and the stack of translucent layers
    (every ray through the resume kernel), overlay off and on, culling on and
    off, through a row band, 8-row blocks, a three-camera batch, a padded
    block list, split tiles of 16, 4 and 1 lanes, latency mode and sr_wave_costs."""
    overlay, cull = CONFIGS[config]
    label = f"launch matrix {key}-{config}"
    with group(u, sq, label):
        pair(u, label, lambda r: matrix_launches(r, sq.wd, key, overlay, cull))


# ---- scene sequences ----------------------------------------------------------------------
@pytest.mark.parametrize("window", [4, 32])
def test_scene_sequences(u, sq, window):
    """The mixed sequence (slot, cylinder and object counts change from frame
    to frame; the translucent stack, whose rays the resume kernel's per-frame
    pass continues, and the empty scene among them), repeated to 32 scenes:
    windows of 4 and of 32 frames with three cameras in turn, the overlay on,
    split tiles on, a padded block list and a supersampled launch."""
    wd = sq.wd
    scenes = [sq.scenes("MIX")[k % len(MIX)] for k in range(32 + 2)]
    first = 2  # general, stacked, large_translucent, the hole alone, small, large, ...
    w, h = (W, H) if window == 4 else (33, 17)
    cams = [wd.cams[wd.batch[f % 3]] for f in range(window)]
    prm = wd.params()

    def launches(r):
        r.set_scene_sequence(scenes)
        out = []
        for overlay in (False, True):
            r.set_test_ray(wd.test_rays[overlay])
            for lanes in (0, 16, 1):
                r.set_split(4 if lanes else 0, lanes or 16, 1)
                for _ in range(2):  # the second launch runs the learned order and the split tiles
                    seq = r.render_sequence(first, cams, prm, w, h, out=filled((window, h, w, 4)))
                out.append((f"sequence overlay {overlay} split {lanes}", seq))
            blocks = LIST if h == H else [1, -1, 0, 2]
            lst = filled((window, len(blocks) * 8, w, 4))
            for _ in range(2):
                r.render_sequence_block_list(first, cams, prm, w, h, 8, blocks, out=lst)
            out.append((f"sequence block list overlay {overlay}", lst))
            r.set_split(0)
        out.append(("sequence ss 2", r.render_sequence(first, cams[:4], prm, w // 2, h // 2, ss=2)))
        out += debug_sequence(r, first + 1, cams[0], prm, w, h)
        r.set_scene_sequence([])
        return out

    def debug_sequence(r, k, cam, prm, w, h):
        f, b, s = r.render_sequence_debug(k, cam, prm, w, h)
        return [("sequence debug FragColor", f), ("sequence debug RGBA8", b), ("sequence debug steps", s)]

    label = f"scene sequence, window {window}"
    with group(u, sq, label):
        pair(u, label, launches)


# ---- projections, supersampling, the sparse launch, retained frames ----------------------
@pytest.mark.parametrize("key", ["small", "large", "stacked"])
@pytest.mark.parametrize("projection", ["rectilinear", "equirect", "fisheye"])
def test_projections_and_sample_paths(u, sq, projection, key):
    """Each projection: a debug frame, a batch, sr_render_ss at ss 2, one
    sr_render_accumulate of three phases, sr_render_adaptive (the sparse
    launch), and sr_reshade, sr_reshade_debug and sr_pick_map after a launch;
    overlay off and on."""
    wd = sq.wd
    prm, cam, cams = wd.params(), wd.cams["view"], wd.cam_array(wd.batch)

    def launches(r):
        r.set_scene(wd.scene(key))
        r.set_projection(projection)
        out = []
        for overlay in (False, True):
            t = f"overlay {overlay} "
            r.set_test_ray(wd.test_rays[overlay])
            # (a batch's buffer holds whole 8-row blocks: the rows past the frame keep the fill)
            out.append((t + "batch", r.render_blocks_batch(cams, prm, W, H, 8, 0, 1, out=filled((3, NB8 * 8, W, 4)))[0]))
            out.append((t + "reshade of the batch", r.reshade(out=filled((3, NB8 * 8, W, 4)))))
            out.append((t + "pick map of the batch", r.pick_map()))
            out.append((t + "ss 2", r.render_ss(cam, prm, W // 2, H // 2, 2)))
            out.append((t + "accumulate", r.render_accumulate(cam, prm, W // 2, H // 2, 2, [(0, 0), (1, 0), (1, 1)])))
            frame, mask = r.render_adaptive(cam, prm, W, H, 2, 32)
            out += [(t + "adaptive", frame), (t + "adaptive tiles", mask)]
            out += debug(r, cam, prm, W, H, what=t + "debug")
            f, b, s = r.reshade_debug()
            out += [(t + "reshade_debug FragColor", f), (t + "reshade_debug RGBA8", b), (t + "reshade_debug steps", s)]
            out.append((t + "pick map", r.pick_map()))
        return out

    label = f"{projection}, {key}"
    with group(u, sq, label):
        pair(u, label, launches)


# ---- non-finite scenes and cameras ---------------------------------------------------------
def test_nonfinite_slot_fields(pkg, u, sq):
    """NaN and inf in slot fields (tests/extreme_cases.py "nonfinite", and
    the zero and signed sizes and broken frames, whose slot records hold inf
    margins), culling on and off: bits are compared, so a NaN field equal in
    every lane is uniform."""
    cells = [c for c in X.cells() if c[0].group in ("nonfinite", "zero", "frames") and c[2] != "100x2"]
    assert sum(c[0].group == "nonfinite" for c in cells) == 4

    def launches(r):
        out = []
        for case, host_key, schedule in cells:
            r.set_scene(X.build(pkg, case, host_key))
            for cull in (True, False):
                r.set_culling(cull)
                out += debug(r, X.camera_of(pkg, case), X.params_of(pkg, case, schedule), X.W, X.H,
                             what=f"{X.cell_id((case, host_key, schedule))} culling {cull}")
        return out

    with group(u, sq, "non-finite slot fields"):
        pair(u, "non-finite slot fields", launches)


@pytest.mark.parametrize("host_key", V.HOSTS)
def test_nonfinite_cameras_and_mixed_batches(pkg, u, sq, host_key):
    """The non-finite rows of tests/view_cases.py (NaN and inf in the camera,
    the field of view, u_f, the split and noise thresholds) and the mixed
    batch of eight cameras with far, NaN, inf and degenerate ones beside the
    default view: one start record per frame, one frame per workgroup."""
    cases = [c for c in V.CASES if not c.finite]
    assert len(cases) >= 10
    cams = [V.default_camera(pkg) if n == "default" else V.camera_of(pkg, V.BY_NAME[n]) for n in BATCHES[host_key]]

    def launches(r):
        r.set_scene(V.host_scene(pkg, host_key))
        out = []
        for case in cases:
            out += debug(r, V.camera_of(pkg, case), V.params_of(pkg, case), *case.size, what=case.name)
        for lanes in (0, 4):
            r.set_split(4 if lanes else 0, lanes or 16, 1)
            for _ in range(2):
                batch, _ = r.render_blocks_batch(cams, V.default_params(pkg), V.W, V.H, 8, 0, 1,
                                                 out=filled((len(cams), (V.H + 7) // 8 * 8, V.W, 4)))
            out.append((f"mixed batch, split {lanes}", batch))
        return out

    label = f"non-finite cameras, {host_key}"
    with group(u, sq, label):
        pair(u, label, launches)


# ---- textured shading: the texture-size pins and the (slot, face) waterfalls ---------------
def test_normal_mapped_primitives(pkg, u, sq):
    """A normal-mapped primitive of each type and the box from its six
    sides (tests/shading_cases.py "normalmap"): shade's waterfall over
    (slot, face), box faces included, alone and before a backdrop."""
    cases = [c for c in S.CASES if c.group == "normalmap" and (c.name in {"nm_" + k for k in S.OBJECTS}
                                                              or c.name.startswith("nm_box_"))]
    assert len(cases) == len(S.OBJECTS) + 6

    def launches(r):
        out = []
        for case in cases:
            bg, arr, _ = S.textures_of(pkg, case.textures)
            r.set_background(bg)
            r.set_texture_array(arr)
            for host_key in ("alone", "stacked"):
                r.set_scene(S.build(pkg, case, host_key))
                out += debug(r, S.camera_of(pkg, case), S.params_of(pkg, case), S.W, S.H, what=f"{case.name} {host_key}")
        return out

    with group(u, sq, "normal-mapped primitives"):
        pair(u, "normal-mapped primitives", launches)


def test_texel_edge_array(pkg, u, sq):
    """One texel-edge array of tests/test_gpu_texel_edges.py (islands, 13x9:
    an odd bitmap stride) on every primitive type with every texture index
    and uv flag combination over the objects, both filters: hit_opacity's
    waterfall and hit_opacity_uniform's pinned texture sizes."""
    import test_gpu_texel_edges as T

    arr = T.texture_array("islands", 13, 9)
    padded = T.padded_array(13, 9, (9, 6))

    def launches(r):
        out = []
        for name, a, sizes in (("islands", arr, [(13, 9)]), ("padded", padded, [(9, 6), (13, 9)])):
            r.set_texture_array(a)
            for k, obj in enumerate(T.OBJECTS):
                texture_index, flags = T.combo_of(2 * k, k)
                r.set_scene(T.textured_scene(pkg, obj, sizes, (13, 9), texture_index, flags))
                for filter_mode in (0, 1):
                    out += debug(r, T.camera(pkg), T.params_of(pkg, filter_mode), T.W, T.H,
                                 what=f"{name} {obj} texture_index {texture_index} flags {flags} filter {filter_mode}")
        return out

    with group(u, sq, "texel-edge arrays"):
        pair(u, "texel-edge arrays", launches)


# ---- the frame round 5's 7-wave build broke -------------------------------------------------
def test_c2t_at_its_fixture_size(pkg, u, sq):
    """c2t (the press-R overlay's 1000 cylinders over config 2, 16,507 pixels
    wrong in round 5's 7-wave build) through the checked library, every row
    against the oracle's hashes (tests/golden/frame_hashes.npz)."""
    from test_gpu_frames import FIXTURE, sha_rows

    A = pkg.assets
    if not A.available():
        pytest.skip("assets/textures missing")
    with np.load(FIXTURE) as z:
        fh = {k: z[k] for k in z.files if k.startswith("c2t/")}
    w, h, n = (int(v) for v in fh["c2t/config"])
    arr, _, _ = A.texture_array()
    sc, abi = pkg.scenes, pkg.abi
    with group(u, sq, "c2t"):
        u.chk.set_background(A.skybox("2k"))
        u.chk.set_texture_array(arr)
        u.chk.set_scene(sc.scene_default(textured=True))
        u.chk.set_test_ray(sc.test_ray_overlay())
        _, b, s = host(u.chk.render_debug(abi.default_camera(), abi.default_params(max_steps=n, percent_black=-1.0), w, h))
        rows = fh["c2t/rows"]
        bad = np.flatnonzero((sha_rows(b[rows]) != fh["c2t/rgba_sha"]).any(-1))
        assert not len(bad), f"c2t (the checked library): {len(bad)} RGBA8 rows differ, first {rows[bad[:5]].tolist()}"
        assert not (sha_rows(s[rows].astype("<i4")) != fh["c2t/steps_sha"]).any(), "c2t: step rows differ"


# ---- coverage: the last test of the module ---------------------------------------------------
def test_zz_every_site_was_reached(u):
    """Over every group above: seen > 0 at every site of the build. A site
    no case reaches is unverified."""
    assert u.groups >= 30, "run the module whole: this test reads the counts of the tests before it"
    lines = u.lines()
    missed = [f"{n} (line {lines[i]})" for i, n in enumerate(u.names) if u.total_seen[i] == 0 and n not in EXEMPT]
    print("MEASURED waves per site: " + ", ".join(f"{n} {u.total_seen[i]}" for i, n in enumerate(u.names)))
    assert not missed, "no wave reached: " + ", ".join(missed)
    for r in u.both:
        assert r.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
