"""The culling shortcuts at cameras and frame parameters no other module sets
(tests/view_cases.py).

The kernel's budgets, windows, exclusions and the coasting loop
are exact by margin, and the host derives their constants (max_dphi, out_dip,
bh_u2, bh_u3, uf_radius2, xplane_s, xlow_need, xperi_e, win_ok) from
max_steps, max_revolutions, u_f and the camera positions. Every case here
puts one of those inputs at or past an edge: u_f from -0.01 to +inf and NaN,
max_revolutions from -2 to 50, fields of view of 0, 180 and 360 degrees and
beyond, cameras at the origin, on the horizon, at r = 100 exactly (win_ok's
<=) and at 1e25, scaled, sheared, mirrored, zero and NaN axes, the split
modes' and the noise mask's thresholds, 65536 steps. Nothing has a tolerance:
test_gpu_parity.compare (RGBA8, float bits with NaN = NaN, step counts).

A. Every case x {small, large} through render_debug with culling on and off:
   unculled == oracle (the base arithmetic), culled == unculled (the margins),
   culled == oracle. The u_f and revolutions groups also with the press-R
   overlay on "small". The finite cases first, the non-finite ones last.
B. Two batches of eight cameras (default, r = 100, r = 1e5, NaN and infinite
   positions, the origin, zero axes, fov 180, left-handed): win_ok is one flag
   per launch and the start records are per frame.
C. Latency mode and split tiles of 16 and 1 lanes for u_f in {0, 0.5, 1, inf}
   and max_revolutions in {-1, 1, 3, 50}; the learning launch must leave
   split tiles. (-1 runs the culling-off kernel since the fix below: split
   tiles apply to it, latency mode's 2-step loop is the small culling
   instantiation's alone.)
D. Fifteen launches on one stream without a host synchronisation through twelve
   (max_steps, max_revolutions) pairs (the step-table cache holds 8) while
   u_f alternates between 0.01, 0.05, -0.0, 0.0 and NaN (the exclusion cache's
   key is compared as floats).
E. sr_render_ss and sr_render_phase at 34x22, ss = 2, against the oracle's
   68x44 frame of section A.

tests/test_view_cases.py shows on the oracle alone that each case's frame is
what the table says.

Why no loop of geodesic.hip can spin on a wave of NaN state (read before the
first run of this module; every `for (;;)` of the file):
- shade() and hit_opacity(): waterfalls over an integer key. The first active
  lane's key equals its own readfirstlane, so each pass retires at least one
  lane: at most 64 passes, no float compare.
- integrate()'s step loop: leaves at i >= N; every pass that does not return
  goes through the slow path's `i++`, or through `continue` after the
  coasting loop's retirement, which has already done `++i`.
- the fast loop: compute() is a ballot of !(vb < 0) || un < ulo || un > uhi. A
  NaN vb is "not inside" and leaves with the step unapplied (the slow path
  then counts it); when every compare is false apply() does `++i >= N`.
- coast(), inner loop: leaves on !(un >= lo && un <= hi), true for NaN, else
  `++i >= N`. Outer loop: re-entered only through `continue`, after `++i` and
  only while i + 1 < N held.
- the slow path's "past the singularity" break needs no compare to be true:
  !(u < inf) && !(un < inf) holds for NaN and sends the ray to the loop's end.
- recover_up(): a counted loop from the fast loop's entry step to ie - 2 < N.
- sr_resume_kernel's rounds: integrate() returns ST_HIT with r.i = the
  stopping step >= the entry step, the round does r.i++, and integrate()
  entered with r.i >= N returns ST_BG, which ends the rounds.
The step table holds max_steps + 4 entries and no index into it or into a
texture is computed from a ray's floats without a clamp (bilinear() zeroes
coordinates beyond 2^24 and NaN; wrap_rep() reduces modulo the size).

Found with this table, on the library of this module's parent commit (pixels
of 2992 in which the culled frame differs from the frame with culling off;
that one equalled the oracle in every cell, so the base arithmetic was right
everywhere and each figure is also the culled frame's distance from the
oracle):
- rev_m2 435 (small), 696 (large), 435 (small, overlay); rev_m1 436, 696,
  436; rev_m1_uf0p2 836 (small), 0 (large), 836 (overlay); rev_m1 with
  latency mode, split tiles of 16 and of 1 lane: 436 each. The step angle is
  negative and "outward" lanes approach what outward_clear declared passed.
- uf_m0p01 2356 (small), 0 (large), 28 (small, overlay): the loops find
  u < 0 through their lower bound u_f.
- uf_nan 205 (small), 0 (large), 0 (overlay); the caches test's launch with
  max_steps 400, one revolution and u_f = NaN: 112 pixels off the oracle.
- every other cell, finite or not, every batch frame, every launch option
  and every sample mapping: 0.
Launches with max_revolutions <= 0, u_f < 0, u_f = -0.0 or NaN now run the
culling-off instantiation (precompute.cpp derive_frame).
"""
import contextlib

import numpy as np
import pytest

import view_cases as V
from test_gpu_launch_matrix import World, host, reset, same, split_count
from test_gpu_parity import compare
from test_gpu_supersample import box_reference

pytestmark = pytest.mark.gpu

FILL = 77


@pytest.fixture(scope="module")
def gpu(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    bg, arr = textures
    r = pkg.Renderer(0)
    r.set_background(bg)
    r.set_texture_array(arr)
    yield r
    r.close()


class Views:
    """The host scenes, the overlay and the oracle's frames, built once."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        w = World(pkg, oracle, textures)
        self.tex, self.test_rays = w.tex, w.test_rays  # the launch matrix's 177-point press-R polyline
        self.scenes = {h: V.host_scene(pkg, h) for h in V.HOSTS}
        self._ref = {}

    def render(self, host_key, cam, params, size, overlay=False):
        out = self.oracle.render(self.scenes[host_key], cam, params, *size, self.tex, self.test_rays[overlay])
        for a in out:
            a.setflags(write=False)
        return out

    def ref(self, case, host_key, overlay=False):
        """The oracle's (rgba8, float rgba, steps) of a case, read-only."""
        k = (case.name, host_key, overlay)
        if k not in self._ref:
            self._ref[k] = self.render(host_key, V.camera_of(self.pkg, case), V.params_of(self.pkg, case), case.size,
                                       overlay)
        return self._ref[k]


@pytest.fixture(scope="module")
def wd(pkg, oracle, textures):
    return Views(pkg, oracle, textures)


@contextlib.contextmanager
def device(gpu, wd):
    """GPU work of one test: the context's state is reset after it; an error
    of the runtime (not a failed comparison) ends the session, so nothing
    more is launched on a device that faulted."""
    try:
        yield
    except AssertionError:
        raise
    except Exception as e:  # noqa: BLE001
        pytest.exit(f"device error, nothing more is launched: {e!r}", returncode=3)
    finally:
        reset(gpu, wd)


def setup(gpu, wd, host_key, overlay=False):
    gpu.set_scene(wd.scenes[host_key])
    gpu.set_test_ray(wd.test_rays[overlay])


def differing(a, b):
    return int(((a[0] != b[0]).any(-1) | (a[2] != b[2])).sum())


def debug_frames(gpu, cam, params, size, launches=1, after_first=None):
    """(rgba8, float, steps) of the last of `launches` render_debug launches."""
    for i in range(launches):
        f, b, s = gpu.render_debug(cam, params, *size)
        if i == 0 and after_first:
            after_first()
    f, b, s = host(f, b, s)
    return b, f, s


# ---- A. the matrix
def matrix_cells(finite):
    out = [(c, h, False) for c, h in V.cells() if c.finite == finite]
    out += [(c, "small", True) for c in V.CASES if c.finite == finite and c.group in V.OVERLAY_GROUPS]
    return out


def matrix_id(cell):
    return f"{cell[0].name}-{cell[1]}" + ("-overlay" if cell[2] else "")


def run_cell(gpu, wd, cell):
    case, host_key, overlay = cell
    label = matrix_id(cell)
    cam, params = V.camera_of(wd.pkg, case), V.params_of(wd.pkg, case)
    o = wd.ref(case, host_key, overlay)
    with device(gpu, wd):
        setup(gpu, wd, host_key, overlay)
        culled = debug_frames(gpu, cam, params, case.size)
        gpu.set_culling(False)
        unculled = debug_frames(gpu, cam, params, case.size)
    eq = [np.array_equal(culled[0], unculled[0]),
          np.array_equal(culled[1].view(np.uint32), unculled[1].view(np.uint32)),
          np.array_equal(culled[2], unculled[2])]
    px = differing(culled, unculled)
    print(f"MEASURED {label}: culled vs unculled {px} pixels, culled vs oracle {differing(culled, o)}, "
          f"unculled vs oracle {differing(unculled, o)}")
    compare(unculled, o, label + " (culling off: the base arithmetic)")
    assert all(eq), f"{label}: culling changes {px} pixels (rgba8, float bits, steps equal: {eq})"
    compare(culled, o, label + " (culling on)")


@pytest.mark.parametrize("cell", matrix_cells(True), ids=matrix_id)
def test_view_finite(gpu, wd, cell):
    run_cell(gpu, wd, cell)


# ---- E. sample mapping (finite cases; the 68x44 frames are section A's)
@pytest.mark.parametrize("name", ["fov_179p0", "fov_181p0", "fov_m90p0", "axes_sheared", "uf_0p5"])
def test_sample_mapping(gpu, wd, name):
    """The 68x44 frame is the 2 x 2 sample frame of a 34x22 one: sr_render_ss
    is its box average, sr_render_phase's phase (1, 0) is S[0::2, 1::2]."""
    case = V.BY_NAME[name]
    cam, params = V.camera_of(wd.pkg, case), V.params_of(wd.pkg, case)
    S = wd.ref(case, "small")[0]
    with device(gpu, wd):
        setup(gpu, wd, "small")
        ss, ph = host(gpu.render_ss(cam, params, V.W // 2, V.H // 2, 2),
                      gpu.render_phase(cam, params, V.W // 2, V.H // 2, 2, 1, 0))
    same(ss, box_reference(S, 2), f"{name}, sr_render_ss")
    same(ph, S[0::2, 1::2], f"{name}, sr_render_phase (1, 0)")


# ---- C. launch options
OPTION_CASES = ["uf_0", "uf_0p5", "uf_1p0", "rev_m1", "rev_1", "rev_3", "rev_50", "uf_inf"]  # (the non-finite one last)


@pytest.mark.parametrize("option", ["latency", "split16", "split1"])
@pytest.mark.parametrize("name", OPTION_CASES)
def test_launch_options(gpu, wd, name, option):
    """Latency mode's 2-step loop and split tiles (the launch after a
    learning launch) leave every pixel as it was."""
    case = V.BY_NAME[name]
    cam, params = V.camera_of(wd.pkg, case), V.params_of(wd.pkg, case)
    with device(gpu, wd):
        setup(gpu, wd, "small")
        if option == "latency":
            gpu.set_latency_mode(True)
            got = debug_frames(gpu, cam, params, case.size)
        else:
            lanes = int(option[5:])
            gpu.set_split(64, lanes, 1)

            def learned():  # every ray of these frames takes a step, so every tile is split
                n = split_count(gpu)
                assert n > 0 and n % (64 // lanes) == 0, (name, option, n)

            assert wd.ref(case, "small")[2].min() >= 1
            got = debug_frames(gpu, cam, params, case.size, launches=2, after_first=learned)
    compare(got, wd.ref(case, "small"), f"{name}, {option}")


# ---- D. the caches under change
SCHEDULES = [(400, 2), (300, 2), (200, 1), (100, 3), (400, 1), (250, 2), (150, 2), (350, 3), (120, 1), (500, 2),
             (400, 2), (300, 2), (200, 1), (7, 50), (400, -1)]
U_FS = [0.01, 0.05, -0.0, 0.0, V.NAN]


def test_caches_under_change(gpu, wd):
    """Fifteen launches into their own buffers on one stream, no host
    synchronisation before the last: twelve distinct (max_steps,
    max_revolutions) pairs, so the 8-entry step-table cache evicts tables
    (and frees them in stream order) while earlier frames are in flight, and
    the first three pairs come back after their eviction; u_f cycles through
    0.01, 0.05, -0.0, 0.0 and NaN, so the exclusion cache sees equal floats of
    both signs and a key that never equals itself."""
    assert len(set(SCHEDULES)) > 8 and len(SCHEDULES) >= 12
    cam = V.default_camera(wd.pkg)
    prms = [wd.pkg.abi.default_params(**{**V.PARAMS, "max_steps": s, "max_revolutions": r, "u_f": U_FS[k % len(U_FS)]})
            for k, (s, r) in enumerate(SCHEDULES)]
    refs = [wd.render("small", cam, p, (V.W, V.H)) for p in prms]
    assert len({r[0].tobytes() for r in refs}) >= 12
    with device(gpu, wd):
        setup(gpu, wd, "small")
        outs = [gpu.render_debug(cam, p, V.W, V.H) for p in prms]  # asynchronous
        flat = host(*[t for o in outs for t in o])
    for k, ref in enumerate(refs):
        f, b, s = flat[3 * k:3 * k + 3]
        compare((b, f, s), ref, f"launch {k}: schedule {SCHEDULES[k]}, u_f {U_FS[k % len(U_FS)]}")


# ---- A again: the non-finite cases
@pytest.mark.parametrize("cell", matrix_cells(False), ids=matrix_id)
def test_view_nonfinite(gpu, wd, cell):
    run_cell(gpu, wd, cell)


# ---- B. mixed batches
BATCHES = {
    "small": ["default", "uf_0p01_r100", "pos_r1e5_fov2", "pos_nan_y", "pos_origin", "axes_zero", "fov_180p0",
              "axes_left_handed"],
    "large": ["axes_zero", "pos_inf_y", "axes_left_handed", "uf_0p01_r100_up", "fov_180p0", "default", "pos_r1e15_fov2",
              "pos_nan_y"],
}


@pytest.mark.parametrize("host_key", list(BATCHES))
def test_mixed_batches(gpu, wd, host_key):
    """Eight cameras in one sr_render_blocks_batch launch, launched twice (the
    second runs the learned order): the default view among cameras beyond
    r = 100 (win_ok off for the whole launch), non-finite and degenerate
    ones. Every frame equals the oracle's frame of its own camera and its own
    single-frame render. The batch has one set of params, the default ones."""
    import torch

    pkg = wd.pkg
    cams = [V.default_camera(pkg) if n == "default" else V.camera_of(pkg, V.BY_NAME[n]) for n in BATCHES[host_key]]
    params = V.default_params(pkg)
    refs = [wd.render(host_key, c, params, (V.W, V.H))[0] for c in cams]
    assert len({r.tobytes() for r in refs}) >= 6  # (the all-NaN frames are one colour)
    nb = (V.H + 7) // 8
    with device(gpu, wd):
        setup(gpu, wd, host_key)
        single = [host(gpu.render(c, params, V.W, V.H))[0] for c in cams]
        out = torch.full((len(cams), nb * 8, V.W, 4), FILL, dtype=torch.uint8, device="cuda")
        for _ in range(2):
            _, rows = gpu.render_blocks_batch(cams, params, V.W, V.H, 8, 0, 1, out=out)
        (got,) = host(out)
    assert rows == V.H
    for f, name in enumerate(BATCHES[host_key]):
        same(single[f], refs[f], f"{host_key}, single frame {name} against the oracle")
        same(got[f, :rows], refs[f], f"{host_key}, batch frame {f} ({name}) against the oracle")
        same(got[f, :rows], single[f], f"{host_key}, batch frame {f} ({name}) against its single-frame render")
        assert (got[f, rows:] == FILL).all(), f"{host_key}, batch frame {f} ({name}): wrote past its rows"


def test_zz_diag_counters_zero(gpu):
    """After every frame of this module on the shared context: no pixel
    stopped at an opaque-classified hit whose shaded alpha was not 1, and no
    stream-ordered free failed."""
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
