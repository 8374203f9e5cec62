"""The host precomputation (csrc/host/precompute.cpp), pinned on the CPU.

The culling is exact by margins this code derives (bounds, budget slots, the
test ray's culling bounds, a frame's xplane_s / out_dip / max_dphi / bh_u2 /
bh_u3 / win_ok, the low-energy exclusions), and a margin that is slightly
wrong need not change a pixel of any test frame. So its output bytes are held
to digests recorded from the revision before the arithmetic was moved out of
sr_api.cpp (tests/golden/make_host_precompute_digests.py says how), over
every scene this suite builds, three kinds of test ray, every view_cases row
on two scenes and the texel-edge texture arrays. The step table is checked
against a restatement instead, and the unit is run under the host sanitizers
in a stand-alone program. No GPU: the sr_debug_* exports call the functions
sr_set_scene, sr_set_test_ray and a launch pack with.
"""
import ctypes as C
import json
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import extreme_cases as X
import host_precompute_cases as cases
import test_low_energy_bounds as L

ROOT = Path(__file__).resolve().parents[1]
DIGESTS = ROOT / "tests" / "golden" / "host_precompute_digests.json"
KINDS = ("scenes", "test_rays", "frames", "opacity")


@pytest.fixture(scope="module")
def computed(pkg):
    return cases.compute(pkg)


@pytest.fixture(scope="module")
def recorded():
    return json.loads(DIGESTS.read_text())


@pytest.mark.parametrize("kind", KINDS)
def test_bytes_match_the_recorded_digests(computed, recorded, kind):
    got, want = computed[kind], recorded[kind]
    assert sorted(got) == sorted(want), "the case list changed: record the new cases from an unchanged library"
    wrong = [name for name in want if got[name] != want[name]]
    assert not wrong, f"{len(wrong)} of {len(want)} {kind} digests differ: {wrong[:8]}"


def test_the_cases_are_not_vacuous(pkg, recorded):
    """Enough cases, distinct outputs, and the non-finite and max-capacity ones among them."""
    assert len(recorded["scenes"]) >= 300 and len(set(recorded["scenes"].values())) >= 200
    assert len(set(recorded["frames"].values())) == len(recorded["frames"]) >= 100
    assert len(set(recorded["test_rays"].values())) == 4
    assert any(c.group == "nonfinite" for c in X.CASES)
    assert pkg.scenes.scene_stress().num_objects == pkg.abi.MAX_OBJECTS
    # a scene the library rejects digests as its status alone
    bad = pkg.scenes.scene_default(False)
    bad.num_objects = pkg.abi.MAX_OBJECTS + 1
    assert pkg.abi.debug_pack_scene(bad) == (pkg.abi.SR_E_CAPACITY, None, None)


class FrameHead(C.Structure):
    """csrc/device_scene.h sr_dev_frame up to max_dphi."""
    _fields_ = ([("cam", C.c_float * (15 * 32)), ("batch", C.c_int32), ("tiles", C.c_int32),
                 ("out_frame_stride", C.c_int64)] +
                [(n, C.c_float) for n in ("max_angle", "res_x", "res_y", "u_f", "uf_radius", "uf_radius2",
                                          "percent_black", "curved_percentage")] +
                [(n, C.c_int32) for n in ("max_steps", "raytrace_type", "crosshair", "filter_mode", "cull", "width",
                                          "height", "grid", "uv_width", "uv_height", "nrows", "row_base", "block_rows",
                                          "block_stride")] +
                [("block_list", C.c_void_p), ("wave_cost", C.c_void_p), ("out_dip", C.c_float)] +
                [(n, C.c_int32) for n in ("bg_w", "bg_h", "arr_w", "arr_h", "arr_layers", "split_tiles", "split_log2",
                                          "split_min_steps", "win_ok", "num_budget", "num_budget_cyl", "tr_visible")] +
                [("max_dphi", C.c_float)])


def frame_head(pkg, max_steps, max_revs, w=68, h=44):
    abi = pkg.abi
    prm = abi.default_params(max_steps=max_steps, max_revolutions=max_revs)
    rc, raw = abi.debug_frame(pkg.scenes.scene_default(True), None, abi.default_camera(), prm, w, h)
    assert rc == abi.SR_OK
    fr = FrameHead.from_buffer_copy(raw.tobytes()[:C.sizeof(FrameHead)])
    # the mirror's layout: fields on both sides of the ones read decode as given
    assert (fr.batch, fr.max_steps, fr.width, fr.height, fr.nrows, fr.block_rows) == (1, max_steps, w, h, h, h)
    # (the default scene's six objects are all budgeted)
    assert fr.block_list is None and fr.wave_cost is None and fr.num_budget == 6 and fr.split_log2 == 4
    return fr


@pytest.mark.parametrize("max_steps,max_revs", L.CASES + [(1, 1), (7, 0), (400, -1), (3000, 5)])
def test_step_table_and_step_angle_match_their_restatement(pkg, max_steps, max_revs):
    """Bit for bit: step and step / 6 are tests/test_low_energy_bounds.py's
    binary32 restatement, cos and sin the binary64 functions of the binary32
    angle rounded once, the padding zero; the frame's max_dphi is that
    module's too."""
    t = pkg.abi.debug_step_table(max_steps, max_revs)
    assert t.shape == (max_steps + 4, 4) and not t[max_steps:].any()
    step = L.step_table(max_steps, max_revs)
    assert np.array_equal(t[:max_steps, 0].view(np.uint32), step.view(np.uint32))
    assert np.array_equal(t[:max_steps, 1].view(np.uint32), (step / np.float32(6.0)).view(np.uint32))
    phi, want = np.float32(0.0), np.empty((max_steps, 2), dtype=np.float32)
    for i in range(max_steps):
        phi = np.float32(phi + step[i])
        want[i] = math.cos(float(phi)), math.sin(float(phi))
    assert np.array_equal(t[:max_steps, 2:].view(np.uint32), want.view(np.uint32))
    if max_revs > 0:
        got = np.float32(frame_head(pkg, max_steps, max_revs).max_dphi)
        assert got.view(np.uint32) == np.float32(L.max_dphi(max_steps, max_revs)).view(np.uint32)


def test_precompute_unit_builds_without_hip_and_runs_clean_under_sanitizers(pkg, tmp_path):
    """csrc/host/precompute.cpp with the host compiler alone (-Wall -Wextra
    -Werror, no ROCm include path), linked into tests/cpp/
    test_precompute_sanitized.cpp with AddressSanitizer and UBSan, over the
    max-capacity scene, the non-finite scenes, a 1000-point test ray and
    frames at u_f = 0, NaN and +inf."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    scenes = [pkg.scenes.scene_stress(), pkg.scenes.scene_default(True)]
    scenes += [X.build(pkg, c, h) for c in X.CASES if c.group == "nonfinite" for h in c.hosts]
    assert len(scenes) > 4
    blob = tmp_path / "scenes.bin"
    blob.write_bytes(b"".join(bytes(s) for s in scenes))
    exe = tmp_path / "test_precompute_sanitized"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}",
           f"-I{pkg.abi.PKG_DIR / 'csrc'}", str(pkg.abi.PKG_DIR / "csrc/host/precompute.cpp"),
           str(ROOT / "tests/cpp/test_precompute_sanitized.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    res = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"ALL OK: {len(scenes)} scenes" in res.stdout
