"""The scene-sequence calls of sr.h exist, with its prototypes, and reject a null context.

No device: everything here returns before the first HIP call.
"""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
INV = -1

# sr.h "Scene sequences", parameter types in order
PROTOTYPES = {
    "sr_set_scene_sequence": "sr_ctx*, const sr_scene*, int",
    "sr_scene_sequence_length": "sr_ctx*",
    "sr_render_sequence": "sr_ctx*, int, const sr_camera*, int, const sr_params*, int, int, int, int, int, uint8_t*, "
                          "size_t, size_t, sr_stream",
    "sr_render_sequence_block_list": "sr_ctx*, int, const sr_camera*, int, const sr_params*, int, int, int, "
                                     "const int*, int, int, uint8_t*, size_t, size_t, sr_stream",
    "sr_render_sequence_debug": "sr_ctx*, int, const sr_camera*, const sr_params*, int, int, int, int, float*, "
                                "uint8_t*, int32_t*, sr_stream",
}


def header_prototype(name):
    text = (ROOT / "include" / "sr" / "sr.h").read_text()
    m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
    assert m, f"{name} is not declared in sr.h"
    types = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        t = re.sub(r"\s*\b[a-z_0-9]+$", "", arg) if re.search(r"[\s*][a-z_0-9]+$", arg) else arg  # drop the name
        types.append(t.replace(" *", "*"))
    return ", ".join(types)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_symbol_and_prototype(pkg, name):
    lib = pkg.abi.load()
    assert hasattr(lib, name), f"libsr.so does not export {name}"
    assert header_prototype(name) == PROTOTYPES[name]
    res, args = pkg.abi.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(PROTOTYPES[name].split(", "))


def test_capacity_constant(pkg):
    text = (ROOT / "include" / "sr" / "sr.h").read_text()
    assert re.search(r"^#define SR_MAX_SEQUENCE 256$", text, re.M)
    assert pkg.abi.MAX_SEQUENCE == 256


def test_null_context_is_invalid(pkg):
    abi = pkg.abi
    lib = abi.load()
    scene, cam, prm = abi.default_scene(), abi.default_camera(), abi.default_params()
    blocks = (C.c_int * 2)(0, 1)
    out = (C.c_uint8 * (16 * 16 * 4))()
    o = C.cast(out, C.c_void_p)
    assert lib.sr_set_scene_sequence(None, C.byref(scene), 1) == INV
    assert lib.sr_set_scene_sequence(None, None, 0) == INV
    assert lib.sr_scene_sequence_length(None) == INV
    for ss in (1, 2):
        assert lib.sr_render_sequence(None, 0, C.byref(cam), 1, C.byref(prm), 16, 16, 0, 16, ss, o, 64, 1024, None) == INV
        assert lib.sr_render_sequence_block_list(None, 0, C.byref(cam), 1, C.byref(prm), 16, 16, 8, blocks, 2, ss, o,
                                                 64, 1024, None) == INV
    assert lib.sr_render_sequence_debug(None, 0, C.byref(cam), C.byref(prm), 16, 16, 0, 16, None, o, None, None) == INV
    assert bytes(out) == bytes(len(out))
