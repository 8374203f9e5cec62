"""sr_scene_shading_only (sr.h "Retained frames") held to a numpy statement of
the field list, without a GPU.

The list: a retained frame outlives a change of num_lights, lights[] and, per
material, color[0..2], ambient, diffuse, specular, shininess and
normal_map_index; every other byte of sr_scene is geometry. The leaves come
from a walk of the ctypes structure itself, which must cover every byte of
it: a field added to sr_scene later is perturbed here too, and is geometry
until the rule below names it.
"""
import ctypes as C
import re

import numpy as np
import pytest

SHADING = re.compile(r"^(num_lights$|lights\[|materials\[\d+\]\.(color\[[012]\]|ambient|diffuse|specular|shininess|"
                     r"normal_map_index)$)")


def leaves(ctype, path="", offset=0):
    """(path, byte offset, simple ctype) of every scalar of a ctypes type."""
    if issubclass(ctype, C.Structure):
        for name, sub in ctype._fields_:
            yield from leaves(sub, f"{path}.{name}" if path else name, offset + getattr(ctype, name).offset)
    elif issubclass(ctype, C.Array):
        for i in range(ctype._length_):
            yield from leaves(ctype._type_, f"{path}[{i}]", offset + i * C.sizeof(ctype._type_))
    else:
        yield path, offset, ctype


@pytest.fixture(scope="module")
def table(pkg):
    out = list(leaves(pkg.abi.Scene))
    covered = np.zeros(C.sizeof(pkg.abi.Scene), dtype=bool)
    for _, off, t in out:
        assert not covered[off:off + C.sizeof(t)].any()
        covered[off:off + C.sizeof(t)] = True
    assert covered.all(), "the walk misses bytes of sr_scene (padding, or a field kind it does not know)"
    return out


@pytest.fixture(scope="module")
def geometry_mask(pkg, table):
    mask = np.ones(C.sizeof(pkg.abi.Scene), dtype=bool)
    for path, off, t in table:
        if SHADING.match(path):
            mask[off:off + C.sizeof(t)] = False
    return mask


def bytes_of(pkg, s):
    return pkg.scenes.struct_bytes(s).view(np.uint8).reshape(-1)


def numpy_rule(pkg, mask, a, b) -> bool:
    return bool(np.array_equal(bytes_of(pkg, a)[mask], bytes_of(pkg, b)[mask]))


def scenes_of(pkg):
    return {"default": pkg.scenes.scene_default(True), "stress": pkg.scenes.scene_stress()}


def perturbed(pkg, scene, off, t, how):
    raw = bytes_of(pkg, scene).copy()
    if t is C.c_float:
        v = raw[off:off + 4].view(np.float32)
        v[0] = {"step": np.nextafter(v[0], np.float32(np.inf)) if np.isfinite(v[0]) else np.float32(1.0),
                "far": np.float32(v[0] + 3.5) if np.isfinite(v[0]) else np.float32(-2.0),
                "nan": np.float32(np.nan)}[how]
    else:
        assert t is C.c_int32, t
        v = raw[off:off + 4].view(np.int32)
        v[0] = {"step": v[0] + 1, "far": v[0] ^ 0x40000000, "nan": -1 if v[0] != -1 else 0}[how]
    return pkg.scenes.struct_from_bytes(pkg.abi.Scene, raw)


def test_field_list_counts(pkg, table):
    """The rule names what sr.h names: 1 + 4 * 19 light scalars and 8 scalars
    of each of the 10 materials."""
    abi = pkg.abi
    n = sum(1 for path, _, _ in table if SHADING.match(path))
    assert n == 1 + abi.MAX_LIGHTS * (C.sizeof(abi.Light) // 4) + abi.MAX_MATERIALS * 8
    assert all(C.sizeof(t) == 4 for _, _, t in table)


@pytest.mark.parametrize("how", ["step", "far", "nan"])
@pytest.mark.parametrize("name", ["default", "stress"])
def test_every_field_one_at_a_time(pkg, table, geometry_mask, name, how):
    a = scenes_of(pkg)[name]
    wrong = []
    kinds = {True: 0, False: 0}
    for path, off, t in table:
        b = perturbed(pkg, a, off, t, how)
        assert not np.array_equal(bytes_of(pkg, a), bytes_of(pkg, b)), path
        want = numpy_rule(pkg, geometry_mask, a, b)
        assert want == bool(SHADING.match(path)), path
        kinds[want] += 1
        for x, y in ((a, b), (b, a)):
            if bool(pkg.abi.scene_shading_only(x, y)) != want:
                wrong.append(path)
    assert not wrong, f"{len(wrong)} fields classified wrongly, first {wrong[:8]}"
    assert kinds[True] > 100 and kinds[False] > 400


def test_identical_null_and_nan(pkg, table, geometry_mask):
    abi, lib = pkg.abi, pkg.abi.load()
    for name, a in scenes_of(pkg).items():
        same = pkg.scenes.struct_from_bytes(abi.Scene, pkg.scenes.struct_bytes(a))
        assert lib.sr_scene_shading_only(C.byref(a), C.byref(same)) == 1, name
        assert lib.sr_scene_shading_only(None, C.byref(a)) == 0
        assert lib.sr_scene_shading_only(C.byref(a), None) == 0
        assert lib.sr_scene_shading_only(None, None) == 0
        # a NaN in a geometry field on both sides equals itself (bytes), on one side it is a change
        for path in ("spheres[0].radius", "materials[3].color[3]", "texture_sizes[1][0]", "boxes[2].transform.axes[4]"):
            off, t = next((o, t) for p, o, t in table if p == path)
            n1, n2 = perturbed(pkg, a, off, t, "nan"), perturbed(pkg, a, off, t, "nan")
            assert lib.sr_scene_shading_only(C.byref(n1), C.byref(n2)) == 1, (name, path)
            assert lib.sr_scene_shading_only(C.byref(a), C.byref(n1)) == 0, (name, path)
            # ... and stays equal under a shading-only change on top
            off2, t2 = next((o, t) for p, o, t in table if p == "lights[1].intensity")
            assert lib.sr_scene_shading_only(C.byref(n1), C.byref(perturbed(pkg, n2, off2, t2, "far"))) == 1


def test_many_shading_fields_at_once(pkg, geometry_mask):
    """The relit scenes of the GPU tests: every shading-only field changed,
    nothing else; one geometry field on top drops it."""
    import reshade_cases as R

    for name, a in scenes_of(pkg).items():
        b = R.relit(pkg, a)
        assert numpy_rule(pkg, geometry_mask, a, b) and pkg.abi.scene_shading_only(a, b), name
        changed = bytes_of(pkg, a) != bytes_of(pkg, b)
        assert changed[~geometry_mask].reshape(-1, 4).any(-1).mean() > 0.5, name  # (the lights' axes stay the identity)
        b.materials[9].flip_normals ^= 1  # a material no object of the default scene uses
        assert not pkg.abi.scene_shading_only(a, b), name
