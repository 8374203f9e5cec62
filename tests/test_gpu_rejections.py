"""The status of every rejected call, on every entry point that launches.

One table: a row is one bad call (or two conditions violated at once, which
pins the precedence of adjacent checks). Every row asserts the status, that
no sentinel-filled buffer was touched and that the retained frame
(sr_can_reshade) is as it was: a rejected call launches nothing and drops
nothing. At the end the good render repeats byte for byte.

The expected statuses are the ones the C ABI returned before its checks were
moved into shared helpers (the table was run on that revision first); the
order of the checks it pins is sr_api.cpp's: an entry point's own arguments,
then the context (null, SR_E_NOT_READY without a scene), the cameras and the
batch size (SR_E_CAPACITY), the params, then pitch and frame stride.

68x44 frame, the small scene; no row launches anything.
"""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

W, H = 68, 44
NB8 = (H + 7) // 8
ROWS = NB8 * 8  # rows of the strided-block paths' output (six 8-row blocks)
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
    empty = pkg.Renderer(0)  # a live context that never saw a scene
    yield r, empty
    empty.close()
    r.close()


def table(abi):
    """[(entry point, state, overrides, expected status)]. state: what the
    context holds before the call: "one" (a retained sr_render frame), "two"
    (a retained batch of two), "ss" (a retained supersampled frame), "none"
    (a scene, no retained frame), "empty" (no scene)."""
    INV, CAP, NR = abi.SR_E_INVALID, abi.SR_E_CAPACITY, abi.SR_E_NOT_READY
    big = abi.SR_MAX_STEPS + 1 if hasattr(abi, "SR_MAX_STEPS") else (1 << 24)
    t = []

    def rows(entry, state, *cases):
        for over, want in cases:
            t.append((entry, state, over, want))

    rows("sr_render", "one",
         (dict(out=None), INV), (dict(y0=-1), INV), (dict(y1=H + 1), INV), (dict(y0=5, y1=4), INV),
         (dict(c=None), INV), (dict(cam=None), INV), (dict(p=None), INV), (dict(w=0), INV),
         (dict(h=0, y1=0), INV), (dict(raytrace_type=-1), INV), (dict(raytrace_type=4), INV),
         (dict(filter_mode=2), INV), (dict(max_steps=-1), INV), (dict(max_steps=big), INV),
         (dict(pitch=4 * W - 4), INV), (dict(c=None, out=None), INV))
    rows("sr_render", "empty",
         ({}, NR), (dict(out=None), INV), (dict(y1=H + 1), INV), (dict(cam=None), NR), (dict(max_steps=-1), NR),
         (dict(pitch=4 * W - 4), NR))
    rows("sr_render_debug", "one",
         (dict(y1=H + 1), INV), (dict(y0=3, y1=2), INV), (dict(f32=None, out=None, steps=None), INV),
         (dict(c=None), INV), (dict(max_steps=big), INV), (dict(filter_mode=-1), INV))
    rows("sr_render_debug", "empty", ({}, NR), (dict(f32=None, out=None, steps=None), INV))
    rows("sr_render_blocks", "one",
         (dict(out=None), INV), (dict(br=0), INV), (dict(bf=-1), INV), (dict(bs=0), INV), (dict(c=None), INV),
         (dict(pitch=4 * W - 4), INV), (dict(filter_mode=2), INV), (dict(max_steps=big), INV))
    rows("sr_render_blocks", "empty", ({}, NR), (dict(br=0), INV), (dict(pitch=4 * W - 4), NR))
    rows("sr_render_blocks_batch", "one",
         (dict(out=None), INV), (dict(br=0), INV), (dict(bf=-1), INV), (dict(bs=0), INV), (dict(n=0), INV),
         (dict(n=abi.MAX_BATCH + 1), CAP), (dict(fs=4 * W * ROWS - 4), INV), (dict(pitch=4 * W - 4), INV),
         (dict(n=abi.MAX_BATCH + 1, cams=None), INV), (dict(n=abi.MAX_BATCH + 1, max_steps=-1), CAP),
         (dict(n=abi.MAX_BATCH + 1, br=0), INV), (dict(n=abi.MAX_BATCH + 1, pitch=4 * W - 4), CAP),
         (dict(max_steps=-1, fs=4 * W * ROWS - 4), INV))
    rows("sr_render_blocks_batch", "empty", ({}, NR), (dict(n=abi.MAX_BATCH + 1), NR), (dict(n=0), NR))
    rows("sr_render_block_list", "one",
         (dict(c=None), INV), (dict(out=None), INV), (dict(blocks=None), INV), (dict(br=0), INV), (dict(nbk=0), INV),
         (dict(h=0), INV), (dict(blocks="big", nbk=(1 << 24) // 8 + 1), INV), (dict(blocks=(0, -2, 1)), INV),
         (dict(blocks=(0, NB8, 1)), INV), (dict(n=0), INV), (dict(n=abi.MAX_BATCH + 1), CAP),
         (dict(pitch=4 * W - 4), INV), (dict(fs=4 * W * 24 - 4), INV), (dict(max_steps=big), INV),
         (dict(n=abi.MAX_BATCH + 1, pitch=4 * W - 4), CAP), (dict(n=abi.MAX_BATCH + 1, blocks=(0, NB8, 1)), INV))
    rows("sr_render_block_list", "empty",
         ({}, NR), (dict(blocks=(0, NB8, 1)), INV), (dict(n=abi.MAX_BATCH + 1), NR), (dict(out=None), INV))
    rows("sr_render_ss", "one",
         (dict(ss=0), INV), (dict(ss=5), INV), (dict(out=None), INV), (dict(y1=H + 1), INV), (dict(y0=-1), INV),
         (dict(c=None), INV), (dict(max_steps=big), INV), (dict(pitch=4 * W - 4), INV),
         (dict(ss=1, pitch=4 * W - 4), INV), (dict(ss=1, out=None), INV), (dict(p=None), INV))
    rows("sr_render_ss", "empty",
         ({}, NR), (dict(ss=5), INV), (dict(out=None), INV), (dict(pitch=4 * W - 4), NR), (dict(ss=1), NR))
    rows("sr_render_block_list_ss", "one",
         (dict(ss=0), INV), (dict(ss=5), INV), (dict(c=None), INV), (dict(out=None), INV), (dict(blocks=None), INV),
         (dict(br=0), INV), (dict(nbk=0), INV), (dict(blocks=(0, NB8, 1)), INV), (dict(blocks=(-2, 0, 1)), INV),
         (dict(blocks="big", nbk=(1 << 24) // 16 + 1), INV), (dict(n=0), INV), (dict(n=abi.MAX_BATCH + 1), CAP),
         (dict(pitch=4 * W - 4), INV), (dict(fs=4 * W * 24 - 4), INV), (dict(max_steps=-1), INV),
         (dict(n=abi.MAX_BATCH + 1, blocks=(0, NB8, 1)), INV), (dict(n=abi.MAX_BATCH + 1, pitch=4 * W - 4), CAP),
         (dict(ss=1, fs=4 * W * 24 - 4), INV))
    rows("sr_render_block_list_ss", "empty",
         ({}, NR), (dict(n=abi.MAX_BATCH + 1), NR), (dict(ss=5), INV), (dict(blocks=(0, NB8, 1)), INV),
         (dict(pitch=4 * W - 4), NR))
    rows("sr_render_phase", "one",
         (dict(ss=0), INV), (dict(ss=5), INV), (dict(px=2), INV), (dict(py=-1), INV), (dict(py=2), INV),
         (dict(out=None), INV), (dict(y0=5, y1=4), INV), (dict(c=None), INV), (dict(max_steps=big), INV),
         (dict(pitch=4 * W - 4), INV))
    rows("sr_render_phase", "empty", ({}, NR), (dict(px=2), INV), (dict(out=None), INV), (dict(max_steps=-1), NR))
    rows("sr_render_accumulate", "one",
         (dict(ss=0), INV), (dict(ss=5), INV), (dict(phases=None), INV), (dict(accum=None), INV), (dict(nph=0), INV),
         (dict(nph=abi.MAX_BATCH + 1), CAP), (dict(phases=(0, 2, 1, 1)), INV), (dict(y1=H + 1), INV),
         (dict(c=None), INV), (dict(max_steps=big), INV), (dict(apitch=8 * W - 8), INV), (dict(accum="odd"), INV),
         (dict(apitch=8 * W + 4), INV), (dict(nph=abi.MAX_BATCH + 1, accum=None), INV),
         (dict(nph=abi.MAX_BATCH + 1, phases="bad66"), CAP), (dict(nph=abi.MAX_BATCH + 1, y1=H + 1), CAP),
         (dict(max_steps=-1, accum="odd"), INV))
    rows("sr_render_accumulate", "empty",
         ({}, NR), (dict(accum="odd"), NR), (dict(phases=(0, 2, 1, 1)), INV), (dict(y1=H + 1), INV),
         (dict(nph=abi.MAX_BATCH + 1), CAP))
    rows("sr_render_adaptive", "one",
         (dict(ss=1), INV), (dict(ss=5), INV), (dict(grow=-1), INV), (dict(grow=3), INV), (dict(out=None), INV),
         (dict(c=None), INV), (dict(max_steps=big), INV), (dict(pitch=4 * W - 4), INV), (dict(w=0), INV))
    rows("sr_render_adaptive", "empty", ({}, NR), (dict(grow=3), INV), (dict(pitch=4 * W - 4), NR))
    rows("sr_wave_costs", "one",
         (dict(c=None), INV), (dict(cam=None), INV), (dict(cost=None), INV), (dict(w=0), INV), (dict(h=0), INV),
         (dict(p=None), INV), (dict(max_steps=big), INV), (dict(raytrace_type=4), INV))
    rows("sr_wave_costs", "empty", ({}, NR), (dict(cost=None), INV), (dict(p=None), NR))
    rows("sr_reshade", "one",
         (dict(c=None), INV), (dict(out=None), INV), (dict(pitch=4 * W - 4), INV))
    rows("sr_reshade", "two", (dict(fs=4 * W * ROWS - 4), INV), (dict(pitch=4 * W - 4), INV))
    rows("sr_reshade", "ss", (dict(pitch=4 * W - 4), INV), (dict(out=None), INV))
    rows("sr_reshade", "none", ({}, NR), (dict(out=None), NR))
    rows("sr_reshade", "empty", ({}, NR))
    rows("sr_reshade_debug", "one", (dict(c=None), INV), (dict(f32=None, out=None, steps=None), INV))
    rows("sr_reshade_debug", "two", ({}, INV))
    rows("sr_reshade_debug", "ss", ({}, INV))
    rows("sr_reshade_debug", "none", ({}, NR), (dict(f32=None, out=None, steps=None), NR))
    rows("sr_pick_map", "one",
         (dict(c=None), INV), (dict(ids=None), INV), (dict(ids="odd"), INV), (dict(pitch=4 * W + 2), INV),
         (dict(pitch=4 * W - 4), INV))
    rows("sr_pick_map", "two", (dict(fs=4 * W * ROWS + 2), INV), (dict(fs=4 * W * ROWS - 4), INV))
    rows("sr_pick_map", "ss", ({}, NR), (dict(ids=None), NR))
    rows("sr_pick_map", "none", ({}, NR), (dict(ids=None), NR))
    rows("sr_pick_map", "empty", ({}, NR))
    return t


def test_rejected_calls(pkg, gpu):
    import numpy as np
    import torch

    r, empty = gpu
    abi, sc, lib = pkg.abi, pkg.scenes, r.lib
    cam = sc.camera_look((0.0, 2.0, 15.0), (0.0, -2.0, -15.0))
    cams = (abi.Camera * (abi.MAX_BATCH + 1))(*([cam] * (abi.MAX_BATCH + 1)))
    st = r._stream(None)
    r.set_scene(sc.scene_default(True))
    r.set_test_ray(abi.default_test_ray())
    good_prm = abi.default_params(max_steps=400, percent_black=-1.0, crosshair=0)
    good = r.render(cam, good_prm, W, H).cpu().numpy()

    dev = dict(device="cuda")
    buf = torch.full((2, ROWS, W, 4), FILL, dtype=torch.uint8, **dev)
    f32 = torch.full((H, W, 4), float(FILL), dtype=torch.float32, **dev)
    steps = torch.full((H, W), FILL, dtype=torch.int32, **dev)
    ids = torch.full((2 * ROWS * W + 2,), FILL, dtype=torch.int32, **dev)
    acc = torch.full((H * W * 4 + 8,), FILL, dtype=torch.int16, **dev)
    cost = torch.full((2 * ((H + 7) // 8) * ((W + 7) // 8),), FILL, dtype=torch.int32, **dev)
    acc_base = acc.data_ptr() + (-acc.data_ptr()) % 8
    bigblocks = np.zeros((1 << 24) // 8 + 2, dtype=np.int32)
    bad66 = (C.c_uint8 * (2 * (abi.MAX_BATCH + 1)))(*([0] * (2 * abi.MAX_BATCH) + [2, 0]))
    keep = []

    def untouched():
        return all(bool((t == FILL).all()) for t in (buf, f32, steps, ids, acc, cost))

    def call(entry, state, over):
        a = dict(c=r.ctx, cam=C.byref(cam), cams=cams, n=2, w=W, h=H, y0=0, y1=H, out=C.c_void_p(buf.data_ptr()),
                 pitch=4 * W, fs=4 * W * ROWS, br=8, bf=0, bs=1, blocks=(0, 3, 1), nbk=3, ss=2, px=0, py=1,
                 phases=(0, 1, 1, 1), nph=2, accum=C.c_void_p(acc_base), apitch=8 * W, grow=1,
                 f32=C.c_void_p(f32.data_ptr()), steps=C.c_void_p(steps.data_ptr()), ids=C.c_void_p(ids.data_ptr()),
                 cost=C.c_void_p(cost.data_ptr()))
        if state == "empty":
            a["c"] = empty.ctx
        pk = {k: over[k] for k in ("raytrace_type", "filter_mode", "max_steps") if k in over}
        prm = abi.default_params(**{**dict(max_steps=400, percent_black=-1.0, crosshair=0), **pk})
        a["p"] = C.byref(prm)
        a.update({k: v for k, v in over.items() if k not in pk})
        if a["accum"] == "odd":
            a["accum"] = C.c_void_p(acc_base + 4)
        if a["ids"] == "odd":
            a["ids"] = C.c_void_p(ids.data_ptr() + 2)
        if isinstance(a["blocks"], str):
            a["blocks"] = bigblocks.ctypes.data_as(C.POINTER(C.c_int))
        elif a["blocks"] is not None:
            a["blocks"] = (C.c_int * len(a["blocks"]))(*a["blocks"])
        if isinstance(a["phases"], str):
            a["phases"] = bad66
        elif a["phases"] is not None:
            a["phases"] = (C.c_uint8 * len(a["phases"]))(*a["phases"])
        keep.append((prm, a))
        c, p, w, h = a["c"], a["p"], a["w"], a["h"]
        fn = {
            "sr_render": lambda: lib.sr_render(c, a["cam"], p, w, h, a["y0"], a["y1"], a["out"], a["pitch"], st),
            "sr_render_debug": lambda: lib.sr_render_debug(c, a["cam"], p, w, h, a["y0"], a["y1"], a["f32"],
                                                           a["out"], a["steps"], st),
            "sr_render_blocks": lambda: lib.sr_render_blocks(c, a["cam"], p, w, h, a["br"], a["bf"], a["bs"],
                                                             a["out"], a["pitch"], st),
            "sr_render_blocks_batch": lambda: lib.sr_render_blocks_batch(c, a["cams"], a["n"], p, w, h, a["br"],
                                                                         a["bf"], a["bs"], a["out"], a["pitch"],
                                                                         a["fs"], st),
            "sr_render_block_list": lambda: lib.sr_render_block_list(c, a["cams"], a["n"], p, w, h, a["br"],
                                                                     a["blocks"], a["nbk"], a["out"], a["pitch"],
                                                                     a["fs"], st),
            "sr_render_ss": lambda: lib.sr_render_ss(c, a["cam"], p, w, h, a["y0"], a["y1"], a["ss"], a["out"],
                                                     a["pitch"], st),
            "sr_render_block_list_ss": lambda: lib.sr_render_block_list_ss(c, a["cams"], a["n"], p, w, h, a["br"],
                                                                           a["blocks"], a["nbk"], a["ss"], a["out"],
                                                                           a["pitch"], a["fs"], st),
            "sr_render_phase": lambda: lib.sr_render_phase(c, a["cam"], p, w, h, a["y0"], a["y1"], a["ss"], a["px"],
                                                           a["py"], a["out"], a["pitch"], st),
            "sr_render_accumulate": lambda: lib.sr_render_accumulate(c, a["cam"], p, w, h, a["y0"], a["y1"], a["ss"],
                                                                     a["phases"], a["nph"], 1, a["accum"],
                                                                     a["apitch"], st),
            "sr_render_adaptive": lambda: lib.sr_render_adaptive(c, a["cam"], p, w, h, a["ss"], 40, a["grow"],
                                                                 a["out"], a["pitch"], None, st),
            "sr_wave_costs": lambda: lib.sr_wave_costs(c, a["cam"], p, w, h, a["cost"], st),
            "sr_reshade": lambda: lib.sr_reshade(c, a["out"], a["pitch"], a["fs"], st),
            "sr_reshade_debug": lambda: lib.sr_reshade_debug(c, a["f32"], a["out"], a["steps"], st),
            "sr_pick_map": lambda: lib.sr_pick_map(c, a["ids"], a["pitch"], a["fs"], st),
        }[entry]
        return fn()

    def enter(state):
        """Leaves the good context in `state` (the set-up launches write their own buffers)."""
        if state == "one":
            r.render(cam, good_prm, W, H)
        elif state == "two":
            r.render_blocks_batch([cam, cam], good_prm, W, H, 8, 0, 1)
        elif state == "ss":
            r.render_ss(cam, good_prm, W, H, 2)
        elif state == "none":
            r.set_test_ray(abi.default_test_ray())  # drops the retained frame
        torch.cuda.synchronize()
        return {"one": 1, "two": 1, "ss": 1, "none": 0, "empty": 0}[state]

    failures = []
    rows = table(abi)
    assert len(rows) >= 70
    for state in ("one", "two", "ss", "none", "empty"):
        kept = enter(state)
        who = empty if state == "empty" else r
        for entry, s, over, want in rows:
            if s != state:
                continue
            got = call(entry, state, over)
            torch.cuda.synchronize()
            what = f"{entry} [{state}] {over}"
            print(f"{what}: {got}")
            if got != want:
                failures.append(f"{what}: status {got}, expected {want}")
            if not untouched():
                failures.append(f"{what}: a buffer was written")
                for t in (buf, f32, steps, ids, acc, cost):
                    t.fill_(FILL)
            if lib.sr_can_reshade(who.ctx) != kept:
                failures.append(f"{what}: sr_can_reshade is {lib.sr_can_reshade(who.ctx)}, was {kept}")
                kept = enter(state)
    assert not failures, "\n".join(failures)
    again = r.render(cam, good_prm, W, H).cpu().numpy()
    assert np.array_equal(again, good), "the good render no longer repeats"
    assert r.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
