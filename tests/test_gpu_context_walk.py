"""The walks of tests/walk_cases.py on one long-lived context.

sr.h's promise is that a context's history never reaches the bytes. Every walk
runs its ops in order on one context A. After every op the returned status
and sr_can_reshade equal the model's prediction. Every op that writes output
is issued again on a fresh context B that was put into the model's declared
state (background, texture array, scene, test ray, sequence, projection, in
that order; split tiles and the latency mode off and culling on, whatever A
has: sr.h says they do not reach the bytes), and A's and B's buffers are equal
byte for byte: every map, float FragColor, RGBA8, step counts, ids,
accumulators, the tile mask, and the sentinel bytes of the padding, of the -1
blocks and of the rows past the frame's end. For a consumer of the retained
frame B first issues the retained call itself with the current scene, which is
sr.h's definition of sr_reshade. B is destroyed after the comparison.

A rejected or SR_E_NOT_READY call leaves its sentinel-filled buffers
untouched; across the trace and the rejected ops the debug accessors
(pixel_state, last_order) do not change. At the end of a walk one
sr_render_debug of the final state equals the oracle's frame and
sr_diag_counters is zero. No comparison has a tolerance.

sr_wave_costs' cost map is compared like every other output, with B at its
default settings: the map comes from a culling kernel whatever the context's
culling, split tiles or latency mode are.

sr_render_accumulate_shutter's accumulator is resolved with sr_accum_resolve,
as sr.h says; sr_shutter_resolve takes no context and has no state to walk
(tests/test_gpu_shutter.py holds it to its host form).

One departure from "fresh": the comparison reads A's buffers after a device
synchronisation, so two launches of a walk are never in flight together; the
stream order of back-to-back launches is tests/test_gpu_launch_matrix.py's.
"""
import ctypes as C

import numpy as np
import pytest

import walk_cases as WC
from test_gpu_launch_matrix import host
from test_gpu_shading_extremes import compare_strict

pytestmark = pytest.mark.gpu

FILL = 77
PAD = 16  # bytes added to every pitch
GAP = 64  # bytes added to every frame stride
BR = WC.BLOCK_ROWS


@pytest.fixture(scope="module")
def rs(pkg, oracle, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return WC.Resolver(pkg, oracle, textures)


class Runner:
    """Issues ops on a Renderer through r.lib / r.ctx: (status, the buffers the call may write)."""

    def __init__(self, pkg, rs, streams):
        import torch

        self.pkg, self.abi, self.rs, self.torch, self.streams = pkg, pkg.abi, rs, torch, streams
        self._rays = {}

    # ---- arguments
    def stream(self, op):
        s = self.streams[op.get("stream", 0)]
        return C.c_void_p(s.cuda_stream if s is not None else 0)

    def buf(self, nbytes):
        return self.torch.full((max(int(nbytes), 1),), FILL, dtype=self.torch.uint8, device="cuda")

    def cams(self, op):
        names = op["cams"]
        return (self.abi.Camera * len(names))(*[self.rs.cam(n) for n in names])

    def rays(self, cam):
        if cam not in self._rays:
            o, d = self.abi.camera_rays(self.rs.cam(cam), 0, 8, 4)
            t = self.torch
            self._rays[cam] = (t.from_numpy(np.ascontiguousarray(o.reshape(-1, 3))).cuda(),
                               t.from_numpy(np.ascontiguousarray(d.reshape(-1, 3))).cuda())
        return self._rays[cam]

    def image(self, w, rows, frames):
        """(buffer, pitch, frame stride) of `frames` RGBA8 images with a padded pitch and stride"""
        pitch = 4 * w + PAD
        stride = pitch * rows + GAP
        return self.buf(stride * frames), pitch, stride

    def maps(self, w, rows, frames):
        pitch = w + 3
        stride = pitch * rows + 5
        ptrs, bufs = self.abi.RayMapPtrs(), []
        for key, (n, _) in self.abi.RAY_MAPS.items():
            b = self.buf(4 * n * stride * frames)
            setattr(ptrs, key, b.data_ptr())
            bufs.append(b)
        return ptrs, bufs, pitch, stride

    def ready(self):
        self.torch.cuda.synchronize()  # the sentinel fills are done before a launch on another stream

    # ---- the state
    def apply(self, r, st):
        if st["bg"] is not None:
            r.set_background(self.rs.bgs[st["bg"]])
        if st["tex"] is not None:
            r.set_texture_array(self.rs.texs[st["tex"]])
        if st["scene"] is not None:
            r.set_scene(self.rs.scene(st["scene"]))
        r.set_test_ray(self.rs.ray(st["ray"]))
        if st["seq"] is not None:
            r.set_scene_sequence(self.rs.sequence(st["seq"]))
        r.set_projection(st["projection"])

    def setter(self, r, op):
        k, lib, ctx, rs = op["kind"], r.lib, r.ctx, self.rs
        if k in ("set_scene_geo", "set_scene_shade"):
            return lib.sr_set_scene(ctx, C.byref(rs.scene(op["scene"])))
        if k == "set_test_ray":
            return lib.sr_set_test_ray(ctx, C.byref(rs.ray(op["ray"])))
        if k == "set_sequence":
            scenes = rs.sequence(op["seq"]) if op["seq"] is not None else []
            arr = (self.abi.Scene * max(1, len(scenes)))(*scenes)
            return lib.sr_set_scene_sequence(ctx, arr, len(scenes))
        if k == "set_background":
            img = np.ascontiguousarray(rs.bgs[op["bg"]])
            return lib.sr_set_background(ctx, img.ctypes.data, img.shape[1], img.shape[0], img.shape[2])
        if k == "set_texture_array":
            arr = np.ascontiguousarray(rs.texs[op["tex"]])
            return lib.sr_set_texture_array(ctx, arr.ctypes.data, arr.shape[2], arr.shape[1], arr.shape[0], arr.shape[3])
        if k == "set_projection":
            return lib.sr_set_projection(ctx, op["projection"])
        if k == "set_split":
            return lib.sr_set_split(ctx, *op["split"])
        if k == "set_latency":
            return lib.sr_set_latency_mode(ctx, op["on"])
        if k == "set_culling":
            return lib.sr_debug_set_culling(ctx, op["on"])
        raise ValueError(k)

    # ---- the calls that write
    def launch(self, r, op):
        k, lib, ctx = op["kind"], r.lib, r.ctx
        w, h = op["w"], op["h"]
        prm = C.byref(self.rs.params(op))
        cams, n = self.cams(op), len(op["cams"])
        s = self.stream(op)
        P = C.c_void_p
        if "blocks" in op:
            blocks = (C.c_int * len(op["blocks"]))(*op["blocks"])
            nbk = len(op["blocks"])
        if k in ("render", "render_ss", "render_phase", "reject_pitch"):
            y0, y1 = (op["y0"], op["y1"]) if "y0" in op else (0, h)
            out, pitch, _ = self.image(w, y1 - y0, 1)
            self.ready()
            if k == "render":
                rc = lib.sr_render(ctx, cams, prm, w, h, y0, y1, P(out.data_ptr()), pitch, s)
            elif k == "reject_pitch":
                rc = lib.sr_render(ctx, cams, prm, w, h, y0, y1, P(out.data_ptr()), 4 * w - 4, s)
            elif k == "render_ss":
                rc = lib.sr_render_ss(ctx, cams, prm, w, h, y0, y1, op["ss"], P(out.data_ptr()), pitch, s)
            else:
                rc = lib.sr_render_phase(ctx, cams, prm, w, h, y0, y1, op["ss"], op["px"], op["py"], P(out.data_ptr()),
                                         pitch, s)
            return rc, [out]
        if k in ("render_blocks", "render_blocks_batch"):
            rows = WC.blocks_rows(h, BR, op["first"], op["step"])[0]
            out, pitch, stride = self.image(w, rows, n)
            self.ready()
            if k == "render_blocks":
                rc = lib.sr_render_blocks(ctx, cams, prm, w, h, BR, op["first"], op["step"], P(out.data_ptr()), pitch, s)
            else:
                rc = lib.sr_render_blocks_batch(ctx, cams, n, prm, w, h, BR, op["first"], op["step"], P(out.data_ptr()),
                                                pitch, stride, s)
            return rc, [out]
        if k in ("render_block_list", "render_block_list_ss", "reject_block"):
            out, pitch, stride = self.image(w, nbk * BR, n)
            self.ready()
            if k == "render_block_list_ss":
                rc = lib.sr_render_block_list_ss(ctx, cams, n, prm, w, h, BR, blocks, nbk, op["ss"], P(out.data_ptr()),
                                                 pitch, stride, s)
            else:
                rc = lib.sr_render_block_list(ctx, cams, n, prm, w, h, BR, blocks, nbk, P(out.data_ptr()), pitch,
                                              stride, s)
            return rc, [out]
        if k in ("render_debug", "render_sequence_debug"):
            y0, y1 = op["y0"], op["y1"]
            px = max(w * (y1 - y0), 1)
            f, b, st = self.buf(16 * px), self.buf(4 * px), self.buf(4 * px)
            self.ready()
            if k == "render_debug":
                rc = lib.sr_render_debug(ctx, cams, prm, w, h, y0, y1, P(f.data_ptr()), P(b.data_ptr()),
                                         P(st.data_ptr()), s)
            else:
                rc = lib.sr_render_sequence_debug(ctx, op["first"], cams, prm, w, h, y0, y1, P(f.data_ptr()),
                                                  P(b.data_ptr()), P(st.data_ptr()), s)
            return rc, [f, b, st]
        if k in ("render_accumulate", "accumulate_shutter"):
            y0, y1 = (op["y0"], op["y1"]) if "y0" in op else (0, h)
            rows = y1 - y0
            apitch = 8 * w + PAD
            acc = self.buf(apitch * rows)
            out, pitch, _ = self.image(w, rows, 1)
            self.ready()
            if k == "render_accumulate":
                flat = [v for ph in op["phases"] for v in ph]
                count = len(op["phases"])
                rc = lib.sr_render_accumulate(ctx, cams, prm, w, h, y0, y1, op["ss"], (C.c_uint8 * len(flat))(*flat),
                                              count, 1, P(acc.data_ptr()), apitch, s)
            else:
                count = n
                rc = lib.sr_render_accumulate_shutter(ctx, op["first"], cams, None, n, prm, w, h, y0, y1, op["ss"], 1,
                                                      P(acc.data_ptr()), apitch, s)
            if rc == WC.OK and rows > 0:
                rc = lib.sr_accum_resolve(P(acc.data_ptr()), apitch, w, rows, count, P(out.data_ptr()), pitch, 1, s)
            return rc, [acc, out]
        if k == "render_adaptive":
            out, pitch, _ = self.image(w, h, 1)
            mask = self.buf(-(-h // 16) * -(-w // 16) + 8)
            self.ready()
            rc = lib.sr_render_adaptive(ctx, cams, prm, w, h, op["ss"], op["threshold"], op["grow"], P(out.data_ptr()),
                                        pitch, P(mask.data_ptr()), s)
            return rc, [out, mask]
        if k == "wave_costs":
            out = self.buf(8 * -(-h // 8) * -(-w // 8) + 8)
            self.ready()
            return lib.sr_wave_costs(ctx, cams, prm, w, h, P(out.data_ptr()), s), [out]
        if k in ("render_sequence", "reject_window"):
            y0, y1 = (op["y0"], op["y1"]) if "y0" in op else (0, h)
            out, pitch, stride = self.image(w, y1 - y0, n)
            self.ready()
            rc = lib.sr_render_sequence(ctx, op["first"], cams, n, prm, w, h, y0, y1, op.get("ss", 1), P(out.data_ptr()),
                                        pitch, stride, s)
            return rc, [out]
        if k == "render_sequence_block_list":
            out, pitch, stride = self.image(w, nbk * BR, n)
            self.ready()
            rc = lib.sr_render_sequence_block_list(ctx, op["first"], cams, n, prm, w, h, BR, blocks, nbk, op["ss"],
                                                   P(out.data_ptr()), pitch, stride, s)
            return rc, [out]
        if k == "render_shutter":
            y0, y1 = op["y0"], op["y1"]
            out, pitch, stride = self.image(w, y1 - y0, op["M"])
            self.ready()
            rc = lib.sr_render_shutter(ctx, op["first"], cams, None, op["K"], op["M"], prm, w, h, y0, y1, op["ss"],
                                       P(out.data_ptr()), pitch, stride, s)
            return rc, [out]
        if k == "render_shutter_block_list":
            out, pitch, stride = self.image(w, nbk * BR, op["M"])
            self.ready()
            rc = lib.sr_render_shutter_block_list(ctx, op["first"], cams, None, op["K"], op["M"], prm, w, h, BR, blocks,
                                                  nbk, op["ss"], P(out.data_ptr()), pitch, stride, s)
            return rc, [out]
        if k in WC.TRACES:
            o, d = self.rays(op["cams"][0])
            nr = int(o.shape[0])
            if k == "trace_rays":
                bufs = [self.buf(16 * nr), self.buf(4 * nr), self.buf(4 * nr), self.buf(4 * nr)]
                self.ready()
                rc = lib.sr_trace_rays(ctx, P(o.data_ptr()), P(d.data_ptr()), nr, prm, *[P(b.data_ptr()) for b in bufs], s)
            else:
                ptrs, bufs, _, _ = self.maps(nr, 1, 1)
                self.ready()
                rc = lib.sr_trace_ray_maps(ctx, P(o.data_ptr()), P(d.data_ptr()), nr, prm, C.byref(ptrs), s)
            return rc, bufs
        raise ValueError(k)

    def consume(self, r, op, retained):
        """A consumer of the retained frame, into buffers of the retained call's shape"""
        k, lib, ctx = op["kind"], r.lib, r.ctx
        w, rows, frames, _ = WC.out_shape(retained) if retained is not None else (4, 4, 1, 1)
        s = self.stream(op)
        P = C.c_void_p
        if k == "reshade":
            out, pitch, stride = self.image(w, rows, frames)
            self.ready()
            return lib.sr_reshade(ctx, P(out.data_ptr()), pitch, stride, s), [out]
        if k == "reshade_debug":
            px = w * rows * frames
            f, b, st = self.buf(16 * px), self.buf(4 * px), self.buf(4 * px)
            self.ready()
            return lib.sr_reshade_debug(ctx, P(f.data_ptr()), P(b.data_ptr()), P(st.data_ptr()), s), [f, b, st]
        if k == "pick_map":
            out, pitch, stride = self.image(w, rows, frames)
            self.ready()
            return lib.sr_pick_map(ctx, P(out.data_ptr()), pitch, stride, s), [out]
        if k == "ray_maps":
            ptrs, bufs, pitch, stride = self.maps(w, rows, frames)
            self.ready()
            return lib.sr_ray_maps(ctx, C.byref(ptrs), pitch, stride, s), bufs
        raise ValueError(k)

    def run(self, r, op, retained):
        k = op["kind"]
        if k in WC.SETTERS:
            return self.setter(r, op), []
        if k == "can_reshade":
            return WC.OK, []
        if k in WC.CONSUMERS:
            return self.consume(r, op, retained)
        return self.launch(r, op)


def describe(name, ops, i):
    last = "\n".join(f"  [{j}] {ops[j]}" for j in range(max(0, i - 5), i))
    return f"walk {name}, op {i}: {ops[i]}\nthe ops before it:\n{last}"


def walk(pkg, rs, name):
    import torch

    ops = WC.walks()[name]
    run = Runner(pkg, rs, [None, torch.cuda.Stream()])
    m = WC.Model()
    A = pkg.Renderer(0)
    try:
        for i, op in enumerate(ops):
            k = op["kind"]
            retained = m.retained  # what a consumer reads
            want, _ = m.step(op)
            where = describe(name, ops, i)
            untouching = k in WC.UNTOUCHING
            if untouching:
                before = (A.pixel_state().tobytes(), A.last_order().tobytes())
            status, bufs = run.run(A, op, retained)
            assert status == want, f"status {status}, the model says {want}\n{where}"
            assert A.lib.sr_can_reshade(A.ctx) == m.can_reshade(), f"sr_can_reshade, the model says {m.can_reshade()}\n{where}"
            if untouching:
                after = (A.pixel_state().tobytes(), A.last_order().tobytes())
                assert before[0] == after[0], f"the pixel state changed\n{where}"
                assert before[1] == after[1], f"the launch order changed\n{where}"
            if not bufs:
                continue
            if status != WC.OK:
                torch.cuda.synchronize()
                for j, b in enumerate(bufs):
                    assert bool((b == FILL).all()), f"a rejected call wrote buffer {j}\n{where}"
                continue
            B = pkg.Renderer(0)
            try:
                st = m.declared()
                run.apply(B, st)
                if k in WC.CONSUMERS:
                    rc, _ = run.run(B, retained, None)
                    assert rc == WC.OK, f"the retained call on the fresh context: {rc}\n{where}"
                rc, ref = run.run(B, op, retained)
                assert rc == WC.OK, f"the fresh context's status: {rc}\n{where}"
                got = host(*bufs)
                exp = host(*ref)
            finally:
                B.close()
            for j, (g, e) in enumerate(zip(got, exp)):
                bad = g != e
                assert not bad.any(), (f"buffer {j}: {int(bad.sum())} of {bad.size} bytes differ from the fresh "
                                       f"context's (first at byte {int(np.flatnonzero(bad)[0])})\n{where}")
        # the final state against the oracle
        st = m.declared()
        w, h = rs.W, rs.H
        A.set_projection(0)
        f, b, s = host(*A.render_debug(rs.cam("view"), rs.wd.params(rs.STEPS), w, h))
        compare_strict((b, f, s), rs.frame(st["scene"], st["ray"], st["bg"], st["tex"]), f"walk {name}, the final state")
        assert A.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}, name
    finally:
        A.close()


@pytest.mark.parametrize("name", ["pressure", "pairs"] + [n for n in WC.WALK_NAMES if n.startswith("random")])
def test_walk(pkg, rs, name):
    """One walk: statuses, sr_can_reshade, every written buffer against a fresh
    context, the untouched sentinels, the debug accessors, the oracle at the end."""
    walk(pkg, rs, name)


def test_default_outputs_are_filled_on_the_launch_stream(pkg, rs):
    """Renderer.ray_maps, pick_map and wave_costs pre-fill the outputs they
    allocate. The fill must be ordered before the launch on the caller's
    stream: with torch's current stream kept busy, a fill queued there would
    land after the launch on another stream and wipe its result."""
    import torch

    r = pkg.Renderer(0)
    try:
        st = {"bg": "bgA", "tex": "texA", "scene": "small", "ray": "off", "seq": None, "projection": 0}
        Runner(pkg, rs, [None]).apply(r, st)
        cam, prm, w, h = rs.cam("view"), rs.wd.params(64), 33, 17
        r.render(cam, prm, w, h)
        want_ids, want_maps = r.pick_map(), r.ray_maps()
        want_cost = r.wave_costs(cam, prm, w, h)
        r.render(cam, prm, w, h)
        torch.cuda.synchronize()
        s2 = torch.cuda.Stream()
        busy = torch.ones((8192, 8192), device="cuda")
        for _ in range(4):  # tens of milliseconds on the current stream
            busy = (busy @ busy) * 1e-4
        ids = r.pick_map(stream=s2)
        maps = r.ray_maps(stream=s2)
        cost = r.wave_costs(cam, prm, w, h, stream=s2)
        torch.cuda.synchronize()
        assert torch.equal(ids, want_ids) and torch.equal(cost, want_cost)
        for key in want_maps:
            assert maps[key].cpu().numpy().tobytes() == want_maps[key].cpu().numpy().tobytes(), key
        assert bool((want_ids != pkg.abi.PICK_NONE).any()) and bool((want_cost != 0).any())
    finally:
        r.close()
