"""GPU renderer: a thin Python handle over the C-ABI (libsr.so).

PyTorch only provides device memory and the HIP stream; every pixel is
computed by the gfx950 kernel in libsr.so. There is no CPU fallback: without a
HIP device `Renderer()` raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi


def camera_rays(cam: abi.Camera, projection, w: int, h: int):
    """The rays the frame kernels start with (sr_camera_rays): host float32
    arrays (origins, dirs) of shape [h, w, 3] for the w x h frame of `cam`
    under `projection` (abi.PROJECTION_* or its name); a pixel without a ray
    has a NaN direction. Renderer.trace_rays of them gives the frame's pixels."""
    return abi.camera_rays(cam, projection, w, h)


class Renderer:
    """One sr_ctx bound to one HIP device (the reference's single GL program)."""

    def __init__(self, device: int = 0, lib=None):
        """lib: a loaded library (abi.load(path)) other than the package's
        libsr.so, e.g. the test-only 7-wave build (tests/test_gpu_allocation.py)."""
        import torch

        self.torch = torch
        self.lib = lib if lib is not None else abi.load()
        self.device = int(device)
        self.tdev = torch.device("cuda", self.device)
        ctx = C.c_void_p()
        abi.check(self.lib.sr_create(C.byref(ctx), self.device), "sr_create")
        self.ctx = ctx
        self._keep = []

    # ---- uploads (src/main.cpp:205-274 equivalents) ----------------------------
    def set_scene(self, scene: abi.Scene) -> None:
        abi.check(self.lib.sr_set_scene(self.ctx, C.byref(scene)), "sr_set_scene")

    def set_test_ray(self, test_ray: abi.TestRay) -> None:
        abi.check(self.lib.sr_set_test_ray(self.ctx, C.byref(test_ray)), "sr_set_test_ray")

    def set_background(self, img: np.ndarray) -> None:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w, ch = img.shape
        abi.check(self.lib.sr_set_background(self.ctx, img.ctypes.data, w, h, ch), "sr_set_background")

    def set_texture_array(self, arr: np.ndarray) -> None:
        arr = np.ascontiguousarray(arr, dtype=np.uint8)
        layers, h, w, ch = arr.shape
        abi.check(self.lib.sr_set_texture_array(self.ctx, arr.ctypes.data, w, h, layers, ch), "sr_set_texture_array")

    def set_culling(self, enabled: bool) -> None:
        abi.check(self.lib.sr_debug_set_culling(self.ctx, 1 if enabled else 0), "sr_debug_set_culling")

    def set_split(self, max_tiles: int, lanes_per_wave: int = 16, min_steps: int = 1) -> None:
        """Run the costliest tiles of the previous frame as sparse waves (sr_set_split; 0 tiles: off)."""
        abi.check(self.lib.sr_set_split(self.ctx, int(max_tiles), int(lanes_per_wave), int(min_steps)), "sr_set_split")

    # ---- rendering -------------------------------------------------------------
    def set_latency_mode(self, on: bool) -> None:
        """sr_set_latency_mode: a 2-step fast loop for one frame at a time (pixels unchanged)."""
        abi.check(self.lib.sr_set_latency_mode(self.ctx, 1 if on else 0), "sr_set_latency_mode")

    def set_projection(self, projection) -> None:
        """sr_set_projection: abi.PROJECTION_* or its name ("rectilinear", "equirect",
        "fisheye") for every later launch; a change drops the retained frame."""
        if isinstance(projection, str):
            if projection not in abi.PROJECTIONS:
                raise ValueError(f"unknown projection {projection!r}; one of {sorted(abi.PROJECTIONS)}")
            projection = abi.PROJECTIONS[projection]
        abi.check(self.lib.sr_set_projection(self.ctx, int(projection)), "sr_set_projection")

    def get_projection(self) -> int:
        """sr_get_projection: the context's abi.PROJECTION_* value."""
        rc = self.lib.sr_get_projection(self.ctx)
        if rc < 0:
            raise abi.SRError(rc, "sr_get_projection")
        return int(rc)

    def set_timing(self, capacity: int) -> None:
        """Record per-kernel HIP events for the next `capacity` frames (0: off)."""
        abi.check(self.lib.sr_debug_set_timing(self.ctx, int(capacity)), "sr_debug_set_timing")

    def kernel_times(self, max_frames: int = 4096) -> np.ndarray:
        """[frames, 3] ms of (integrate, shade, resume) for the recorded frames."""
        buf = (C.c_float * (3 * max_frames))()
        n = C.c_int()
        abi.check(self.lib.sr_debug_kernel_times(self.ctx, buf, max_frames, C.byref(n)), "sr_debug_kernel_times")
        k = min(n.value, max_frames)
        return np.frombuffer(buf, dtype=np.float32, count=3 * k).reshape(k, 3).copy()

    def diag_counters(self) -> dict:
        """sr_diag_counters after this context's frames: opaque-classified hits
        whose shaded alpha was not 1 (must stay 0) and failed stream-ordered frees."""
        buf = (C.c_int64 * 2)()
        abi.check(self.lib.sr_diag_counters(self.ctx, buf, 2), "sr_diag_counters")
        return {"hit_not_opaque": int(buf[0]), "free_errors": int(buf[1])}

    def last_order(self) -> np.ndarray:
        """The launch codes the last frame left for the next one (tile << 8, | 0x80 | sub when split, -1 unused)."""
        n = C.c_int()
        abi.check(self.lib.sr_debug_last_order(self.ctx, None, 0, C.byref(n)), "sr_debug_last_order")
        buf = (C.c_int * max(1, n.value))()
        abi.check(self.lib.sr_debug_last_order(self.ctx, buf, n.value, C.byref(n)), "sr_debug_last_order")
        return np.frombuffer(buf, dtype=np.int32, count=n.value).copy()

    def pixel_state(self) -> np.ndarray:
        """The integrate -> shade hand-off after the last frame (post-mortems):
        float32 [SR_PS_FIELDS * n] in geodesic.hip's PS layout, n pixel ids."""
        n = C.c_size_t()
        abi.check(self.lib.sr_debug_pixel_state(self.ctx, None, 0, C.byref(n)), "sr_debug_pixel_state")
        buf = np.empty(max(1, n.value * abi.PS_FIELDS), dtype=np.float32)
        abi.check(self.lib.sr_debug_pixel_state(self.ctx, buf.ctypes.data_as(C.POINTER(C.c_float)),
                                                n.value * abi.PS_FIELDS, C.byref(n)), "sr_debug_pixel_state")
        return buf[:n.value * abi.PS_FIELDS]

    def _stream(self, stream):
        if stream is None:
            stream = self.torch.cuda.current_stream(self.tdev)
        return C.c_void_p(stream.cuda_stream)

    def _filled(self, shape, value, dtype, stream):
        """A tensor filled on the launch's own stream: a fill on the current
        stream is not ordered before a launch on another one."""
        if stream is None:
            return self.torch.full(shape, value, dtype=dtype, device=self.tdev)
        with self.torch.cuda.stream(stream):
            return self.torch.full(shape, value, dtype=dtype, device=self.tdev)

    def render(self, cam: abi.Camera, params: abi.Params, width: int, height: int, row_begin: int = 0,
               row_end: int | None = None, out=None, stream=None):
        """RGBA8 rows [row_begin, row_end) (GL order, row 0 = bottom) into a
        uint8 tensor [rows, width, 4] on this device. Asynchronous."""
        row_end = height if row_end is None else row_end
        rows = row_end - row_begin
        if out is None:
            out = self.torch.empty((max(rows, 0), width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and out.numel() >= rows * width * 4
        abi.check(
            self.lib.sr_render(self.ctx, C.byref(cam), C.byref(params), width, height, row_begin, row_end,
                               C.c_void_p(out.data_ptr()), width * 4, self._stream(stream)),
            "sr_render",
        )
        return out

    def render_blocks(self, cam: abi.Camera, params: abi.Params, width: int, height: int, block_rows: int,
                      block_first: int, block_step: int, out=None, stream=None):
        """Block-cyclic row bands (multi-GPU tiling), packed densely."""
        rows = self.lib.sr_blocks_row_count(height, block_rows, block_first, block_step)
        nblocks = -(-rows // block_rows) if rows else 0
        cap = nblocks * block_rows
        if out is None:
            out = self.torch.empty((cap, width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.numel() >= cap * width * 4
        abi.check(
            self.lib.sr_render_blocks(self.ctx, C.byref(cam), C.byref(params), width, height, block_rows,
                                      block_first, block_step, C.c_void_p(out.data_ptr()), width * 4,
                                      self._stream(stream)),
            "sr_render_blocks",
        )
        return out, rows

    def render_blocks_batch(self, cams, params: abi.Params, width: int, height: int, block_rows: int,
                            block_first: int, block_step: int, out=None, stream=None):
        """sr_render_blocks' rows of len(cams) frames in one launch -> ([B, tile_rows, W, 4], rows)."""
        rows = self.lib.sr_blocks_row_count(height, block_rows, block_first, block_step)
        nblocks = -(-rows // block_rows) if rows else 0
        cap = nblocks * block_rows
        B = len(cams)
        arr = (abi.Camera * B)(*cams)
        if out is None:
            out = self.torch.empty((B, cap, width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and tuple(out.shape[:1]) == (B,)
        assert out[0].numel() >= cap * width * 4
        abi.check(
            self.lib.sr_render_blocks_batch(self.ctx, arr, B, C.byref(params), width, height, block_rows, block_first,
                                            block_step, C.c_void_p(out.data_ptr()), width * 4,
                                            out[0].numel(), self._stream(stream)),
            "sr_render_blocks_batch",
        )
        return out, rows

    def wave_costs(self, cam: abi.Camera, params: abi.Params, width: int, height: int, stream=None):
        """sr_wave_costs: int32 [ceil(H / 8), ceil(W / 8), 2] per 8x8 wave tile of
        the frame: {longest ray's steps, budget events}. Asynchronous."""
        out = self._filled(((height + 7) // 8, (width + 7) // 8, 2), 0, self.torch.int32, stream)
        abi.check(self.lib.sr_wave_costs(self.ctx, C.byref(cam), C.byref(params), width, height,
                                         C.c_void_p(out.data_ptr()), self._stream(stream)), "sr_wave_costs")
        return out

    def render_block_list(self, cams, params: abi.Params, width: int, height: int, block_rows: int, blocks,
                          out=None, stream=None):
        """Rows of an explicit block list (sr_render_block_list; -1 = padding)
        for len(cams) frames in one launch -> [B, len(blocks) * block_rows, W, 4]."""
        blocks = [int(b) for b in blocks]
        B = len(cams)
        arr = (abi.Camera * B)(*cams)
        lst = (C.c_int * len(blocks))(*blocks)
        rows = len(blocks) * block_rows
        if out is None:
            out = self.torch.empty((B, rows, width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and tuple(out.shape[:1]) == (B,)
        assert out[0].numel() >= rows * width * 4
        abi.check(
            self.lib.sr_render_block_list(self.ctx, arr, B, C.byref(params), width, height, block_rows, lst,
                                          len(blocks), C.c_void_p(out.data_ptr()), width * 4, out[0].numel(),
                                          self._stream(stream)),
            "sr_render_block_list",
        )
        return out

    def render_ss(self, cam: abi.Camera, params: abi.Params, width: int, height: int, ss: int, row_begin: int = 0,
                  row_end: int | None = None, out=None, stream=None):
        """render with ss x ss samples per pixel and a box resolve
        (sr_render_ss; ss 1 .. abi.MAX_SUPERSAMPLE, 1: the plain frame):
        rows [row_begin, row_end) of the width x height frame -> [rows, width, 4]."""
        row_end = height if row_end is None else row_end
        rows = row_end - row_begin
        if out is None:
            out = self.torch.empty((max(rows, 0), width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and out.numel() >= rows * width * 4
        abi.check(
            self.lib.sr_render_ss(self.ctx, C.byref(cam), C.byref(params), width, height, row_begin, row_end, int(ss),
                                  C.c_void_p(out.data_ptr()), width * 4, self._stream(stream)),
            "sr_render_ss",
        )
        return out

    def render_block_list_ss(self, cams, params: abi.Params, width: int, height: int, block_rows: int, blocks,
                             ss: int, out=None, stream=None):
        """render_block_list with ss x ss samples per pixel (sr_render_block_list_ss):
        sizes and block_rows in output pixels -> [B, len(blocks) * block_rows, W, 4]."""
        blocks = [int(b) for b in blocks]
        B = len(cams)
        arr = (abi.Camera * B)(*cams)
        lst = (C.c_int * len(blocks))(*blocks)
        rows = len(blocks) * block_rows
        if out is None:
            out = self.torch.empty((B, rows, width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and tuple(out.shape[:1]) == (B,)
        assert out[0].numel() >= rows * width * 4
        abi.check(
            self.lib.sr_render_block_list_ss(self.ctx, arr, B, C.byref(params), width, height, block_rows, lst,
                                             len(blocks), int(ss), C.c_void_p(out.data_ptr()), width * 4,
                                             out[0].numel(), self._stream(stream)),
            "sr_render_block_list_ss",
        )
        return out

    def render_phase(self, cam: abi.Camera, params: abi.Params, width: int, height: int, ss: int, phase_x: int,
                     phase_y: int, row_begin: int = 0, row_end: int | None = None, out=None, stream=None):
        """One sub-sample position of every pixel (sr_render_phase): rows
        [row_begin, row_end) of phase (phase_x, phase_y) of the ss x ss grid,
        S[ss * y + phase_y][ss * x + phase_x] of the sample frame -> [rows, width, 4]."""
        row_end = height if row_end is None else row_end
        rows = row_end - row_begin
        if out is None:
            out = self.torch.empty((max(rows, 0), width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and out.numel() >= rows * width * 4
        abi.check(
            self.lib.sr_render_phase(self.ctx, C.byref(cam), C.byref(params), width, height, row_begin, row_end,
                                     int(ss), int(phase_x), int(phase_y), C.c_void_p(out.data_ptr()), width * 4,
                                     self._stream(stream)),
            "sr_render_phase",
        )
        return out

    def new_accum(self, width: int, rows: int):
        """A zeroed accumulator for render_accumulate / accum_add: int16 [rows, width, 4]
        on this device (torch has no uint16 arithmetic; the bits are the ABI's uint16)."""
        return self.torch.zeros((rows, width, 4), dtype=self.torch.int16, device=self.tdev)

    def _check_accum(self, accum):
        assert accum.dtype == self.torch.int16 and accum.dim() == 3 and accum.shape[2] == 4 and accum.is_contiguous()
        return int(accum.shape[0]), int(accum.shape[1])

    def render_accumulate(self, cam: abi.Camera, params: abi.Params, width: int, height: int, ss: int, phases,
                          accum=None, reset: bool = False, row_begin: int = 0, row_end: int | None = None,
                          stream=None):
        """sr_render_accumulate: the phases [(x, y), ...] (at most abi.MAX_BATCH)
        of the ss x ss grid in one launch, added to `accum` (new_accum; a new
        one when None), or stored over it when reset -> accum."""
        row_end = height if row_end is None else row_end
        rows = row_end - row_begin
        if accum is None:
            accum, reset = self.new_accum(width, max(rows, 0)), True
        assert self._check_accum(accum) == (max(rows, 0), width)
        flat = [int(v) for ph in phases for v in ph]
        arr = (C.c_uint8 * max(1, len(flat)))(*flat)
        abi.check(
            self.lib.sr_render_accumulate(self.ctx, C.byref(cam), C.byref(params), width, height, row_begin, row_end,
                                          int(ss), arr, len(flat) // 2, 1 if reset else 0,
                                          C.c_void_p(accum.data_ptr()), width * 8, self._stream(stream)),
            "sr_render_accumulate",
        )
        return accum

    def accum_add(self, images, accum=None, reset: bool = False, stream=None):
        """sr_accum_add on the device: uint8 images [n, rows, W, 4] (or one
        [rows, W, 4]) on this device added to `accum` (a new one when None) -> accum."""
        if images.dim() == 3:
            images = images[None]
        assert images.dtype == self.torch.uint8 and images.dim() == 4 and images.shape[3] == 4 and images.is_contiguous()
        n, rows, w = (int(v) for v in images.shape[:3])
        if accum is None:
            accum, reset = self.new_accum(w, rows), True
        assert self._check_accum(accum) == (rows, w)
        abi.check(
            self.lib.sr_accum_add(C.c_void_p(images.data_ptr()), 4 * w, 4 * w * rows, n, w, rows, 1 if reset else 0,
                                  C.c_void_p(accum.data_ptr()), 8 * w, 1, self._stream(stream)),
            "sr_accum_add",
        )
        return accum

    def accum_resolve(self, accum, n: int, out=None, stream=None):
        """sr_accum_resolve on the device: min(255, (accum + n // 2) // n) of an
        accumulator of n images -> uint8 [rows, W, 4]."""
        rows, w = self._check_accum(accum)
        if out is None:
            out = self.torch.empty((rows, w, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and out.numel() >= rows * w * 4
        abi.check(
            self.lib.sr_accum_resolve(C.c_void_p(accum.data_ptr()), 8 * w, w, rows, int(n), C.c_void_p(out.data_ptr()),
                                      4 * w, 1, self._stream(stream)),
            "sr_accum_resolve",
        )
        return out

    def progressive(self, cam: abi.Camera, params: abi.Params, width: int, height: int, ss: int,
                    phases_per_launch: int = 1, stream=None):
        """Progressive supersampling: renders the ss * ss phases in
        abi.phase_order, phases_per_launch (1 .. abi.MAX_BATCH) per launch,
        and yields (passes_done, frame) after each launch: the [height, width,
        4] frame of the passes so far (a new tensor each time). The last one
        equals render_ss's frame."""
        order = abi.phase_order(ss)
        if not 1 <= int(phases_per_launch) <= abi.MAX_BATCH:
            raise ValueError(f"phases_per_launch must be in 1 .. {abi.MAX_BATCH}")
        accum = self.new_accum(width, height)
        done = 0
        while done < len(order):
            group = order[done:done + int(phases_per_launch)]
            self.render_accumulate(cam, params, width, height, ss, group, accum=accum, reset=done == 0, stream=stream)
            done += len(group)
            yield done, self.accum_resolve(accum, done, stream=stream)

    def render_adaptive(self, cam: abi.Camera, params: abi.Params, width: int, height: int, ss: int, threshold: int,
                        grow: int = 0, out=None, stream=None):
        """The whole frame with ss x ss samples only in the 16x16 tiles that
        hold an edge of the plain frame (sr_render_adaptive) ->
        ([height, width, 4] frame, uint8 [ceil(H / 16), ceil(W / 16)] flagged tiles)."""
        if out is None:
            out = self.torch.empty((height, width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and out.numel() >= height * width * 4
        mask = self.torch.empty(((height + 15) // 16, (width + 15) // 16), dtype=self.torch.uint8, device=self.tdev)
        abi.check(
            self.lib.sr_render_adaptive(self.ctx, C.byref(cam), C.byref(params), width, height, int(ss), int(threshold),
                                        int(grow), C.c_void_p(out.data_ptr()), width * 4, C.c_void_p(mask.data_ptr()),
                                        self._stream(stream)),
            "sr_render_adaptive",
        )
        return out, mask

    def edge_tiles(self, frame, threshold: int, grow: int = 0, stream=None):
        """sr_edge_tiles on the device: an [H, W, 4] uint8 tensor on this device
        -> its flagged tiles, uint8 [ceil(H / 16), ceil(W / 16)]. Asynchronous."""
        assert frame.dtype == self.torch.uint8 and frame.dim() == 3 and frame.shape[2] == 4 and frame.is_contiguous()
        h, w = int(frame.shape[0]), int(frame.shape[1])
        mask = self.torch.empty(((h + 15) // 16, (w + 15) // 16), dtype=self.torch.uint8, device=self.tdev)
        abi.check(
            self.lib.sr_edge_tiles(C.c_void_p(frame.data_ptr()), w * 4, w, h, int(threshold), int(grow),
                                   C.c_void_p(mask.data_ptr()), 1, self._stream(stream)),
            "sr_edge_tiles",
        )
        return mask

    def render_debug(self, cam: abi.Camera, params: abi.Params, width: int, height: int, row_begin: int = 0,
                     row_end: int | None = None, stream=None):
        """(float RGBA FragColor, RGBA8, executed steps) for rows [row_begin, row_end)."""
        t = self.torch
        row_end = height if row_end is None else row_end
        rows = row_end - row_begin
        f = t.empty((rows, width, 4), dtype=t.float32, device=self.tdev)
        b = t.empty((rows, width, 4), dtype=t.uint8, device=self.tdev)
        s = t.empty((rows, width), dtype=t.int32, device=self.tdev)
        abi.check(
            self.lib.sr_render_debug(self.ctx, C.byref(cam), C.byref(params), width, height, row_begin, row_end,
                                     C.c_void_p(f.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(s.data_ptr()),
                                     self._stream(stream)),
            "sr_render_debug",
        )
        return f, b, s

    # ---- scene sequences (sr.h): one launch renders frames of different scenes ----
    def set_scene_sequence(self, scenes) -> None:
        """sr_set_scene_sequence: snapshot copies of the scenes (at most
        abi.MAX_SEQUENCE) as the context's sequence; an empty list clears it."""
        scenes = list(scenes)
        arr = (abi.Scene * max(1, len(scenes)))(*scenes)
        abi.check(self.lib.sr_set_scene_sequence(self.ctx, arr, len(scenes)), "sr_set_scene_sequence")

    def scene_sequence_length(self) -> int:
        return int(self.lib.sr_scene_sequence_length(self.ctx))

    def render_sequence(self, first_scene: int, cams, params: abi.Params, width: int, height: int, row_begin: int = 0,
                        row_end: int | None = None, ss: int = 1, out=None, stream=None):
        """sr_render_sequence: rows [row_begin, row_end) of len(cams) frames in
        one launch, frame f of scene first_scene + f of the sequence with
        cams[f] -> [B, rows, W, 4]. Asynchronous."""
        row_end = height if row_end is None else row_end
        rows = max(row_end - row_begin, 0)
        B = len(cams)
        arr = (abi.Camera * B)(*cams)
        if out is None:
            out = self.torch.empty((B, rows, width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and tuple(out.shape[:1]) == (B,)
        assert out[0].numel() >= rows * width * 4
        abi.check(
            self.lib.sr_render_sequence(self.ctx, int(first_scene), arr, B, C.byref(params), width, height, row_begin,
                                        row_end, int(ss), C.c_void_p(out.data_ptr()), width * 4, out[0].numel(),
                                        self._stream(stream)),
            "sr_render_sequence",
        )
        return out

    def render_sequence_block_list(self, first_scene: int, cams, params: abi.Params, width: int, height: int,
                                   block_rows: int, blocks, ss: int = 1, out=None, stream=None):
        """render_sequence for the rows of an explicit block list (-1 = padding)
        -> [B, len(blocks) * block_rows, W, 4]."""
        blocks = [int(b) for b in blocks]
        B = len(cams)
        arr = (abi.Camera * B)(*cams)
        lst = (C.c_int * len(blocks))(*blocks)
        rows = len(blocks) * block_rows
        if out is None:
            out = self.torch.empty((B, rows, width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and tuple(out.shape[:1]) == (B,)
        assert out[0].numel() >= rows * width * 4
        abi.check(
            self.lib.sr_render_sequence_block_list(self.ctx, int(first_scene), arr, B, C.byref(params), width, height,
                                                   block_rows, lst, len(blocks), int(ss), C.c_void_p(out.data_ptr()),
                                                   width * 4, out[0].numel(), self._stream(stream)),
            "sr_render_sequence_block_list",
        )
        return out

    def render_sequence_debug(self, scene_index: int, cam: abi.Camera, params: abi.Params, width: int, height: int,
                              row_begin: int = 0, row_end: int | None = None, stream=None):
        """render_debug of scene scene_index of the sequence."""
        t = self.torch
        row_end = height if row_end is None else row_end
        rows = row_end - row_begin
        f = t.empty((rows, width, 4), dtype=t.float32, device=self.tdev)
        b = t.empty((rows, width, 4), dtype=t.uint8, device=self.tdev)
        s = t.empty((rows, width), dtype=t.int32, device=self.tdev)
        abi.check(
            self.lib.sr_render_sequence_debug(self.ctx, int(scene_index), C.byref(cam), C.byref(params), width, height,
                                              row_begin, row_end, C.c_void_p(f.data_ptr()), C.c_void_p(b.data_ptr()),
                                              C.c_void_p(s.data_ptr()), self._stream(stream)),
            "sr_render_sequence_debug",
        )
        return f, b, s

    # ---- shutter frames (sr.h): motion blur and anti-aliasing from one batched launch ----
    def _shutter_args(self, cams, sub_frames: int, phases):
        """(camera array, phase bytes or None, M) of M * sub_frames sub-frames."""
        n, k = len(cams), int(sub_frames)
        if k < 1 or n < 1 or n % k:
            raise ValueError(f"expected M * {k} cameras, got {n}")
        arr = (abi.Camera * n)(*cams)
        ph = None
        if phases is not None:
            flat = [int(v) for pair in phases for v in pair]
            if len(flat) != 2 * n:
                raise ValueError(f"expected {n} phase pairs, got {len(flat) // 2}")
            ph = (C.c_uint8 * len(flat))(*flat)
        return arr, ph, n // k

    def render_shutter(self, first_scene: int, cams, sub_frames: int, params: abi.Params, width: int, height: int,
                       ss: int = 1, phases=None, row_begin: int = 0, row_end: int | None = None, out=None, stream=None):
        """sr_render_shutter: rows [row_begin, row_end) of M = len(cams) //
        sub_frames shutter frames in one launch; frame m is the rounded mean of
        its sub_frames sub-frames, sub-frame j of scene first_scene + j of the
        sequence (abi.SHUTTER_OWN_SCENE: the context's own scene) with cams[j]
        and phase phases[j] of the ss x ss grid (None: the progressive order)
        -> [M, rows, W, 4]. Asynchronous."""
        row_end = height if row_end is None else row_end
        rows = max(row_end - row_begin, 0)
        arr, ph, M = self._shutter_args(cams, sub_frames, phases)
        if out is None:
            out = self.torch.empty((M, rows, width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and tuple(out.shape[:1]) == (M,)
        assert out[0].numel() >= rows * width * 4
        abi.check(
            self.lib.sr_render_shutter(self.ctx, int(first_scene), arr, ph, int(sub_frames), M, C.byref(params), width,
                                       height, row_begin, row_end, int(ss), C.c_void_p(out.data_ptr()), width * 4,
                                       out[0].numel(), self._stream(stream)),
            "sr_render_shutter",
        )
        return out

    def render_shutter_block_list(self, first_scene: int, cams, sub_frames: int, params: abi.Params, width: int,
                                  height: int, block_rows: int, blocks, ss: int = 1, phases=None, out=None,
                                  stream=None):
        """render_shutter for the rows of an explicit block list (-1 = padding)
        -> [M, len(blocks) * block_rows, W, 4]."""
        blocks = [int(b) for b in blocks]
        arr, ph, M = self._shutter_args(cams, sub_frames, phases)
        lst = (C.c_int * len(blocks))(*blocks)
        rows = len(blocks) * block_rows
        if out is None:
            out = self.torch.empty((M, rows, width, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and tuple(out.shape[:1]) == (M,)
        assert out[0].numel() >= rows * width * 4
        abi.check(
            self.lib.sr_render_shutter_block_list(self.ctx, int(first_scene), arr, ph, int(sub_frames), M,
                                                  C.byref(params), width, height, block_rows, lst, len(blocks), int(ss),
                                                  C.c_void_p(out.data_ptr()), width * 4, out[0].numel(),
                                                  self._stream(stream)),
            "sr_render_shutter_block_list",
        )
        return out

    def accumulate_shutter(self, first_scene: int, cams, params: abi.Params, width: int, height: int, ss: int = 1,
                           phases=None, accum=None, reset: bool = False, row_begin: int = 0,
                           row_end: int | None = None, stream=None):
        """sr_render_accumulate_shutter: the len(cams) (at most abi.MAX_BATCH)
        sub-frames of one group in one launch, added to `accum` (new_accum; a
        new one when None), or stored over it when reset -> accum. Resolve
        with accum_resolve and the number of sub-frames added."""
        row_end = height if row_end is None else row_end
        rows = row_end - row_begin
        if accum is None:
            accum, reset = self.new_accum(width, max(rows, 0)), True
        assert self._check_accum(accum) == (max(rows, 0), width)
        arr, ph, _ = self._shutter_args(cams, len(cams), phases)
        abi.check(
            self.lib.sr_render_accumulate_shutter(self.ctx, int(first_scene), arr, ph, len(cams), C.byref(params), width,
                                                  height, row_begin, row_end, int(ss), 1 if reset else 0,
                                                  C.c_void_p(accum.data_ptr()), width * 8, self._stream(stream)),
            "sr_render_accumulate_shutter",
        )
        return accum

    def shutter_resolve(self, images, sub_frames: int, out=None, stream=None):
        """sr_shutter_resolve on the device: uint8 images [M * sub_frames, rows,
        W, 4] on this device -> the M frames [M, rows, W, 4]. Asynchronous."""
        assert images.dtype == self.torch.uint8 and images.dim() == 4 and images.shape[3] == 4 and images.is_contiguous()
        n, rows, w = (int(v) for v in images.shape[:3])
        k = int(sub_frames)
        if k < 1 or n < 1 or n % k:
            raise ValueError(f"expected M * {k} images, got {n}")
        if out is None:
            out = self.torch.empty((n // k, rows, w, 4), dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and out.numel() >= (n // k) * rows * w * 4
        abi.check(
            self.lib.sr_shutter_resolve(C.c_void_p(images.data_ptr()), 4 * w, 4 * w * rows, k, n // k, w, rows,
                                        C.c_void_p(out.data_ptr()), 4 * w, 4 * w * rows, 1, self._stream(stream)),
            "sr_shutter_resolve",
        )
        return out

    # ---- retained frames (sr.h): relight and pick from the last launch's rays ----
    def can_reshade(self) -> bool:
        """sr_can_reshade: the context holds a retained frame reshade() would accept."""
        return bool(self.lib.sr_can_reshade(self.ctx))

    def _retained_shape(self, what: str):
        """(width, rows, frames, ss) of the retained launch's output."""
        buf = (C.c_int * 4)()
        abi.check(self.lib.sr_debug_retained_shape(self.ctx, buf), what)
        return tuple(int(v) for v in buf)

    def reshade(self, out=None, stream=None):
        """sr_reshade: the retained launch's frame(s) again from its rays, with
        the current scene, background and textures -> a uint8 tensor shaped
        like that launch's output ([rows, W, 4], or [B, rows, W, 4] for a batch
        or a block list). Asynchronous."""
        w, rows, frames, _ = self._retained_shape("sr_reshade")
        if out is None:
            shape = (rows, w, 4) if frames == 1 else (frames, rows, w, 4)
            out = self.torch.empty(shape, dtype=self.torch.uint8, device=self.tdev)
        assert out.is_contiguous() and out.dtype == self.torch.uint8 and out.numel() >= frames * rows * w * 4
        abi.check(self.lib.sr_reshade(self.ctx, C.c_void_p(out.data_ptr()), w * 4, rows * w * 4, self._stream(stream)),
                  "sr_reshade")
        return out

    def reshade_debug(self, stream=None):
        """sr_reshade_debug: (float RGBA FragColor, RGBA8, executed steps) of the
        retained launch (one frame, not supersampled), as render_debug returns them."""
        t = self.torch
        w, rows, _, _ = self._retained_shape("sr_reshade_debug")
        f = t.empty((rows, w, 4), dtype=t.float32, device=self.tdev)
        b = t.empty((rows, w, 4), dtype=t.uint8, device=self.tdev)
        s = t.empty((rows, w), dtype=t.int32, device=self.tdev)
        abi.check(self.lib.sr_reshade_debug(self.ctx, C.c_void_p(f.data_ptr()), C.c_void_p(b.data_ptr()),
                                            C.c_void_p(s.data_ptr()), self._stream(stream)), "sr_reshade_debug")
        return f, b, s

    def pick_map(self, out=None, stream=None):
        """sr_pick_map: per pixel of the retained launch the index into
        scene.objects[] of the first surface on its (bent) ray, or an
        abi.PICK_* code -> int32 [rows, W] ([B, rows, W] for a batch or a
        block list; rows the launch left unwritten are left unwritten). Asynchronous."""
        w, rows, frames, ss = self._retained_shape("sr_pick_map")
        if out is None:
            shape = (rows, w) if frames == 1 else (frames, rows, w)
            out = self._filled(shape, abi.PICK_NONE, self.torch.int32, stream)
        assert out.is_contiguous() and out.dtype == self.torch.int32 and out.numel() >= frames * rows * w
        abi.check(self.lib.sr_pick_map(self.ctx, C.c_void_p(out.data_ptr()), w * 4, rows * w * 4, self._stream(stream)),
                  "sr_pick_map")
        return out

    def pick(self, x: int, y: int, frame: int = 0) -> int:
        """One entry of pick_map: output column x, output row y (row 0 = the
        launch's first row, GL order) of frame `frame`. Waits for the map."""
        m = self.pick_map()
        if m.dim() == 3:
            m = m[frame]
        return int(m[int(y), int(x)].item())

    # ---- ray maps (sr.h): the lens map and the first surface's G-buffer ----
    def ray_maps(self, which=tuple(abi.RAY_MAPS), out=None, stream=None):
        """sr_ray_maps: the maps named in `which` (keys of abi.RAY_MAPS) of the
        retained launch -> a dict of tensors shaped like pick_map's with the
        map's components last: [rows, W, n], or [B, rows, W, n] for a batch or
        a block list (int32 for "end", "id" and "hit_step", float32 otherwise;
        rows the launch left unwritten hold NaN, -1, RAY_END_NONE or PICK_NONE).
        out: a dict of such tensors to write into instead. Asynchronous."""
        t = self.torch
        which = tuple(which)
        if not which or any(k not in abi.RAY_MAPS for k in which):
            raise ValueError(f"ray_maps: maps are {tuple(abi.RAY_MAPS)}, at least one")
        w, rows, frames, _ = self._retained_shape("sr_ray_maps")
        fill = {"end": abi.RAY_END_NONE, "id": abi.PICK_NONE, "hit_step": -1}
        maps, ptrs = {}, abi.RayMapPtrs()
        for key in which:
            n, dtype = abi.RAY_MAPS[key]
            dt = getattr(t, dtype)
            if out is not None and key in out:
                m = out[key]
                assert m.is_contiguous() and m.dtype == dt and m.numel() >= frames * rows * w * n
            else:
                shape = (rows, w, n) if frames == 1 else (frames, rows, w, n)
                m = self._filled(shape, fill.get(key, float("nan")), dt, stream)
            maps[key] = m
            setattr(ptrs, key, m.data_ptr())
        abi.check(self.lib.sr_ray_maps(self.ctx, C.byref(ptrs), w, rows * w, self._stream(stream)), "sr_ray_maps")
        return maps

    # ---- ray queries (sr.h): caller-supplied rays through the current scene ----
    def trace_rays(self, origins, dirs, params: abi.Params, rgba32: bool = False, rgba8: bool = True,
                   steps: bool = False, ids: bool = False, stream=None):
        """sr_trace_rays: ray i from origins[i] along dirs[i] ((N, 3) float32
        tensors on this device; the directions need not be normalised) -> a
        dict of the requested tensors, one entry per ray: "rgba32" float32
        [N, 4] FragColor, "rgba8" uint8 [N, 4], "steps" int32 [N] and "ids"
        int32 [N] (pick_map's codes). Asynchronous."""
        t = self.torch
        for a in (origins, dirs):
            assert a.dtype == t.float32 and a.dim() == 2 and a.shape[1] == 3 and a.is_contiguous()
            assert a.device == self.tdev
        n = int(origins.shape[0])
        assert int(dirs.shape[0]) == n
        if not (rgba32 or rgba8 or steps or ids):
            raise ValueError("trace_rays: no output requested")
        out = {}
        if rgba32:
            out["rgba32"] = t.empty((n, 4), dtype=t.float32, device=self.tdev)
        if rgba8:
            out["rgba8"] = t.empty((n, 4), dtype=t.uint8, device=self.tdev)
        if steps:
            out["steps"] = t.empty((n,), dtype=t.int32, device=self.tdev)
        if ids:
            out["ids"] = t.empty((n,), dtype=t.int32, device=self.tdev)

        def ptr(key):
            return C.c_void_p(out[key].data_ptr()) if key in out and n else None

        abi.check(
            self.lib.sr_trace_rays(self.ctx, C.c_void_p(origins.data_ptr()) if n else None,
                                   C.c_void_p(dirs.data_ptr()) if n else None, n, C.byref(params), ptr("rgba32"),
                                   ptr("rgba8"), ptr("steps"), ptr("ids"), self._stream(stream)),
            "sr_trace_rays",
        )
        return out

    # ---- ray maps of ray queries (sr.h): the maps of caller-supplied rays ----
    def trace_ray_maps(self, origins, dirs, params: abi.Params, which=tuple(abi.RAY_MAPS), out=None, stream=None):
        """sr_trace_ray_maps: the maps named in `which` (keys of abi.RAY_MAPS)
        of trace_rays' rays -> a dict of [N, n] tensors, one row per ray
        (int32 for "end", "id" and "hit_step", float32 otherwise). out: a dict
        of such tensors to write into instead. Asynchronous."""
        t = self.torch
        for a in (origins, dirs):
            assert a.dtype == t.float32 and a.dim() == 2 and a.shape[1] == 3 and a.is_contiguous()
            assert a.device == self.tdev
        n = int(origins.shape[0])
        assert int(dirs.shape[0]) == n
        which = tuple(which)
        if not which or any(k not in abi.RAY_MAPS for k in which):
            raise ValueError(f"trace_ray_maps: maps are {tuple(abi.RAY_MAPS)}, at least one")
        maps, ptrs = {}, abi.RayMapPtrs()
        for key in which:
            c, dtype = abi.RAY_MAPS[key]
            dt = getattr(t, dtype)
            if out is not None and key in out:
                m = out[key]
                assert m.is_contiguous() and m.dtype == dt and m.numel() >= n * c and m.device == self.tdev
            else:
                m = t.empty((n, c), dtype=dt, device=self.tdev)
            maps[key] = m
            if n:
                setattr(ptrs, key, m.data_ptr())
        abi.check(
            self.lib.sr_trace_ray_maps(self.ctx, C.c_void_p(origins.data_ptr()) if n else None,
                                       C.c_void_p(dirs.data_ptr()) if n else None, n, C.byref(params), C.byref(ptrs),
                                       self._stream(stream)),
            "sr_trace_ray_maps",
        )
        return maps

    def close(self) -> None:
        if self.ctx:
            self.lib.sr_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
