#!/usr/bin/env python3
"""Render frames of the app's default scene on the GPU and write them as PNG
(sr_write_png): the offline counterpart of the reference's window present
(src/main.cpp:318-319, 432). A flyby renders N frames along the H-key
hyperbolic trajectory (src/main.cpp:404-410) in batched launches.

  python tools/render.py --out frame.png [--width 1920 --height 1080 --max-steps 2000]
  python tools/render.py --flyby 8 --out flyby_%02d.png
  python tools/render.py --ssaa 2 --out frame_ss2.png      (2 x 2 samples per pixel, box resolve)
  python tools/render.py --ssaa 4 --adaptive 32 --grow 1 --out frame_a4.png
                                  (4 x 4 samples only in the 16x16 tiles with an edge above 32 levels)
  python tools/render.py --progressive 4 --out pass_%02d.png
                                  (progressive supersampling: the frame after each of the 16 passes)
  python tools/render.py --projection equirect --fov 360 --width 2048 --height 1024 --out pano.png
  python tools/render.py --projection fisheye --fov 180 --width 1080 --height 1080 --out dome.png
                                  (sr_set_projection: a 360 degree panorama, a dome master)
  python tools/render.py --aperture 0.15 --focus 5.4 --lens-samples 16 --out dof.png
                                  (thin-lens depth of field: per-ray origins on the lens disk, traced with
                                   sr_trace_rays, the samples' frames averaged)
  python tools/render.py --orbit-frames 48 --out orbit_%02d.png
                                  (the default scene's sphere on a circular orbit: the scenes as one
                                   sequence, sr_set_scene_sequence, rendered 32 frames per launch)
  python tools/render.py --orbit-frames 24 --shutter 4 --ssaa 2 --out blur_%02d.png
  python tools/render.py --flyby 8 --shutter 16 --ssaa 4 --shutter-angle 180 --out flyby_blur_%02d.png
                                  (shutter frames, sr_render_shutter: every frame the mean of K sub-frames at
                                   times spread over the shutter's open part of the frame interval, each with
                                   its own scene or camera and its own sub-pixel phase of the --ssaa grid)
"""
import argparse
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

MODES = {"curved": 0, "flat": 1, "half_width": 2, "half_height": 3}


def thin_lens_frame(pkg, r, cam, params, width, height, aperture, focus, samples, seed=0):
    """Thin-lens depth of field through Renderer.trace_rays -> uint8 [height,
    width, 4] on the device. Every pixel's pinhole ray (sr_camera_rays) meets
    the plane of focus at P = O + focus * V / |V|; sample k starts at a point
    O + aperture * (x c0 + y c1) of the lens, (x, y) uniform on the unit disk
    (c0, c1: the camera's right and up axes), and heads for P. The rays are
    made with torch on the device; the `samples` frames are averaged with
    sr_accum_resolve's rounding, (sum + n / 2) / n per channel. aperture 0:
    the pinhole's own rays, so one sample is the plain render's frame byte for
    byte (the crosshair and the noise mask apart, which a trace launch does
    not draw)."""
    import numpy as np
    import torch

    O, V = pkg.camera_rays(cam, "rectilinear", width, height)
    O = torch.from_numpy(O.reshape(-1, 3)).to(r.tdev)
    V = torch.from_numpy(V.reshape(-1, 3)).to(r.tdev)
    n = O.shape[0]
    ax = torch.tensor(np.array(list(cam.transform.axes), dtype=np.float32).reshape(3, 3), device=r.tdev)
    P = O + float(focus) * V / V.norm(dim=1, keepdim=True)
    gen = torch.Generator(device=r.tdev)
    gen.manual_seed(int(seed))
    total = torch.zeros((n, 4), dtype=torch.int32, device=r.tdev)
    for _ in range(int(samples)):
        if aperture > 0.0:
            rad = float(aperture) * torch.sqrt(torch.rand(n, generator=gen, device=r.tdev))
            ang = 2.0 * math.pi * torch.rand(n, generator=gen, device=r.tdev)
            o = O + (rad * torch.cos(ang))[:, None] * ax[0] + (rad * torch.sin(ang))[:, None] * ax[1]
            o, v = o.contiguous(), (P - o).contiguous()
        else:
            o, v = O, V
        total += r.trace_rays(o, v, params)["rgba8"].to(torch.int32)
    k = int(samples)
    return ((total + k // 2) // k).to(torch.uint8).reshape(height, width, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="PNG path (with %%d for --flyby frames)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-steps", type=int, default=2000)
    ap.add_argument("--mode", choices=sorted(MODES), default="curved")
    ap.add_argument("--percent-black", type=float, default=-1.0)
    ap.add_argument("--crosshair", action="store_true")
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    ap.add_argument("--flyby", type=int, default=0, help="frames along the hyperbolic flyby (0: the default camera)")
    ap.add_argument("--ssaa", type=int, default=1, choices=[1, 2, 3, 4],
                    help="supersampling: N x N samples per pixel, box resolve (sr_render_ss; 1: off)")
    ap.add_argument("--adaptive", type=int, default=None, metavar="THRESHOLD",
                    help="with --ssaa 2 .. 4: supersample only the 16x16 tiles of the plain frame that hold two "
                         "neighbouring pixels more than THRESHOLD levels apart in a channel (sr_render_adaptive)")
    ap.add_argument("--grow", type=int, default=0, choices=[0, 1, 2],
                    help="--adaptive: dilate the flagged tiles this many times by their 3x3 neighbourhood")
    ap.add_argument("--progressive", type=int, default=None, choices=[1, 2, 3, 4], metavar="SS",
                    help="progressive supersampling on an SS x SS grid (Renderer.progressive): one sample phase per "
                         "launch in sr_phase_order, the frame so far written after each pass (--out with %%d for the "
                         "pass number); the last one is --ssaa SS's frame")
    ap.add_argument("--projection", choices=["rectilinear", "equirect", "fisheye"], default="rectilinear",
                    help="the camera projection of every frame (sr_set_projection): the reference's pinhole, "
                         "longitude / latitude, or the equidistant fisheye")
    ap.add_argument("--fov", type=float, default=None,
                    help="the camera's field of view in degrees (default: the app's); under equirect and fisheye "
                         "the angle the frame's width spans, up to 360")
    ap.add_argument("--orbit-frames", type=int, default=0, metavar="N",
                    help="N frames (1 .. 256) of the default scene with its sphere on a circular orbit of its own radius "
                         "about the hole, rendered through one scene sequence (sr_render_sequence; --out with %%d)")
    ap.add_argument("--aperture", type=float, default=None, metavar="R",
                    help="thin-lens depth of field: the lens radius in scene units (0: a pinhole); the frame is "
                         "traced ray by ray (sr_trace_rays) from origins jittered on the lens disk")
    ap.add_argument("--focus", type=float, default=10.0, metavar="D",
                    help="--aperture: the distance along each pixel's pinhole ray that stays sharp")
    ap.add_argument("--lens-samples", type=int, default=16, metavar="K", help="--aperture: lens samples per pixel")
    ap.add_argument("--shutter", type=int, default=0, metavar="K",
                    help="with --orbit-frames or --flyby: motion blur, every frame the mean of K (1 .. 32) sub-frames "
                         "(sr_render_shutter); sub-frame k of frame m of N is at time (m + (k + 1/2) / K * DEG / 360) / N "
                         "and takes phase k of the --ssaa grid in sr_phase_order")
    ap.add_argument("--shutter-angle", type=float, default=360.0, metavar="DEG",
                    help="--shutter: the part of the frame interval the shutter is open, in degrees of 360")
    args = ap.parse_args()
    if args.shutter:
        if not 1 <= args.shutter <= 32 or not 0.0 <= args.shutter_angle <= 360.0:
            ap.error("--shutter takes 1 .. 32 sub-frames (SR_MAX_BATCH) and --shutter-angle 0 .. 360 degrees")
        if bool(args.orbit_frames) == (args.flyby > 0) or args.adaptive is not None or args.progressive is not None \
                or args.aperture is not None:
            ap.error("--shutter blurs the frames of --orbit-frames or of --flyby")
        if args.orbit_frames * args.shutter > 256:
            ap.error("--orbit-frames x --shutter scenes must fit a sequence (SR_MAX_SEQUENCE = 256)")
    if args.aperture is not None:
        if (args.flyby > 0 or args.adaptive is not None or args.progressive is not None or args.orbit_frames or
                args.ssaa != 1 or args.projection != "rectilinear" or args.crosshair or args.percent_black >= 0.0 or
                args.mode not in ("curved", "flat")):
            ap.error("--aperture renders one pinhole frame of traced rays: no other mode, crosshair, noise mask or "
                     "split screen")
        if args.aperture < 0.0 or args.lens_samples < 1:
            ap.error("--aperture takes R >= 0 and --lens-samples K >= 1")
    if args.orbit_frames and (args.flyby > 0 or args.adaptive is not None or args.progressive is not None):
        ap.error("--orbit-frames is a mode of its own: no --flyby, --adaptive or --progressive")
    if not 0 <= args.orbit_frames <= 256:
        ap.error("--orbit-frames takes 1 .. 256 frames (SR_MAX_SEQUENCE)")
    if args.progressive is not None and (args.ssaa != 1 or args.adaptive is not None or args.flyby > 0):
        ap.error("--progressive takes the grid itself: no --ssaa, --adaptive or --flyby")
    if args.adaptive is not None and (args.ssaa < 2 or args.flyby > 0):
        ap.error("--adaptive needs --ssaa 2 .. 4 and a single frame (no --flyby)")
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    r = pkg.Renderer(0)
    r.set_scene(sc.scene_default(textured=True))
    if args.textures == "assets":
        r.set_background(pkg.assets.skybox("8k" if args.width * args.height > 4096 * 2160 else "2k"))
        arr, _, _ = pkg.assets.texture_array()
    else:
        r.set_background(sc.skybox(2048, 1024))
        arr, _, _ = sc.default_texture_array()
    r.set_texture_array(arr)
    r.set_projection(args.projection)
    params = abi.default_params(max_steps=args.max_steps, percent_black=args.percent_black,
                                raytrace_type=MODES[args.mode])
    params.crosshair = 1 if args.crosshair else 0
    W, H = args.width, args.height

    def camera():
        cam = abi.default_camera()
        if args.fov is not None:
            cam.fov = args.fov
        return cam

    def write_frames(out, first):
        torch.cuda.synchronize()
        for k, fr in enumerate(out.cpu().numpy()):
            path = args.out % (first + k) if "%" in args.out else f"{Path(args.out).stem}_{first + k:03d}.png"
            abi.write_png(path, fr)
            print(f"wrote {path}")

    def orbit_scene(t):
        """The default scene with its sphere at turn t of a circle about the hole, in the plane and at the distance it starts at"""
        s = sc.scene_default(textured=True)
        pos = s.spheres[0].transform.pos
        radius, phase = math.hypot(pos[0], pos[2]), math.atan2(pos[2], pos[0])
        pos[0] = radius * math.cos(phase + 2.0 * math.pi * t)
        pos[2] = radius * math.sin(phase + 2.0 * math.pi * t)
        return s

    if args.shutter:
        K = args.shutter
        n = args.orbit_frames or args.flyby
        times = [(j // K + ((j % K) + 0.5) / K * args.shutter_angle / 360.0) / n for j in range(n * K)]
        if args.orbit_frames:  # a scene per sub-frame, one camera
            r.set_scene_sequence([orbit_scene(t) for t in times])
            cams = [camera()] * (n * K)
        else:  # the context's own scene, the flyby camera at the sub-frames' times
            cams = [abi.camera_flyby(t, 30.0, 10.0, cam=camera()) for t in times]
        per = max(1, 32 // K)  # frames per launch: 32 sub-frames
        for first in range(0, n, per):
            m = min(per, n - first)
            out = r.render_shutter(first * K if args.orbit_frames else abi.SHUTTER_OWN_SCENE,
                                   cams[first * K:(first + m) * K], K, params, W, H, args.ssaa)
            write_frames(out, first)
    elif args.aperture is not None:
        frame = thin_lens_frame(pkg, r, camera(), params, W, H, args.aperture, args.focus, args.lens_samples)
        torch.cuda.synchronize()
        abi.write_png(args.out, frame.cpu().numpy())
        print(f"wrote {args.out} ({args.lens_samples} lens samples)")
    elif args.orbit_frames:
        n = args.orbit_frames
        scenes = []
        for k in range(n):  # the sphere once around the hole, in the plane and at the distance it starts at
            s = sc.scene_default(textured=True)
            pos = s.spheres[0].transform.pos
            radius, phase = math.hypot(pos[0], pos[2]), math.atan2(pos[2], pos[0])
            pos[0] = radius * math.cos(phase + 2.0 * math.pi * k / n)
            pos[2] = radius * math.sin(phase + 2.0 * math.pi * k / n)
            scenes.append(s)
        r.set_scene_sequence(scenes)
        per = max(1, min(32, (2 << 30) // (4 * args.ssaa ** 2 * W * H)))
        for first in range(0, n, per):
            m = min(per, n - first)
            out = r.render_sequence(first, [camera()] * m, params, W, H, ss=args.ssaa)
            torch.cuda.synchronize()
            for k, fr in enumerate(out.cpu().numpy()):
                path = args.out % (first + k) if "%" in args.out else f"{Path(args.out).stem}_{first + k:03d}.png"
                abi.write_png(path, fr)
                print(f"wrote {path}")
    elif args.progressive is not None:
        for k, frame in r.progressive(camera(), params, W, H, args.progressive):
            torch.cuda.synchronize()
            path = args.out % k if "%" in args.out else f"{Path(args.out).stem}_{k:02d}.png"
            abi.write_png(path, frame.cpu().numpy())
            print(f"wrote {path} ({k} of {args.progressive ** 2} passes)")
    elif args.flyby <= 0:
        if args.adaptive is not None:
            frame, tiles = r.render_adaptive(camera(), params, W, H, args.ssaa, args.adaptive, args.grow)
            torch.cuda.synchronize()
            print(f"supersampled {int(tiles.sum())} of {tiles.numel()} tiles")
        else:
            frame = r.render_ss(camera(), params, W, H, args.ssaa)
        torch.cuda.synchronize()
        abi.write_png(args.out, frame.cpu().numpy())
        print(f"wrote {args.out}")
    else:
        n = args.flyby
        cams = [abi.camera_flyby((f + 0.5) / n, 30.0, 10.0, cam=camera()) for f in range(n)]
        # up to 32 frames per launch, fewer while the sample scratch of a batch
        # (4 ssaa^2 W H bytes per frame) would pass 2 GiB
        per = max(1, min(32, (2 << 30) // (4 * args.ssaa ** 2 * W * H)))
        for first in range(0, n, per):  # one block of H rows: the whole frame
            out, rows = r.render_block_list_ss(cams[first:first + per], params, W, H, H, [0], args.ssaa), H
            torch.cuda.synchronize()
            for k, fr in enumerate(out.cpu().numpy()):
                path = args.out % (first + k) if "%" in args.out else f"{Path(args.out).stem}_{first + k:03d}.png"
                abi.write_png(path, fr[:rows])
                print(f"wrote {path}")
    r.close()


if __name__ == "__main__":
    main()
