#!/usr/bin/env python3
"""Put another sky behind a frame without tracing it again: the usage example
of sr_ray_maps' lens map (sr.h "Ray maps").

Renders the app's default scene once, takes `end` and `sky_uv` of the retained
rays, and writes a PNG in which every pixel whose ray ends in the sky is
looked up in the image given on the command line: any size (not the 8-bit
equirectangular skybox baked into the frame by sr_set_background), bilinear,
in numpy. Pixels that end at a surface keep the frame's colour; a sky seen
through a translucent surface is mixed in under the surface's alpha as the
shader adds it (frag:935: FragColor += get_bg).

  python tools/resky.py --sky panorama.png --out frame.png [--width 1920 --height 1080 --max-steps 2000]
  python tools/resky.py --sky stars.jpg --projection equirect --fov 360 --width 2048 --height 1024 --out pano.png
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def bilinear(img, u, v):
    """img [h, w, c] float at (u, v) in [0, 1]^2, texel centres at (i + 0.5) / n, u wrapping and v clamped;
    v = 0 is the image's bottom row (the skybox convention of sr_set_background)."""
    import numpy as np

    h, w, _ = img.shape
    x = u * w - 0.5
    y = (1.0 - v) * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    x0, x1 = x0.astype(np.int64) % w, (x0.astype(np.int64) + 1) % w
    y0, y1 = np.clip(y0.astype(np.int64), 0, h - 1), np.clip(y0.astype(np.int64) + 1, 0, h - 1)
    top = img[y0, x0] * (1.0 - fx) + img[y0, x1] * fx
    bottom = img[y1, x0] * (1.0 - fx) + img[y1, x1] * fx
    return top * (1.0 - fy) + bottom * fy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sky", required=True, help="an equirectangular image of any size (what PIL opens)")
    ap.add_argument("--out", required=True, help="PNG path")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-steps", type=int, default=2000)
    ap.add_argument("--projection", choices=["rectilinear", "equirect", "fisheye"], default="rectilinear")
    ap.add_argument("--fov", type=float, default=None)
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    sky = np.asarray(Image.open(args.sky).convert("RGB"), dtype=np.float32) / 255.0
    arr = (pkg.assets.texture_array() if args.textures == "assets" else sc.default_texture_array())[0]
    cam = abi.default_camera()
    if args.fov is not None:
        cam.fov = args.fov
    params = abi.default_params(max_steps=args.max_steps, percent_black=-1.0)
    with pkg.Renderer(0) as r:
        r.set_scene(sc.scene_default(textured=True))
        r.set_texture_array(arr)
        r.set_background(np.zeros((1, 1, 4), dtype=np.uint8))  # a sky that adds nothing: the surfaces alone
        r.set_projection(args.projection)
        frame = r.render(cam, params, args.width, args.height)
        maps = r.ray_maps(("end", "sky_uv"))
        torch.cuda.synchronize()
        frame = frame.cpu().numpy().astype(np.float32) / 255.0
        end = maps["end"].cpu().numpy()[..., 0]
        uv = maps["sky_uv"].cpu().numpy()
    ends_in_sky = end == abi.RAY_END_SKY
    u, v = uv[ends_in_sky, 0], uv[ends_in_sky, 1]
    ok = np.isfinite(u) & np.isfinite(v)  # (a NaN v: a direction of |y| > 1, from a non-finite camera only)
    colour = np.zeros((ends_in_sky.sum(), 3), dtype=np.float32)
    colour[ok] = bilinear(sky, u[ok], np.clip(v[ok], 0.0, 1.0))
    out = frame.copy()
    out[ends_in_sky, :3] += colour  # FragColor += get_bg(dir), on top of the translucent hits' sum
    out[ends_in_sky, 3] = 1.0
    out8 = np.ascontiguousarray((np.clip(out, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8))
    abi.write_png(args.out, out8)
    print(f"{args.out}: {int(ends_in_sky.sum())} of {end.size} pixels from {args.sky} "
          f"({sky.shape[1]} x {sky.shape[0]}), {int((end == abi.RAY_END_OPAQUE).sum())} end at a surface")


if __name__ == "__main__":
    main()
