#!/usr/bin/env python3
"""Times one frame of the default scene under each camera projection
(sr_set_projection): every leg renders frames back to back on one stream
after a warm-up, one device event between frames; the legs run one after the
other in each of --rounds interleaved rounds on one context (a change of
projection only picks another launch order and kernel instantiation). One
JSON line out (per leg: the rounds' medians and their median).

Legs (the app's camera with the leg's fov):
  rectilinear  1920 x 1080, the camera's own fov: the headline frame
  equirect     2048 x 1024 at fov 360: the whole sphere
  fisheye      1080 x 1080 at fov 180: a dome master

  python tools/projection_time.py [--steps 2000 --frames 40 --rounds 3]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

# (leg, width, height, fov; None: the camera's own)
LEGS = [("rectilinear", 1920, 1080, None), ("equirect", 2048, 1024, 360.0), ("fisheye", 1080, 1080, 180.0)]


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(l[0] for l in LEGS), help="comma-separated subset of the legs")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    args = ap.parse_args()
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    r = pkg.Renderer(0)
    r.set_scene(sc.scene_default(textured=True))
    if args.textures == "assets":
        r.set_background(pkg.assets.skybox("2k"))
        arr, _, _ = pkg.assets.texture_array()
    else:
        r.set_background(sc.skybox(2048, 1024))
        arr, _, _ = sc.default_texture_array()
    r.set_texture_array(arr)
    params = abi.default_params(max_steps=args.steps, percent_black=-1.0)
    names = [n for n in args.legs.split(",") if n]
    results = []
    for name, w, h, fov in LEGS:
        if name not in names:
            continue
        cam = abi.default_camera()
        if fov is not None:
            cam.fov = fov
        results.append({"leg": name, "width": w, "height": h, "fov": float(cam.fov), "cam": cam,
                        "out": torch.empty((h, w, 4), dtype=torch.uint8, device=dev),
                        "ms_median": [], "ms_min": [], "ms_mean": []})
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for res in results:
            r.set_projection(res["leg"])

            def frame():
                r.render(res["cam"], params, res["width"], res["height"], out=res["out"], stream=stream)

            for _ in range(args.warmup):
                frame()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.frames + 1)]
            ev[0].record(stream)
            for i in range(args.frames):
                frame()
                ev[i + 1].record(stream)
            torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.frames))
            res["ms_median"].append(round(ms[len(ms) // 2], 4))
            res["ms_min"].append(round(ms[0], 4))
            res["ms_mean"].append(round(ev[0].elapsed_time(ev[-1]) / args.frames, 4))
    for res in results:
        res["ms"] = median(res["ms_median"])
        res["mpix_s"] = round(res["width"] * res["height"] / res["ms"] / 1e3, 1)
        del res["cam"], res["out"]
    print(json.dumps({
        "tool": "projection_time", "steps": args.steps, "frames": args.frames, "warmup": args.warmup,
        "rounds": args.rounds, "textures": args.textures, "legs": results, "diag": r.diag_counters(),
    }))
    r.close()


if __name__ == "__main__":
    main()
