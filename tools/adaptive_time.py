#!/usr/bin/env python3
"""Times adaptive supersampling against the plain and the fully supersampled
frame: every leg renders frames back to back on one stream after a warm-up,
one device event between frames; the legs run one after the other in each of
--rounds interleaved rounds on one context. One JSON line out.

Legs: sr_render of the WIDTH x HEIGHT frame ("plain"), sr_render_ss at --ss
("ss"), and sr_render_adaptive at --ss for each threshold of --thresholds
("adaptive", with the flagged tiles / all tiles beside each time).

  python tools/adaptive_time.py --ss 2 --thresholds -1,8,32,128,254 [--grow 0 --width 1920 --height 1080 --steps 2000]
  python tools/adaptive_time.py --ss 4 --thresholds 254 --legs adaptive --rounds 1
      (under `rocprofv3 --kernel-trace --stats`: a threshold that flags nothing and is below 255 launches the
       whole sample grid with every workgroup exiting at once, the price of the empty grid)
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ss", type=int, default=2)
    ap.add_argument("--thresholds", default="-1,8,32,128,254", help="comma-separated sr_render_adaptive thresholds")
    ap.add_argument("--grow", type=int, default=0)
    ap.add_argument("--legs", default="plain,ss,adaptive", help="comma-separated subset of plain, ss, adaptive")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--flyby", type=int, default=0,
                    help="cycle through this many cameras of the hyperbolic flyby, a new one every frame (0: the default camera)")
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    args = ap.parse_args()
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    W, H, ss = args.width, args.height, args.ss
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
    cams = ([abi.camera_flyby((f + 0.5) / args.flyby, 30.0, 10.0) for f in range(args.flyby)]
            if args.flyby > 0 else [abi.default_camera()])
    out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    legs = []
    names = [n for n in args.legs.split(",") if n]
    if "plain" in names:
        legs.append(("plain", None, lambda cam: r.render(cam, params, W, H, out=out, stream=stream)))
    if "ss" in names:
        legs.append(("ss", None, lambda cam: r.render_ss(cam, params, W, H, ss, out=out, stream=stream)))
    if "adaptive" in names:
        for t in (int(v) for v in args.thresholds.split(",")):
            legs.append(("adaptive", t, lambda cam, t=t: r.render_adaptive(cam, params, W, H, ss, t, args.grow, out=out,
                                                                          stream=stream)))
    results = [{"leg": name, "threshold": t, "ms_median": [], "ms_min": [], "ms_mean": []} for name, t, _ in legs]
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for (name, t, frame), res in zip(legs, results):
            for i in range(args.warmup):
                got = frame(cams[i % len(cams)])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.frames + 1)]
            ev[0].record(stream)
            for i in range(args.frames):
                got = frame(cams[i % len(cams)])
                ev[i + 1].record(stream)
            torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.frames))
            res["ms_median"].append(round(ms[len(ms) // 2], 4))
            res["ms_min"].append(round(ms[0], 4))
            res["ms_mean"].append(round(ev[0].elapsed_time(ev[-1]) / args.frames, 4))
            if name == "adaptive":  # the last frame's flagged set
                res["flagged_tiles"] = int(got[1].sum())
                res["tiles"] = int(got[1].numel())
                res["flagged_share"] = round(res["flagged_tiles"] / res["tiles"], 4)
    print(json.dumps({
        "tool": "adaptive_time", "ss": ss, "grow": args.grow, "width": W, "height": H, "steps": args.steps,
        "frames": args.frames, "warmup": args.warmup, "rounds": args.rounds, "flyby": args.flyby,
        "textures": args.textures, "legs": results, "diag": r.diag_counters(),
    }))
    r.close()


if __name__ == "__main__":
    main()
