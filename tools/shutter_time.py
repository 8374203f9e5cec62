#!/usr/bin/env python3
"""Times shutter frames (sr_render_shutter) against what they replace and
against anti-aliasing without blur. Every leg runs calls back to back on one
stream after a warm-up, one device event between calls; the legs run one after
the other in each of --rounds interleaved rounds. One JSON line out (per leg:
the rounds' medians, their median and their max - min).

The scenes are an orbit sequence (the default scene's sphere once around the
hole, 32 scenes at the sub-frame times of 8 frames x 4 sub-frames), the camera
the app's default one. Legs:
  A  the composition an earlier revision can express for ss 1, on --render-lib
     when given (another build of the library, e.g. the parent commit's, in a
     context of its own), else on this tree's: sr_render_sequence of the 32
     sub-frames, then eight sr_accum_add (4 images, reset) and eight
     sr_accum_resolve
  B  sr_render_shutter, 8 frames x 4 sub-frames, ss 1: the same sub-frames
  C  the same at ss 2 with the default phases
  D  sr_render_sequence ss 2 of 8 frames: C's sample count, no blur
  E  sr_render_shutter, 2 frames x 16 sub-frames, ss 4
  F  sr_render_sequence ss 4 of 2 frames: E's sample count, no blur
(run leg B under `rocprofv3 --kernel-trace --stats` for the resolve kernel's
own duration; --resolve-stats reads that run's kernel statistics)

  python tools/shutter_time.py [--width 1920 --height 1080 --steps 2000]
  python tools/shutter_time.py --render-lib path/to/parent/libsr.so
  python tools/shutter_time.py --resolve-stats DIR_OR_CSV   (no GPU: the resolve kernel's time and bytes/s)
"""
import argparse
import csv
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

M, K = 8, 4  # leg B's frames and sub-frames


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def resolve_stats(path, width, height):
    """The shutter resolve kernel's row of a rocprofv3 --stats run (its
    kernel_stats CSV, or the directory that holds it): calls, mean ns, and the
    achieved rate over leg B's algorithmic bytes, (4 K + 4) per pixel of M frames."""
    p = Path(path)
    files = [p] if p.is_file() else sorted(p.rglob("*kernel_stats.csv"))
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                if "sr_shutter_resolve_kernel" in row.get("Name", ""):
                    calls, total = int(row["Calls"]), float(row["TotalDurationNs"])
                    mean_ns = total / calls
                    nbytes = (4 * K + 4) * width * height * M
                    return {"kernel": row["Name"], "calls": calls, "mean_us": round(mean_ns / 1e3, 3),
                            "bytes_per_call": nbytes, "gbytes_per_s": round(nbytes / mean_ns, 2)}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="A,B,C,D,E,F")
    ap.add_argument("--render-lib", default=None, help="the library of leg A (default: this tree's)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per leg and round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    ap.add_argument("--resolve-stats", default=None, metavar="PATH")
    args = ap.parse_args()
    W, H = args.width, args.height
    if args.resolve_stats:
        print(json.dumps({"tool": "shutter_time", "width": W, "height": H, "frames": M, "sub_frames": K,
                          "resolve": resolve_stats(args.resolve_stats, W, H)}))
        return
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    if args.textures == "assets":
        bg = pkg.assets.skybox("2k")
        arr, _, _ = pkg.assets.texture_array()
    else:
        bg = sc.skybox(2048, 1024)
        arr, _, _ = sc.default_texture_array()
    params = abi.default_params(max_steps=args.steps, percent_black=-1.0)
    cam = abi.default_camera()
    other = abi.load(args.render_lib) if args.render_lib else None

    def orbit_scene(t):
        s = sc.scene_default(textured=True)
        pos = s.spheres[0].transform.pos
        radius, phase = math.hypot(pos[0], pos[2]), math.atan2(pos[2], pos[0])
        pos[0] = radius * math.cos(phase + 2.0 * math.pi * t)
        pos[2] = radius * math.sin(phase + 2.0 * math.pi * t)
        return s

    scenes = [orbit_scene((j // K + ((j % K) + 0.5) / K) / M) for j in range(M * K)]

    def context(lib):
        r = pkg.Renderer(0, lib=lib)
        r.set_background(bg)
        r.set_texture_array(arr)
        r.set_scene_sequence(scenes)
        return r

    mine = context(None)
    theirs = context(other) if other is not None else mine
    cams = [cam] * (M * K)
    u8 = dict(dtype=torch.uint8, device=dev)
    subs = torch.empty((M * K, H, W, 4), **u8)  # leg A's sub-frames
    out = torch.empty((M, H, W, 4), **u8)
    acc = theirs.new_accum(W, H)

    def leg_a(r=theirs):
        r.render_sequence(0, cams, params, W, H, out=subs, stream=stream)
        for m in range(M):
            r.accum_add(subs[m * K:(m + 1) * K], accum=acc, reset=True, stream=stream)
            r.accum_resolve(acc, K, out=out[m], stream=stream)

    calls = {
        "A": leg_a,
        "B": lambda: mine.render_shutter(0, cams, K, params, W, H, 1, out=out, stream=stream),
        "C": lambda: mine.render_shutter(0, cams, K, params, W, H, 2, out=out, stream=stream),
        "D": lambda: mine.render_sequence(0, cams[:M], params, W, H, ss=2, out=out, stream=stream),
        "E": lambda: mine.render_shutter(0, cams, 16, params, W, H, 4, out=out[:2], stream=stream),
        "F": lambda: mine.render_sequence(0, cams[:2], params, W, H, ss=4, out=out[:2], stream=stream),
    }
    what = {"A": "sr_render_sequence 32 + 8 x (sr_accum_add 4, sr_accum_resolve)", "B": "sr_render_shutter 8 x 4, ss 1",
            "C": "sr_render_shutter 8 x 4, ss 2", "D": "sr_render_sequence 8, ss 2", "E": "sr_render_shutter 2 x 16, ss 4",
            "F": "sr_render_sequence 2, ss 4"}
    legs = [{"leg": n, "what": what[n], "lib": "render-lib" if n == "A" and other is not None else "this",
             "ms_median": [], "ms_min": []} for n in args.legs.split(",") if n]
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for res in legs:
            call = calls[res["leg"]]
            for _ in range(args.warmup):
                call()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.calls + 1)]
            ev[0].record(stream)
            for i in range(args.calls):
                call()
                ev[i + 1].record(stream)
            torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.calls))
            res["ms_median"].append(round(ms[len(ms) // 2], 4))
            res["ms_min"].append(round(ms[0], 4))
    by = {}
    for res in legs:
        res["ms"] = median(res["ms_median"])
        res["spread_ms"] = round(max(res["ms_median"]) - min(res["ms_median"]), 4)
        by[res["leg"]] = res
    ratios = {}
    for a, b in (("B", "A"), ("C", "D"), ("E", "F"), ("C", "B")):
        if a in by and b in by:
            ratios[f"{a}/{b}"] = round(by[a]["ms"] / by[b]["ms"], 4)
    verdict = None
    if "A" in by and "B" in by:  # B within A's median plus A's own spread over the rounds
        verdict = by["B"]["ms"] <= by["A"]["ms"] + by["A"]["spread_ms"]
    diag = {}
    for r in {id(r): r for r in (mine, theirs)}.values():
        for k, v in r.diag_counters().items():
            diag[k] = diag.get(k, 0) + v
    print(json.dumps({
        "tool": "shutter_time", "width": W, "height": H, "steps": args.steps, "calls": args.calls, "warmup": args.warmup,
        "rounds": args.rounds, "textures": args.textures, "render_lib": args.render_lib, "legs": legs, "ratios": ratios,
        "b_within_a_plus_spread": verdict, "diag": diag,
    }))
    for r in {id(r): r for r in (mine, theirs)}.values():
        r.close()


if __name__ == "__main__":
    main()
