#!/usr/bin/env python3
"""Times sample-phase rendering against the plain and the fully supersampled
frame: every leg renders frames back to back on one stream after a warm-up,
one device event between frames; the legs run one after the other in each of
--rounds interleaved rounds on one context. One JSON line out (per leg: the
rounds' medians and their median).

Legs, each "frame" a complete WIDTH x HEIGHT output frame at --ss:
  plain      sr_render (one sample per pixel)
  ss         sr_render_ss
  acc_all    every phase in sr_render_accumulate launches of --per-launch
             phases (default: all ss ss, at most 32) + sr_accum_resolve
  acc_each   one phase per sr_render_accumulate launch back to back in
             sr_phase_order, an sr_accum_resolve after each (the progressive
             viewer: ss ss displayable frames)
  phase      one sr_render_phase launch (phase (0, 0): one pass alone)
  add        sr_accum_add of --per-launch random images alone
  resolve    sr_accum_resolve alone
(run add / resolve under `rocprofv3 --kernel-trace --stats` for the kernels'
own durations)

  python tools/phase_time.py --ss 2 [--width 1920 --height 1080 --steps 2000]
  python tools/phase_time.py --ss 4 --legs add,resolve --rounds 1
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ss", type=int, default=2)
    ap.add_argument("--legs", default="plain,ss,acc_all,acc_each",
                    help="comma-separated subset of plain, ss, acc_all, acc_each, phase, add, resolve")
    ap.add_argument("--per-launch", type=int, default=0, help="phases per launch of acc_all / images of add (0: ss ss)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
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
    W, H, ss = args.width, args.height, args.ss
    order = abi.phase_order(ss)
    per = min(args.per_launch or len(order), abi.MAX_BATCH)
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
    cam = abi.default_camera()
    out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    accum = r.new_accum(W, H)
    names = [n for n in args.legs.split(",") if n]
    images = None
    if "add" in names:
        g = torch.Generator(device=dev).manual_seed(1)
        images = torch.randint(0, 256, (per, H, W, 4), dtype=torch.uint8, device=dev, generator=g)

    def acc_all():
        for k in range(0, len(order), per):
            r.render_accumulate(cam, params, W, H, ss, order[k:k + per], accum=accum, reset=k == 0, stream=stream)
        r.accum_resolve(accum, len(order), out=out, stream=stream)

    def acc_each():
        for k, ph in enumerate(order):
            r.render_accumulate(cam, params, W, H, ss, [ph], accum=accum, reset=k == 0, stream=stream)
            r.accum_resolve(accum, k + 1, out=out, stream=stream)

    frames = {
        "plain": lambda: r.render(cam, params, W, H, out=out, stream=stream),
        "ss": lambda: r.render_ss(cam, params, W, H, ss, out=out, stream=stream),
        "acc_all": acc_all,
        "acc_each": acc_each,
        "phase": lambda: r.render_phase(cam, params, W, H, ss, 0, 0, out=out, stream=stream),
        "add": lambda: r.accum_add(images, accum, stream=stream),
        "resolve": lambda: r.accum_resolve(accum, len(order), out=out, stream=stream),
    }
    results = [{"leg": n, "ms_median": [], "ms_min": [], "ms_mean": []} for n in names]
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for res in results:
            frame = frames[res["leg"]]
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
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    ids = C.c_size_t()  # the context's pixel-state size (the largest launch so far), without the copy
    abi.check(r.lib.sr_debug_pixel_state(r.ctx, None, 0, C.byref(ids)), "sr_debug_pixel_state")
    print(json.dumps({
        "tool": "phase_time", "ss": ss, "per_launch": per, "width": W, "height": H, "steps": args.steps,
        "frames": args.frames, "warmup": args.warmup, "rounds": args.rounds, "textures": args.textures,
        "legs": results, "pixel_state_ids": int(ids.value), "pixel_state_bytes": int(ids.value) * 4 * (abi.PS_FIELDS + 1),
        "plain_frame_ids": tiles * 256, "diag": r.diag_counters(),
    }))
    r.close()


if __name__ == "__main__":
    main()
