#!/usr/bin/env python3
"""Times supersampled frames: frames back to back on one stream after a
warm-up, one device event between frames, one JSON line out.

  --mode ss       sr_render_ss of the WIDTH x HEIGHT frame at --ss
  --mode plain    sr_render of the (ss WIDTH) x (ss HEIGHT) frame: the sample
                  frame alone. Needs nothing newer than sr_render, so --lib
                  may name a library built from an earlier commit.
  --mode resolve  sr_resolve_box on the device alone, on random samples (run
                  it under `rocprofv3 --kernel-trace --stats` for the kernel's
                  own duration)

  python tools/ssaa_time.py --mode ss --ss 2 [--width 1920 --height 1080 --steps 2000]
  python tools/ssaa_time.py --mode plain --ss 2 --lib /path/to/parent/libsr.so
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

# what --mode plain calls (the Renderer's set-up and sr_render)
PLAIN_SYMBOLS = ("sr_create", "sr_destroy", "sr_set_scene", "sr_set_background", "sr_set_texture_array", "sr_render",
                 "sr_diag_counters", "sr_version")


def load_plain(abi, path):
    """A library that may lack the supersampling entry points: only the
    symbols the plain leg calls get their signatures."""
    lib = C.CDLL(str(path), mode=C.RTLD_LOCAL)
    for name in PLAIN_SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = abi.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["ss", "plain", "resolve"], default="ss")
    ap.add_argument("--ss", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    ap.add_argument("--lib", default=None, help="another libsr.so (--mode plain: may predate supersampling)")
    args = ap.parse_args()
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    W, H, ss = args.width, args.height, args.ss
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    r = None
    if args.mode == "resolve":
        lib = abi.load(args.lib)
        g = torch.Generator(device=dev).manual_seed(1)
        samples = torch.randint(0, 256, (ss * H, ss * W, 4), dtype=torch.uint8, device=dev, generator=g)
        out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
        st = C.c_void_p(stream.cuda_stream)

        def frame():
            abi.check(lib.sr_resolve_box(C.c_void_p(samples.data_ptr()), 4 * ss * W, 0, W, H, ss,
                                         C.c_void_p(out.data_ptr()), 4 * W, 0, 1, 1, st), "sr_resolve_box")
    else:
        lib = None if args.lib is None else (load_plain(abi, args.lib) if args.mode == "plain" else abi.load(args.lib))
        r = pkg.Renderer(0, lib=lib)
        r.set_scene(sc.scene_default(textured=True))
        if args.textures == "assets":
            r.set_background(pkg.assets.skybox("2k"))
            arr, _, _ = pkg.assets.texture_array()
        else:
            r.set_background(sc.skybox(2048, 1024))
            arr, _, _ = sc.default_texture_array()
        r.set_texture_array(arr)
        cam = abi.default_camera()
        params = abi.default_params(max_steps=args.steps, percent_black=-1.0)
        if args.mode == "ss":
            out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)

            def frame():
                r.render_ss(cam, params, W, H, ss, out=out, stream=stream)
        else:
            out = torch.empty((ss * H, ss * W, 4), dtype=torch.uint8, device=dev)

            def frame():
                r.render(cam, params, ss * W, ss * H, out=out, stream=stream)
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        frame()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.frames + 1)]
    ev[0].record(stream)
    for i in range(args.frames):
        frame()
        ev[i + 1].record(stream)
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.frames))
    res = {
        "tool": "ssaa_time", "mode": args.mode, "ss": ss, "width": W, "height": H, "steps": args.steps,
        "frames": args.frames, "warmup": args.warmup, "textures": args.textures,
        "lib": str(args.lib) if args.lib else "in-tree",
        "ms_mean": ev[0].elapsed_time(ev[-1]) / args.frames, "ms_median": ms[len(ms) // 2], "ms_min": ms[0],
        "ms_max": ms[-1],
        "scratch_bytes_per_frame": 4 * ss * ss * W * H if args.mode == "ss" and ss > 1 else 0,
        "resolve_bytes": (4 * ss * ss + 4) * W * H if args.mode != "plain" and ss > 1 else 0,
    }
    if r is not None:
        res["diag"] = r.diag_counters()
        r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
