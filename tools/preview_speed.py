"""What a perturbed preview frame costs: the 800 x 800 bench scene through `DeviceLoop.render` unperturbed and with a perturbed first
march (`noises`, a fixed vector per subject so that every run takes the same samples), and the finishing passes alone --
`sdn_render_finish` (the loop's own), `sdn_preview_finish` at downscale 1 (with and without the running mean) and at downscale 0.5
(400 x 400 rays blown up to the 800 x 800 window) -- on the accumulators a frame leaves behind.

ms per frame / us per launch from device events around --frames calls, the subjects taking turns within every repeat, after warm-up;
medians of --repeats runs.  Also the sample counts of both frames (the perturbed one should march about as many).
Prints one JSON line; --out also writes it to a file (profiles/preview_speed.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seald-nerf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8, help="frames per timed run")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preview_speed.py needs a GPU")
    import sdn_backend as B
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.fused import FusedField
    from dnerf_amd.renderer import DeviceLoop

    S = args.size
    sc = build_scene(H=S, W=S, device="cuda", seed=0, time=0.5)
    half = build_scene(H=S // 2, W=S // 2, device="cuda", seed=0, time=0.5)
    N = sc.rays_o.shape[0]
    field = FusedField(sc.model, sc.time)
    loop, loop_p = DeviceLoop(sc.model, field, N, "cuda"), DeviceLoop(sc.model, field, N, "cuda")
    loop_h = DeviceLoop(sc.model, field, half.rays_o.shape[0], "cuda")
    z = torch.rand(N, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    zh = torch.rand(half.rays_o.shape[0], device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    plain = loop.render(sc.rays_o, sc.rays_d, sc.time)
    pert = loop_p.render(sc.rays_o, sc.rays_d, sc.time, noises=z)
    loop_h.render(half.rays_o, half.rays_d, sc.time, noises=zh)
    torch.cuda.synchronize()
    image, depth = torch.empty(S, S, 3, device="cuda"), torch.empty(S, S, device="cuda")
    accum = torch.zeros(S, S, 3, device="cuda")
    bg = (ctypes.c_float * 3)(1, 1, 1)

    def finish(lp, rS, acc, spp, srgb=0):
        B.check(B.lib.sdn_preview_finish(ctypes.byref(lp.ctx), rS, rS, S, S, bg, None, 1, srgb, B.ptr(image), B.ptr(depth), None, B.ptr(acc), spp,
                                         B.stream()), "preview_finish")

    frames = {
        "device_loop_unperturbed": lambda: loop.render(sc.rays_o, sc.rays_d, sc.time, want_stats=False),
        "device_loop_perturbed": lambda: loop_p.render(sc.rays_o, sc.rays_d, sc.time, want_stats=False, noises=z),
        "device_loop_perturbed_no_finish": lambda: loop_p.render(sc.rays_o, sc.rays_d, sc.time, want_stats=False, noises=z, finish=False),
    }
    passes = {
        "render_finish": lambda: B.check(B.lib.sdn_render_finish(ctypes.byref(loop_p.ctx), 1.0, B.ptr(loop_p.image_out), B.ptr(loop_p.depth_out), B.stream()),
                                         "render_finish"),
        "preview_finish_downscale_1": lambda: finish(loop_p, S, None, 0),
        "preview_finish_downscale_1_srgb": lambda: finish(loop_p, S, None, 0, 1),
        "preview_finish_downscale_1_running_mean": lambda: finish(loop_p, S, accum, 3),
        "preview_finish_downscale_0.5": lambda: finish(loop_h, S // 2, None, 0),
        "preview_finish_downscale_0.5_running_mean": lambda: finish(loop_h, S // 2, accum, 3),
    }

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    out = {"metric": f"preview frame, {S} x {S} bench scene, -O device loop", "device": torch.cuda.get_device_name(0),
           "command": "python tools/preview_speed.py --out profiles/preview_speed.json", "repeats": args.repeats, "frames_per_run": args.frames,
           "samples_unperturbed": plain["n_samples"], "samples_perturbed": pert["n_samples"],
           "iterations_unperturbed": len(plain["trace"]), "iterations_perturbed": len(pert["trace"])}
    for _ in range(args.warmup):
        for fn in list(frames.values()) + list(passes.values()):
            fn()
    ms = {k: [] for k in frames}
    us = {k: [] for k in passes}
    for _ in range(args.repeats):
        for k, fn in frames.items():
            ms[k].append(timed(fn, args.frames))
        for k, fn in passes.items():
            us[k].append(1e3 * timed(fn, 50))          # back-to-back launches: the pass's device time, not a launch's latency
    for k, v in ms.items():
        out[k] = {"ms_per_frame_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "runs": [round(x, 4) for x in v]}
    for k, v in us.items():
        out[k] = {"us_per_launch_median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    out["perturbed_over_unperturbed"] = round(out["device_loop_perturbed"]["ms_per_frame_median"] / out["device_loop_unperturbed"]["ms_per_frame_median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
