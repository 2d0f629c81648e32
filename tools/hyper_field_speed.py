"""What a frame of the ambient-dimension model costs natively: the 800 x 800 bench scene (dnerf_amd.bench_scene.build_hyper_scene)
through `DeviceLoop.render` with `FusedHyperField`, and through the mirror's reference-shaped `run_cuda` op by op under autocast (the
only path such a model had before the fused field); plus the field launch alone on the samples of one frame.

ms per frame from device events around --frames calls, the subjects taking turns within every repeat in one process, after warm-up;
medians of --repeats runs.  Prints one JSON line; --out also writes it to a file (profiles/hyper_field_speed.json)."""
import argparse
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8, help="frames per timed run")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hyper_field_speed.py needs a GPU")
    from dnerf_amd.bench_scene import build_hyper_scene
    from dnerf_amd.fused_hyper import FusedHyperField
    from dnerf_amd.renderer import DeviceLoop

    S = args.size
    sc = build_hyper_scene(H=S, W=S, device="cuda", seed=0, time=0.5)
    N = sc.rays_o.shape[0]
    field = FusedHyperField(sc.model, sc.time)
    loop = DeviceLoop(sc.model, field, N, "cuda")
    first = loop.render(sc.rays_o, sc.rays_d, sc.time)
    sc.model.fused_inference = False      # the op-by-op subject: every launch of the reference-shaped loop is an existing operator

    def op_by_op():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return sc.model.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=False, bg_color=1)

    ref = op_by_op()
    torch.cuda.synchronize()
    diff = float((ref["image"][0].float() - first["image"]).abs().max())
    frames = {
        "hyper_device_loop": lambda: loop.render(sc.rays_o, sc.rays_d, sc.time, want_stats=False),
        "hyper_run_cuda_op_by_op": op_by_op,
    }
    # the field launch alone: the sample positions one frame's loop left in its buffers, every slot evaluated
    M = min(int(first["n_samples"]), loop.buf["xyzs"].shape[0])
    xs, ds = loop.buf["xyzs"][:M].clone(), loop.buf["dirs"][:M].clone()
    field._alloc(M)

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    out = {"metric": f"ambient-dimension frame, {S} x {S} bench scene, -O", "device": torch.cuda.get_device_name(0),
           "command": "python tools/hyper_field_speed.py --out profiles/hyper_field_speed.json", "repeats": args.repeats, "frames_per_run": args.frames,
           "samples": first["n_samples"], "iterations": len(first["trace"]), "ambient": float(field.bias0[0]),
           "max_abs_image_diff_native_vs_op_by_op": diff, "field_launch_points": M}
    for _ in range(args.warmup):
        for fn in frames.values():
            fn()
    ms = {k: [] for k in frames}
    us = []
    for _ in range(args.repeats):
        for k, fn in frames.items():
            ms[k].append(timed(fn, args.frames))
        us.append(1e3 * timed(lambda: field(xs, ds), 50))      # back-to-back launches: the launch's device time, not its latency
    for k, v in ms.items():
        out[k] = {"ms_per_frame_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "runs": [round(x, 4) for x in v]}
    out["hyper_field_launch"] = {"us_per_launch_median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2),
                                 "ns_per_point": round(statistics.median(us) * 1e3 / M, 4)}
    out["native_over_op_by_op"] = round(out["hyper_device_loop"]["ms_per_frame_median"] / out["hyper_run_cuda_op_by_op"]["ms_per_frame_median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
