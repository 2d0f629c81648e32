"""What a frame of the temporal-basis model costs natively: the 800 x 800 bench scene (dnerf_amd.bench_scene.build_basis_scene) through
`DeviceLoop.render` with `FusedBasisField`, through the mirror's reference-shaped `run_cuda` op by op under autocast (the path such a
model had before the fused field), and -- for scale -- the deformation model's frame through `DeviceLoop.render` with `FusedField`;
plus the basis field launch alone on the samples of one frame's first iterations.

ms per frame from device events around --frames calls, the subjects taking turns within every repeat in one process, after warm-up;
medians of --repeats runs.  The two models are different scenes in the sense that matters for time: the same occupancy and camera, but
their own densities, so their frames differ in samples and iterations -- both are reported next to the times.
Prints one JSON line; --out also writes it to a file (profiles/basis_field_speed.json)."""
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
        raise SystemExit("basis_field_speed.py needs a GPU")
    from dnerf_amd.bench_scene import build_basis_scene, build_scene
    from dnerf_amd.fused import FusedField
    from dnerf_amd.fused_basis import FusedBasisField
    from dnerf_amd.renderer import DeviceLoop

    S = args.size
    sb = build_basis_scene(H=S, W=S, device="cuda", seed=0, time=0.5)
    sd = build_scene(H=S, W=S, device="cuda", seed=0, time=0.5)
    N = sb.rays_o.shape[0]
    fb, fd = FusedBasisField(sb.model, sb.time), FusedField(sd.model, sd.time)
    lb, ld = DeviceLoop(sb.model, fb, N, "cuda"), DeviceLoop(sd.model, fd, N, "cuda")
    first_b, first_d = lb.render(sb.rays_o, sb.rays_d, sb.time), ld.render(sd.rays_o, sd.rays_d, sd.time)
    sb.model.fused_inference = False      # the op-by-op subject: every launch of the reference-shaped loop is an existing operator

    def op_by_op():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return sb.model.render(sb.rays_o[None], sb.rays_d[None], sb.time, staged=False, perturb=False, bg_color=1)

    ref = op_by_op()
    torch.cuda.synchronize()
    diff = float((ref["image"][0].float() - first_b["image"]).abs().max())
    frames = {
        "basis_device_loop": lambda: lb.render(sb.rays_o, sb.rays_d, sb.time, want_stats=False),
        "basis_run_cuda_op_by_op": op_by_op,
        "deform_device_loop": lambda: ld.render(sd.rays_o, sd.rays_d, sd.time, want_stats=False),
    }
    # the field launch alone: the sample positions one frame's loop left in its buffers, every slot evaluated
    M = min(int(first_b["n_samples"]), lb.buf["xyzs"].shape[0])
    xs, ds = lb.buf["xyzs"][:M].clone(), lb.buf["dirs"][:M].clone()
    fb._alloc(M)

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    out = {"metric": f"temporal-basis frame, {S} x {S} bench scene, -O", "device": torch.cuda.get_device_name(0),
           "command": "python tools/basis_field_speed.py --out profiles/basis_field_speed.json", "repeats": args.repeats, "frames_per_run": args.frames,
           "samples_basis": first_b["n_samples"], "iterations_basis": len(first_b["trace"]), "samples_deform": first_d["n_samples"],
           "iterations_deform": len(first_d["trace"]), "max_abs_image_diff_native_vs_op_by_op": diff, "field_launch_points": M}
    for _ in range(args.warmup):
        for fn in frames.values():
            fn()
    ms = {k: [] for k in frames}
    us = []
    for _ in range(args.repeats):
        for k, fn in frames.items():
            ms[k].append(timed(fn, args.frames))
        us.append(1e3 * timed(lambda: fb(xs, ds), 50))      # back-to-back launches: the launch's device time, not its latency
    for k, v in ms.items():
        out[k] = {"ms_per_frame_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "runs": [round(x, 4) for x in v]}
    out["basis_field_launch"] = {"us_per_launch_median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2),
                                 "ns_per_point": round(statistics.median(us) * 1e3 / M, 4)}
    out["native_over_op_by_op"] = round(out["basis_device_loop"]["ms_per_frame_median"] / out["basis_run_cuda_op_by_op"]["ms_per_frame_median"], 4)
    out["basis_over_deform"] = round(out["basis_device_loop"]["ms_per_frame_median"] / out["deform_device_loop"]["ms_per_frame_median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
