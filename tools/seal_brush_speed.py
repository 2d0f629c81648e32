"""The brush seal mapper's cost in a frame: the 800 x 800 bench scene with a curve stroke on the figure's torso, the cells of its
`force_fill_bound` marked occupied for every subject.

Frames (ms per frame, device events around a number of frames, the subjects taking turns within every repeat, after warm-up):
  * `device_loop_plain`   DeviceLoop without a mapper
  * `device_loop_brush`   DeviceLoop with the brush kernel (sdn_seal_brush_map)
  * `host_loop_brush`     the host-stepped loop (render_frame, fused -O field) with the brush kernel
  * `host_loop_restated`  the same loop with `SealBrushMapper._map_to_origin_torch` on the same device -- the native DeviceLoop has no
                          hook for torch code, so the restatement is compared where both forms can run
Iterations: the sample buffers of every iteration of one host-stepped frame are kept, and the kernel (on a scratch copy; the copy is
timed alone and subtracted) and the restatement are timed on each: `kernel_us` / `restated_us` per iteration, and their sums per frame.
Prints one JSON line; --out also writes it to a file (profiles/seal_brush_speed.json)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seald-nerf_amd"))


def curve_stroke(center, normal, length=0.3, sway=0.05, width=0.08, count=48):
    """48 points drawn densely along a swaying path on the plane through `center`, zig-zagging over the brush's width."""
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    u = np.cross(n, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    k = np.arange(count)
    s = (k / (count - 1) - 0.5) * length
    w = sway * np.sin(2.0 * np.pi * s / length) + np.where(k % 2 == 0, 0.5, -0.5) * width
    return (np.asarray(center, np.float64) + s[:, None] * v + w[:, None] * u + (0.003 * np.sin(0.7 * k))[:, None] * n).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8, help="frames per timed run")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seal_brush_speed.py needs a GPU")
    from dnerf_amd import seal_mapper as SM
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.fused import FusedField
    from dnerf_amd.renderer import DeviceLoop, render_frame

    sc = build_scene(H=args.size, W=args.size, device="cuda", seed=0, time=0.5)
    normal = np.array([-0.8660254037844386, 0.0, 0.5])               # the torso capsule's outward normal at azimuth 300 degrees
    cfg = dict(type="brush", normal=normal.tolist(), brushType="curve", simplifyVoxel=16, brushDepth=0.5, brushPressure=0.12, attenuationDistance=0.05,
               attenuationMode="linear", hsv=[0.33, 0.0, 0.0], raw=curve_stroke(np.array([0.0, 0.08, 0.0]) + 0.11 * normal, normal))
    mapper = SM.SealBrushMapper(cfg)

    class Restated(SM.SealBrushMapper):            # the same mapper, never taking the kernel
        def _native_ok(self, points, dirs):
            return False

    restated = Restated(cfg)
    cells = SM.fill_bitfield(sc.model.density_bitfield, mapper.map_data["force_fill_bound"])
    N = sc.rays_o.shape[0]
    field = FusedField(sc.model, sc.time)
    plain_loop = DeviceLoop(sc.model, field, N, "cuda")
    brush_loop = DeviceLoop(sc.model, field, N, "cuda", mapper=mapper)
    subjects = {
        "device_loop_plain": lambda: plain_loop.render(sc.rays_o, sc.rays_d, sc.time),
        "device_loop_brush": lambda: brush_loop.render(sc.rays_o, sc.rays_d, sc.time),
        "host_loop_brush": lambda: render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=True, field=field, mapper=mapper),
        "host_loop_restated": lambda: render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=True, field=field, mapper=restated),
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

    a = subjects["device_loop_brush"]()["image"].clone()
    b = subjects["host_loop_brush"]()["image"].clone()
    c = subjects["host_loop_restated"]()["image"].clone()
    p = subjects["device_loop_plain"]()["image"].clone()
    torch.cuda.synchronize()
    out = {"metric": f"brush seal mapper, {args.size} x {args.size} bench scene, curve stroke", "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "frames_per_run": args.frames, "triangles": int(mapper.map_triangles.shape[0]),
           "border_points": int(mapper.map_data["border_points"].shape[0]), "cells_filled": int(cells),
           "pixels_changed_by_the_edit": int(((a - p).abs().amax(1) > 1e-3).sum()), "device_loop_equals_host_loop": bool(torch.equal(a, b)),
           "kernel_vs_restated_image_max_abs": float((b - c).abs().max())}
    for _ in range(args.warmup):
        for fn in subjects.values():
            fn()
    ms = {k: [] for k in subjects}
    for _ in range(args.repeats):
        for k, fn in subjects.items():
            ms[k].append(timed(fn, args.frames))
    for k, v in ms.items():
        out[k] = {"ms_per_frame_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "runs": [round(x, 4) for x in v]}
    out["brush_cost_ms_per_frame_device_loop"] = round(out["device_loop_brush"]["ms_per_frame_median"] - out["device_loop_plain"]["ms_per_frame_median"], 4)

    # ---- the map alone, on the sample buffers of every iteration of one frame ----
    kept = []
    inner = mapper.map_to_origin_

    def keeping(points, dirs):
        kept.append(points.clone())
        return inner(points, dirs)

    mapper.map_to_origin_ = keeping
    subjects["host_loop_brush"]()
    torch.cuda.synchronize()
    mapper.map_to_origin_ = inner
    rows, reps = [], 20
    for src in kept:
        work, dirs = src.clone(), torch.zeros_like(src)
        mapped = int(mapper.map_to_origin_(work, dirs).sum())

        def kernel():
            work.copy_(src)
            mapper.map_to_origin_(work, dirs)

        for fn in (kernel, lambda: work.copy_(src), lambda: restated._map_to_origin_torch(src, dirs)):
            fn()
        k_us = [1e3 * (timed(kernel, reps) - timed(lambda: work.copy_(src), reps)) for _ in range(args.repeats)]
        r_us = [1e3 * timed(lambda: restated._map_to_origin_torch(src, dirs), 3) for _ in range(args.repeats)]
        rows.append({"slots": int(src.shape[0]), "mapped": mapped, "kernel_us": round(statistics.median(k_us), 2), "kernel_us_min_max": [round(min(k_us), 2), round(max(k_us), 2)],
                     "restated_us": round(statistics.median(r_us), 1), "restated_us_min_max": [round(min(r_us), 1), round(max(r_us), 1)]})
    out["iterations"] = rows
    out["kernel_us_per_frame"] = round(sum(r["kernel_us"] for r in rows), 1)
    out["restated_us_per_frame"] = round(sum(r["restated_us"] for r in rows), 1)
    out["kernel_us_per_iteration_mean"] = round(out["kernel_us_per_frame"] / max(len(rows), 1), 2)
    out["restated_over_kernel"] = round(out["restated_us_per_frame"] / max(out["kernel_us_per_frame"], 1e-9), 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
