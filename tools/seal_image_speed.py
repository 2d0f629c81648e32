"""The brush's texture stamp (`imageConfig`, sdn_seal_modify_image) in a frame: the 800 x 800 bench scene with the curve stroke of
tools/seal_brush_speed.py on the figure's torso and a procedural 256 x 256 RGBA stamp over it, the cells of `force_fill_bound` marked
occupied for every subject.

Frames (ms per frame, device events around a number of frames, the subjects taking turns within every repeat, after warm-up; medians
of --repeats runs):
  * `device_loop_brush`        DeviceLoop with the brush alone
  * `device_loop_brush_stamp`  DeviceLoop with the brush and the stamp
  * `host_loop_stamp`          the host-stepped loop (render_frame, fused -O field) with the kernels
  * `host_loop_restated`       the same loop with the brush kernel but the torch restatement of map_color on the same device -- the
                               native DeviceLoop has no hook for torch code, so the restatement is compared where both forms can run
Iterations: the colour / position / mask buffers of every iteration of one host-stepped frame are kept, and the stamp's three stream
operations (on a scratch copy of the colours; the copy is timed alone and subtracted) and the restatement are timed on each.
Prints one JSON line; --out also writes it to a file (profiles/seal_image_speed.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seald-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stamp_texture(size=256):
    """A procedural RGBA stamp: colour gradients, a transparent margin, a soft edge, an opaque centre."""
    y, x = np.mgrid[0:size, 0:size]
    rgb = np.stack([(x * 255) // (size - 1), (y * 255) // (size - 1), ((x + y) * 37) % 256], -1)
    edge = np.minimum(np.minimum(x, size - 1 - x), np.minimum(y, size - 1 - y))
    alpha = np.clip((edge - size // 8) * 255 // (size // 8), 0, 255)
    return np.concatenate([rgb, alpha[..., None]], -1).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8, help="frames per timed run")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seal_image_speed.py needs a GPU")
    from PIL import Image
    from seal_brush_speed import curve_stroke
    from dnerf_amd import seal_mapper as SM
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.fused import FusedField
    from dnerf_amd.renderer import DeviceLoop, render_frame

    sc = build_scene(H=args.size, W=args.size, device="cuda", seed=0, time=0.5)
    normal = np.array([-0.8660254037844386, 0.0, 0.5])               # the torso capsule's outward normal at azimuth 300 degrees
    centre = np.array([0.0, 0.08, 0.0]) + 0.11 * normal
    u = np.cross(normal, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(normal, u)
    o = centre - 0.07 * u - 0.13 * v                                   # a 0.14 x 0.26 rectangle inside the stroke's 0.18 x 0.3
    brush = dict(type="brush", normal=normal.tolist(), brushType="curve", simplifyVoxel=16, brushDepth=0.5, brushPressure=0.12, attenuationDistance=0.05,
                 attenuationMode="linear", raw=curve_stroke(centre, normal))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "stamp.png")
        Image.fromarray(stamp_texture(), "RGBA").save(path)
        cfg = dict(brush, rgbLightOffset=0.05, imageConfig=dict(path=path, o=o.tolist(), w=(o + 0.14 * u).tolist(), h=(o + 0.26 * v).tolist()))
        plain, mapper = SM.SealBrushMapper(brush), SM.SealBrushMapper(cfg)

        class Restated(SM.SealBrushMapper):        # the same mapper; its colours never take the kernels
            def map_color_(self, rgbs, mask, whole_rays=None, points=None):
                if bool(mask.any()):
                    rgbs[mask] = self.map_color(points[mask], None, rgbs[mask]).to(rgbs.dtype)
                return rgbs

        restated = Restated(cfg)
    cells = SM.fill_bitfield(sc.model.density_bitfield, mapper.map_data["force_fill_bound"])
    N = sc.rays_o.shape[0]
    field = FusedField(sc.model, sc.time)
    brush_loop = DeviceLoop(sc.model, field, N, "cuda", mapper=plain)
    stamp_loop = DeviceLoop(sc.model, field, N, "cuda", mapper=mapper)
    subjects = {
        "device_loop_brush": lambda: brush_loop.render(sc.rays_o, sc.rays_d, sc.time),
        "device_loop_brush_stamp": lambda: stamp_loop.render(sc.rays_o, sc.rays_d, sc.time),
        "host_loop_stamp": lambda: render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=True, field=field, mapper=mapper),
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

    a = subjects["device_loop_brush_stamp"]()["image"].clone()
    b = subjects["host_loop_stamp"]()["image"].clone()
    c = subjects["host_loop_restated"]()["image"].clone()
    p = subjects["device_loop_brush"]()["image"].clone()
    torch.cuda.synchronize()
    out = {"metric": f"brush texture stamp, {args.size} x {args.size} bench scene, curve stroke, 256 x 256 RGBA stamp", "device": torch.cuda.get_device_name(0),
           "command": "python tools/seal_image_speed.py --out profiles/seal_image_speed.json",
           "repeats": args.repeats, "frames_per_run": args.frames, "triangles": int(mapper.map_triangles.shape[0]), "cells_filled": int(cells),
           "pixels_changed_by_the_stamp": int(((a - p).abs().amax(1) > 1e-3).sum()), "device_loop_equals_host_loop": bool(torch.equal(a, b)),
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
    out["stamp_cost_ms_per_frame_device_loop"] = round(out["device_loop_brush_stamp"]["ms_per_frame_median"] - out["device_loop_brush"]["ms_per_frame_median"], 4)

    # ---- the stamp alone, on the buffers of every iteration of one frame ----
    kept = []
    inner = mapper.map_color_

    def keeping(rgbs, mask, whole_rays=None, points=None):
        kept.append((rgbs.clone(), mask.clone(), points.clone()))
        return inner(rgbs, mask, whole_rays=whole_rays, points=points)

    mapper.map_color_ = keeping
    subjects["host_loop_stamp"]()
    torch.cuda.synchronize()
    mapper.map_color_ = inner
    rows, reps = [], 20
    for src, mask, pts in kept:
        work = src.clone()

        def kernel():
            work.copy_(src)
            inner(work, mask, points=pts)

        def torch_form():
            work.copy_(src)
            Restated.map_color_(restated, work, mask, points=pts)

        for fn in (kernel, torch_form, lambda: work.copy_(src)):
            fn()
        k_us = [1e3 * (timed(kernel, reps) - timed(lambda: work.copy_(src), reps)) for _ in range(args.repeats)]
        r_us = [1e3 * (timed(torch_form, 3) - timed(lambda: work.copy_(src), 3)) for _ in range(args.repeats)]
        rows.append({"slots": int(src.shape[0]), "masked": int(mask.sum()), "kernel_us": round(statistics.median(k_us), 2),
                     "kernel_us_min_max": [round(min(k_us), 2), round(max(k_us), 2)], "restated_us": round(statistics.median(r_us), 1),
                     "restated_us_min_max": [round(min(r_us), 1), round(max(r_us), 1)]})
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
