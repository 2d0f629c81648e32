"""What a temporal-basis model trained WITHOUT -O costs natively: the 800 x 800 bench scene (dnerf_amd.bench_scene.build_basis_scene,
fp32 weights) through `DeviceLoop.render` with `FusedBasisFieldF32`, against the mirror's reference-shaped `run_cuda` op by op without
autocast (the only path such a model had before the fp32 field); the field launch alone on one frame's sample slots; and one full
density update through the field's CELLS kernel against the op-by-op fp32 `update_extra_state`.

ms from device events around --frames calls (one call for an update), the subjects taking turns within every repeat in one process,
after warm-up; medians of --repeats runs with min / max as the spread of each subject.
Prints one JSON line; --out also writes it to a file (profiles/basis_f32_speed.json)."""
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
        raise SystemExit("basis_f32_speed.py needs a GPU")
    from dnerf_amd.bench_scene import build_basis_scene
    from dnerf_amd.fused_basis import FusedBasisFieldF32
    from dnerf_amd.renderer import DeviceLoop

    S = args.size
    sc = build_basis_scene(H=S, W=S, device="cuda", seed=0, time=0.5)
    model = sc.model
    assert model.encoder.embeddings.dtype == torch.float32
    N = sc.rays_o.shape[0]
    field = FusedBasisFieldF32(model, sc.time)
    loop = DeviceLoop(model, field, N, "cuda")
    first = loop.render(sc.rays_o, sc.rays_d, sc.time)

    def op_by_op():
        with torch.no_grad():
            return model.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=False, bg_color=1)

    ref = op_by_op()
    torch.cuda.synchronize()
    diff = float((ref["image"][0].float() - first["image"]).abs().max())
    frames = {"device_loop_fp32_field": lambda: loop.render(sc.rays_o, sc.rays_d, sc.time, want_stats=False), "run_cuda_op_by_op_fp32": op_by_op}
    # the field launch alone: the sample positions one frame's loop left in its buffers, every slot evaluated
    M = min(int(first["n_samples"]), loop.buf["xyzs"].shape[0])
    xs, ds = loop.buf["xyzs"][:M].clone(), loop.buf["dirs"][:M].clone()
    field._alloc(M)

    # the density update: full passes (iter_density < 16) on a copy of the grid's state, restored after the measurement
    keep = (model.density_grid.clone(), model.density_bitfield.clone(), model.iter_density, model.mean_density)

    def restore():      # (the frames of the next repeat march the scene's own occupancy)
        model.density_grid.copy_(keep[0])
        model.density_bitfield.copy_(keep[1])
        torch.autograd.graph.increment_version((model.density_bitfield, model.density_grid))
        model.iter_density, model.mean_density = keep[2], keep[3]
    from dnerf_amd.fused import DensityGridUpdater
    up = DensityGridUpdater(model, field=field)

    def native_update():
        model.iter_density = 0
        up.update(0.95)

    def op_by_op_update():
        model.iter_density = 0
        model.update_extra_state()

    updates = {"update_native_fp32_field": native_update, "update_extra_state_op_by_op_fp32": op_by_op_update}

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    out = {"metric": f"temporal-basis model without -O, {S} x {S} bench scene, fp32", "device": torch.cuda.get_device_name(0),
           "command": "python tools/basis_f32_speed.py --out profiles/basis_f32_speed.json", "repeats": args.repeats, "frames_per_run": args.frames,
           "samples": first["n_samples"], "iterations": len(first["trace"]), "max_abs_image_diff_native_vs_op_by_op": diff, "field_launch_points": M,
           "workgroup": "4 waves, 32 points per wave, 60 KiB of weights + 8 KiB of basis rows in LDS: two workgroups per CU"}
    for _ in range(args.warmup):
        for fn in frames.values():
            fn()
    for fn in updates.values():
        fn()
    restore()
    ms = {k: [] for k in list(frames) + list(updates)}
    us = []
    for _ in range(args.repeats):
        for k, fn in frames.items():
            ms[k].append(timed(fn, args.frames))
        us.append(1e3 * timed(lambda: field(xs, ds), 50))      # back-to-back launches: the launch's device time, not its latency
        for k, fn in updates.items():
            ms[k].append(timed(fn, 1))
        restore()

    def spread(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                "spread_over_median": round((max(v) - min(v)) / statistics.median(v), 4), "runs": [round(x, 4) for x in v]}

    for k in frames:
        out[k] = {"unit": "ms per frame", **spread(ms[k])}
    for k in updates:
        out[k] = {"unit": "ms per full update (64 slices x 128^3 cells)", **spread(ms[k])}
    out["field_launch"] = {"unit": "us per launch", **spread(us), "ns_per_point": round(statistics.median(us) * 1e3 / M, 4)}
    out["frame_native_over_op_by_op"] = round(out["device_loop_fp32_field"]["median"] / out["run_cuda_op_by_op_fp32"]["median"], 4)
    out["update_native_over_op_by_op"] = round(out["update_native_fp32_field"]["median"] / out["update_extra_state_op_by_op_fp32"]["median"], 4)
    out["not_measured"] = ["what bounds the field launch (gather-address rate, vector issue or the matrix pipe): no counters were collected",
                           "other occupancies: 8 waves per workgroup, a smaller LDS footprint (the sigma net only resident, the colour net staged), "
                           "more than two workgroups per CU", "the CELLS kernel at its LDS limit of four workgroups per CU against two",
                           "the split-operand (f32x3) form of this network"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
