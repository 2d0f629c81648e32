"""Error-map training on the device, at the reference's sizes (800 x 800 image, 4096 rays, 128 x 128 map):

  * the draw: `sample_error_map` (one launch, csrc/error_map.hip) against torch.multinomial without replacement plus the fine-pixel
    expressions of nerf/utils.py:105-118 on the same device;
  * the step: the native fp16 step (`NativeTrainStep`, the workload of `bench.py --mode train`) with the map's update inside its
    compositing launch against the same step without it.

Each pair runs in one process, alternating: a repeat times a number of calls of one, then of the other, with device events around
them after warm-up, growing the count until a repeat holds at least 0.25 s of timed work.

`--parent-tree DIR` (a built checkout of the commit before the update existed) adds the comparison across commits: child processes
time the plain step of DIR and of this tree in turn, `--rounds` times each, and the result holds every round's median -- the spread
of the parent's rounds is the run-to-run spread the step with the update is held against.

Writes the result to profiles/error_map_speed.json (`--out`) and prints it as one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS, H, W, S = 4096, 800, 800, 128


def timed(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3


def alternate(fns, args):
    """name -> per-call milliseconds of every repeat, the functions taking turns inside each repeat."""
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    n = {}
    for k, fn in fns.items():
        c = 4
        while timed(fn, c) < args.min_seconds:
            c *= 2
        n[k] = c
    ms = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items():
            ms[k].append(timed(fn, n[k]) / n[k] * 1e3)
    return ms, n


def build_step():
    """The workload of `bench.py --mode train`: 4096 rays of the bench scene's 800 x 800 camera, perturbed starts, the budget of two
    first steps, the fp16 native step."""
    import torch
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.train_native import NativeTrainStep
    dev = torch.device("cuda", 0)
    sc = build_scene(H=H, W=W, device=dev, seed=0)
    model = sc.model
    model.train()
    idx = torch.randint(0, sc.rays_o.shape[0], (N_RAYS,), generator=torch.Generator(device="cpu").manual_seed(0)).to(dev)
    rays_o, rays_d = sc.rays_o[idx].contiguous(), sc.rays_d[idx].contiguous()
    target = torch.rand(N_RAYS, 3, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for _ in range(2):
            model.render(rays_o[None], rays_d[None], sc.time, staged=False, perturb=True, bg_color=1, force_all_rays=False, max_steps=1024)
    model.mean_count = int(model.step_counter[:2, 0].sum().item() / 2)
    model.local_step = 0
    opt = torch.optim.Adam(model.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    step = NativeTrainStep(model, opt, torch.amp.GradScaler("cuda"), N_RAYS, dev, perturb=True, bg_color=1)
    return step, (rays_o, rays_d, target, sc.time)


def child(args):
    """The plain step of the tree on sys.path: one JSON line with the median per-step milliseconds of `--repeats` repeats."""
    step, batch = build_step()
    ms, n = alternate({"step": lambda: step(*batch)}, args)
    print(json.dumps({"step_ms": statistics.median(ms["step"]), "step_ms_all": ms["step"], "steps_per_repeat": n["step"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_map_speed.json"))
    ap.add_argument("--child-tree", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.child_tree or ROOT, "seald-nerf_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("error_map_speed.py needs a GPU")
    if args.child_tree:
        return child(args)
    from dnerf_amd.utils import sample_error_map
    dev = torch.device("cuda", 0)
    out = {"metric": f"error-map sampling and update, {H} x {W}, {N_RAYS} rays, {S} x {S} map", "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats}

    # ---- the draw ------------------------------------------------------------------------------------------------------------------------
    emap = (torch.rand(1, S * S, generator=torch.Generator().manual_seed(0)) ** 4 + 1e-6).to(dev)
    row = emap[0]

    def native_draw():
        return sample_error_map(row, N_RAYS, H, W)

    def torch_draw():      # nerf/utils.py:105-112
        inds_coarse = torch.multinomial(emap, N_RAYS, replacement=False)
        inds_x, inds_y = inds_coarse // 128, inds_coarse % 128
        sx, sy = H / 128, W / 128
        inds_x = (inds_x * sx + torch.rand(1, N_RAYS, device=dev) * sx).long().clamp(max=H - 1)
        inds_y = (inds_y * sy + torch.rand(1, N_RAYS, device=dev) * sy).long().clamp(max=W - 1)
        return inds_coarse, inds_x * W + inds_y

    ms, n = alternate({"native": native_draw, "torch": torch_draw}, args)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["draw"] = {"native_ms": round(med["native"], 5), "torch_ms": round(med["torch"], 5), "speedup": round(med["torch"] / med["native"], 1),
                   "calls_per_repeat": n, "native_ms_all": [round(x, 5) for x in ms["native"]], "torch_ms_all": [round(x, 5) for x in ms["torch"]]}

    # ---- the step with and without the update -----------------------------------------------------------------------------------------------
    step, batch = build_step()
    full_map = torch.ones(4, S * S, device=dev)
    cells, _ = sample_error_map(row, N_RAYS, H, W, seed=1)
    ms, n = alternate({"plain": lambda: step(*batch), "with_update": lambda: step(*batch, error_map=full_map, index=1, inds_coarse=cells),
                       "draw_and_update": lambda: step(*batch, error_map=full_map, index=1, inds_coarse=sample_error_map(full_map[1], N_RAYS, H, W)[0])},
                      args)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["step"] = {k + "_ms": round(v, 5) for k, v in med.items()}
    out["step"].update({"steps_per_repeat": n, **{k + "_ms_all": [round(x, 5) for x in v] for k, v in ms.items()}})

    # ---- against the commit before: child processes, taking turns ---------------------------------------------------------------------------
    if args.parent_tree:
        rounds = {"parent": [], "this": []}
        for _ in range(args.rounds):
            for name, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
                cmd = [sys.executable, os.path.abspath(__file__), "--child-tree", tree, "--repeats", str(args.repeats), "--warmup", str(args.warmup),
                       "--min-seconds", str(args.min_seconds)]
                res = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
                rounds[name].append(json.loads(res.stdout.strip().split("\n")[-1])["step_ms"])
        spread = max(rounds["parent"]) - min(rounds["parent"])
        out["against_parent"] = {"parent_plain_ms_rounds": [round(x, 5) for x in rounds["parent"]], "this_plain_ms_rounds": [round(x, 5) for x in rounds["this"]],
                                 "parent_median_ms": round(statistics.median(rounds["parent"]), 5), "parent_spread_ms": round(spread, 5),
                                 "with_update_ms": out["step"]["with_update_ms"],
                                 "with_update_within_parent_plus_spread": bool(med["with_update"] <= statistics.median(rounds["parent"]) + spread)}
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
