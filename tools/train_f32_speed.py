"""The fp32 training step (the reference without `-O`): the native step (`NativeTrainStep` with a disabled GradScaler ->
sdn_train_step_f32) against the eager fp32 step (op-by-op render, autograd, disabled GradScaler, torch Adam) on the workload of
`bench.py --mode train --fp32`: 4096 rays of the bench scene's 800 x 800 camera, perturbed starts, the budget of two first steps.

The two run in one process, alternating: each repeat times `--steps` steps of one, then of the other, with device events around them
after warm-up, growing the step count until a repeat holds at least 0.25 s of timed work.  Prints one JSON line with the medians."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seald-nerf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_f32_speed.py needs a GPU")
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.train_native import NativeTrainStep
    dev = torch.device("cuda", 0)
    sc = build_scene(H=800, W=800, device=dev, seed=0)
    model = sc.model
    model.train()
    n_rays = 4096
    idx = torch.randint(0, sc.rays_o.shape[0], (n_rays,), generator=torch.Generator(device="cpu").manual_seed(0)).to(dev)
    rays_o, rays_d = sc.rays_o[idx][None].contiguous(), sc.rays_d[idx][None].contiguous()
    target = torch.rand(1, n_rays, 3, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)
    opt = torch.optim.Adam(model.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", enabled=False)

    def eager_step():
        opt.zero_grad(set_to_none=True)
        out = model.render(rays_o, rays_d, sc.time, staged=False, perturb=True, bg_color=1, force_all_rays=False, max_steps=1024)
        loss = ((out["image"] - target) ** 2).mean()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return loss

    torch.manual_seed(1)
    for _ in range(2):      # first steps: unknown budget, as bench.py
        eager_step()
    model.mean_count = int(model.step_counter[:2, 0].sum().item() / 2)
    n_model = copy.deepcopy(model)
    n_opt = torch.optim.Adam(n_model.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    n_opt.load_state_dict(opt.state_dict())
    nstep = NativeTrainStep(n_model, n_opt, torch.amp.GradScaler("cuda", enabled=False), n_rays, dev, perturb=True, bg_color=1)
    nstep.load(rays_o, rays_d, target, sc.time)

    def native_step():
        return nstep()

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / 1e3

    for _ in range(args.warmup):
        eager_step()
        native_step()
    n = {}
    for name, fn in (("eager", eager_step), ("native", native_step)):
        k = 4
        while timed(fn, k) < args.min_seconds:
            k *= 2
        n[name] = k
    ms = {"eager": [], "native": []}
    for _ in range(args.repeats):
        for name, fn in (("eager", eager_step), ("native", native_step)):
            ms[name].append(timed(fn, n[name]) / n[name] * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    n_points = int(n_model.step_counter[(n_model.local_step - 1) % 16, 0].item())
    print(json.dumps({"metric": "fp32 training step, 4096 rays (bench.py --mode train --fp32 workload)", "native_ms": round(med["native"], 4),
                      "eager_ms": round(med["eager"], 4), "speedup": round(med["eager"] / med["native"], 2), "samples": n_points,
                      "steps_per_repeat": n, "repeats": args.repeats, "native_ms_all": [round(x, 4) for x in ms["native"]],
                      "eager_ms_all": [round(x, 4) for x in ms["eager"]], "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
