"""Times the SealD teacher's proxy render (EditTrainStep.proxy_truth) of 4096 rays with an rgb-tint mapper -- through the iteration
loop (one_pass=False) and in one pass (the default) -- and the untinted one-pass render; torch events, subjects taking turns.
--root: the checkout whose package and library are measured (default: this one); a checkout from before the one-pass tint refuses
the mapper and is measured without that line.  Prints one JSON line per subject.  profiles/one_pass_tint_timing.txt."""
import argparse, json, os, statistics, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=None)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = os.path.abspath(args.root) if args.root else ROOT
for p in (BASE, os.path.join(BASE, "seald-nerf_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch
import sdn_backend
assert sdn_backend.LIB_PATH.startswith(BASE), sdn_backend.LIB_PATH
from dnerf_amd import fused, seal_mapper as SM
from dnerf_amd.bench_scene import build_scene
from dnerf_amd.network import NeRFNetwork
from dnerf_amd.renderer import RayBatchRenderer
from dnerf_amd.seald_train import EditTrainStep, freeze_deformation

N, TIME = 4096, 0.5
sc = build_scene(H=128, W=128, device="cuda", seed=0, time=TIME)
idx = torch.randperm(sc.rays_o.shape[0], generator=torch.Generator().manual_seed(5))[:N].cuda()
ro, rd = sc.rays_o[idx].contiguous(), sc.rays_d[idx].contiguous()
half, c = 0.06, (0.0, 0.08, 0.0)
raw = [[c[0] + sx * half, c[1] + sy * half, c[2] + sz * half] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]
mapper = SM.get_seal_mapper({"type": "bbox", "raw": raw, "transform": np.eye(4).tolist(), "scale": [1.0, 1.0, 1.0], "boundType": "to",
                             "rgb": [0.9, 0.3, 0.1], "rgbLightOffset": 0.05})


def edit_step(one_pass):
    student = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).to("cuda").train()
    student.load_state_dict(sc.model.state_dict())
    student.mean_count, student.local_step = 64 * N, 0
    opt = torch.optim.Adam(freeze_deformation(student), lr=2e-3, betas=(0.9, 0.99), eps=1e-15)
    return EditTrainStep(sc.model, student, mapper, opt, torch.amp.GradScaler("cuda"), N, "cuda", TIME, native=True, one_pass=one_pass, perturb=False)


subjects = {}
loop_edit = edit_step(False)
subjects["tint_loop"] = lambda: loop_edit.proxy_truth(ro, rd, TIME)
plain = RayBatchRenderer(sc.model, fused.FusedField(sc.model, TIME, fp16=True), N, "cuda", T_thresh=1e-4)
subjects["untinted_one_pass"] = lambda: plain.render(ro, rd, TIME, bg_color=1.0)["image"]
try:
    once_edit = edit_step(True)
except NotImplementedError:
    once_edit = None
if once_edit is not None:
    subjects["tint_one_pass"] = lambda: once_edit.proxy_truth(ro, rd, TIME)
    a, b = subjects["tint_loop"]().clone(), subjects["tint_one_pass"]().clone()
    torch.cuda.synchronize()
    print(json.dumps({"root": BASE, "tint images equal": bool(torch.equal(a, b)), "tinted pixels": int(((a - subjects["untinted_one_pass"]()).abs().amax(1) > 1e-3).sum())}), flush=True)

for name, fn in subjects.items():
    for _ in range(30):
        fn()
torch.cuda.synchronize()
res = {k: {"event_ms": [], "wall_ms": []} for k in subjects}
for rep in range(args.repeats):              # subjects alternate within every repeat
    for name, fn in subjects.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res[name]["wall_ms"].append(1e3 * (time.perf_counter() - t0) / args.calls)
        res[name]["event_ms"].append(e0.elapsed_time(e1) / args.calls)
for name, r in res.items():
    ev = sorted(r["event_ms"])
    print(json.dumps({"root": BASE, "subject": name, "calls": args.calls, "event_ms_median": round(statistics.median(ev), 5), "event_ms_min": round(ev[0], 5),
                      "event_ms_max": round(ev[-1], 5), "wall_ms_median": round(statistics.median(r["wall_ms"]), 5), "event_ms_runs": [round(v, 5) for v in r["event_ms"]]}), flush=True)
