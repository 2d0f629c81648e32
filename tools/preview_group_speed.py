"""What accumulating a resting preview costs, one jittered frame per loop against several: the 800 x 800 bench scene through
`PreviewRenderer.accumulate` (64 loops for 64 spp) and through `PreviewRenderer.accumulate_group` with samples = 2, 4, 8 (32, 16, 8
loops), every subject replaying the same 64 noise vectors, so that all of them take the same samples and end in the same buffer.

ms per 64-spp accumulation from a host clock around the calls, ending in a device synchronise (the driver waits on the device every
iteration anyway: what a viewer waits for is wall time); the subjects take turns within every repeat, after warm-up; medians of
--repeats runs.  Also the iteration and sample counts of a group against a lone frame, and whether the buffers came out bit-identical.

--only-accumulate measures `accumulate` alone and needs nothing this feature added, so it runs on an older tree as well:
--root <checkout> imports the package from there.  --baseline <json> merges such a run (the parent commit's, taken in the same job on
the same machine) into the result.  Prints one JSON line; --out also writes it to a file (profiles/preview_group_speed.json)."""
import argparse
import json
import os
import statistics
import sys
from time import perf_counter

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--samples", default="2,4,8")
    ap.add_argument("--root", default=ROOT, help="checkout to import the package from")
    ap.add_argument("--only-accumulate", action="store_true")
    ap.add_argument("--baseline", nargs="+", default=None, help="JSON(s) of --only-accumulate runs of the parent commit; ratios use the first")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preview_group_speed.py needs a GPU")
    sys.path.insert(0, os.path.join(os.path.abspath(args.root), "seald-nerf_amd"))
    from dnerf_amd import scene
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.fused import FusedField
    from dnerf_amd.preview import PreviewRenderer

    S, spp = args.size, args.spp
    groups = [] if args.only_accumulate else [int(v) for v in args.samples.split(",")]
    sc = build_scene(H=S, W=S, device="cuda", seed=0, time=0.5)
    N = S * S
    field = FusedField(sc.model, sc.time)
    pose, intr = scene.look_at_pose(30.0, 30.0), scene.intrinsics(S, S)
    z = torch.rand(spp, N, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    pvs = {"accumulate": PreviewRenderer(sc.model, field, S, S, "cuda")}
    for F in groups:
        pvs[f"accumulate_group_{F}"] = PreviewRenderer(sc.model, field, S, S, "cuda")

    def run(key):
        pv = pvs[key]
        if key == "accumulate":
            for k in range(spp):
                pv.accumulate(pose, intr, 0.5, need_update=k == 0, max_spp=spp, noises=z[k])
        else:
            F = int(key.rsplit("_", 1)[1])
            for k in range(0, spp, F):
                rows = z[k:k + F] if k + F <= spp else torch.cat([z[k:], z[:k + F - spp]])     # the last group folds spp - k of its rows
                pv.accumulate_group(pose, intr, 0.5, need_update=k == 0, max_spp=spp, samples=F, noises=rows)
        assert pv.spp == spp

    def timed(key):
        torch.cuda.synchronize()
        t0 = perf_counter()
        run(key)
        torch.cuda.synchronize()
        return 1e3 * (perf_counter() - t0)

    out = {"metric": f"{spp} spp of a resting preview, {S} x {S} bench scene, -O device loop, wall ms per accumulation",
           "device": torch.cuda.get_device_name(0), "root": os.path.relpath(os.path.abspath(args.root), ROOT),
           "command": "python tools/preview_group_speed.py " + " ".join(sys.argv[1:]), "repeats": args.repeats, "spp": spp}
    for _ in range(args.warmup):
        for key in pvs:
            run(key)
    torch.cuda.synchronize()
    ms = {key: [] for key in pvs}
    for _ in range(args.repeats):
        for key in pvs:
            ms[key].append(timed(key))
    for key, v in ms.items():
        med = statistics.median(v)
        out[key] = {"ms_median": round(med, 3), "ms_per_sample_median": round(med / spp, 4), "min": round(min(v), 3), "max": round(max(v), 3),
                    "runs": [round(x, 3) for x in v]}
    if groups:
        base = out["accumulate"]["ms_median"]
        ref = pvs["accumulate"].render_buffer
        for F in groups:
            key = f"accumulate_group_{F}"
            out[key]["speedup_over_accumulate"] = round(base / out[key]["ms_median"], 4)
            out[key]["buffer_bit_identical_to_accumulate"] = bool(torch.equal(pvs[key].render_buffer.view(torch.int32), ref.view(torch.int32)))
        # iterations and samples: a lone jittered frame against a group (rows 0 .. F-1), through the renderers' own loops
        rays_o, rays_d = pvs["accumulate"]._refs[0], pvs["accumulate"]._refs[1]
        lone = pvs["accumulate"].loop_for(N).render(rays_o, rays_d, sc.time, noises=z[0], finish=False)
        out["lone_frame"] = {"iterations": len(lone["trace"]), "samples": lone["n_samples"]}
        for F in groups:
            g = pvs[f"accumulate_group_{F}"].group_loop_for(N, F).render_samples(rays_o, rays_d, sc.time, z[:F].contiguous())
            out[f"accumulate_group_{F}"].update(iterations=len(g["trace"]), samples_per_frame=round(g["n_samples"] / F, 1))
    if args.baseline:
        runs = []
        for path in args.baseline:
            with open(path) as f:
                runs.append(json.loads(f.readline()))
        parent = runs[0]
        out["parent_accumulate"] = parent["accumulate"]
        out["parent_accumulate_ms_median_per_run"] = [r["accumulate"]["ms_median"] for r in runs]
        for F in groups:
            key = f"accumulate_group_{F}"
            out[key]["speedup_over_parent_accumulate"] = round(parent["accumulate"]["ms_median"] / out[key]["ms_median"], 4)
        out["accumulate_over_parent_accumulate"] = round(out["accumulate"]["ms_median"] / parent["accumulate"]["ms_median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
