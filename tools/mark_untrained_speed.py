"""NeRFRenderer.mark_untrained_grid at the model's real size (64 slices x 2 cascades x 128^3, bound 2): the native pass
(sdn_mark_untrained_grid) against the torch restatement on the same device (`_untrained_cells` + the masked store: the reference's
algorithm, dnerf/renderer.py:389-451), for the test fixture's three narrow cameras and for a D-NeRF-sized set of 150 cameras of the
bench scene's field of view on a sphere around the origin.

The two run in one process, alternating: each repeat times a number of calls of one, then of the other, with device events around
them after warm-up, growing the count until a repeat holds at least 0.25 s of timed work.  Which cells are unseen does not depend on
what the grid holds, so every call stores the same cells and the grid needs no reset in between.  Achieved store bandwidth = unseen
cells x 64 slices x 4 B / native time.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seald-nerf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mark_untrained_speed.py needs a GPU")
    from dnerf_amd.renderer import NeRFRenderer
    from dnerf_amd.scene import intrinsics, look_at_pose as look_at
    dev = torch.device("cuda", 0)
    model = NeRFRenderer(bound=2, cuda_ray=True).to(dev)
    grid = model.density_grid
    rng = np.random.default_rng(0)
    sets = {"fixture_3_poses": (np.stack([look_at(30.0, 30.0, 1.4), look_at(150.0, 10.0, 1.6), look_at(260.0, 50.0, 1.8)]), (220.0, 220.0, 50.0, 50.0)),
            "dnerf_150_poses": (np.stack([look_at(rng.uniform(0, 360), rng.uniform(0, 80), 4.0) for _ in range(150)]), tuple(intrinsics(800, 800)))}

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / 1e3

    out = {"metric": "mark_untrained_grid, 64 x 2 x 128^3 (bound 2)", "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    for name, (poses, intr) in sets.items():
        poses = torch.from_numpy(poses).to(dev)

        def native():
            model.mark_untrained_grid(poses, intr)

        def restated():
            unseen = model._untrained_cells(poses, intr, 64)
            grid[unseen.unsqueeze(0).expand_as(grid)] = -1

        grid.zero_()
        restated()
        want = grid == -1
        grid.zero_()
        native()
        unseen = model.untrained_cells.cpu().tolist()
        differ = int(((grid == -1) != want).sum())          # borderline cells only: a handful
        fns = {"native": native, "restated": restated}
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        n = {}
        for k, fn in fns.items():
            c = 1
            while timed(fn, c) < args.min_seconds:
                c *= 2
            n[k] = c
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                ms[k].append(timed(fn, n[k]) / n[k] * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        native_ms, restated_ms = med["native"], med["restated"]
        stored = sum(unseen) * grid.shape[0] * 4
        out[name] = {"poses": int(poses.shape[0]), "unseen_cells": unseen, "cells_differing_from_restatement": differ,
                     "native_ms": round(native_ms, 4), "restated_ms": round(restated_ms, 3), "speedup": round(restated_ms / native_ms, 1),
                     "stored_bytes": stored, "store_GBps": round(stored / native_ms / 1e6, 1),
                     "calls_per_repeat": n, "native_ms_all": [round(x, 4) for x in ms["native"]],
                     "restated_ms_all": [round(x, 3) for x in ms["restated"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
