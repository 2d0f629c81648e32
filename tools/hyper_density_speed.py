"""What update_extra_state of the ambient-dimension model costs: the native full update (`iter_density` < 16: 64 x 128^3 cells), the native
partial update (16 <= `iter_density` < 100: 64 x 128^3 / 2 listed cells) and the mirror's op-by-op full and partial updates under fp16
autocast -- the only path such a model had before the CELLS variant of csrc/field_hyper.hip -- on the same model
(dnerf_amd.bench_scene.build_hyper_scene).

ms per update, timed on the host from a device synchronise to a device synchronise (the op-by-op pass reads back on the host; the native
one does not), the subjects taking turns within every repeat in one process, after warm-up; medians of --repeats runs with the range.
Also: the host time of the 64 one-stamp ambient rows (`FusedHyperField.time_bias`) inside a native update, and the query launch alone on
one full slice, back to back, in the given table layout (--layout both: QUAD, the default binding, and PAD), with its per-cell figure
next to the forward kernel's per-point figure of profiles/hyper_field_speed.json.
Prints one JSON line; --out also writes it to a file (profiles/hyper_density_speed.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seald-nerf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layout", default="both", choices=("quad", "both"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hyper_density_speed.py needs a GPU")
    from dnerf_amd.bench_scene import build_hyper_scene
    from dnerf_amd.fused import DensityGridUpdater
    from dnerf_amd.fused_hyper import FusedHyperField

    sc = build_hyper_scene(H=64, W=64, device="cuda", seed=0, time=0.5)
    m = sc.model
    up = DensityGridUpdater(m)
    f = up.field
    assert f.ctx_kind == 4 and f.has_density_query and f.layout == "quad"
    H3 = m.grid_size ** 3
    state = {}

    def reset(iter_density):
        # a grid as the first full update leaves it, so that the partial passes draw from a populated one
        if "grid" not in state:
            m.density_grid.zero_()
            m.iter_density = 0
            up.update(0.95)
            state["grid"] = m.density_grid.clone()
        m.density_grid.copy_(state["grid"])
        m.iter_density = iter_density

    def native():
        up.refresh()
        up.update(0.95)

    def op_by_op():
        with torch.autocast("cuda", dtype=torch.float16):
            m.update_extra_state()      # the op-by-op pass: `m` has no updater hooked in (asserted below)

    assert getattr(m, "_density_updater", None) is None
    subjects = {"native_full": (0, native), "native_partial": (16, native), "op_by_op_full": (0, op_by_op), "op_by_op_partial": (16, op_by_op)}

    def timed(iter_density, fn):
        reset(iter_density)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(args.warmup):
        for it, fn in subjects.values():
            timed(it, fn)
    ms = {k: [] for k in subjects}
    fields = {"quad": f}
    if args.layout == "both":
        fields["pad"] = FusedHyperField(m, 0.5, table_layout="pad", density_query=True)
    rows_ms, launch_us = [], {k: [] for k in fields}
    times = (m.times.reshape(-1) + 0.003).contiguous()
    out_slice = torch.empty(H3, dtype=torch.float32, device="cuda")
    for _ in range(args.repeats):
        for k, (it, fn) in subjects.items():
            ms[k].append(timed(it, fn))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f.time_bias(times)
        torch.cuda.synchronize()
        rows_ms.append(1e3 * (time.perf_counter() - t0))
        for name, fld in fields.items():
            row = fld.time_constants(0.5)[0]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fld.query_cells(out_slice, row, 0, 1.0, n=H3, seed=1)
            torch.cuda.synchronize()
            a.record()
            for i in range(50):
                fld.query_cells(out_slice, row, 0, 1.0, n=H3, seed=i)
            b.record()
            b.synchronize()
            launch_us[name].append(1e3 * a.elapsed_time(b) / 50)

    def summary(v, digits=3):
        return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits), "runs": [round(x, digits) for x in v]}

    out = {"metric": "update_extra_state of the ambient-dimension model, 64 slices x 128^3 cells, -O", "device": torch.cuda.get_device_name(0),
           "command": "python tools/hyper_density_speed.py --out profiles/hyper_density_speed.json", "repeats": args.repeats,
           "timing": "host clock between device synchronises, one update per run"}
    for k, v in ms.items():
        out[k + "_ms"] = summary(v)
    out["native_over_op_by_op_full"] = round(out["native_full_ms"]["median"] / out["op_by_op_full_ms"]["median"], 4)
    out["native_over_op_by_op_partial"] = round(out["native_partial_ms"]["median"] / out["op_by_op_partial_ms"]["median"], 4)
    out["time_bias_64_one_stamp_rows_host_ms"] = summary(rows_ms)
    for name, v in launch_us.items():
        out["query_launch_full_slice_" + name] = {"cells": H3, "us_per_launch": summary(v, 2), "ns_per_cell": round(statistics.median(v) * 1e3 / H3, 4),
                                                  "in_kernel_generator": True}
    out["forward_kernel_ns_per_point"] = "profiles/hyper_field_speed.json"
    out["not_measured"] = ("what bounds the query launch (no counter run); a batched time_bias (one ambient() call for the 64 stamps); "
                           "an update on the PAD layout (only its query launch is timed)")
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
