#!/usr/bin/env python3
"""Generates tests/golden/caller_preview.npz by EXECUTING THE REFERENCE'S OWN caller code -- dnerf/renderer.py `run_cuda` with
`perturb=True` (what `Trainer.test_gui` renders: SealDNeRF/utils.py:174-240 calls `test_step(..., perturb=spp)` with spp >= 1),
`torch.nn.functional.interpolate(mode='nearest')` as `test_gui` calls it, and nerf/utils.py `linear_to_srgb` -- imported from
/root/reference, never copied, over the oracle-backed operator shims of tests/ref_shims/, the way gen_caller_fixtures.py makes the
other caller fixtures.

(a) frame: the fixture scene and model at 64 x 64, time 0.5, `run_cuda(perturb=True)`; the per-ray offsets of iteration 0 are
    seeded here and handed to the shim through `ref_shims.raymarching.NOISES["infer"]` (the reference draws them with torch.rand
    inside its CUDA wrapper; later iterations pass perturb=False).  Recorded: the offsets, the loop trace, the live sample count,
    image, depth, weights_sum.  Some offsets are pinned to 0 and to nextafter(1, 0).
(b) `F.interpolate(nearest)` of an 18 x 26 frame to 37 x 53: the frame holds each pixel's own index, so the output IS the source
    index of every output pixel.
(c) `linear_to_srgb` of a ramp with values on both sides of 0.0031308.

Run in the build container only:   python tests/golden/gen_preview_fixture.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import gen_caller_fixtures as G  # noqa: E402  (installs the stubs and the operator shims)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import preview_support as PS  # noqa: E402

RM = G.RM


def gen_frame(out):
    import dnerf.network as ref_network
    model, bits = G.build_reference_model(ref_network.NeRFNetwork)
    ro, rd, _ = G.camera_rays(64, 64)
    noises = PS.draw_noises(ro.shape[1], PS.FRAME_SEED)
    samples = []
    inner = RM.O.march_rays

    def counting(*a, **k):                     # the live samples of every march: slots with a non-zero step
        r = inner(*a, **k)
        samples.append(int((r[2][:, 0] > 0).sum()))
        return r
    RM.NOISES["infer"] = noises
    RM.O.march_rays = counting
    try:
        RM.TRACE.clear()
        RM.LAST.clear()
        res = model.render(ro, rd, torch.tensor([[0.5]], dtype=torch.float32), staged=False, bg_color=None, perturb=True)
    finally:
        RM.NOISES["infer"] = None
        RM.O.march_rays = inner
    out["noises"] = noises
    out["trace"] = np.array(RM.TRACE, np.int32)
    out["n_samples"] = np.int64(sum(samples))
    out["image"], out["depth"] = res["image"][0].numpy().copy(), res["depth"][0].numpy().copy()
    out["weights_sum"] = RM.LAST["weights_sum"].numpy().copy()
    plain = G.run_infer(model, ro, rd, 0.5)
    moved = int((np.abs(plain["image"] - out["image"]).max(1) > 1e-4).sum())
    print(f"[frame] iterations {len(out['trace'])}, samples {int(out['n_samples'])}, pixels the jitter moves by more than 1e-4: {moved}")
    assert moved >= 100, "the perturbed frame must differ from the unperturbed one"


def gen_interpolate(out):
    import torch.nn.functional as F
    rH, rW, H, W = PS.NEAREST_CASE
    src = torch.arange(rH * rW, dtype=torch.float32).view(1, 1, rH, rW)
    up = F.interpolate(src, size=(H, W), mode="nearest")          # test_gui's call (SealDNeRF/utils.py:212-213)
    out["nearest_index"] = up[0, 0].numpy().astype(np.int32)


def gen_srgb(out):
    from nerf.utils import linear_to_srgb
    x = PS.srgb_ramp()
    out["srgb_in"] = x
    out["srgb_out"] = linear_to_srgb(torch.from_numpy(x)).numpy().copy()


def main():
    out = {}
    gen_frame(out)
    gen_interpolate(out)
    gen_srgb(out)
    np.savez_compressed(PS.FIXTURE, **out)
    print("wrote", PS.FIXTURE, f"{os.path.getsize(PS.FIXTURE) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
