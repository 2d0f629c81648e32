"""The temporal-basis model through the native frame drivers (dnerf_amd/frame_loops.py) with `FusedBasisField`: the 64 x 64 frames of
tests/golden/caller_basis.npz (the reference's own `run_cuda` on dnerf/network_basis.py) at the three fixture times.  The image bars
are measured, not chosen: the mirror's op-by-op `-O` frame through the reference-shaped `run_cuda` keeps some distance to the fixture's
fp32 frame, and a natively rendered frame must stay within twice each of its max, p99.9 and mean."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import basis_support as BS  # noqa: E402
from tests_support import assert_dist, dist_stats  # noqa: E402

N = 64 * 64


@pytest.fixture(scope="module")
def rig():
    from dnerf_amd import fused_basis, scene
    model, bits = BS.mirror_model("cuda")
    ro, rd = scene.get_rays(scene.look_at_pose(30.0, 30.0), scene.intrinsics(64, 64), 64, 64)
    ro, rd = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    fx = BS.load()
    bars = {}
    model.fused_inference = False          # the op-by-op -O frame: reference-shaped run_cuda over the existing operators
    try:
        for t in BS.TIMES:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                a = model.render(ro[None], rd[None], torch.tensor([[t]], dtype=torch.float32, device="cuda"), staged=False, perturb=False, bg_color=None)
            st = dist_stats(a["image"][0].float().cpu().numpy(), fx[f"t{t}_image"])
            bars[t] = dict(max=2 * st["max"], p999=2 * st["p99.9"], mean=2 * st["mean"])
            print(f"[basis-render] t={t} op-by-op -O frame vs fixture: {st}")
    finally:
        del model.fused_inference
    return dict(model=model, bits=bits, ro=ro, rd=rd, fx=fx, bars=bars, field=fused_basis.FusedBasisField(model, 0.5))


@pytest.mark.parametrize("t", BS.TIMES)
def test_render_frame_and_device_loop_reproduce_the_fixture_frames(rig, t):
    from dnerf_amd.renderer import DeviceLoop, render_frame
    r = rig
    r["field"].set_time(t)
    out = render_frame(r["model"], r["ro"], r["rd"], torch.tensor([[t]], dtype=torch.float32, device="cuda"), fp16=True, field=r["field"])
    print("render_frame", assert_dist(out["image"].cpu().numpy(), r["fx"][f"t{t}_image"], f"render_frame t={t}", **r["bars"][t]))
    assert abs(len(out["trace"]) - len(r["fx"][f"t{t}_trace"])) <= 1 and out["trace"][0] == tuple(r["fx"][f"t{t}_trace"][0])
    loop = DeviceLoop(r["model"], r["field"], N, "cuda")
    fast = loop.render(r["ro"], r["rd"], t)
    torch.cuda.synchronize()
    print("DeviceLoop", assert_dist(fast["image"].cpu().numpy(), r["fx"][f"t{t}_image"], f"DeviceLoop t={t}", **r["bars"][t]))
    assert abs(fast["n_samples"] - out["n_samples"]) <= 0.02 * out["n_samples"]      # (the device loop sizes iterations from a bound of the survivors)


def test_frame_group_pipeline_and_ray_batches_agree_with_frames_rendered_alone(rig):
    from dnerf_amd.renderer import DeviceLoop, PipelinedDeviceLoop, RayBatchRenderer
    r = rig
    model, field, ro, rd = r["model"], r["field"], r["ro"], r["rd"]
    times = [0.0, 0.93]
    one = DeviceLoop(model, field, N, "cuda")
    want = []
    for t in times:
        o = one.render(ro, rd, t)
        want.append(o["image"].clone())
    assert not torch.equal(want[0], want[1])
    grp = DeviceLoop(model, field, 2 * N, "cuda", frames=2)
    out = grp.render(torch.cat([ro, ro]).contiguous(), torch.cat([rd, rd]).contiguous(), times)
    torch.cuda.synchronize()
    for f in range(2):
        assert torch.equal(out["image"][f * N:(f + 1) * N], want[f]), f
    pl = PipelinedDeviceLoop(model, field, N, "cuda", contexts=2)
    outs = [(torch.empty(N, 3, device="cuda"), torch.empty(N, device="cuda")) for _ in times]
    pl.render_frames([ro, ro], [rd, rd], times, outputs=outs)
    torch.cuda.synchronize()
    for f in range(2):
        assert torch.equal(outs[f][0], want[f]), f
    # 256 of the rays in one pass: the same pixels, within the frame's bars (the one-pass schedule composites in another order)
    sel = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:256].cuda()
    once = RayBatchRenderer(model, field, 256, "cuda")
    got = once.render(ro[sel].contiguous(), rd[sel].contiguous(), 0.93, check=True)
    assert_dist(got["image"].cpu().numpy(), want[1][sel].cpu().numpy(), "RayBatchRenderer vs DeviceLoop", **r["bars"][0.93])


def test_bbox_seal_mapper_changes_pixels_inside_the_box_projection_only(rig):
    from caller_fixtures import fill_bitfield_host
    from dnerf_amd.renderer import DeviceLoop
    from dnerf_amd.seal_mapper import SealBBoxMapper
    from test_caller_fixtures_cpu import SEAL_CONFIG
    r = rig
    model, field = r["model"], r["field"]
    keep = model.density_bitfield.clone()
    try:
        mapper = SealBBoxMapper(SEAL_CONFIG)
        bounds = mapper.map_data["force_fill_bound"].cpu().numpy()
        model.density_bitfield.copy_(torch.from_numpy(fill_bitfield_host(r["bits"], bounds)))
        plain = DeviceLoop(model, field, N, "cuda", T_thresh=1e-4).render(r["ro"], r["rd"], 0.5)["image"].clone()
        edited = DeviceLoop(model, field, N, "cuda", T_thresh=1e-4, mapper=mapper).render(r["ro"], r["rd"], 0.5)["image"].clone()
        torch.cuda.synchronize()
    finally:
        model.density_bitfield.copy_(keep)
    changed = ((edited - plain).abs().max(1).values > 1e-4).cpu().numpy()
    assert changed.sum() >= 20 and np.isfinite(edited.cpu().numpy()).all()
    # the target box's projection: pixels whose ray passes through the box `map_bound` (slab test, a pixel of slack)
    lo, hi = np.asarray(mapper.map_data["map_bound"].cpu().numpy(), np.float64).reshape(2, 3)
    o, d = r["ro"].cpu().numpy().astype(np.float64), r["rd"].cpu().numpy().astype(np.float64)
    pad = 2.0 * 4.0 / 64
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - pad - o) / d, (hi + pad - o) / d
    near, far = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    inside = (near <= far) & (far > 0)
    assert not (changed & ~inside).any(), int((changed & ~inside).sum())
