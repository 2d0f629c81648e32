"""The ambient-dimension model through the native frame drivers (dnerf_amd/frame_loops.py) with `FusedHyperField`: the 64 x 64 frames of
tests/golden/caller_hyper.npz (the reference's own `run_cuda` on dnerf/network_hyper.py) at the three fixture times.  The image bars
are those of tests/test_gpu_basis_render.py: the mirror's op-by-op `-O` frame through the reference-shaped `run_cuda` keeps some
distance to the fixture's fp32 frame, and a natively rendered frame must stay within twice each of its max, p99.9 and mean."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hyper_support as HS  # noqa: E402
from tests_support import assert_dist, dist_stats  # noqa: E402

N = 64 * 64


@pytest.fixture(scope="module")
def rig():
    from dnerf_amd import fused_hyper, scene
    model, bits = HS.mirror_model("cuda")
    ro, rd = scene.get_rays(scene.look_at_pose(30.0, 30.0), scene.intrinsics(64, 64), 64, 64)
    ro, rd = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    fx = HS.load()
    bars = {}
    model.fused_inference = False          # the op-by-op -O frame: reference-shaped run_cuda over the existing operators
    try:
        for t in HS.TIMES:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                a = model.render(ro[None], rd[None], torch.tensor([[t]], dtype=torch.float32, device="cuda"), staged=False, perturb=False, bg_color=None)
            st = dist_stats(a["image"][0].float().cpu().numpy(), fx[f"t{t}_image"])
            bars[t] = dict(max=2 * st["max"], p999=2 * st["p99.9"], mean=2 * st["mean"])
            print(f"[hyper-render] t={t} op-by-op -O frame vs fixture: {st}")
    finally:
        del model.fused_inference
    return dict(model=model, bits=bits, ro=ro, rd=rd, fx=fx, bars=bars, field=fused_hyper.FusedHyperField(model, 0.5))


@pytest.mark.parametrize("t", HS.TIMES)
def test_render_frame_and_device_loop_reproduce_the_fixture_frames(rig, t):
    from dnerf_amd.renderer import DeviceLoop, render_frame
    r = rig
    r["field"].set_time(t)
    out = render_frame(r["model"], r["ro"], r["rd"], torch.tensor([[t]], dtype=torch.float32, device="cuda"), fp16=True, field=r["field"])
    print("render_frame", assert_dist(out["image"].cpu().numpy(), r["fx"][f"t{t}_image"], f"render_frame t={t}", **r["bars"][t]))
    # (the -O sigmas may flip a threshold: the trace is held to the fixture's as the basis render test holds it)
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
    times = list(HS.TIMES)
    one = DeviceLoop(model, field, N, "cuda")
    want = []
    for t in times:
        o = one.render(ro, rd, t)
        want.append(o["image"].clone())
    assert not torch.equal(want[0], want[2]) and not torch.equal(want[0], want[1])
    grp = DeviceLoop(model, field, 3 * N, "cuda", frames=3)
    out = grp.render(torch.cat([ro, ro, ro]).contiguous(), torch.cat([rd, rd, rd]).contiguous(), times)
    torch.cuda.synchronize()
    for f in range(3):
        assert torch.equal(out["image"][f * N:(f + 1) * N], want[f]), f
    pl = PipelinedDeviceLoop(model, field, N, "cuda", contexts=2)
    outs = [(torch.empty(N, 3, device="cuda"), torch.empty(N, device="cuda")) for _ in times]
    pl.render_frames([ro] * 3, [rd] * 3, times, outputs=outs)
    torch.cuda.synchronize()
    for f in range(3):
        assert torch.equal(outs[f][0], want[f]), f
    # 256 of the rays in one pass: the same pixels, within the frame's bars (the one-pass schedule composites in another order)
    sel = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:256].cuda()
    once = RayBatchRenderer(model, field, 256, "cuda")
    got = once.render(ro[sel].contiguous(), rd[sel].contiguous(), 0.93, check=True)
    assert_dist(got["image"].cpu().numpy(), want[2][sel].cpu().numpy(), "RayBatchRenderer vs DeviceLoop", **r["bars"][0.93])


def test_preview_renderer_serves_the_field(rig):
    """`PreviewRenderer` with kind 4: an unperturbed frame is the device loop's frame of the same rays bit for bit, and a grouped
    accumulation of two jittered samples of the view (one frame-group loop: two rows of constants) stays a finite image near it."""
    from dnerf_amd import scene
    from dnerf_amd.preview import PreviewRenderer
    from dnerf_amd.renderer import DeviceLoop
    from dnerf_amd.utils import get_rays
    r = rig
    model, field = r["model"], r["field"]
    H = W = 64
    pose, intr = scene.look_at_pose(30.0, 30.0), scene.intrinsics(H, W)
    pv = PreviewRenderer(model, field, W, H, "cuda")
    out = pv.frame(pose, intr, 0.5, spp=0)["image"].clone()
    rays = get_rays(torch.from_numpy(pose).cuda()[None], intr, H, W, -1)
    ref = DeviceLoop(model, field, N, "cuda").render(rays["rays_o"][0].contiguous(), rays["rays_d"][0].contiguous(), 0.5)
    assert ref["n_samples"] > 100 and torch.equal(out.view(-1, 3), ref["image"])
    mean = pv.accumulate_group(pose, intr, 0.5, need_update=True, samples=2)
    torch.cuda.synchronize()
    assert pv.spp == 2 and torch.isfinite(mean).all() and float((mean.view(-1, 3) - ref["image"]).abs().max()) < 0.25
