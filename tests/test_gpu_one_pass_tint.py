"""The rgb tint (`modify_rgb`) in the one-pass ray-batch renderer: `RayBatchRenderer` replays the inference loop's schedule on the device
(`sdn_whole_rays_schedule`) and tints every masked sample by the mean brightness of its own loop iteration
(`sdn_seal_modify_rgb_whole_rays`).  The yardstick is `DeviceLoop` with the same mapper, model, rays and T_thresh = 1e-4: image and
weights_sum bit for bit, depth to the fp32-rounding bound of the existing one-pass tests (1e-5, `test_one_pass_ray_batch_render_equals_
the_loop`: the loop re-bases t at every iteration).

256 rays (a 16 x 16 grid of pixels on the capsule figure, time 0.5; 200 of them miss it).  The figure's density is raised by half so
that some thirty rays through the torso are terminated (T < 1e-4) inside the figure while others run out of samples; the tint box lies
strictly inside the torso, so no ray's first sample is in it.  What the scene has to exercise is asserted from the loop's own trace and the replay's buffers, see `check_scene`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_SIDE, TIME, T_THRESH, DENSITY = 16, 0.5, 1e-4, 1.5
TINT = dict(rgb=[0.9, 0.3, 0.1], rgbLightOffset=0.05)
_HALF, _CENTRE = 0.06, (0.0, 0.08, 0.0)                       # inside the torso capsule (radius 0.11 about the segment y in [-0.15, 0.30])
RAW = [[_CENTRE[0] + sx * _HALF, _CENTRE[1] + sy * _HALF, _CENTRE[2] + sz * _HALF] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]


def bbox_config(shift=(0.0, 0.0, 0.0), **extra):
    T = np.eye(4)
    T[:3, 3] = shift
    return dict({"type": "bbox", "raw": RAW, "transform": T.tolist(), "scale": [1.0, 1.0, 1.0], "boundType": "to"}, **extra)


def build(density=DENSITY):
    """The 256 rays: every second pixel of the central half of the 64 x 64 camera, where about a quarter of them meet the figure."""
    from dnerf_amd.bench_scene import build_scene
    s = build_scene(H=4 * N_SIDE, W=4 * N_SIDE, device="cuda", seed=0, time=TIME)
    with torch.no_grad():
        s.model.sigma_net[-1].weight[0].mul_(density)
    px = torch.arange(N_SIDE, device="cuda") * 2 + N_SIDE
    pick = (px[:, None] * 4 * N_SIDE + px[None, :]).reshape(-1)
    s.rays_o, s.rays_d = s.rays_o[pick].contiguous(), s.rays_d[pick].contiguous()
    return s


@pytest.fixture(scope="module")
def sc():
    return build()


def render_both(sc, mapper, fill=False):
    """-> (the device loop's outputs, the one-pass renderer's, the one-pass renderer) for the scene's 256 rays."""
    from dnerf_amd import fused, seal_mapper as SM
    from dnerf_amd.renderer import DeviceLoop, RayBatchRenderer
    keep = sc.model.density_bitfield.clone()
    try:
        if fill:      # content is moved INTO the target box: the marcher has to sample there
            SM.fill_bitfield(sc.model.density_bitfield, mapper.map_data["force_fill_bound"].cpu().numpy(), sc.model.grid_size, sc.model.bound)
        n = sc.rays_o.shape[0]
        loop = DeviceLoop(sc.model, fused.FusedField(sc.model, TIME, fp16=True), n, "cuda", T_thresh=T_THRESH, mapper=mapper)
        want = loop.render(sc.rays_o, sc.rays_d, TIME, bg_color=1.0)
        want = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in want.items()}
        once = RayBatchRenderer(sc.model, fused.FusedField(sc.model, TIME, fp16=True), n, "cuda", T_thresh=T_THRESH, mapper=mapper, samples_per_ray=320)
        got = once.render(sc.rays_o, sc.rays_d, TIME, bg_color=1.0, check=True)
        torch.cuda.synchronize()
        return want, got, once
    finally:
        sc.model.density_bitfield.copy_(keep)


def assert_the_loops_render(got, want):
    assert torch.equal(got["image"], want["image"]), float((got["image"] - want["image"]).abs().max())
    assert torch.equal(got["weights_sum"], want["weights_sum"])
    d0, d1 = got["depth"], want["depth"]
    assert torch.equal(torch.isnan(d0), torch.isnan(d1))
    assert float((torch.nan_to_num(d0) - torch.nan_to_num(d1)).abs().max()) < 1e-5


def check_scene(once, want, demanding=True):
    """The replay against the loop and against its Python statement, and -- demanding -- what the scene must exercise:
      * the replayed (n_alive, n_step) of every iteration are the device loop's trace, the iteration count is the loop's;
      * the kernel's iteration of every sample slot equals `loop_schedule`'s, exactly, and every slot outside the rays' samples is -1;
      * rays without samples exist; n_step takes at least three values; a ray is killed strictly inside a window (a marched sample
        follows the kill in the same iteration); an iteration holds masked samples and another none; two iterations with masked
        samples differ in mean V."""
    from dnerf_amd.renderer import loop_schedule
    w = once._tint
    rays, stop = once.rays.cpu().numpy(), w.ray_stop.cpu().numpy()
    slot_iter, n_iter = w.slot_iter.cpu().numpy(), int(w.n_iter[0])
    counts, stops = rays[:, 2].astype(np.int64), stop[:, 0].astype(np.int64)
    assert np.array_equal(stop[:, 1], counts) and np.all(stops <= counts)           # (check=True: every ray fits the buffer)
    first = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(rays[:, 1], first[:-1])
    ids, trace = loop_schedule(counts, stops, once.max_steps)
    loop_trace = [(a, s) for a, s, _ in want["trace"]]
    print("trace", loop_trace, "samples", int(first[-1]), "empty rays", int((counts == 0).sum()), "killed rays", int((stops < counts).sum()))
    assert trace == loop_trace and n_iter == len(loop_trace)
    assert np.array_equal(slot_iter[: first[-1]], ids) and np.all(slot_iter[first[-1]:] == -1)
    acc = w.scratch.view(torch.int64).cpu().numpy().reshape(-1, 2)
    assert np.all(acc[n_iter:] == 0)
    masked = acc[:n_iter, 1]
    mean_v = acc[:n_iter, 0][masked > 0] / 2.0 ** 40 / masked[masked > 0]
    inside = [r for r in range(len(counts)) if stops[r] + 1 < counts[r] and ids[first[r] + stops[r] + 1] == ids[first[r] + stops[r]]]
    print("masked per iteration", masked.tolist(), "mean V", np.round(mean_v, 4).tolist(), "kills inside a window", len(inside))
    if demanding:
        assert (counts == 0).any()
        assert len({s for _, s in loop_trace}) >= 3
        assert inside
        assert (masked > 0).any() and (masked == 0).any()
        assert len(set(mean_v.tolist())) >= 2
    return masked


def test_tint_only(sc):
    from dnerf_amd import seal_mapper as SM
    want, got, once = render_both(sc, SM.get_seal_mapper(bbox_config(**TINT)))
    check_scene(once, want)
    assert_the_loops_render(got, want)
    again = once.render(sc.rays_o, sc.rays_d, TIME, bg_color=1.0)       # the per-iteration sums are cleared by every render
    torch.cuda.synchronize()
    assert torch.equal(again["image"], want["image"])


def test_tint_with_transform_and_hsv(sc):
    from dnerf_amd import seal_mapper as SM
    mapper = SM.get_seal_mapper(bbox_config(shift=(0.02, 0.02, 0.0), hsv=[0.3, -0.1, 0.05], **TINT))
    want, got, once = render_both(sc, mapper, fill=True)
    check_scene(once, want)
    assert_the_loops_render(got, want)


def test_tint_with_the_anchor_mapper(sc):
    import seal_anchor_support as AS
    from dnerf_amd.seal_mapper import SealAnchorMapper
    cfg = {k: v for k, v in AS.FRAME_CONFIG.items() if k != "hsv"}
    mapper = SealAnchorMapper(dict(cfg, **TINT))
    want, got, once = render_both(sc, mapper, fill=True)
    masked = check_scene(once, want, demanding=False)
    assert (masked > 0).any()
    assert_the_loops_render(got, want)


def test_a_tint_box_no_sample_enters(sc):
    from dnerf_amd import fused, seal_mapper as SM
    from dnerf_amd.renderer import RayBatchRenderer
    far = [[0.7 + sx * 0.05, 0.7 + sy * 0.05, 0.7 + sz * 0.05] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]
    mapper = SM.get_seal_mapper(dict(bbox_config(**TINT), raw=far))
    want, got, once = render_both(sc, mapper)
    masked = check_scene(once, want, demanding=False)
    assert not (masked > 0).any()
    assert_the_loops_render(got, want)
    plain = RayBatchRenderer(sc.model, fused.FusedField(sc.model, TIME, fp16=True), sc.rays_o.shape[0], "cuda", T_thresh=T_THRESH)
    ref = plain.render(sc.rays_o, sc.rays_d, TIME, bg_color=1.0, check=True)
    torch.cuda.synchronize()
    assert torch.equal(got["image"], ref["image"])


def test_edit_train_step_takes_a_tint_mapper_in_one_pass(sc):
    from dnerf_amd import fused, seal_mapper as SM
    from dnerf_amd.network import NeRFNetwork
    from dnerf_amd.renderer import DeviceLoop, RayBatchRenderer
    from dnerf_amd.seald_train import EditTrainStep, freeze_deformation
    mapper = SM.get_seal_mapper(bbox_config(**TINT))
    student = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).to("cuda").train()
    student.load_state_dict(sc.model.state_dict())
    student.mean_count, student.local_step = 64 * sc.rays_o.shape[0], 0          # a sample budget: the native step needs one to be built
    opt = torch.optim.Adam(freeze_deformation(student), lr=2e-3, betas=(0.9, 0.99), eps=1e-15)
    n = sc.rays_o.shape[0]
    edit = EditTrainStep(sc.model, student, mapper, opt, torch.amp.GradScaler("cuda"), n, "cuda", TIME, native=True, perturb=False)
    assert isinstance(edit.loop, RayBatchRenderer)
    got = edit.proxy_truth(sc.rays_o, sc.rays_d, TIME).clone()
    loop = DeviceLoop(sc.model, fused.FusedField(sc.model, TIME, fp16=True), n, "cuda", T_thresh=T_THRESH, mapper=mapper)
    want = loop.render(sc.rays_o, sc.rays_d, TIME, bg_color=1.0)["image"]
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    untinted = DeviceLoop(sc.model, fused.FusedField(sc.model, TIME, fp16=True), n, "cuda", T_thresh=T_THRESH).render(sc.rays_o, sc.rays_d, TIME)["image"]
    assert float((want - untinted).abs().max()) > 0.05          # the edit is visible


def test_map_source_is_still_refused(sc):
    from dnerf_amd import fused, seal_mapper as SM
    from dnerf_amd.renderer import RayBatchRenderer
    mapper = SM.get_seal_mapper(bbox_config(shift=(0.3, 0.0, 0.0), mapSource=[0.9, 0.9, 0.9], **TINT))
    assert mapper.redirects_source
    with pytest.raises(NotImplementedError, match="mapSource") as e:
        RayBatchRenderer(sc.model, fused.FusedField(sc.model, TIME, fp16=True), sc.rays_o.shape[0], "cuda", T_thresh=T_THRESH, mapper=mapper)
    assert "tint" not in str(e.value)
