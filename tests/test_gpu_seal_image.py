"""The brush's texture stamp (`imageConfig`) on the GPU: `sdn_seal_modify_image` (csrc/seal.hip) against what the reference's own
map_color produced (tests/golden/caller_seald_image.npz, data only) and against the torch restatement run on the CPU; lane and wave
tails; the reference teacher's frame through the three render paths; the one-pass teacher of an edit-training step.

Colours: the project's fp32 bar, 1e-4, on the clear points -- both float64 texel coordinates at least 1e-3 texel from every integer
1..W-1 / 1..H-1; the fixture has no unclear point among its 389.  Texel indices are read off the output colours of an index texture."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import seal_image_support as IS  # noqa: E402
from caller_fixtures import fill_bitfield_host, fixture_model, fixture_scene  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(IS.FIXTURE)


@pytest.fixture(scope="module")
def pngs(tmp_path_factory):
    d = tmp_path_factory.mktemp("stamp")
    return dict(rgba=IS.write_png(d / "stamp_rgba.png", IS.stamp_texture()), rgb=IS.write_png(d / "stamp_rgb.png", IS.stamp_texture()[:, :, :3].copy()),
                index=IS.write_png(d / "index.png", IS.index_texture()))


def _buffers(fx, spread=2, seed=5):
    """The fixture's masked samples in every `spread`-th slot of the sample buffers, unmasked slots with colours and points of their own
    between them -> (points, colours, mask) on the host."""
    n = fx["points"].shape[0]
    g = torch.Generator().manual_seed(seed)
    pts, cols, mask = torch.rand(spread * n, 3, generator=g) - 0.5, torch.rand(spread * n, 3, generator=g), torch.zeros(spread * n, dtype=torch.bool)
    pts[::spread], cols[::spread], mask[::spread] = torch.from_numpy(fx["points"]), torch.from_numpy(fx["colors_in"]), True
    return pts, cols, mask


@pytest.mark.parametrize("name,rgb", [("stamp", False), ("rgb_stamp", True)])
def test_map_color_reproduces_the_reference(fx, pngs, name, rgb):
    from dnerf_amd.seal_mapper import SealBrushMapper
    m = SealBrushMapper(IS.point_config(pngs["rgba"], rgb=rgb))
    pts, cols, mask = _buffers(fx)
    clear = fx["clear"]
    assert (~clear).mean() <= IS.CLEAR_CAP
    got = m.map_color_(cols.cuda(), mask.cuda(), points=pts.cuda().contiguous()).cpu()
    err = float(np.abs(got[::2].numpy() - fx[f"colors_out_{name}"])[clear].max())
    print(name, "unclear", int((~clear).sum()), "largest colour difference against the reference on clear points", err)
    assert err <= 1e-4
    assert torch.equal(got[1::2], cols[1::2])                                          # unmasked slots: bit-identical
    cpu = SealBrushMapper(IS.point_config(pngs["rgba"], rgb=rgb)).map_color_(cols.clone(), mask, points=pts)
    np.testing.assert_allclose(got.numpy()[::2][clear], cpu.numpy()[::2][clear], rtol=0, atol=1e-4)
    if rgb:
        return
    # transparent texels: the colour comes back bit-identical; opaque ones: the unblended modify_rgb value, the mean being the whole call's
    alpha = IS.stamp_texture()[fx["idx_h"], fx["idx_w"], 3]
    t0, t255 = torch.from_numpy(clear & (alpha == 0)), torch.from_numpy(clear & (alpha == 255))
    assert int(t0.sum()) >= 50 and torch.equal(got[::2][t0], cols[::2][t0])
    assert int(t255.sum()) >= 50
    opaque = SealBrushMapper(IS.point_config(pngs["rgb"]))                             # the same colours, no alpha channel: nothing is blended
    unblended = opaque.map_color_(cols.cuda(), mask.cuda(), points=pts.cuda().contiguous()).cpu()
    assert torch.equal(got[::2][t255], unblended[::2][t255]) and not torch.equal(got[::2][t0], unblended[::2][t0])
    from dnerf_amd.seal_mapper import modify_rgb
    target = torch.from_numpy(IS.stamp_texture()[fx["idx_h"], fx["idx_w"], :3].astype(np.float32) / 255)
    whole = modify_rgb(cols[::2].clone(), target, IS.LIGHT_OFFSET)                     # (the CPU's modify_rgb: its mean is torch's, not the fixed-point one)
    np.testing.assert_allclose(got[::2][t255].numpy(), whole[t255].numpy(), rtol=0, atol=1e-4)


def test_texel_indices_on_the_device(fx, pngs):
    from dnerf_amd.seal_mapper import SealBrushMapper
    m = SealBrushMapper(IS.point_config(pngs["index"]))
    pts, cols = torch.from_numpy(fx["points"]).cuda(), torch.from_numpy(fx["colors_in"]).cuda()
    got = m.map_color_(cols, torch.ones(pts.shape[0], dtype=torch.bool, device="cuda"), points=pts).cpu().numpy()
    iw, ih = IS.decode_index(got)
    clear = fx["clear"]
    print("unclear", int((~clear).sum()), "index mismatches in all", int(((iw != fx["idx_w"]) | (ih != fx["idx_h"])).sum()))
    assert np.array_equal(iw[clear], fx["idx_w"][clear]) and np.array_equal(ih[clear], fx["idx_h"][clear])


@pytest.mark.parametrize("M", [1, 63, 65, 257])
@pytest.mark.parametrize("rgb", [False, True])
def test_tails_through_the_c_calls(fx, pngs, M, rgb):
    """A call of M slots (a lane tail, a wave tail, a second workgroup): the first M slots are the call -- their mean is their own --, the
    slots beyond M and the unmasked ones stay bit-identical.  The yardstick is the restatement on the CPU on the same M slots."""
    from dnerf_amd.seal_mapper import SealBrushMapper
    from sdn_backend import lib, check, ptr, stream
    m = SealBrushMapper(IS.point_config(pngs["rgba"], rgb=rgb))
    pts, cols, mask = _buffers(fx, spread=3 if M > 1 else 1)
    want = SealBrushMapper(IS.point_config(pngs["rgba"], rgb=rgb)).map_color_(cols[:M].clone(), mask[:M], points=pts[:M])
    a = m._native_args(torch.device("cuda", torch.cuda.current_device()))
    d_pts, d_cols, d_mask = pts.cuda(), cols.cuda(), mask.cuda().view(torch.uint8)
    if rgb:
        check(lib.sdn_seal_modify_rgb(ptr(d_cols), ptr(d_mask), M, a["rgb"][0], a["rgb"][1], a["rgb"][2], a["rgb_light_offset"], ptr(a["scratch"]),
                                      None, None, None, stream()), "seal_modify_rgb")
    check(lib.sdn_seal_modify_image(ptr(d_cols), ptr(d_pts), ptr(d_mask), M, ctypes.addressof(a["image"]), ptr(a["image_scratch"]), None, None, None, stream()),
          "seal_modify_image")
    got = d_cols.cpu()
    assert torch.equal(got[M:], cols[M:]) and torch.equal(got[:M][~mask[:M]], cols[:M][~mask[:M]])
    assert torch.equal(d_pts.cpu(), pts)
    clear = np.zeros(M, bool)
    step = 3 if M > 1 else 1
    clear[::step] = fx["clear"][:len(range(0, M, step))]
    np.testing.assert_allclose(got[:M].numpy()[clear], want.numpy()[clear], rtol=0, atol=1e-4)
    assert not torch.equal(got[:M][mask[:M]], cols[:M][mask[:M]]) or M == 1


def test_nothing_masked_changes_nothing(fx, pngs):
    from dnerf_amd.seal_mapper import SealBrushMapper
    m = SealBrushMapper(IS.point_config(pngs["rgba"], rgb=True))
    pts, cols, mask = _buffers(fx)
    got = m.map_color_(cols.cuda(), torch.zeros_like(mask).cuda(), points=pts.cuda())
    assert torch.equal(got.cpu(), cols)
    with pytest.raises(ValueError, match="points"):
        m.map_color_(cols.cuda(), mask.cuda())


@pytest.fixture(scope="module")
def model_bits():
    return fixture_model("cuda")


def test_teacher_frame_through_the_render_paths(fx, pngs, model_bits):
    """The reference teacher's frame with the textured brush (64 x 64, time 0.5, T_thresh 1e-4, force_fill_bound marked occupied), at the
    brush test's bars: the host-stepped loop on the fp32 operators reproduces it (trace exact, image and weights_sum 1e-4); the
    host-stepped loop with the fused -O field and the device loop agree bit for bit; the one-pass renderer gives the device loop's image
    bit for bit, its depth to 1e-5; a frame group refuses the stamp; the edit-training step's one-pass teacher takes it."""
    from dnerf_amd.fused import FusedField
    from dnerf_amd.network import NeRFNetwork
    from dnerf_amd.renderer import DeviceLoop, RayBatchRenderer, render_frame
    from dnerf_amd.seal_mapper import SealBrushMapper
    from dnerf_amd.seald_train import EditTrainStep, freeze_deformation
    model, bits = model_bits
    sc = fixture_scene("cuda", model_bits=model_bits)
    keep = model.density_bitfield.clone()
    N = sc.rays_o.shape[0]
    try:
        mapper = SealBrushMapper(IS.frame_config(pngs["rgba"]))
        filled = fill_bitfield_host(bits, mapper.map_data["force_fill_bound"].cpu().numpy())
        model.density_bitfield.copy_(torch.from_numpy(filled))
        out = render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=False, T_thresh=1e-4, mapper=mapper)
        assert fx["frame_trace"].tolist() == [list(r) for r in out["trace"]]
        print("frame: largest image difference against the reference", float(np.abs(out["image"].cpu().numpy() - fx["frame_image"]).max()),
              "weights_sum", float(np.abs(out["weights_sum"].cpu().numpy() - fx["frame_weights_sum"]).max()))
        np.testing.assert_allclose(out["image"].cpu().numpy(), fx["frame_image"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(out["weights_sum"].cpu().numpy(), fx["frame_weights_sum"], rtol=0, atol=1e-4)
        assert (np.abs(out["image"].cpu().numpy() - fx["frame_plain_image"]).max(1) > 1e-3).sum() >= 100
        field = FusedField(sc.model, sc.time)
        host = render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=True, field=field, T_thresh=1e-4, mapper=mapper)
        loop = DeviceLoop(sc.model, field, N, "cuda", T_thresh=1e-4, mapper=mapper)
        fast = loop.render(sc.rays_o, sc.rays_d, sc.time)
        torch.cuda.synchronize()
        fast = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in fast.items()}
        assert torch.equal(host["image"], fast["image"]) and host["n_samples"] == fast["n_samples"]
        no_stamp = SealBrushMapper({k: v for k, v in IS.frame_config("unused").items() if k != "imageConfig"})
        bare = DeviceLoop(sc.model, field, N, "cuda", T_thresh=1e-4, mapper=no_stamp).render(sc.rays_o, sc.rays_d, sc.time)["image"]
        torch.cuda.synchronize()
        assert int(((fast["image"] - bare).abs().amax(1) > 1e-3).sum()) >= 100          # the stamp is in the device loop's frame
        once = RayBatchRenderer(sc.model, FusedField(sc.model, sc.time), N, "cuda", T_thresh=1e-4, mapper=mapper, samples_per_ray=160)
        got = once.render(sc.rays_o, sc.rays_d, sc.time, bg_color=1.0, check=True)
        torch.cuda.synchronize()
        assert torch.equal(got["image"], fast["image"]), float((got["image"] - fast["image"]).abs().max())
        d0, d1 = got["depth"], fast["depth"]
        assert torch.equal(torch.isnan(d0), torch.isnan(d1))
        assert float((torch.nan_to_num(d0) - torch.nan_to_num(d1)).abs().max()) < 1e-5
        # one mean per iteration: not in a frame group
        with pytest.raises(NotImplementedError):
            DeviceLoop(sc.model, field, 2 * N, "cuda", T_thresh=1e-4, mapper=mapper, frames=2)
        # one edit-training step with the textured brush: the default one-pass teacher's target is the device loop's image
        student = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).to("cuda").train()
        student.load_state_dict(sc.model.state_dict())
        student.mean_count, student.local_step = 64 * N, 0
        opt = torch.optim.Adam(freeze_deformation(student), lr=2e-3, betas=(0.9, 0.99), eps=1e-15)
        edit = EditTrainStep(sc.model, student, mapper, opt, torch.amp.GradScaler("cuda"), N, "cuda", sc.time, native=True, perturb=False)
        assert isinstance(edit.loop, RayBatchRenderer)
        target = edit.proxy_truth(sc.rays_o, sc.rays_d, sc.time).clone()
        assert torch.equal(target, fast["image"])
        loss = float(edit(sc.rays_o, sc.rays_d, sc.time))
        torch.cuda.synchronize()
        assert np.isfinite(loss)
    finally:
        model.density_bitfield.copy_(keep)
