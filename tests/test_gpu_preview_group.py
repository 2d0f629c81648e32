"""Several jittered samples of one view in one loop, on the GPU: `DeviceLoop.render_samples` (a frame group whose context carries
`noises`), the group finishing pass `sdn_preview_finish_group`, and `PreviewRenderer.accumulate_group`.

The oracle is the merged one-frame preview path (tests/test_gpu_preview.py pins it against the reference's fixture): F frames rendered
one at a time with the same noise vectors, and F successive `sdn_preview_finish` calls.  Every comparison is bit for bit -- the group
runs the same per-ray arithmetic on the same inputs; no tolerance is involved."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import preview_group_support as GS  # noqa: E402
from caller_fixtures import fill_bitfield_host, fixture_model, fixture_scene  # noqa: E402

DEV = "cuda"
SIZES = [(50, 50), (5, 7), (1, 1)]          # 2 500 rays: frame boundaries inside 256-entry workgroups; 35; 1
ACCS = ("image", "depth", "weights_sum")


@pytest.fixture(scope="module")
def model_bits():
    return fixture_model(DEV)


@pytest.fixture(scope="module")
def singles():
    """(field kind, H, W, time, row name) -> what `DeviceLoop(frames=1).render(noises=row)` leaves; rendered once, shared, never written."""
    return {}


def _field(model, t, fp16):
    from dnerf_amd.fused import FusedField
    from dnerf_amd.fused_f32 import FusedFieldF32
    return FusedField(model, t) if fp16 else FusedFieldF32(model, t)


def _rays(model_bits, H, W, time):
    """The small synthetic scene's rays; from 35 rays on the last three miss the box (origin outside, looking away)."""
    sc = fixture_scene(DEV, model_bits=model_bits, H=H, W=W, time=time)
    ro, rd = sc.rays_o.clone(), sc.rays_d.clone()
    if H * W >= 35:
        ro[-3:] = torch.tensor([3.0, 3.0, 3.0], device=DEV)
        rd[-3:] = torch.tensor([0.0, 1.0, 0.0], device=DEV)
    return sc, ro, rd


def _single(singles, model_bits, fp16, H, W, time, name):
    from dnerf_amd.renderer import DeviceLoop
    key = (fp16, H, W, time, name)
    if key not in singles:
        sc, ro, rd = _rays(model_bits, H, W, time)
        loop = DeviceLoop(sc.model, _field(sc.model, sc.time, fp16), H * W, DEV)
        out = loop.render(ro, rd, sc.time, noises=torch.from_numpy(GS.noise_row(name, H * W)).to(DEV))
        torch.cuda.synchronize()
        singles[key] = dict({k: loop.buf[k].clone() for k in ACCS}, trace=[tuple(r) for r in out["trace"]], n_samples=out["n_samples"],
                            first=int(loop.buf["live_counts"][0].item()))
    return singles[key]


def _assert_frames(loop, refs, n):
    for f, ref in enumerate(refs):
        for k in ACCS:
            got = loop.buf[k][f * n:(f + 1) * n]
            assert torch.equal(got.view(torch.int32), ref[k].view(torch.int32)), (f, k)


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("F,time", [(2, 0.5), (3, 0.0), (4, 0.5)])
@pytest.mark.parametrize("fp16", [True, False])
def test_render_samples_leaves_every_frame_as_rendered_alone(model_bits, singles, fp16, F, time, H, W):
    """Per frame, the accumulators of the group are those of the one-frame loop with that frame's noise row.  Rows: the seeded draw
    (0 and nextafter(1, 0) among its entries), all 0, all nextafter(1, 0), and a row equal to row 0 -- identical frames.  F = 3 runs
    at t = 0, the canonical frame.  Of trace and sample count what does not depend on which rays share a loop: iteration 0 is one step
    of all rays (the reference's N // N), its samples and its survivors are the sums over the frames."""
    from dnerf_amd.renderer import DeviceLoop
    n = H * W
    sc, ro, rd = _rays(model_bits, H, W, time)
    names = GS.ROW_NAMES[F]
    refs = [_single(singles, model_bits, fp16, H, W, time, name) for name in names]
    loop = DeviceLoop(sc.model, _field(sc.model, sc.time, fp16), F * n, DEV, frames=F)
    out = loop.render_samples(ro, rd, sc.time, torch.from_numpy(GS.noise_rows(F, n)).to(DEV))
    torch.cuda.synchronize()
    _assert_frames(loop, refs, n)
    for f in range(1, F):                                   # equal rows, equal frames
        if names[f] == names[0]:
            for k in ACCS:
                assert torch.equal(loop.buf[k][f * n:(f + 1) * n].view(torch.int32), loop.buf[k][:n].view(torch.int32)), (f, k)
    tr = [tuple(r) for r in out["trace"]]
    assert tr[0][:2] == (F * n, 1) and all(r["trace"][0][:2] == (n, 1) for r in refs)
    assert int(loop.buf["live_counts"][0].item()) == sum(r["first"] for r in refs)
    survivors = sum(r["trace"][1][0] if len(r["trace"]) > 1 else 0 for r in refs)
    assert (tr[1][0] if len(tr) > 1 else 0) == survivors
    if n >= 35:
        assert out["n_samples"] > 0 and refs[0]["n_samples"] > 0
        assert not torch.equal(refs[0]["image"], refs[1]["image"])      # distinct jitter, distinct frames
    # finish=True: the loop's own finish over all F * n rays
    done = loop.render_samples(ro, rd, sc.time, torch.from_numpy(GS.noise_rows(F, n)).to(DEV), finish=True, want_stats=False)
    assert done["image"].shape == (F * n, 3)
    want = loop.buf["image"] + (1 - loop.buf["weights_sum"])[:, None] * 1.0
    assert torch.equal(done["image"], want)


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_group_culled_start_and_jump_change_nothing(model_bits, H, W):
    """A group context with the per-ray t_end cache runs the culled start over all F * n rays and jumps each ray from ITS perturbed
    start (the noise of the group's ray id); one without it marches all rays from there.  Same noises: bit-identical accumulators,
    identical traces and counts."""
    import sdn_backend
    from dnerf_amd.renderer import DeviceLoop
    F, n = 3, H * W
    sc, ro, rd = _rays(model_bits, H, W, 0.5)
    assert sc.model.grid_size == 128 and sc.model.cascade == 1 and sc.model.bound == 1
    field = _field(sc.model, sc.time, True)
    z = torch.from_numpy(GS.noise_rows(F, n)).to(DEV)
    culled = DeviceLoop(sc.model, field, F * n, DEV, frames=F)
    plain = DeviceLoop(sc.model, field, F * n, DEV, frames=F)
    plain.ctx.rays_tend = None
    a = culled.render_samples(ro, rd, sc.time, z)
    b = plain.render_samples(ro, rd, sc.time, z)
    torch.cuda.synchronize()
    assert [tuple(r) for r in a["trace"]] == [tuple(r) for r in b["trace"]] and a["n_samples"] == b["n_samples"]
    started = [int(lp.buf["state"][sdn_backend.LOOP_CULLED_START].item()) for lp in (culled, plain)]
    assert started == [1, 0]
    for k in ACCS:
        assert torch.equal(culled.buf[k].view(torch.int32), plain.buf[k].view(torch.int32)), k


# 3 --------------------------------------------------------------------------------------------------------------------
def _ctx(dev, first, count, group=None):
    import sdn_backend as B
    c = B.SdnRenderCtx()
    for k, v in dev.items():
        setattr(c, k, v[first:first + count].data_ptr())
    c.N = count
    if group:
        c.n_group_frames, c.rays_per_frame = group
    return c


@pytest.mark.parametrize("rH,rW,H,W", [(5, 7, 5, 7), (37, 53, 37, 53), (50, 50, 100, 100)])
@pytest.mark.parametrize("per_ray_bg", [False, True])
def test_group_finish_equals_successive_single_finishes(rH, rW, H, W, per_ray_bg):
    """`sdn_preview_finish_group` over n_fold frames against n_fold `sdn_preview_finish` calls on the frames' blocks: accum, image_out,
    depth_out and pos_out bit for bit, from spp = 0 and spp = 5, folding all 4 frames and fewer (3, 1), sRGB on and off, depth
    normalised and raw, downscale 1 (one block and several) and a 50 x 50 render blown up to 100 x 100, with NaN / inf depths and a NaN
    in one colour accumulator.  Pixels are independent and every output is compared whole, so nothing is written out of place."""
    import sdn_backend as B
    F, n = 4, rH * rW
    acc = GS.fake_group(F, rH, rW, seed=rH * 100 + rW)
    dev = {k: torch.from_numpy(v).to(DEV).contiguous() for k, v in acc.items()}
    rng = np.random.default_rng(9)
    bg = (ctypes.c_float * 3)(0.001, 0.5, 1.0)
    bgr = torch.from_numpy(rng.random((F * n, 3), dtype=np.float32)).to(DEV) if per_ray_bg else None
    old = torch.from_numpy(rng.random((H, W, 3), dtype=np.float32)).to(DEV)
    old[0, 0, 0] = float("nan")                                   # spp == 0 must overwrite it unread
    identity = (rH, rW) == (H, W)
    group = _ctx(dev, 0, F * n, group=(F, n))
    frames = [_ctx(dev, f * n, n) for f in range(F)]
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    nan_seen = False
    for to_srgb in (0, 1):
        for normalize in (1, 0):
            for spp in (0, 5):
                for n_fold in (4, 3, 1):
                    outs = []
                    for which in ("single", "group"):
                        image, depth = torch.full((H, W, 3), -7.0, device=DEV), torch.full((H, W), -7.0, device=DEV)
                        pos = torch.full((H, W, 3), -7.0, device=DEV) if identity else None
                        mean = old.clone()
                        if which == "single":
                            for f in range(n_fold):
                                B.check(B.lib.sdn_preview_finish(ctypes.byref(frames[f]), rH, rW, H, W, bg, B.ptr(bgr[f * n:(f + 1) * n]) if per_ray_bg else None,
                                                                 normalize, to_srgb, B.ptr(image), B.ptr(depth), B.ptr(pos), B.ptr(mean), spp + f,
                                                                 B.stream()), "preview_finish")
                        else:
                            B.check(B.lib.sdn_preview_finish_group(ctypes.byref(group), rH, rW, H, W, bg, B.ptr(bgr), normalize, to_srgb, B.ptr(image),
                                                                   B.ptr(depth), B.ptr(pos), B.ptr(mean), spp, n_fold, B.stream()), "preview_finish_group")
                        outs.append((mean, image, depth, pos))
                    torch.cuda.synchronize()
                    for name, a, b in zip(("accum", "image_out", "depth_out", "pos_out"), *outs):
                        if a is not None:
                            assert torch.equal(bits(a), bits(b)), (name, to_srgb, normalize, spp, n_fold)
                    assert torch.isfinite(outs[1][2]).all() and (outs[1][1] != -7.0).any()
                    if spp == 0 and n_fold == 1:
                        assert torch.equal(bits(outs[1][0]), bits(outs[1][1]))          # the mean of one frame is the frame
                    nan_seen = nan_seen or bool(torch.isnan(outs[1][0]).any())
    assert nan_seen                                               # the planted NaN reached the mean, alike on both sides
    # refusals: more frames to fold than the group holds, none, a one-frame context, another ray count per frame, no buffer to fold into
    image, depth = torch.empty(H, W, 3, device=DEV), torch.empty(H, W, device=DEV)
    call = lambda c, rh, nf, ac: B.lib.sdn_preview_finish_group(ctypes.byref(c), rh, rW, H, W, bg, None, 1, 0, B.ptr(image), B.ptr(depth), None,  # noqa: E731
                                                               B.ptr(ac), 0, nf, B.stream())
    assert call(group, rH, F + 1, old) == -1 and call(group, rH, 0, old) == -1 and call(frames[0], rH, 1, old) == -1
    assert call(group, rH + 1, 1, old) == -1 and call(group, rH, 1, None) == -1


# 4 --------------------------------------------------------------------------------------------------------------------
def test_accumulate_group_equals_accumulate(model_bits):
    """The same 8 noise vectors through `accumulate` (6 loops) and `accumulate_group(samples=4)` up to max_spp = 6 -- the second group
    renders 4 frames and folds 2: render_buffer bit-identical, spp == 6, image / depth those of the last folded frame; full at
    max_spp nothing is rendered.  Then at downscale 0.5 in linear colour, and with drawn noises after the same seed."""
    from dnerf_amd import scene
    from dnerf_amd.preview import PreviewRenderer
    import preview_support as PS
    model = model_bits[0]
    H, W = 36, 52
    pose, intr = scene.look_at_pose(30.0, 30.0), scene.intrinsics(H, W)
    field = _field(model, 0.5, True)
    one, grp = PreviewRenderer(model, field, W, H, DEV), PreviewRenderer(model, field, W, H, DEV)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    for down, space in ((1, "srgb"), (0.5, "linear")):
        n = int(H * down) * int(W * down)
        zs = torch.from_numpy(np.stack([PS.draw_noises(n, 100 + k) for k in range(8)])).to(DEV)
        kw = dict(downscale=down, color_space=space)
        for k in range(6):
            want = one.accumulate(pose, intr, 0.5, need_update=k == 0, max_spp=6, noises=zs[k], **kw)
        grp.accumulate_group(pose, intr, 0.5, need_update=True, max_spp=6, samples=4, noises=zs[:4], **kw)
        assert grp.spp == 4
        got = grp.accumulate_group(pose, intr, 0.5, max_spp=6, samples=4, noises=zs[4:], **kw)
        torch.cuda.synchronize()
        assert grp.spp == 6 == one.spp
        assert torch.equal(bits(got), bits(want)) and got is grp.render_buffer
        assert torch.equal(bits(grp.image), bits(one.image)) and torch.equal(bits(grp.depth), bits(one.depth))
        before = got.clone()
        assert torch.equal(grp.accumulate_group(pose, intr, 0.5, max_spp=6, samples=4, noises=zs[:4], **kw), before) and grp.spp == 6
    assert sorted(grp.group_loops) == [((H // 2) * (W // 2), 4), (H * W, 4)] and not grp.loops      # a cache of their own
    assert float((one.render_buffer - one.image).abs().max()) > 1e-4            # a mean of distinct frames
    torch.manual_seed(5)
    for k in range(4):
        want = one.accumulate(pose, intr, 0.5, need_update=k == 0)
    torch.manual_seed(5)
    got = grp.accumulate_group(pose, intr, 0.5, need_update=True, samples=4, return_pos=True)
    assert grp.spp == 4 and torch.equal(bits(got), bits(want))
    assert torch.equal(grp.pos, grp._refs[0].view(H, W, 3) + grp.depth[..., None] * grp._refs[1].view(H, W, 3))


# 5 --------------------------------------------------------------------------------------------------------------------
def test_group_with_a_bbox_mapper_and_the_edits_groups_refuse(model_bits):
    """The SealD teacher's preview (T_thresh 1e-4) of the bbox edit: the group's frames are the single frames' bit for bit.  The anchor
    mapper keeps raising `set_mapper`'s NotImplementedError, from the loop and from `accumulate_group`."""
    import seal_anchor_support as AS
    from dnerf_amd import scene
    from dnerf_amd.preview import PreviewRenderer
    from dnerf_amd.renderer import DeviceLoop
    from dnerf_amd.seal_mapper import SealAnchorMapper, SealBBoxMapper
    from test_caller_fixtures_cpu import SEAL_CONFIG
    model, bits = model_bits
    H, W, F = 50, 50, 3
    n = H * W
    keep = model.density_bitfield.clone()
    try:
        mapper = SealBBoxMapper(SEAL_CONFIG)
        filled = fill_bitfield_host(bits, mapper.map_data["force_fill_bound"].cpu().numpy())
        model.density_bitfield.copy_(torch.from_numpy(filled))
        sc, ro, rd = _rays(model_bits, H, W, 0.5)
        field = _field(model, sc.time, True)
        z = GS.noise_rows(F, n)
        refs = []
        for f in range(F):
            one = DeviceLoop(model, field, n, DEV, T_thresh=1e-4, mapper=mapper)
            one.render(ro, rd, sc.time, noises=torch.from_numpy(z[f]).to(DEV))
            refs.append({k: one.buf[k].clone() for k in ACCS})
        plain = DeviceLoop(model, field, n, DEV, T_thresh=1e-4)
        plain.render(ro, rd, sc.time, noises=torch.from_numpy(z[0]).to(DEV))
        assert not torch.equal(plain.buf["image"], refs[0]["image"])            # the edit is in the frame
        loop = DeviceLoop(model, field, F * n, DEV, T_thresh=1e-4, mapper=mapper, frames=F)
        loop.render_samples(ro, rd, sc.time, torch.from_numpy(z).to(DEV), want_stats=False)
        torch.cuda.synchronize()
        _assert_frames(loop, refs, n)
        anchor = SealAnchorMapper(AS.FRAME_CONFIG)
        with pytest.raises(NotImplementedError):
            DeviceLoop(model, field, 2 * n, DEV, T_thresh=1e-4, mapper=anchor, frames=2)
        pv = PreviewRenderer(model, field, W, H, DEV, mapper=anchor, T_thresh=1e-4)
        pose, intr = scene.look_at_pose(30.0, 30.0), scene.intrinsics(H, W)
        with pytest.raises(NotImplementedError):
            pv.accumulate_group(pose, intr, 0.5, need_update=True, samples=2)
        assert pv.spp == 0 and not pv.group_loops
        pv.set_mapper(mapper)                                                   # the bbox edit: previewed by groups
        pv.accumulate_group(pose, intr, 0.5, need_update=True, samples=2)
        assert pv.spp == 2 and list(pv.group_loops) == [(n, 2)]
        pv.set_mapper(anchor)                                                   # back to the anchor: the group loop is dropped, not kept half set
        assert not pv.group_loops
    finally:
        model.density_bitfield.copy_(keep)
