"""Preview frames on the GPU: the perturbed first march in the native loops (`SdnRenderCtx.noises`, `DeviceLoop.render(noises=)`,
`render_frame(noises=)`), the one-launch finishing pass `sdn_preview_finish`, and `PreviewRenderer` (frame + running mean), against
tests/golden/caller_preview.npz -- the reference's own `run_cuda(perturb=True)` -- and the restatements of tests/preview_support.py.

Bars.  Indices, traces and sample counts: exact wherever both sides evaluate the field in the same precision (the fp32 field against
the fp32 fixture / oracle; the -O loop against the -O reference-shaped loop, which run the same kernel).  The -O loop against the
FP32 fixture keeps the bars tests/test_gpu_caller_fixtures.py states for that pairing: an fp16 network moves early-termination ties, so
the first trace row is exact, the length within 1 and the counts within 3."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import preview_support as PS  # noqa: E402
from caller_fixtures import fill_bitfield_host, fixture_model, fixture_scene  # noqa: E402
from tests_support import assert_dist  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def model_bits():
    return fixture_model(DEV)


@pytest.fixture(scope="module")
def fx():
    return PS.load()


def _tr(out):
    return [tuple(r) for r in out["trace"]]


def _cmp_fp32(out, fx):
    assert [tuple(r) for r in fx["trace"].tolist()] == _tr(out)
    assert out["n_samples"] == int(fx["n_samples"])
    img, dep, ws = out["image"].cpu().numpy(), out["depth"].cpu().numpy(), out["weights_sum"].cpu().numpy()
    np.testing.assert_allclose(ws, fx["weights_sum"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(img, fx["image"], rtol=0, atol=1e-4)
    miss = np.isnan(fx["depth"])
    assert np.array_equal(miss, np.isnan(dep))
    np.testing.assert_allclose(dep[~miss], fx["depth"][~miss], rtol=0, atol=1e-4)


# 1 --------------------------------------------------------------------------------------------------------------------
def test_noises_reach_the_first_march_of_the_native_loops(model_bits, fx):
    """The fixture's offsets through `DeviceLoop.render(noises=)` (culled start + certified jump from the perturbed start) and the
    host-stepped `render_frame(noises=)`."""
    from dnerf_amd.fused import FusedField
    from dnerf_amd.fused_f32 import FusedFieldF32
    from dnerf_amd.renderer import DeviceLoop, render_frame
    sc = fixture_scene(DEV, model_bits=model_bits)
    z = torch.from_numpy(fx["noises"]).to(DEV)
    N = sc.rays_o.shape[0]
    # fp32 field in the device loop, fp32 op-by-op network and fp32 fused field in the host-stepped loop: exact trace and count, 1e-4
    _cmp_fp32(DeviceLoop(sc.model, FusedFieldF32(sc.model, sc.time), N, DEV).render(sc.rays_o, sc.rays_d, sc.time, noises=z), fx)
    _cmp_fp32(render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=False, noises=z), fx)
    _cmp_fp32(render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=False, field=FusedFieldF32(sc.model, sc.time), noises=z), fx)
    # -O: the product path, at fp16 distance from the fp32 fixture (bars of test_native_device_loop_f16_reproduces_reference_run_cuda)
    field = FusedField(sc.model, sc.time)
    fast = DeviceLoop(sc.model, field, N, DEV).render(sc.rays_o, sc.rays_d, sc.time, noises=z)
    host = render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=True, field=field, noises=z)
    assert _tr(fast) == _tr(host) and fast["n_samples"] == host["n_samples"]            # same kernel on both sides: exact
    assert torch.equal(fast["image"], host["image"])
    ref_tr, tr = fx["trace"], np.array(fast["trace"])
    assert tuple(tr[0]) == tuple(ref_tr[0]) and abs(len(tr) - len(ref_tr)) <= 1
    assert np.abs(tr[:len(ref_tr), 0] - ref_tr[:len(tr), 0]).max() <= 3
    print("perturbed -O device loop vs reference run_cuda(perturb=True) (fp32):",
          assert_dist(fast["image"].cpu().numpy(), fx["image"], "image, perturbed -O device loop vs the reference's fp32 render",
                      max=2e-3, p999=5e-4, p99=2.5e-4, mean=1e-5, frac_above_1e3=5e-4))
    # the jitter took effect: the unperturbed frame differs
    plain = DeviceLoop(sc.model, field, N, DEV).render(sc.rays_o, sc.rays_d, sc.time)
    assert plain["n_samples"] != fast["n_samples"] or not torch.equal(plain["image"], fast["image"])


def _scene(model_bits, H, W):
    return fixture_scene(DEV, model_bits=model_bits, H=H, W=W)


SIZES = [(64, 64), (5, 7), (1, 1)]


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_zero_noises_are_bit_identical_to_no_noises(model_bits, H, W):
    from dnerf_amd.fused import FusedField
    from dnerf_amd.renderer import DeviceLoop, render_frame
    sc = _scene(model_bits, H, W)
    N = H * W
    field = FusedField(sc.model, sc.time)
    loop = DeviceLoop(sc.model, field, N, DEV)
    a = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in loop.render(sc.rays_o, sc.rays_d, sc.time).items()}
    b = loop.render(sc.rays_o, sc.rays_d, sc.time, noises=torch.zeros(N, device=DEV))
    assert _tr(a) == _tr(b) and a["n_samples"] == b["n_samples"]
    for k in ("image", "weights_sum"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(torch.nan_to_num(a["depth"]), torch.nan_to_num(b["depth"]))
    h0 = render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=True, field=field)
    h1 = render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=True, field=field, noises=torch.zeros(N, device=DEV))
    assert _tr(h0) == _tr(h1) and torch.equal(h0["image"], h1["image"])


# 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_certified_jump_from_a_perturbed_start_changes_nothing(model_bits, H, W):
    """H = 128, C = 1, bound = 1 (the fixture model): a context with the per-ray t_end cache runs the culled start and jumps each ray
    to a certified later point of the lattice that starts at its PERTURBED parameter; a context without it marches all N rays from
    there.  Same noises -> bit-identical image, depth, weights_sum, identical traces and counts.  Rays that miss the box, noise 0 and
    the largest float below 1 are among the rays."""
    from dnerf_amd.fused import FusedField
    from dnerf_amd.renderer import DeviceLoop
    sc = _scene(model_bits, H, W)
    assert sc.model.grid_size == 128 and sc.model.cascade == 1 and sc.model.bound == 1
    ro, rd = sc.rays_o.clone(), sc.rays_d.clone()
    N = H * W
    z = PS.draw_noises(N, 3)
    if N >= 35:                                   # rays that miss the box: origin outside, looking away
        ro[-3:] = torch.tensor([3.0, 3.0, 3.0], device=DEV)
        rd[-3:] = torch.tensor([0.0, 1.0, 0.0], device=DEV)
        z[N // 2], z[N // 2 + 1] = 0.0, PS.ONE_BELOW      # on rays through the middle of the frame: they hit the figure
    else:
        z[0] = PS.ONE_BELOW
    z = torch.from_numpy(z).to(DEV)
    field = FusedField(sc.model, sc.time)
    culled = DeviceLoop(sc.model, field, N, DEV)
    plain = DeviceLoop(sc.model, field, N, DEV)
    plain.ctx.rays_tend = None                    # no t_end cache: no culled start, no jump
    a = culled.render(ro, rd, sc.time, noises=z)
    b = plain.render(ro, rd, sc.time, noises=z)
    assert _tr(a) == _tr(b) and a["n_samples"] == b["n_samples"]
    if N >= 35:
        assert a["n_samples"] > 0
    for k in ("image", "weights_sum"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(torch.isnan(a["depth"]), torch.isnan(b["depth"]))
    assert torch.equal(torch.nan_to_num(a["depth"]), torch.nan_to_num(b["depth"]))
    assert torch.equal(culled.buf["depth"], plain.buf["depth"])           # the raw accumulators too


# 4 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True])
def test_seeded_perturb_agrees_with_the_op_by_op_run_cuda(model_bits, monkeypatch, fp16):
    """After `torch.manual_seed(s)` the reference-shaped loop on the drop-in operators (`march_rays(perturb=True)` draws torch.rand(N) for
    iteration 0) and `DeviceLoop.render(perturb=True)` jitter every ray alike: same trace, same sample counts, images within the
    bars of test 1 (fp32: 1e-4 between the op-by-op network and the fused fp32 field; -O: both sides run the fused fp16 kernel)."""
    import raymarching
    from dnerf_amd.fused import FusedField
    from dnerf_amd.fused_f32 import FusedFieldF32
    from dnerf_amd.renderer import DeviceLoop
    sc = _scene(model_bits, 64, 64)
    sc.model.eval()
    N = 64 * 64
    calls = []
    inner = raymarching.march_rays

    def spy(n_alive, n_step, *a, **k):
        r = inner(n_alive, n_step, *a, **k)
        calls.append((int(n_alive), int(n_step), r[2]))
        return r
    monkeypatch.setattr(raymarching, "march_rays", spy)
    torch.manual_seed(1234)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
        ref = sc.model.render(sc.rays_o[None], sc.rays_d[None], sc.time, staged=False, perturb=True, bg_color=None)
    monkeypatch.setattr(raymarching, "march_rays", inner)
    ref_trace = [(a, s) for a, s, _ in calls]
    ref_samples = sum(int((d[: a * s, 0] > 0).sum()) for a, s, d in calls)
    field = FusedField(sc.model, sc.time) if fp16 else FusedFieldF32(sc.model, sc.time)
    torch.manual_seed(1234)
    out = DeviceLoop(sc.model, field, N, DEV).render(sc.rays_o, sc.rays_d, sc.time, perturb=True)
    assert [(a, s) for a, s, _ in out["trace"]] == ref_trace and out["n_samples"] == ref_samples
    np.testing.assert_allclose(out["image"].cpu().numpy(), ref["image"][0].float().cpu().numpy(), rtol=0, atol=1e-4)
    torch.manual_seed(4321)                       # another seed, another frame
    other = DeviceLoop(sc.model, field, N, DEV).render(sc.rays_o, sc.rays_d, sc.time, perturb=True)
    assert other["n_samples"] != out["n_samples"] or not torch.equal(other["image"], out["image"])


# 5 --------------------------------------------------------------------------------------------------------------------
def _fake_frame(rH, rW, seed):
    """Loop accumulators of rH x rW rays as a finished loop would leave them, with NaN / inf depths among them."""
    rng = np.random.default_rng(seed)
    n = rH * rW
    acc = dict(image=(rng.random((n, 3), dtype=np.float32) * np.float32(0.6)), weights_sum=rng.random(n, dtype=np.float32),
               depth=(rng.random(n, dtype=np.float32) * np.float32(2.0)), nears=(np.float32(0.2) + rng.random(n, dtype=np.float32) * np.float32(0.3)),
               rays_o=rng.standard_normal((n, 3)).astype(np.float32), rays_d=rng.standard_normal((n, 3)).astype(np.float32))
    acc["fars"] = (acc["nears"] + np.float32(0.5) + rng.random(n, dtype=np.float32)).astype(np.float32)
    acc["image"][:: 5] *= np.float32(0.004)          # dark pixels: both sides of the sRGB edge with a dark background
    special = [np.nan, np.inf, -np.inf]
    for k, v in enumerate(special[: n]):
        acc["depth"][(k * 7) % n] = v
    if n > 8:
        acc["fars"][8] = acc["nears"][8]                # a ray that misses the box: 0 / 0
        acc["depth"][8] = 0
    return acc


def _run_finish(acc, rH, rW, H, W, bg, bg_rays, normalize, to_srgb, pos, accum, spp):
    import sdn_backend as B
    dev = {k: torch.from_numpy(v).to(DEV).contiguous() for k, v in acc.items()}
    c = B.SdnRenderCtx()
    for k, v in dev.items():
        setattr(c, k, v.data_ptr())
    c.N = rH * rW
    image = torch.full((H, W, 3), -7.0, device=DEV)
    depth = torch.full((H, W), -7.0, device=DEV)
    pos_t = torch.full((H, W, 3), -7.0, device=DEV) if pos else None
    acc_t = torch.from_numpy(accum).to(DEV).contiguous() if accum is not None else None
    bgr = torch.from_numpy(bg_rays).to(DEV).contiguous() if bg_rays is not None else None
    B.check(B.lib.sdn_preview_finish(ctypes.byref(c), rH, rW, H, W, (ctypes.c_float * 3)(*bg), B.ptr(bgr), int(normalize), int(to_srgb),
                                     B.ptr(image), B.ptr(depth), B.ptr(pos_t), B.ptr(acc_t), int(spp), B.stream()), "preview_finish")
    torch.cuda.synchronize()
    g = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return g(image), g(depth), g(pos_t), g(acc_t)


@pytest.mark.parametrize("rH,rW,H,W", [PS.NEAREST_CASE, (5, 7, 5, 7), (1, 1, 1, 1), (37, 53, 18, 26)])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("per_ray_bg", [False, True])
def test_preview_finish_against_the_numpy_restatement(fx, rH, rW, H, W, normalize, per_ray_bg):
    """Bars.  The source index, depth, position and the LINEAR colour are fp32 expressions the restatement rounds step by step like the
    kernel (the library is built without contraction): exact (the issue allows 1e-6 on the colour; none is needed).  sRGB: the
    kernel's powf is not correctly rounded -- its result enters 1.055 p - 0.055 with two more roundings -- so the pow term recovered
    from the output, (out + 0.055) / 1.055, is held within 4e-7 relative of the float64 pow (about 3 ulp: <= 1-2 ulp of powf plus the
    two roundings measured against 1.055 p), and the output itself within 1e-6 absolute of the float64 restatement rounded to fp32.
    The running mean is three fp32 operations rounded like numpy's: exact given the same colour, so it is compared on the linear path
    exactly and on the sRGB path within 1e-6."""
    acc = _fake_frame(rH, rW, seed=rH * 100 + rW)
    n = rH * rW
    rng = np.random.default_rng(9)
    bg = (0.001, 0.5, 1.0)                                  # three components, one dark enough to land below the sRGB edge
    bg_rays = rng.random((n, 3), dtype=np.float32) if per_ray_bg else None
    identity = (rH, rW) == (H, W)
    old = rng.random((H, W, 3), dtype=np.float32)
    # the index rule on its own: every ray carries its own index as colour
    idx_acc = dict(acc, image=np.repeat(np.arange(n, dtype=np.float32)[:, None], 3, 1), weights_sum=np.ones(n, np.float32))
    img, _, _, _ = _run_finish(idx_acc, rH, rW, H, W, bg, None, False, False, False, None, 0)
    want_idx = PS.source_index(rH, rW, H, W)
    assert np.array_equal(img[..., 0].astype(np.int64), want_idx)
    if (rH, rW, H, W) == PS.NEAREST_CASE:
        assert np.array_equal(want_idx, fx["nearest_index"])                 # ... and it is torch's
    for to_srgb in (False, True):
        for spp in (0, 5):
            ref = PS.finish_numpy(acc, rH, rW, H, W, bg=bg, bg_rays=bg_rays, normalize=normalize, to_srgb=to_srgb, pos=identity, accum=old, spp=spp)
            img, dep, pos, mean = _run_finish(acc, rH, rW, H, W, bg, bg_rays, normalize, to_srgb, identity, old, spp)
            assert np.isfinite(dep).all() and np.array_equal(dep, ref["depth"])
            if identity:
                assert np.array_equal(pos, ref["pos"])
            if not to_srgb:
                assert np.array_equal(img, ref["image"]) and np.array_equal(mean, ref["accum"])
                continue
            lin = ref["linear"]
            below = lin < np.float32(PS.SRGB_EDGE)
            assert np.abs(img - ref["image"]).max() <= 1e-6
            assert np.array_equal(img[below], np.float32(12.92) * lin[below])    # the linear branch: one fp32 multiplication, exact
            if (~below).any():
                p_got = (img[~below].astype(np.float64) + 0.055) / 1.055
                p_ref = np.power(lin[~below].astype(np.float64), 0.41666)
                rel = np.abs(p_got / p_ref - 1).max()
                print(f"sRGB pow term, {rH}x{rW}->{H}x{W}: max relative distance to float64 {rel:.2e}")
                assert rel <= 4e-7
            assert np.abs(mean - ref["accum"]).max() <= 1e-6
    if n > 8 and not per_ray_bg:
        assert below.any() and (~below).any()


def test_preview_finish_pos_needs_one_ray_per_pixel():
    import sdn_backend as B
    acc = _fake_frame(18, 26, 1)
    with pytest.raises(B.SdnError):
        _run_finish(acc, 18, 26, 37, 53, (1, 1, 1), None, True, False, True, None, 0)


# 6 --------------------------------------------------------------------------------------------------------------------
def test_preview_renderer_frame_and_running_mean(model_bits):
    """`PreviewRenderer.frame` is the loop + finishing pass on the window's rays (against `DeviceLoop.render` + the restatement), at
    downscale 1 and 0.5; `accumulate` over 8 frames with 8 distinct noise vectors against the float64 mean of the 8 individually
    finished frames.  Bar 8 * 2^-22: each step of the fp32 recurrence rounds three times on values <= 1 after the divide, the error of
    step k is damped by k / (k + 1), so after k frames the bound is about k * 2^-23; the bar is twice that.  `need_update=True` then
    restarts from the next frame alone, bit-identical to `frame()`."""
    from dnerf_amd import scene
    from dnerf_amd.fused import FusedField
    from dnerf_amd.preview import PreviewRenderer
    from dnerf_amd.renderer import DeviceLoop
    from dnerf_amd.utils import get_rays
    model = model_bits[0]
    H, W = 36, 52
    pose, intr = scene.look_at_pose(30.0, 30.0), scene.intrinsics(H, W)
    field = FusedField(model, 0.5)
    pv = PreviewRenderer(model, field, W, H, DEV)
    t = torch.tensor([[0.5]], device=DEV)
    for down, lin in ((1, False), (0.5, True)):
        rH, rW = int(H * down), int(W * down)
        z = torch.from_numpy(PS.draw_noises(rH * rW, 11)).to(DEV)
        out = pv.frame(pose, intr, 0.5, downscale=down, noises=z, return_pos=down == 1, color_space="linear" if lin else "srgb")
        rays = get_rays(torch.from_numpy(pose).to(DEV)[None], intr * down, rH, rW, -1)
        ro, rd = rays["rays_o"][0].contiguous(), rays["rays_d"][0].contiguous()
        loop = DeviceLoop(model, field, rH * rW, DEV)
        ref = loop.render(ro, rd, t, noises=z)
        assert ref["n_samples"] > 100
        acc = {k: loop.buf[k].cpu().numpy() for k in ("image", "weights_sum", "depth", "nears", "fars")}
        acc.update(rays_o=ro.cpu().numpy(), rays_d=rd.cpu().numpy())
        want = PS.finish_numpy(acc, rH, rW, H, W, to_srgb=lin, pos=down == 1)
        assert np.array_equal(out["depth"].cpu().numpy(), want["depth"])
        if lin:
            assert np.abs(out["image"].cpu().numpy() - want["image"]).max() <= 1e-6
        else:
            assert np.array_equal(out["image"].cpu().numpy(), want["image"])
            assert np.array_equal(out["pos"].cpu().numpy(), want["pos"])
            # unnormalised in the loop's own finish: the same frame
            assert torch.equal(out["image"].view(-1, 3), ref["image"])
    assert sorted(pv.loops) == [(H // 2) * (W // 2), H * W]                # one loop per distinct ray count, kept
    # the running mean
    zs = [torch.from_numpy(PS.draw_noises(H * W, 100 + k)).to(DEV) for k in range(8)]
    singles = [pv.frame(pose, intr, 0.5, noises=z)["image"].double().cpu().numpy() for z in zs]
    assert np.abs(singles[0] - singles[1]).max() > 1e-4                   # distinct jitter, distinct frames
    for k, z in enumerate(zs):
        mean = pv.accumulate(pose, intr, 0.5, need_update=k == 0, noises=z)
    assert pv.spp == 8
    err = np.abs(mean.double().cpu().numpy() - np.mean(singles, axis=0)).max()
    print(f"running mean of 8 frames vs the float64 mean: {err:.2e} (bar {8 * 2.0 ** -22:.2e})")
    assert err <= 8 * 2.0 ** -22
    again = pv.accumulate(pose, intr, 0.5, need_update=True, noises=zs[3])
    assert pv.spp == 1 and np.array_equal(again.double().cpu().numpy(), singles[3])
    # max_spp: the mean stops taking frames
    pv.spp = 64
    before = pv.render_buffer.clone()
    assert torch.equal(pv.accumulate(pose, intr, 0.5), before) and pv.spp == 64
    # spp truthy without noises draws them (seeded like the op-by-op path): two seeds, two frames; spp = 0: the unperturbed frame
    torch.manual_seed(1)
    a = pv.frame(pose, intr, 0.5, spp=1)["image"].clone()
    torch.manual_seed(2)
    b = pv.frame(pose, intr, 0.5, spp=1)["image"].clone()
    torch.manual_seed(1)
    assert torch.equal(pv.frame(pose, intr, 0.5, spp=1)["image"], a) and not torch.equal(a, b)
    plain = pv.frame(pose, intr, 0.5, spp=0)["image"].clone()
    rays = get_rays(torch.from_numpy(pose).to(DEV)[None], intr, H, W, -1)
    ro, rd = rays["rays_o"][0].contiguous(), rays["rays_d"][0].contiguous()
    assert torch.equal(plain.view(-1, 3), DeviceLoop(model, field, H * W, DEV).render(ro, rd, t)["image"])


# 7 --------------------------------------------------------------------------------------------------------------------
def test_edit_preview_with_the_bbox_mapper(model_bits):
    """The SealD teacher's preview (T_thresh 1e-4, raw depth) of caller_seald's bbox edit with a perturbed first march: the native loops
    against the oracle loop restatement with the same mapper and noises.  fp32 field: trace exact, image 1e-4; -O: the teacher's
    bars of test_seald_teacher_native_loop_reproduces_reference."""
    from dnerf_amd.fused import FusedField
    from dnerf_amd.fused_f32 import FusedFieldF32
    from dnerf_amd.renderer import DeviceLoop
    from dnerf_amd.seal_mapper import SealBBoxMapper
    from test_caller_fixtures_cpu import SEAL_CONFIG
    model, bits = model_bits
    sc = fixture_scene(DEV, model_bits=model_bits)
    keep = model.density_bitfield.clone()
    try:
        cpu_mapper = SealBBoxMapper(SEAL_CONFIG)
        filled = fill_bitfield_host(bits, cpu_mapper.map_data["force_fill_bound"].cpu().numpy())
        model.density_bitfield.copy_(torch.from_numpy(filled))
        z = PS.draw_noises(sc.rays_o.shape[0], 21)
        cpu_sc = fixture_scene("cpu", model_bits=(fixture_model("cpu", check=False)[0], filled))       # (its bitfield: the filled slice)
        want = PS.render_loop_oracle(cpu_sc, noises=z, T_thresh=1e-4, normalize_depth=False, mapper=cpu_mapper)
        plain = PS.render_loop_oracle(cpu_sc, noises=None, T_thresh=1e-4, normalize_depth=False, mapper=cpu_mapper)
        assert np.abs(plain["image"] - want["image"]).max() > 1e-4
        zt = torch.from_numpy(z).to(DEV)
        N = sc.rays_o.shape[0]
        mapper = SealBBoxMapper(SEAL_CONFIG)
        out = DeviceLoop(sc.model, FusedFieldF32(sc.model, sc.time), N, DEV, T_thresh=1e-4, mapper=mapper).render(sc.rays_o, sc.rays_d, sc.time, noises=zt)
        assert _tr(out) == [tuple(r) for r in want["trace"]] and out["n_samples"] == want["n_samples"]
        np.testing.assert_allclose(out["image"].cpu().numpy(), want["image"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(out["weights_sum"].cpu().numpy(), want["weights_sum"], rtol=0, atol=1e-4)
        fast = DeviceLoop(sc.model, FusedField(sc.model, sc.time), N, DEV, T_thresh=1e-4, mapper=mapper).render(sc.rays_o, sc.rays_d, sc.time, noises=zt)
        print("perturbed seald frame, -O device loop vs the oracle teacher loop (fp32):",
              assert_dist(fast["image"].cpu().numpy(), want["image"], "mapped image, perturbed -O device loop vs the fp32 teacher loop",
                          max=4e-3, p999=1e-3, mean=2e-5, frac_above_1e3=2e-3))
        assert abs(len(fast["trace"]) - len(want["trace"])) <= 1 and tuple(fast["trace"][0]) == tuple(want["trace"][0])
    finally:
        model.density_bitfield.copy_(keep)
