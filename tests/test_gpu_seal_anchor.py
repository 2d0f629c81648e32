"""The SealD anchor (control-point) seal mapper on the GPU: `sdn_seal_anchor_map` (csrc/seal.hip) against the torch restatement
of SealAnchorMapper.map_to_origin run on the CPU and against what the reference's own code produced
(tests/golden/caller_seald_anchor.npz, data only), its "does this call map anything" gate in both forms of a call, and the
reference teacher's frame through the three render paths.

Masks are compared outside an analytic margin of 1e-5 (float64) from the three predicate boundaries, which may exclude at most
0.5 % of the points (seal_anchor_support.clear_of_boundaries asserts the cap); mapped coordinates to 2e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import seal_anchor_support as AS  # noqa: E402
from caller_fixtures import fill_bitfield_host, fixture_model, fixture_scene  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(AS.FIXTURE)


def _check_against(cfg, pts, dirs, got_pts, got_dirs, got_mask, want_pts, want_mask, min_valid):
    """got_*: the kernel's in-place results (numpy); want_*: a reference evaluation of the same points."""
    clear = AS.clear_of_boundaries(cfg, pts)
    print(f"{pts.shape[0]} points: {int((~clear).sum())} within the margin, {int(want_mask.sum())} valid, "
          f"{int((got_mask != want_mask).sum())} mask mismatches in all, largest coordinate difference "
          f"{float(np.abs(got_pts - want_pts)[got_mask & want_mask].max()):.2e}")
    assert np.array_equal(got_mask[clear], want_mask[clear])
    assert int(want_mask.sum()) >= min_valid
    both = got_mask & want_mask
    np.testing.assert_allclose(got_pts[both], want_pts[both], rtol=0, atol=2e-6)
    assert np.array_equal(got_pts[~got_mask], pts[~got_mask])
    assert np.array_equal(got_dirs, dirs)


def test_kernel_matches_the_torch_restatement_on_the_cpu():
    from dnerf_amd.seal_mapper import SealAnchorMapper
    cfg = AS.POINTS_CONFIG
    pts = AS.draw_points(cfg, 50000, 100, seed=41)
    dirs = torch.nn.functional.normalize(torch.randn(50000, 3, generator=torch.Generator().manual_seed(42)), dim=-1).numpy()
    want_pts, _, want_mask = SealAnchorMapper(cfg)._map_to_origin_torch(torch.from_numpy(pts), torch.from_numpy(dirs))
    m = SealAnchorMapper(cfg)
    p, d = torch.from_numpy(pts).cuda(), torch.from_numpy(dirs).cuda()
    m.map_data_conversion(p)
    mask = m.map_to_origin_(p, d)
    _check_against(cfg, pts, dirs, p.cpu().numpy(), d.cpu().numpy(), mask.cpu().numpy(), want_pts.numpy(), want_mask.numpy(), 1000)
    # map_to_origin takes the same kernel on copies
    q = torch.from_numpy(pts).cuda()
    q2, d2, mask2 = m.map_to_origin(q, d)
    assert torch.equal(q2, p) and torch.equal(mask2, mask) and torch.equal(q, torch.from_numpy(pts).cuda()) and q2.data_ptr() != q.data_ptr()


@pytest.mark.parametrize("name", ["hsv", "rgb"])
def test_kernels_reproduce_the_reference_fixture(fx, name):
    from dnerf_amd.seal_mapper import SealAnchorMapper
    cfg = AS.POINTS_CONFIG_HSV if name == "hsv" else AS.POINTS_CONFIG_RGB
    m = SealAnchorMapper(cfg)
    p, d = torch.from_numpy(fx["pts"]).cuda(), torch.from_numpy(fx["dirs"]).cuda()
    m.map_data_conversion(p)
    mask = m.map_to_origin_(p, d)
    _check_against(cfg, fx["pts"], fx["dirs"], p.cpu().numpy(), d.cpu().numpy(), mask.cpu().numpy(), fx["points"], fx["mask"], 100)
    want = torch.from_numpy(fx["mask"]).cuda()
    cols_in = torch.zeros(p.shape[0], 3, device="cuda")
    cols_in[want] = torch.from_numpy(fx["colors_in"]).cuda()
    got = m.map_color_(cols_in.clone(), want)
    # (the rgb tint's mean brightness is summed in fixed point here, by torch.mean there: 5e-6, the bar of the bbox kernels' test)
    np.testing.assert_allclose(got.cpu().numpy()[fx["mask"]], fx[f"colors_out_{name}"], rtol=0, atol=5e-6 if name == "rgb" else 2e-6)
    assert torch.equal(got[~want], cols_in[~want])
    # the early return: a set wholly outside the box comes back untouched
    far = torch.from_numpy(fx["far_pts"]).cuda()
    mask = m.map_to_origin_(far, d)
    assert not bool(mask.any()) and np.array_equal(far.cpu().numpy(), fx["far_points"])


def _zero_y_config():
    """POINTS_CONFIG moved so that the anchor has y == 0: points with a zero y (empty-slot-like: they fail the box test's
    `points.all(1)`) then lie inside the cone."""
    y = AS.anchor_geometry(AS.POINTS_CONFIG)["v_anchor"][1]
    return dict(AS.POINTS_CONFIG, raw=[[p[0], p[1] - y, p[2]] for p in AS.POINTS_CONFIG["raw"]])


def _gate_inputs():
    cfg = _zero_y_config()
    g = AS.anchor_geometry(cfg)
    rng = np.random.default_rng(51)
    cand = (g["v_anchor"] + rng.uniform(-0.1, 0.1, (4000, 3))).astype(np.float32)
    cand[:, 1] = 0.0
    valid, margin = AS.predicates64(cfg, cand)
    cone = cand[valid & (margin > AS.MARGIN)][:300]
    assert cone.shape[0] >= 50
    far = (g["v_anchor"] + np.array([0.9, -0.8, 0.85]) + rng.uniform(-0.2, 0.2, (700, 3))).astype(np.float32)
    inbox = (g["v_anchor"] + 0.5 * np.asarray(cfg["translation"]))[None].astype(np.float32)     # on the cone's axis: in the box and valid
    return cfg, cone, far, inbox


def test_gate_is_the_whole_calls():
    """Zero-coordinate points never count as inside the box, but are candidates for the cone like any other point: alone with far
    points they come back untouched; one in-box point in the call and they are mapped."""
    from dnerf_amd.seal_mapper import SealAnchorMapper
    cfg, cone, far, inbox = _gate_inputs()
    m = SealAnchorMapper(cfg)
    buf = np.concatenate([cone, far])
    p = torch.from_numpy(buf).cuda()
    d = torch.zeros_like(p)
    m.map_data_conversion(p)
    mask = m.map_to_origin_(p, d)
    assert not bool(mask.any()) and np.array_equal(p.cpu().numpy(), buf)
    buf1 = np.concatenate([cone, far, inbox])
    p = torch.from_numpy(buf1).cuda()
    mask = m.map_to_origin_(p, torch.zeros_like(p)).cpu().numpy()
    want_pts, _, want_mask = SealAnchorMapper(cfg)._map_to_origin_torch(torch.from_numpy(buf1), None)
    want_mask = want_mask.numpy()
    assert want_mask[:cone.shape[0]].all() and not want_mask[cone.shape[0]:-1].any() and want_mask[-1]
    assert np.array_equal(mask, want_mask)
    np.testing.assert_allclose(p.cpu().numpy(), want_pts.numpy(), rtol=0, atol=2e-6)
    # ... and a later call without the in-box point is gated again (tags only grow: the raised flag word is not this call's)
    p = torch.from_numpy(buf).cuda()
    assert not bool(m.map_to_origin_(p, torch.zeros_like(p)).any()) and np.array_equal(p.cpu().numpy(), buf)


def test_live_list_form_ignores_stale_slots():
    """The device loop's form of a call: its samples are the slots of a live list.  Stale in-box slots beyond the live ones do not
    open the gate; a listed one does, and then every slot is tested."""
    from dnerf_amd.seal_mapper import SealAnchorMapper
    from sdn_backend import lib, check, ptr, stream
    cfg, cone, far, inbox = _gate_inputs()
    m = SealAnchorMapper(cfg)
    stale = np.repeat(inbox, 40, axis=0)
    buf = np.concatenate([far, cone, stale])                       # slots: far | zero-y cone points | stale in-box
    n_far, n_cone = far.shape[0], cone.shape[0]
    flag = torch.zeros(4, dtype=torch.uint8, device="cuda")

    def run(listed):
        p = torch.from_numpy(buf).cuda()
        a = m._native_args(p.device)
        live = torch.zeros(buf.shape[0], dtype=torch.int32, device="cuda")
        live[:len(listed)] = torch.tensor(listed, dtype=torch.int32)
        count = torch.tensor([len(listed)], dtype=torch.int32, device="cuda")
        mask = torch.full((buf.shape[0],), 7, dtype=torch.uint8, device="cuda")
        check(lib.sdn_seal_anchor_map(ptr(p), None, buf.shape[0], a["bounds"], a["n_bounds"], ptr(a["tris"]), a["n_tris"], a["test_dir"],
                                      a["v_anchor"], a["v_offset"], a["v_h"], a["len_h"], a["radius"], a["scale"], flag.data_ptr(), ptr(mask),
                                      ptr(live), ptr(count), None, stream()), "seal_anchor_map")
        return p.cpu().numpy(), mask.cpu().numpy()

    listed = list(range(n_far + n_cone))                            # every slot but the stale ones
    p, mask = run(listed)
    assert not mask.any() and np.array_equal(p, buf)
    p, mask = run(listed + [n_far + n_cone + 3])
    assert mask[n_far:].all() and not mask[:n_far].any()            # the cone points AND every stale slot: step 2 runs over all slots
    assert not np.array_equal(p[n_far:], buf[n_far:]) and np.array_equal(p[:n_far], buf[:n_far])


@pytest.fixture(scope="module")
def model_bits():
    return fixture_model("cuda")


def test_teacher_frame_through_the_three_render_paths(fx, model_bits):
    """The reference teacher's frame with the anchor mapper (64 x 64, time 0.5, T_thresh 1e-4, force_fill_bound marked occupied):
    the host-stepped loop on the fp32 operators reproduces it with the bars of the `caller_seald` test (trace exact, image and
    weights_sum 1e-4, raw depth 1e-3 on hit pixels); the host-stepped loop with the fused -O field and the device loop run the same
    kernels on the same samples and agree bit for bit; the small-batch renderer gives the device loop's image bit for bit, its depth to
    1e-5; the -O image against the reference's fp32 one within that test's distribution bars.  A frame group refuses the mapper."""
    from dnerf_amd.fused import FusedField
    from dnerf_amd.renderer import DeviceLoop, RayBatchRenderer, render_frame
    from dnerf_amd.seal_mapper import SealAnchorMapper
    from tests_support import assert_dist
    model, bits = model_bits
    sc = fixture_scene("cuda", model_bits=model_bits)
    keep = model.density_bitfield.clone()
    try:
        mapper = SealAnchorMapper(AS.FRAME_CONFIG)
        filled = fill_bitfield_host(bits, mapper.map_data["force_fill_bound"].cpu().numpy())
        model.density_bitfield.copy_(torch.from_numpy(filled))
        out = render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=False, T_thresh=1e-4, mapper=mapper)
        assert fx["frame_trace"].tolist() == [list(r) for r in out["trace"]]
        np.testing.assert_allclose(out["image"].cpu().numpy(), fx["frame_image"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(out["weights_sum"].cpu().numpy(), fx["frame_weights_sum"], rtol=0, atol=1e-4)
        raw_depth = out["depth"] * (out["fars"] - out["nears"]) + out["nears"]      # the teacher returns the un-normalised depth
        hit = (fx["frame_weights_sum"] > 0.5) & (fx["frame_depth"] > out["nears"].cpu().numpy() + 1e-3)
        assert hit.sum() > 200
        np.testing.assert_allclose(raw_depth.cpu().numpy()[hit], fx["frame_depth"][hit], rtol=1e-3, atol=1e-3)
        assert (np.abs(out["image"].cpu().numpy() - fx["frame_plain_image"]).max(1) > 1e-3).sum() >= 100
        field = FusedField(sc.model, sc.time)
        host = render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=True, field=field, T_thresh=1e-4, mapper=mapper)
        loop = DeviceLoop(sc.model, field, sc.rays_o.shape[0], "cuda", T_thresh=1e-4, mapper=mapper)
        fast = loop.render(sc.rays_o, sc.rays_d, sc.time)
        torch.cuda.synchronize()
        assert torch.equal(host["image"], fast["image"]) and host["n_samples"] == fast["n_samples"]
        again = loop.render(sc.rays_o, sc.rays_d, sc.time)
        assert torch.equal(again["image"], fast["image"])
        print("anchor frame, -O device loop vs reference teacher (fp32):",
              assert_dist(fast["image"].cpu().numpy(), fx["frame_image"], "anchor-mapped image, -O device loop vs SealDNeRF teacher run_cuda (fp32)",
                          max=4e-3, p999=1e-3, mean=2e-5, frac_above_1e3=2e-3))
        assert abs(len(fast["trace"]) - len(fx["frame_trace"])) <= 1
        once = RayBatchRenderer(sc.model, FusedField(sc.model, sc.time), sc.rays_o.shape[0], "cuda", T_thresh=1e-4, mapper=mapper, samples_per_ray=160)
        got = once.render(sc.rays_o, sc.rays_d, sc.time, bg_color=1.0, check=True)
        torch.cuda.synchronize()
        assert torch.equal(got["image"], fast["image"]), float((got["image"] - fast["image"]).abs().max())
        d0, d1 = got["depth"], fast["depth"]
        assert torch.equal(torch.isnan(d0), torch.isnan(d1))
        assert float((torch.nan_to_num(d0) - torch.nan_to_num(d1)).abs().max()) < 1e-5
        with pytest.raises(NotImplementedError):
            DeviceLoop(sc.model, field, 2 * sc.rays_o.shape[0], "cuda", T_thresh=1e-4, mapper=mapper, frames=2)
    finally:
        model.density_bitfield.copy_(keep)
