"""The SealD brush seal mapper on the GPU: `sdn_seal_brush_map` (csrc/seal.hip) against the float64 restatement, the torch
restatement of SealBrushMapper.map_to_origin run on the CPU and what the reference's own code produced
(tests/golden/caller_seald_brush.npz, data only); the edges of its triangle chunks and of the border list; the reference teacher's
frame through the three render paths, and a frame group.

Masks are compared on the clear points: those on which map_mask in float64 is the same with every threshold (t, u, v >= 0, u + v
<= 1, the AABB sides) moved in and moved out by 1e-5; at most 0.5 % of a set may be unclear (the fixture's sets: 0 of 6000 each).
Mapped coordinates: 2e-6 against float64; ref_fp32_error + 2e-6 against the reference's fp32 outputs, whose cdist takes the
matrix-product form (ref_fp32_error, stored in the fixture, is the reference's own distance from float64: 2.6e-6 / 2.1e-6)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import seal_brush_support as BS  # noqa: E402
from caller_fixtures import fill_bitfield_host, fixture_model, fixture_scene  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(BS.FIXTURE)


@pytest.mark.parametrize("name", list(BS.POINT_CONFIGS))
def test_kernel_matches_float64_the_cpu_restatement_and_the_reference(fx, name):
    from dnerf_amd.seal_mapper import SealBrushMapper
    m = SealBrushMapper(BS.POINT_CONFIGS[name])
    pts, dirs = fx[f"{name}_pts"], fx["dirs"]
    clear, mask64, points64, dist64 = fx[f"{name}_clear"], fx[f"{name}_mask64"], fx[f"{name}_points64"], fx[f"{name}_dist64"]
    assert (~clear).mean() <= BS.MARGIN_CAP
    att = float(m.map_data["attenuation_distance"])
    near = int((dist64[mask64] < att).sum())
    assert int(mask64.sum()) >= 300 and near >= 50 and int(mask64.sum()) - near >= 50
    cpu_pts, _, cpu_mask = SealBrushMapper(BS.POINT_CONFIGS[name])._map_to_origin_torch(torch.from_numpy(pts), torch.from_numpy(dirs))
    cpu_pts, cpu_mask = cpu_pts.numpy(), cpu_mask.numpy()
    linear = name != "curve_dry"
    bar_ref = float(fx[f"{name}_ref_fp32_error"]) + 2e-6 if linear else 0.0
    full = None
    for M in (BS.N_POINTS, BS.N_POINTS - 1, 65):                  # the last workgroup / the last wave partly filled
        p, d = torch.from_numpy(pts[:M]).cuda(), torch.from_numpy(dirs[:M]).cuda()
        m.map_data_conversion(p)
        mask = m.map_to_origin_(p, d).cpu().numpy()
        got = p.cpu().numpy()
        c = clear[:M]
        e64 = float(np.abs(got - points64[:M])[mask & mask64[:M]].max()) if (mask & mask64[:M]).any() else 0.0
        print(f"{name} M={M}: unclear {int((~c).sum())}, mapped {int(mask.sum())}, mask mismatches in all vs float64 {int((mask != mask64[:M]).sum())} "
              f"vs reference {int((mask != fx[f'{name}_mask'][:M]).sum())}, largest coordinate difference vs float64 {e64:.2e}")
        assert np.array_equal(mask[c], mask64[:M][c]) and np.array_equal(mask[c], fx[f"{name}_mask"][:M][c]) and np.array_equal(mask[c], cpu_mask[:M][c])
        assert not mask[:min(M, 16)].any()
        assert np.array_equal(got[~mask], pts[:M][~mask]) and np.array_equal(d.cpu().numpy(), dirs[:M])
        both = mask & mask64[:M]
        np.testing.assert_allclose(got[both], points64[:M][both], rtol=0, atol=2e-6 if linear else 0)
        both = mask & fx[f"{name}_mask"][:M]
        np.testing.assert_allclose(got[both], fx[f"{name}_points"][:M][both], rtol=0, atol=bar_ref)
        both = mask & cpu_mask[:M]
        np.testing.assert_allclose(got[both], cpu_pts[:M][both], rtol=0, atol=bar_ref)
        if M == BS.N_POINTS:
            full = (p, mask)
            assert linear == (not np.array_equal(got[mask], pts[mask]))
    # map_to_origin takes the same kernel on copies
    q, d = torch.from_numpy(pts).cuda(), torch.from_numpy(dirs).cuda()
    q2, d2, mask2 = m.map_to_origin(q, d)
    assert torch.equal(q2, full[0]) and np.array_equal(mask2.cpu().numpy(), full[1]) and torch.equal(q, torch.from_numpy(pts).cuda())
    assert q2.data_ptr() != q.data_ptr() and torch.equal(d2, d)
    if name == "curve":                                            # the early return's case: nothing inside the bounds, nothing touched
        far = torch.from_numpy(fx["far_pts"]).cuda()
        assert not bool(m.map_to_origin_(far, d).any()) and np.array_equal(far.cpu().numpy(), fx["far_points"])


def _ordered_triangles(m):
    """The curve mesh's triangles, the large faces across the ray direction first, top and bottom in turn: a truncated list then
    still holds faces on both sides of the points."""
    tri = m.map_triangles.double().numpy()
    d = m.map_test_dir.double().numpy()[0]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    height = (tri.mean(1) - m.map_data["center"].double().numpy()) @ d
    flux = np.abs(n @ d)
    top, bottom = np.nonzero(height > 0)[0], np.nonzero(height <= 0)[0]
    top, bottom = top[np.argsort(-flux[top], kind="stable")], bottom[np.argsort(-flux[bottom], kind="stable")]
    k = min(top.size, bottom.size)
    return tri[np.stack([top[:k], bottom[:k]], 1).reshape(-1)]


# a wave walks LDS tiles of 64 triangles (kBrushTile) and checks for an early end every 16 (kBrushChunk): 1, 15 / 16 / 17 and 63 / 64 / 65
# triangles with the mesh's own 25 border points, then 1 / 63 / 65 border points
@pytest.mark.parametrize("n_tris,n_border", [(1, None), (15, None), (16, None), (17, None), (63, None), (64, None), (65, None), (65, 1), (65, 63), (64, 65)])
def test_list_edges_through_the_c_call(fx, n_tris, n_border):
    from dnerf_amd.seal_mapper import SealBrushMapper, brush_triangle_records
    from sdn_backend import lib, check, ptr, stream
    m = SealBrushMapper(BS.CURVE_CONFIG)
    tri = _ordered_triangles(m)[:n_tris].astype(np.float32)
    border = m.map_data["border_points"].numpy()
    if n_border is not None:                                       # truncated, or padded with copies moved away along the stroke
        reps = -(-n_border // border.shape[0])
        border = np.concatenate([border + np.float32(0.01 * r) for r in range(reps)])[:n_border].astype(np.float32)
    cut = copy.copy(m)
    cut.map_data = dict(m.map_data, border_points=torch.from_numpy(border))
    cut.map_triangles = torch.from_numpy(tri)
    pts, dirs = fx["curve_pts"], fx["dirs"]
    g = BS.mapper_geometry(cut)
    clear, mask64 = BS.clear_of_boundaries(g, pts)
    points64, _ = BS.map_to_origin64(g, pts, mask64)
    cpu_pts, _, cpu_mask = cut._map_to_origin_torch(torch.from_numpy(pts), None)
    cpu_pts, cpu_mask = cpu_pts.numpy(), cpu_mask.numpy()
    a = m._native_args(torch.device("cuda", torch.cuda.current_device()))
    rec = torch.from_numpy(brush_triangle_records(tri, m.map_test_dir.numpy())).cuda()
    bdev = torch.from_numpy(border).cuda()
    p = torch.from_numpy(pts).cuda()
    mask = torch.full((pts.shape[0],), 7, dtype=torch.uint8, device="cuda")
    check(lib.sdn_seal_brush_map(ptr(p), None, pts.shape[0], a["bounds"], a["n_bounds"], ptr(rec), tri.shape[0], a["test_dir"], a["normal_expand"],
                                 a["center"], a["attenuation_distance"], 0, ptr(bdev), border.shape[0], ptr(mask), stream()), "seal_brush_map")
    mask, got = mask.cpu().numpy(), p.cpu().numpy()
    assert set(np.unique(mask).tolist()) <= {0, 1}
    mask = mask.astype(bool)
    own = float(np.abs(cpu_pts - points64)[cpu_mask & mask64].max()) if (cpu_mask & mask64).any() else 0.0      # the restatement's own distance from float64
    print(f"n_tris {n_tris} n_border {border.shape[0]}: unclear {int((~clear).sum())}, mapped {int(mask.sum())}, mask mismatches in all "
          f"{int((mask != cpu_mask).sum())}, restatement vs float64 {own:.2e}")
    assert np.array_equal(mask[clear], cpu_mask[clear]) and np.array_equal(mask[clear], mask64[clear])
    assert (int(mask.sum()) == 0) if n_tris == 1 else (int(mask.sum()) >= 20)
    np.testing.assert_allclose(got[mask & mask64], points64[mask & mask64], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got[mask & cpu_mask], cpu_pts[mask & cpu_mask], rtol=0, atol=own + 2e-6)
    assert np.array_equal(got[~mask], pts[~mask])


@pytest.fixture(scope="module")
def model_bits():
    return fixture_model("cuda")


def test_teacher_frame_through_the_three_render_paths(fx, model_bits):
    """The reference teacher's frame with the brush mapper (64 x 64, time 0.5, T_thresh 1e-4, force_fill_bound marked occupied), with
    the bars of the anchor mapper's frame test: the host-stepped loop on the fp32 operators reproduces it (trace exact, image and
    weights_sum 1e-4); the host-stepped loop with the fused -O field and the device loop agree bit for bit; the small-batch renderer
    gives the device loop's image bit for bit, its depth to 1e-5.  A frame group of two takes the mapper and renders each frame as the
    single-frame loop does, bit for bit; with an rgb tint it is refused."""
    from dnerf_amd.fused import FusedField
    from dnerf_amd.renderer import DeviceLoop, RayBatchRenderer, render_frame
    from dnerf_amd.seal_mapper import SealBrushMapper
    model, bits = model_bits
    sc = fixture_scene("cuda", model_bits=model_bits)
    keep = model.density_bitfield.clone()
    N = sc.rays_o.shape[0]
    try:
        mapper = SealBrushMapper(BS.FRAME_CONFIG)
        filled = fill_bitfield_host(bits, mapper.map_data["force_fill_bound"].cpu().numpy())
        model.density_bitfield.copy_(torch.from_numpy(filled))
        out = render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=False, T_thresh=1e-4, mapper=mapper)
        assert fx["frame_trace"].tolist() == [list(r) for r in out["trace"]]
        np.testing.assert_allclose(out["image"].cpu().numpy(), fx["frame_image"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(out["weights_sum"].cpu().numpy(), fx["frame_weights_sum"], rtol=0, atol=1e-4)
        assert (np.abs(out["image"].cpu().numpy() - fx["frame_plain_image"]).max(1) > 1e-3).sum() >= 100
        field = FusedField(sc.model, sc.time)
        host = render_frame(sc.model, sc.rays_o, sc.rays_d, sc.time, fp16=True, field=field, T_thresh=1e-4, mapper=mapper)
        loop = DeviceLoop(sc.model, field, N, "cuda", T_thresh=1e-4, mapper=mapper)
        fast = loop.render(sc.rays_o, sc.rays_d, sc.time)
        torch.cuda.synchronize()
        fast = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in fast.items()}      # (the loop is used again below)
        assert torch.equal(host["image"], fast["image"]) and host["n_samples"] == fast["n_samples"]
        once = RayBatchRenderer(sc.model, FusedField(sc.model, sc.time), N, "cuda", T_thresh=1e-4, mapper=mapper, samples_per_ray=160)
        got = once.render(sc.rays_o, sc.rays_d, sc.time, bg_color=1.0, check=True)
        torch.cuda.synchronize()
        assert torch.equal(got["image"], fast["image"]), float((got["image"] - fast["image"]).abs().max())
        d0, d1 = got["depth"], fast["depth"]
        assert torch.equal(torch.isnan(d0), torch.isnan(d1))
        assert float((torch.nan_to_num(d0) - torch.nan_to_num(d1)).abs().max()) < 1e-5
        # a frame group: the brush maps every sample on its own
        times = [sc.time, 0.25]
        grp = DeviceLoop(sc.model, field, 2 * N, "cuda", T_thresh=1e-4, mapper=mapper, frames=2).render(sc.rays_o.repeat(2, 1), sc.rays_d.repeat(2, 1), times)
        torch.cuda.synchronize()
        grp = {"image": grp["image"].clone()}
        for k, t in enumerate(times):
            alone = loop.render(sc.rays_o, sc.rays_d, t)
            torch.cuda.synchronize()
            assert torch.equal(grp["image"][k * N:(k + 1) * N], alone["image"]), k
        assert torch.equal(grp["image"][:N], fast["image"]) and not torch.equal(grp["image"][N:], fast["image"])
        with pytest.raises(NotImplementedError):
            DeviceLoop(sc.model, field, 2 * N, "cuda", T_thresh=1e-4, mapper=SealBrushMapper(BS.FRAME_CONFIG_RGB), frames=2)
    finally:
        model.density_bitfield.copy_(keep)
