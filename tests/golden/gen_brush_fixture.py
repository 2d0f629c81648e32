#!/usr/bin/env python3
"""Generates tests/golden/caller_seald_brush.npz by EXECUTING THE REFERENCE'S OWN brush seal mapper (SealNeRF/seal_utils.py:
SealBrushMapper.map_to_origin :415-461, mesh_surface_points_mask :720-733, project_points :736-744, SealMapper.map_mask /
map_color, modify_hsv, modify_rgb) and its teacher renderer (SealDNeRF/renderer.py + network.py) on the CPU, imported from the
reference tree, never copied -- over the oracle-backed operator shims of tests/ref_shims/, the way gen_anchor_fixture.py does.

The reference's constructor needs trimesh, pytorch3d, open3d, scikit-learn and scikit-spatial, which are absent: the mapper object
is made through `__new__` and its `map_data` / `map_triangles` / `map_test_dir` are filled as `__init__` would (:304-413) from
`seal_brush_support.brush_construction`, a numpy restatement of the constructor's geometry whose border points come from the
reference's own `mesh_surface_points_mask`.  Every METHOD that then runs is the reference's.

(a) points, per config of seal_brush_support.POINT_CONFIGS (a 48-point curve stroke, linear and dry, and a line + curve pair): the
    geometry, 6000 seeded points of the strokes' bounds +- 0.03 (the first 8 all-zero, the next 8 with one zero coordinate), the
    reference's map_to_origin outputs, the float64 mask / coordinates / border distances and the points clear of every predicate
    boundary (the reference's own mask must agree with the float64 one on each of them), and for `linear` `ref_fp32_error`: the
    largest coordinate distance between the reference's fp32 outputs and the float64 ones -- what cdist's matrix-product form
    costs.  For the curve: map_color outputs for an `hsv` and an `rgb` config, and a point set wholly outside the bounds.
(b) frame: the teacher at 64 x 64, time 0.5, on the generator's model, with a curve and a line stroke on the torso's surface and
    the cells of `force_fill_bound` marked occupied first: trace, image, depth, weights_sum, the filled bitfield's digest.

Run in the build container only:   python tests/golden/gen_brush_fixture.py
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

import seal_brush_support as BS  # noqa: E402


def reference_brush_mapper(SU, cfg):
    m = SU.SealBrushMapper.__new__(SU.SealBrushMapper)
    SU.SealMapper.__init__(m, cfg)
    md, tris, test_dir = BS.brush_construction(cfg, SU.mesh_surface_points_mask)
    m.map_triangles = torch.from_numpy(tris)
    m.map_test_dir = torch.from_numpy(test_dir)
    m.map_data = md
    m.map_data_conversion(force=True)
    return m


def reference_geometry(m):
    md = m.map_data
    return BS.geometry(m.map_triangles.numpy(), md["map_bound"].numpy(), m.map_test_dir.numpy(), md["normal_expand"].numpy(), md["center"].numpy(),
                       md["border_points"].numpy(), md["attenuation_distance"], md["attenuation_mode"])


def gen_points(SU, out):
    dirs = torch.nn.functional.normalize(torch.randn(BS.N_POINTS, 3, generator=torch.Generator().manual_seed(62)), dim=-1)
    out["dirs"] = dirs.numpy()
    for name, cfg in BS.POINT_CONFIGS.items():
        md64, tris64, _ = BS.brush_construction(cfg, SU.mesh_surface_points_mask)
        m = reference_brush_mapper(SU, cfg)
        g = reference_geometry(m)
        pts = torch.from_numpy(BS.draw_points(g["bounds"]))
        p2, d2, mask = m.map_to_origin(pts.clone(), dirs.clone())
        assert d2 is not None and torch.equal(d2, dirs)
        clear, mask64 = BS.clear_of_boundaries(g, pts.numpy())
        points64, dist64 = BS.map_to_origin64(g, pts.numpy(), mask64)
        mask = mask.numpy().copy()
        assert np.array_equal(mask[clear], mask64[clear]), "the reference's own mask leaves the float64 one on a clear point"
        both = mask & mask64
        err = float(np.abs(p2.numpy().astype(np.float64) - points64)[both].max())
        near = int((dist64[mask64] < g["att"]).sum())
        print(f"[{name}] triangles {tris64.shape[0]}, border points {md64['border_points'].shape[0]}, mapped {int(mask.sum())} of {mask.size}, "
              f"unclear {int((~clear).sum())}, near the border {near}, beyond {int(mask64.sum()) - near}, reference fp32 vs float64 {err:.3e}")
        assert int(mask.sum()) >= 300 and near >= 50 and int(mask64.sum()) - near >= 50
        out[f"{name}_triangles"] = tris64
        for k in ("map_bound", "force_fill_bound", "normal_expand", "center"):
            out[f"{name}_{k}"] = np.asarray(md64[k], np.float64)
        out[f"{name}_border_points"] = md64["border_points"].numpy()
        out[f"{name}_pts"], out[f"{name}_points"], out[f"{name}_mask"] = pts.numpy(), p2.numpy().copy(), mask
        out[f"{name}_clear"], out[f"{name}_mask64"], out[f"{name}_points64"], out[f"{name}_dist64"] = clear, mask64, points64, dist64
        if cfg["attenuationMode"] == "linear":
            out[f"{name}_ref_fp32_error"] = np.float64(err)
        else:
            assert torch.equal(p2, pts)
        if name == "curve":
            cols = torch.rand(int(mask.sum()), 3, generator=torch.Generator().manual_seed(63))
            cols[:16] = torch.round(cols[:16] * 2) / 2
            out["colors_in"] = cols.numpy().copy()
            for cname, c in (("hsv", BS.CURVE_CONFIG_HSV), ("rgb", BS.CURVE_CONFIG_RGB)):
                mc = reference_brush_mapper(SU, c)
                out[f"colors_out_{cname}"] = mc.map_color(p2[torch.from_numpy(mask)], None, cols.clone()).numpy().copy()
            # the early return (:421-422): a set wholly outside the bounds comes back as it went in
            far = pts + torch.tensor([0.9, -0.8, 0.85])
            p3, d3, mask3 = m.map_to_origin(far.clone(), dirs.clone())
            assert not bool(mask3.any()) and torch.equal(p3, far)
            out["far_pts"], out["far_points"], out["far_mask"] = far.numpy(), p3.numpy().copy(), mask3.numpy().copy()


def gen_frame(SU, out):
    import SealDNeRF.network as seald_network
    cfg = BS.FRAME_CONFIG
    model, bits = G.build_reference_model(seald_network.NeRFNetwork)
    ro, rd, _ = G.camera_rays(64, 64)
    mapper = reference_brush_mapper(SU, cfg)
    filled = G.fill_bitfield_np(bits, mapper.map_data["force_fill_bound"].numpy())
    model.density_bitfield.copy_(torch.from_numpy(filled))
    plain = G.run_infer(model, ro, rd, 0.5)               # (filled occupancy, no mapper: what the edit is compared with)
    model.seal_mapper = mapper
    r = G.run_infer(model, ro, rd, 0.5)
    for k, v in r.items():
        out[f"frame_{k}"] = v
    out["frame_plain_image"] = plain["image"]
    out["frame_filled_bitfield_sha"] = np.array(G.sha(filled[32]))
    out["frame_force_fill_bound"] = mapper.map_data["force_fill_bound"].numpy().astype(np.float64)
    changed = int((np.abs(r["image"] - plain["image"]).max(1) > 1e-3).sum())
    print(f"[frame] triangles {mapper.map_triangles.shape[0]}, iterations {len(r['trace'])}, pixels changed by the edit {changed}")
    assert changed >= 100, "move the strokes: the edit must change at least 100 pixels by more than 1e-3"


def main():
    import SealNeRF.seal_utils as SU
    out = {}
    gen_points(SU, out)
    gen_frame(SU, out)
    np.savez_compressed(BS.FIXTURE, **out)
    print("wrote", BS.FIXTURE, f"{os.path.getsize(BS.FIXTURE) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
