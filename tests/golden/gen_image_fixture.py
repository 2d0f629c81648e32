#!/usr/bin/env python3
"""Generates tests/golden/caller_seald_image.npz by EXECUTING THE REFERENCE'S OWN texture stamp -- the `image` branch of
SealMapper.map_color (SealNeRF/seal_utils.py:58-79, with project_points :736-744 and modify_rgb :761-777) -- and its teacher renderer
(SealDNeRF/renderer.py + network.py, which hands map_color the mapped positions, :272) on the CPU, imported from the reference tree,
never copied, over the oracle-backed operator shims of tests/ref_shims/, the way gen_brush_fixture.py does.

The reference's brush constructor cannot run here (trimesh, pytorch3d, open3d, scikit-learn, scikit-spatial and cv2 are absent): the
mapper object is gen_brush_fixture's (`__new__`, `map_data` filled as `__init__` would), and the six `imageConfig` entries are added as
:389-411 fill them -- `image` = RGB / 255 as float32, `image_mask` = alpha / 255, the three corners, the normal of their plane --
from the texture ARRAY of seal_image_support (no file, no decoder).  Every METHOD that then runs is the reference's.

(a) points: the masked points of the brush fixture's `curve` set (mapped by the reference's map_to_origin), seeded colours (the first
    16 rounded to halves), the reference's map_color outputs for a stamp-only config and for `rgb` + stamp, the float64 texel
    coordinates, the clear points (both coordinates >= 1e-3 texel from every integer 1..W-1 / 1..H-1), and the reference's own fp32
    texel indices, read off its output for the index texture (column in the hue, row in the saturation) -- they must equal the
    float64 ones on every clear point.
(b) frame: the brush fixture's frame (64 x 64, time 0.5, `force_fill_bound` filled), strokes without the hue shift, the stamp over the
    disc stroke: trace, image, depth, weights_sum, and the same frame without the stamp.

Run in the build container only:   python tests/golden/gen_image_fixture.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import gen_brush_fixture as GB  # noqa: E402  (imports gen_caller_fixtures: installs the stubs and the operator shims)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import seal_brush_support as BS  # noqa: E402
import seal_image_support as IS  # noqa: E402

G = GB.G


def reference_stamp_mapper(SU, cfg, texture):
    """cfg: a brush config with `imageConfig` (its `path` is not read); texture: uint8 [H,W,3|4]."""
    m = GB.reference_brush_mapper(SU, cfg)
    conf = cfg["imageConfig"]
    v_o, v_w, v_h = np.asarray(conf["o"]), np.asarray(conf["w"]), np.asarray(conf["h"])
    corners = np.stack([v_o, v_w, v_h])
    m.map_data["rgb_light_offset"] = cfg["rgbLightOffset"] if "rgbLightOffset" in cfg else 0
    m.map_data["image"] = texture[:, :, :3].astype(np.float32) / 255
    m.map_data["image_mask"] = texture[:, :, 3] / 255 if texture.shape[2] == 4 else np.ones(texture.shape[:2])
    m.map_data["v_image_norm"] = np.linalg.svd((corners - corners.mean(0)).T, full_matrices=False)[0][:, -1]     # Plane.best_fit's normal
    m.map_data["v_image_o"], m.map_data["v_image_w"], m.map_data["v_image_h"] = v_o, v_w, v_h
    m.map_data_conversion(force=True)
    return m


def gen_points(SU, out):
    brush = np.load(BS.FIXTURE)
    mask = brush["curve_mask"]
    pts = torch.from_numpy(brush["curve_points"][mask])                # the reference's mapped_xyzs[mapped_mask]
    n = pts.shape[0]
    cols = torch.rand(n, 3, generator=torch.Generator().manual_seed(63))
    cols[:16] = torch.round(cols[:16] * 2) / 2
    tex = IS.stamp_texture()
    out["points"], out["colors_in"] = pts.numpy().copy(), cols.numpy().copy()
    for name, rgb in (("stamp", False), ("rgb_stamp", True)):
        m = reference_stamp_mapper(SU, IS.point_config("unused.png", rgb=rgb), tex)
        out[f"colors_out_{name}"] = m.map_color(pts.clone(), None, cols.clone()).numpy().copy()
    u, v, clear, iw, ih = IS.texel_coordinates64(pts.numpy())
    mi = reference_stamp_mapper(SU, IS.point_config("unused.png"), IS.index_texture())
    ref_w, ref_h = IS.decode_index(mi.map_color(pts.clone(), None, cols.clone()).numpy())
    assert np.array_equal(ref_w[clear], iw[clear]) and np.array_equal(ref_h[clear], ih[clear]), "move the rectangle: the reference's fp32 index leaves float64 on a clear point"
    alpha = tex[ih, iw, 3]
    clamped = (u < 0) | (u >= IS.W) | (v < 0) | (v >= IS.H)
    share = dict(unclear=float((~clear).mean()), alpha0=float((alpha == 0).mean()), alpha255=float((alpha == 255).mean()),
                 fractional=float(((alpha > 0) & (alpha < 255)).mean()), clamped=float(clamped.mean()))
    sides = [int((u < 0).sum()), int((u >= IS.W).sum()), int((v < 0).sum()), int((v >= IS.H).sum())]
    print(f"[points] masked {n}, shares {share}, clamped per side (left, right, top, bottom) {sides}, texels hit {np.unique(ih * IS.W + iw).size} of {IS.W * IS.H}, "
          f"index mismatches reference vs float64 in all {int(((ref_w != iw) | (ref_h != ih)).sum())}")
    assert share["unclear"] <= IS.CLEAR_CAP and share["alpha0"] >= 0.15 and share["alpha255"] >= 0.15 and share["fractional"] >= 0.05 and share["clamped"] >= 0.05
    assert min(sides) >= 1, "some samples must clamp on every side"
    out["u64"], out["v64"], out["clear"], out["idx_w"], out["idx_h"] = u, v, clear, iw.astype(np.int32), ih.astype(np.int32)
    out["ref_idx_w"], out["ref_idx_h"] = ref_w.astype(np.int32), ref_h.astype(np.int32)


def gen_frame(SU, out):
    import SealDNeRF.network as seald_network
    cfg = IS.frame_config("unused.png")
    model, bits = G.build_reference_model(seald_network.NeRFNetwork)
    ro, rd, _ = G.camera_rays(64, 64)
    mapper = reference_stamp_mapper(SU, cfg, IS.stamp_texture())
    filled = G.fill_bitfield_np(bits, mapper.map_data["force_fill_bound"].numpy())
    model.density_bitfield.copy_(torch.from_numpy(filled))
    model.seal_mapper = GB.reference_brush_mapper(SU, {k: v for k, v in cfg.items() if k != "imageConfig"})
    plain = G.run_infer(model, ro, rd, 0.5)               # (the same strokes without the stamp: what the stamp is compared with)
    model.seal_mapper = mapper
    r = G.run_infer(model, ro, rd, 0.5)
    for k, v in r.items():
        out[f"frame_{k}"] = v
    out["frame_plain_image"] = plain["image"]
    out["frame_filled_bitfield_sha"] = np.array(G.sha(filled[32]))
    changed = int((np.abs(r["image"] - plain["image"]).max(1) > 1e-3).sum())
    print(f"[frame] iterations {len(r['trace'])}, pixels changed by the stamp {changed}")
    assert changed >= 100, "move the rectangle: the stamp must change at least 100 pixels by more than 1e-3"


def main():
    import SealNeRF.seal_utils as SU
    out = {}
    gen_points(SU, out)
    gen_frame(SU, out)
    np.savez_compressed(IS.FIXTURE, **out)
    size = os.path.getsize(IS.FIXTURE)
    print("wrote", IS.FIXTURE, f"{size / 1024:.0f} KiB")
    assert size < 400 * 1024


if __name__ == "__main__":
    main()
