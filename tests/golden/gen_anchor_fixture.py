#!/usr/bin/env python3
"""Generates tests/golden/caller_seald_anchor.npz by EXECUTING THE REFERENCE'S OWN anchor seal mapper (SealNeRF/seal_utils.py:
SealAnchorMapper.map_to_origin :522-578, project_points :736-744, SealMapper.map_mask / map_color, modify_hsv, modify_rgb) and its
teacher renderer (SealDNeRF/renderer.py + network.py) on the CPU, imported from /root/reference, never copied -- over the
oracle-backed operator shims of tests/ref_shims/, the way gen_caller_fixtures.py makes the other caller fixtures.

The reference's constructor needs trimesh, pytorch3d and scikit-spatial, which are absent: the mapper object is made through
`__new__` and its `map_data` / `map_triangles` are filled as `__init__` would (:477-520) from `anchor_construction` below, a numpy
restatement of the constructor's geometry (the precedent is gen_caller_fixtures.reference_bbox_mapper).  Every METHOD that then
runs is the reference's.

(a) points: 6000 seeded points of v_anchor +- 0.2 (the first 8 all-zero, the next 8 with a zero y), the reference's map_to_origin
    outputs, its map_color outputs for an `hsv` and for an `rgb` config, the map_data scalars and vectors, and a second point set
    wholly outside the box (the early return).
(b) frame: the teacher at 64 x 64, time 0.5, on the generator's model, with the anchor on the torso's surface and the cells of
    `force_fill_bound` marked occupied first: trace, image, depth, weights_sum, the filled bitfield's digest.

Run in the build container only:   python tests/golden/gen_anchor_fixture.py
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

import seal_anchor_support as AS  # noqa: E402

BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def anchor_construction(cfg):
    """seal_utils.py:477-520 in numpy: Plane.best_fit = (centroid, left singular vector of the centred points with the smallest
    singular value); uv_sphere = a 32 x 32 latitude / longitude point set; bounding_box_oriented = the PCA-aligned box of the
    point set (vertex k = lo/hi per PCA axis by bit k&1, k>>1&1, k>>2).  -> (map_data, triangles [12,3,3])."""
    t = np.array(cfg["translation"], np.float64)
    raw = np.asarray(cfg["raw"], np.float64)
    v_anchor = np.mean(raw, 0)
    radius = cfg["radius"]
    u, _, _ = np.linalg.svd((raw - raw.mean(0)).T, full_matrices=False)
    normal = u[:, -1]
    translated = v_anchor + t
    projected = translated - ((translated - raw.mean(0)) @ normal) * normal
    v_offset, v_h = projected - v_anchor, projected - translated
    theta, phi = np.linspace(0.0, np.pi, 32), np.linspace(0.0, 2.0 * np.pi, 32, endpoint=False)
    st = np.sin(theta)[:, None]
    sphere = radius * 1.1 * np.stack([st * np.cos(phi)[None], st * np.sin(phi)[None], np.cos(theta)[:, None] * np.ones_like(phi)[None]], -1).reshape(-1, 3) + v_anchor
    pts = np.vstack([sphere, v_anchor + 1.1 * t, sphere - 0.1 * t])
    c = pts.mean(0)
    _, _, vt = np.linalg.svd(pts - c, full_matrices=False)
    q = (pts - c) @ vt.T
    lo, hi = q.min(0), q.max(0)
    verts = np.stack([c + np.array([(hi if (k >> a) & 1 else lo)[a] for a in range(3)]) @ vt for k in range(8)])
    bounds = np.stack([verts.min(0), verts.max(0)])
    md = {"force_fill_bound": bounds, "map_bound": bounds.copy(), "pose_center": verts.mean(0), "pose_radius": np.linalg.norm(t, 2) * 10,
          "v_anchor": v_anchor, "v_offset": v_offset, "v_h": v_h, "len_h": np.linalg.norm(v_h, 2), "radius": radius, "scale": cfg["scale"],
          "map_source": True}
    if "hsv" in cfg:
        md["hsv"] = cfg["hsv"]
    if "rgb" in cfg:
        md["rgb"] = cfg["rgb"]
        md["rgb_light_offset"] = cfg["rgbLightOffset"] if "rgbLightOffset" in cfg else 0
    return md, verts[BOX_FACES], pts


def reference_anchor_mapper(SU, cfg):
    m = SU.SealAnchorMapper.__new__(SU.SealAnchorMapper)
    SU.SealMapper.__init__(m, cfg)
    md, tris, _ = anchor_construction(cfg)
    m.map_triangles = torch.from_numpy(tris)
    m.map_data = md
    m.map_data_conversion(force=True)
    return m


def gen_points(SU, out):
    cfg = AS.POINTS_CONFIG
    md64, tris, generating = anchor_construction(cfg)
    for k in ("v_anchor", "v_offset", "v_h", "len_h", "radius", "pose_center", "pose_radius", "force_fill_bound", "map_bound"):
        out[f"md_{k}"] = np.asarray(md64[k], np.float64)
    out["md_scale"] = np.asarray(md64["scale"], np.float64)
    out["generating_points"] = generating
    pts = torch.from_numpy(AS.draw_points(cfg, 6000, 8, seed=31, n_zero_y=8))
    dirs = torch.nn.functional.normalize(torch.randn(6000, 3, generator=torch.Generator().manual_seed(32)), dim=-1)
    m = reference_anchor_mapper(SU, cfg)
    p2, d2, mask = m.map_to_origin(pts.clone(), dirs.clone())
    assert torch.equal(d2, dirs)
    out["pts"], out["dirs"] = pts.numpy(), dirs.numpy()
    out["points"], out["mask"] = p2.numpy().copy(), mask.numpy().copy()
    _, margin = AS.predicates64(cfg, pts.numpy())
    print(f"[points] valid {int(mask.sum())} of {mask.numel()}, inside the box {int(m.map_mask(pts.clone()).sum())}, "
          f"within {AS.MARGIN} of a predicate boundary {int((margin <= AS.MARGIN).sum())}")
    assert int(mask.sum()) >= 100
    g = torch.Generator().manual_seed(33)
    cols = torch.rand(int(mask.sum()), 3, generator=g)
    cols[:16] = torch.round(cols[:16] * 2) / 2
    out["colors_in"] = cols.numpy().copy()
    for name, c in (("hsv", AS.POINTS_CONFIG_HSV), ("rgb", AS.POINTS_CONFIG_RGB)):
        mc = reference_anchor_mapper(SU, c)
        out[f"colors_out_{name}"] = mc.map_color(p2[mask], d2[mask], cols.clone()).numpy().copy()
    # the early return (:527-528): a set wholly outside the box comes back as it went in
    far = pts + torch.tensor([0.9, -0.8, 0.85])
    p3, d3, mask3 = m.map_to_origin(far.clone(), dirs.clone())
    assert not bool(mask3.any()) and torch.equal(p3, far)
    out["far_pts"], out["far_points"], out["far_mask"] = far.numpy(), p3.numpy().copy(), mask3.numpy().copy()


def gen_frame(SU, out):
    import SealDNeRF.network as seald_network
    cfg = AS.FRAME_CONFIG
    model, bits = G.build_reference_model(seald_network.NeRFNetwork)
    ro, rd, _ = G.camera_rays(64, 64)
    mapper = reference_anchor_mapper(SU, cfg)
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
    print(f"[frame] iterations {len(r['trace'])}, pixels changed by the edit {changed}")
    assert changed >= 100, "move the anchor: the edit must change at least 100 pixels by more than 1e-3"


def main():
    import SealNeRF.seal_utils as SU
    out = {}
    gen_points(SU, out)
    gen_frame(SU, out)
    np.savez_compressed(AS.FIXTURE, **out)
    print("wrote", AS.FIXTURE, f"{os.path.getsize(AS.FIXTURE) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
