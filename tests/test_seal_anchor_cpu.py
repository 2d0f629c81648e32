"""The SealD anchor (control-point) mapper (dnerf_amd/seal_mapper.SealAnchorMapper) on the CPU, against what the reference's own
SealAnchorMapper.map_to_origin / map_color produced (tests/golden/caller_seald_anchor.npz, made by gen_anchor_fixture.py): the
constructor's geometry, the torch restatement of map_to_origin, the colours, the early return, the dispatch."""
import ctypes

import numpy as np
import pytest
import torch

import seal_anchor_support as AS
from dnerf_amd import seal_mapper as SM


@pytest.fixture(scope="module")
def fx():
    return np.load(AS.FIXTURE)


@pytest.fixture(scope="module")
def mapper():
    return SM.SealAnchorMapper(AS.POINTS_CONFIG)


def _inside(vertices, points, slack=0.0):
    """Analytic oriented-box test on the 8 vertices (corner order of seal_mapper._BOX_FACES)."""
    o = vertices[0]
    inside = np.ones(len(points), bool)
    for k in (1, 2, 4):
        e = vertices[k] - o
        s = (points - o) @ e / (e @ e)
        inside &= (s >= -slack) & (s <= 1 + slack)
    return inside


def test_constructor_reproduces_the_fixture_geometry(fx):
    m = SM.SealAnchorMapper.__new__(SM.SealAnchorMapper)
    keep = SM.SealMapper.map_data_conversion
    try:                                       # the float64 values, before map_data_conversion rounds them to fp32
        SM.SealMapper.map_data_conversion = lambda self, T=None, force=False: None
        m.__init__(AS.POINTS_CONFIG)
    finally:
        SM.SealMapper.map_data_conversion = keep
    for k in ("v_anchor", "v_offset", "v_h", "len_h", "pose_center", "pose_radius"):
        np.testing.assert_allclose(np.asarray(m.map_data[k], np.float64), fx[f"md_{k}"], rtol=1e-9, atol=0, err_msg=k)
    assert set(m.map_data) == {"force_fill_bound", "map_bound", "pose_center", "pose_radius", "v_anchor", "v_offset", "v_h", "len_h", "radius",
                               "scale", "map_source"}
    assert m.map_data["map_source"] is True and not m.redirects_source
    # v_h and v_offset do not depend on the sign the SVD gives the normal
    g = AS.anchor_geometry(AS.POINTS_CONFIG)
    np.testing.assert_allclose(np.asarray(m.map_data["v_h"]), g["v_h"], rtol=1e-12, atol=1e-15)
    t = np.asarray(AS.POINTS_CONFIG["translation"])
    np.testing.assert_allclose(np.asarray(m.map_data["v_offset"]) - np.asarray(m.map_data["v_h"]), t, rtol=1e-12, atol=1e-15)


def test_one_box_serves_triangles_bounds_and_fill_and_contains_the_cone(fx, mapper):
    v = mapper.to_vertices
    assert mapper.map_triangles.shape == (12, 3, 3)
    np.testing.assert_array_equal(mapper.map_triangles.double().numpy(), v[SM._BOX_FACES].astype(np.float32).astype(np.float64))
    bounds = np.stack([v.min(0), v.max(0)]).astype(np.float32)
    np.testing.assert_array_equal(mapper.map_data["map_bound"].numpy(), bounds)
    np.testing.assert_array_equal(mapper.map_data["force_fill_bound"].numpy(), bounds)
    e1, e2, e3 = v[1] - v[0], v[2] - v[0], v[4] - v[0]
    assert abs(e1 @ e2) < 1e-12 and abs(e1 @ e3) < 1e-12 and abs(e2 @ e3) < 1e-12
    assert _inside(v, fx["generating_points"], slack=1e-9).all()
    valid = fx["mask"]
    assert valid.sum() >= 100 and _inside(v, fx["pts"][valid].astype(np.float64)).all()
    assert bool(mapper.map_mask(torch.from_numpy(fx["pts"][valid])).all())        # ... and by the mapper's own (ray-casting) test


def test_torch_restatement_reproduces_the_reference(fx, mapper):
    pts, dirs = torch.from_numpy(fx["pts"]), torch.from_numpy(fx["dirs"])
    p2, d2, mask = mapper._map_to_origin_torch(pts.clone(), dirs.clone())
    assert np.array_equal(mask.numpy(), fx["mask"])
    np.testing.assert_allclose(p2.numpy(), fx["points"], rtol=0, atol=2e-6)
    assert np.array_equal(p2.numpy()[~fx["mask"]], fx["pts"][~fx["mask"]])
    assert torch.equal(d2, dirs)
    # map_to_origin on CPU tensors is the restatement
    q2, _, qmask = mapper.map_to_origin(pts.clone(), dirs.clone())
    assert torch.equal(q2, p2) and torch.equal(qmask, mask)


@pytest.mark.parametrize("name", ["hsv", "rgb"])
def test_colours_reproduce_the_reference(fx, name):
    m = SM.SealAnchorMapper(AS.POINTS_CONFIG_HSV if name == "hsv" else AS.POINTS_CONFIG_RGB)
    mask = torch.from_numpy(fx["mask"])
    cols = torch.from_numpy(fx["colors_in"])
    m.map_data_conversion(cols)
    out = m.map_color(None, None, cols.clone())
    np.testing.assert_allclose(out.numpy(), fx[f"colors_out_{name}"], rtol=0, atol=2e-6)
    # the in-place form the loops use (the torch path on CPU tensors) writes the masked rows only
    full = torch.zeros(mask.shape[0], 3)
    full[mask] = cols
    got = m.map_color_(full.clone(), mask)
    np.testing.assert_allclose(got.numpy()[fx["mask"]], fx[f"colors_out_{name}"], rtol=0, atol=2e-6)
    assert torch.equal(got[~mask], full[~mask])


def test_early_return_leaves_a_set_outside_the_box_untouched(fx, mapper):
    far, dirs = torch.from_numpy(fx["far_pts"]), torch.from_numpy(fx["dirs"])
    p, d, mask = mapper._map_to_origin_torch(far, dirs)
    assert p is far and d is dirs and not bool(mask.any()) and mask.shape == (far.shape[0],)
    assert np.array_equal(p.numpy(), fx["far_points"]) and np.array_equal(mask.numpy(), fx["far_mask"])
    # the gate is the whole call's: the same cone points ARE mapped once one point of the call lies in the box
    valid, _ = AS.predicates64(AS.POINTS_CONFIG, fx["pts"])
    assert valid[16:].any()


def test_get_seal_mapper_dispatch():
    assert isinstance(SM.get_seal_mapper(dict(AS.POINTS_CONFIG)), SM.SealAnchorMapper)
    with pytest.raises(NotImplementedError) as e:
        SM.get_seal_mapper({"type": "brush"})
    assert "anchor" not in str(e.value)


def test_in_plane_translation_raises():
    cfg = dict(AS.POINTS_CONFIG, raw=[[0.1, 0.0, 0.3], [-0.1, 0.0, 0.3], [0.0, 0.1, 0.3], [0.0, -0.1, 0.3]], translation=[0.1, 0.05, 0.0])
    with pytest.raises(ValueError):
        SM.SealAnchorMapper(cfg)
    SM.SealAnchorMapper(dict(cfg, translation=[0.1, 0.05, 0.02]))


def test_frame_config_fills_the_cells_the_fixture_was_rendered_with(fx):
    """The occupancy the teacher frame of the fixture was rendered with is the one the product's box marks."""
    from caller_fixtures import _sha, fill_bitfield_host, fixture_model
    _, bits = fixture_model("cpu", check=False)
    m = SM.SealAnchorMapper(AS.FRAME_CONFIG)
    filled = fill_bitfield_host(bits, m.map_data["force_fill_bound"].numpy())
    assert _sha(filled[32]) == str(fx["frame_filled_bitfield_sha"])
    assert (np.abs(fx["frame_image"] - fx["frame_plain_image"]).max(1) > 1e-3).sum() >= 100


def test_seal_record_mirror_carries_the_anchor_fields():
    import sdn_backend as B
    box = B.SdnSealBox()
    assert box.kind == B.SEAL_BBOX == 0 and B.SEAL_ANCHOR == 1
    assert B.SdnSealBox.kind.offset == B.SdnSealBox.scratch.offset + ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(B.SdnSealBox) == B.SdnSealBox.kind.offset + 4 * 12
