"""The SealD brush mapper (dnerf_amd/seal_mapper.SealBrushMapper) on the CPU, against what the reference's own
SealBrushMapper.map_to_origin / map_color / mesh_surface_points_mask produced (tests/golden/caller_seald_brush.npz, made by
gen_brush_fixture.py): the constructor's meshes and border points, its errors, the torch restatement of map_to_origin, the
colours, the early return, the dispatch, the C records.

Masks are compared on the points the fixture marks clear: those on which map_mask in float64 gives the same answer with every
threshold moved in and moved out by 1e-5 (seal_brush_support.map_mask64; at most 0.5 % of a set may be unclear -- the generator found
0 of 6000 in each set).  Coordinates against the reference's fp32 outputs are within ref_fp32_error + 2e-6: the reference's own
distance from exact arithmetic (its cdist takes the matrix-product form), stored in the fixture, plus the bar the other mappers'
tests use for fp32 statement order."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import seal_brush_support as BS
from dnerf_amd import seal_mapper as SM


@pytest.fixture(scope="module")
def fx():
    return np.load(BS.FIXTURE)


@pytest.fixture(scope="module")
def mappers():
    return {name: SM.SealBrushMapper(cfg) for name, cfg in dict(BS.POINT_CONFIGS, line=BS.LINE_CONFIG).items()}


def _rows(tri):
    t = np.asarray(tri, np.float64).reshape(-1, 9)
    return t[np.lexsort(t.T[::-1])]


@pytest.mark.parametrize("name,strokes", [("line", 1), ("curve", 1), ("two_stroke", 2)])
def test_constructor_geometry(fx, mappers, name, strokes):
    m = mappers[name]
    md = m.map_data
    assert md["map_bound"].shape == (strokes, 2, 3) and md["force_fill_bound"].shape == (strokes, 2, 3)
    assert torch.equal(md["map_bound"], md["force_fill_bound"])
    assert m.map_triangles.ndim == 3 and m.map_triangles.shape[1:] == (3, 3) and bool(torch.isfinite(m.map_triangles).all())
    assert md["border_points"].shape[0] > 0 and md["border_points"].shape[1] == 3
    assert md["attenuation_mode"] == "linear" and m.map_test_dir.shape == (1, 3)
    assert torch.equal(m.map_test_dir[0], md["normal_expand"])                    # the last stroke's, not normalised
    assert len(m.stroke_triangles) == strokes and sum(t.shape[0] for t in m.stroke_triangles) == m.map_triangles.shape[0]
    for b, t in zip(md["map_bound"].numpy(), m.stroke_triangles):
        v = t.reshape(-1, 3).astype(np.float32)
        assert np.array_equal(b[0], v.min(0)) and np.array_equal(b[1], v.max(0))
    if name == "line":
        assert m.map_triangles.shape[0] == 12
        return
    print(name, "triangles", m.map_triangles.shape[0], "border points", md["border_points"].shape[0])
    # the reference's mapper object of the fixture was built from the same meshes (any face order) and border points
    np.testing.assert_allclose(_rows(m.map_triangles.numpy()), _rows(fx[f"{name}_triangles"].astype(np.float32)), rtol=0, atol=1e-7)
    np.testing.assert_allclose(md["border_points"].numpy(), fx[f"{name}_border_points"], rtol=0, atol=1e-7)
    for k in ("map_bound", "normal_expand", "center"):
        np.testing.assert_allclose(md[k].numpy(), fx[f"{name}_{k}"], rtol=0, atol=1e-7, err_msg=k)


def test_curve_mesh_is_a_clustered_prism(mappers):
    """48 stroke points: 96 prism vertices and 48 * 36 * 4 faces before the simplification, far fewer after it; a coarser voxel grid
    leaves fewer faces still."""
    pts = np.asarray(BS.CURVE_CONFIG["raw"])
    faces = SM.knn_prism_faces(pts)
    assert faces.shape == (48 * 36 * 4, 3) and faces.min() == 0 and faces.max() == 95
    first = faces[:4].tolist()
    d = np.linalg.norm(pts - pts[0], axis=1)
    d[0] = -1
    nn = np.argsort(d, kind="stable")
    assert first == [[0, nn[1], nn[2]], [48, nn[1] + 48, nn[2] + 48], [0, nn[1], 48], [48, nn[1], nn[1] + 48]]
    n16 = mappers["curve"].map_triangles.shape[0]
    n8 = SM.SealBrushMapper(dict(BS.CURVE_CONFIG, simplifyVoxel=8)).map_triangles.shape[0]
    assert 0 < n8 < n16 < faces.shape[0]
    # clustering: two vertices of one voxel become their mean, the face between them and a third collapses
    v, f = SM.cluster_vertices(np.array([[0.0, 0, 0], [0.1, 0, 0], [1.0, 0, 0], [1.0, 1.0, 0]]), np.array([[0, 1, 2], [1, 2, 3], [2, 3, 0], [3, 0, 2]]), 0.5)
    np.testing.assert_allclose(v, [[0.05, 0, 0], [1.0, 0, 0], [1.0, 1.0, 0]])
    assert f.tolist() == [[0, 1, 2]]                                               # three faces of one vertex cycle, one degenerate


def test_normal_decides_the_side():
    a = SM.SealBrushMapper(BS.CURVE_CONFIG)
    b = SM.SealBrushMapper(dict(BS.CURVE_CONFIG, normal=[-v for v in BS.CURVE_CONFIG["normal"]]))
    np.testing.assert_allclose(a.map_data["normal_expand"].numpy(), -b.map_data["normal_expand"].numpy(), rtol=0, atol=1e-9)
    assert abs(float(a.map_data["normal_expand"].norm()) - BS.CURVE_CONFIG["brushPressure"]) < 1e-7
    assert float(a.map_data["normal_expand"] @ torch.tensor(BS.CURVE_CONFIG["normal"])) > 0


def test_constructor_errors(monkeypatch):
    stroke = BS.CURVE_CONFIG["raw"]
    with pytest.raises(ValueError):
        SM.SealBrushMapper(dict(BS.LINE_CONFIG, raw=[BS.LINE_CONFIG["raw"]] * 5))
    SM.SealBrushMapper(dict(BS.LINE_CONFIG, raw=[BS.LINE_CONFIG["raw"]] * 4))
    with pytest.raises(NotImplementedError):
        SM.SealBrushMapper(dict(BS.CURVE_CONFIG, imageConfig={"path": "stamp.png", "o": [0, 0, 0], "w": [1, 0, 0], "h": [0, 1, 0]}))
    for mode in ("ease-in", "ease-out"):
        with pytest.raises(NotImplementedError):
            SM.SealBrushMapper(dict(BS.CURVE_CONFIG, attenuationMode=mode))
    with pytest.raises(ValueError):
        SM.SealBrushMapper(dict(BS.CURVE_CONFIG, raw=stroke[:9]))                  # fewer points than neighbours
    # A stroke none of whose projected points is a border point of its mesh.  No config reaches this in exact arithmetic: the outermost
    # projected point leaves the hull of its own mesh by one of the six axis steps, and outside the hull the two opposite rays cannot
    # both hit.  The check guards against rounding (the steps are 1e-4 in fp32) and against a failing `cdist(...).min(1)` later, so the
    # branch is driven through the predicate it depends on.
    monkeypatch.setattr(SM, "mesh_surface_points_mask", lambda tri, pts: torch.zeros(pts.shape[0], dtype=torch.bool))
    with pytest.raises(ValueError, match="border"):
        SM.SealBrushMapper(BS.LINE_CONFIG)


def test_get_seal_mapper_dispatch():
    assert isinstance(SM.get_seal_mapper(dict(BS.CURVE_CONFIG)), SM.SealBrushMapper)
    with pytest.raises(NotImplementedError) as e:
        SM.get_seal_mapper({"type": "brush"})
    assert "raw" in str(e.value) and "brushType" in str(e.value) and "anchor" not in str(e.value)
    with pytest.raises(NotImplementedError):
        SM.get_seal_mapper({"type": "lasso"})


@pytest.mark.parametrize("name", list(BS.POINT_CONFIGS))
def test_torch_restatement_reproduces_the_reference(fx, mappers, name):
    m = mappers[name]
    pts, dirs = torch.from_numpy(fx[f"{name}_pts"]), torch.from_numpy(fx["dirs"])
    np.testing.assert_array_equal(fx[f"{name}_pts"], BS.draw_points(BS.mapper_geometry(m)["bounds"]))     # the fixture's points are the seeded ones
    p2, d2, mask = m._map_to_origin_torch(pts.clone(), dirs.clone())
    clear, want = fx[f"{name}_clear"], fx[f"{name}_mask"]
    print(name, "unclear", int((~clear).sum()), "mapped", int(want.sum()), "mask mismatches in all", int((mask.numpy() != want).sum()))
    assert (~clear).mean() <= BS.MARGIN_CAP
    assert np.array_equal(mask.numpy()[clear], want[clear]) and np.array_equal(want[clear], fx[f"{name}_mask64"][clear])
    assert not mask.numpy()[:16].any()                                             # zero coordinates are never mapped
    both = mask.numpy() & want
    if name == "curve_dry":
        assert torch.equal(p2, pts)
    else:
        bar = float(fx[f"{name}_ref_fp32_error"]) + 2e-6
        print(name, "ref_fp32_error", float(fx[f"{name}_ref_fp32_error"]), "largest difference", float(np.abs(p2.numpy() - fx[f"{name}_points"])[both].max()))
        np.testing.assert_allclose(p2.numpy()[both], fx[f"{name}_points"][both], rtol=0, atol=bar)
        assert both.sum() >= 300 and not np.array_equal(p2.numpy()[both], fx[f"{name}_pts"][both])
    assert np.array_equal(p2.numpy()[~mask.numpy()], fx[f"{name}_pts"][~mask.numpy()])
    assert d2 is dirs or torch.equal(d2, dirs)
    q2, _, qmask = m.map_to_origin(pts.clone(), dirs.clone())                      # on CPU tensors map_to_origin is the restatement
    assert torch.equal(q2, p2) and torch.equal(qmask, mask)


def test_early_return_hands_back_the_inputs(fx, mappers):
    far, dirs = torch.from_numpy(fx["far_pts"]), torch.from_numpy(fx["dirs"])
    p, d, mask = mappers["curve"]._map_to_origin_torch(far, dirs)
    assert p is far and d is dirs and not bool(mask.any()) and mask.shape == (far.shape[0],)
    assert np.array_equal(p.numpy(), fx["far_points"]) and np.array_equal(mask.numpy(), fx["far_mask"])


def test_a_zero_coordinate_inside_the_mesh_is_not_mapped():
    """`points.all(1)`: the mapped set is map_mask's.  A stroke around the plane z = 0: the points above and below its middle are
    mapped, the point between them, with z == 0 exactly, is not."""
    cfg = dict(BS.LINE_CONFIG, normal=[0.0, 0.0, 1.0], raw=BS.band_stroke([0.1, 0.2, 0.0], [0.0, 0.0, 1.0], 0.22, 0.05))
    m = SM.SealBrushMapper(cfg)
    pts = torch.tensor([[0.1, 0.2, 0.003], [0.1, 0.2, 0.0], [0.1, 0.2, -0.003]])
    _, _, mask = m._map_to_origin_torch(pts, None)
    assert mask.tolist() == [True, False, True]


@pytest.mark.parametrize("name", ["hsv", "rgb"])
def test_colours_reproduce_the_reference(fx, name):
    m = SM.SealBrushMapper(BS.CURVE_CONFIG_HSV if name == "hsv" else BS.CURVE_CONFIG_RGB)
    cols = torch.from_numpy(fx["colors_in"])
    m.map_data_conversion(cols)
    np.testing.assert_allclose(m.map_color(None, None, cols.clone()).numpy(), fx[f"colors_out_{name}"], rtol=0, atol=2e-6)


def test_triangle_records_hold_the_lane_independent_part():
    m = SM.SealBrushMapper(BS.LINE_CONFIG)
    tri = m.map_triangles.double().numpy()
    d = m.map_test_dir.double().numpy()[0]
    rec = SM.brush_triangle_records(tri, d)
    assert rec.dtype == np.float32 and rec.shape == (12, 16) and not rec[:, 14:].any()
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    np.testing.assert_allclose(rec[:, :3], tri[:, 0], rtol=0, atol=0)
    np.testing.assert_allclose(rec[:, 9:12], n, rtol=1e-6, atol=1e-12)
    # (the box's side faces are parallel to the direction: d . N is rounding noise there and eps decides, so compare the determinants)
    np.testing.assert_allclose(-1.0 / rec[:, 12].astype(np.float64), n @ d + 1e-8, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(-1.0 / rec[:, 13].astype(np.float64), -(n @ d) + 1e-8, rtol=1e-5, atol=1e-9)


def test_frame_config_fills_the_cells_the_fixture_was_rendered_with(fx):
    from caller_fixtures import _sha, fill_bitfield_host, fixture_model
    _, bits = fixture_model("cpu", check=False)
    m = SM.SealBrushMapper(BS.FRAME_CONFIG)
    assert m.map_data["force_fill_bound"].shape == (2, 2, 3)
    filled = fill_bitfield_host(bits, m.map_data["force_fill_bound"].numpy())
    assert _sha(filled[32]) == str(fx["frame_filled_bitfield_sha"])
    assert (np.abs(fx["frame_image"] - fx["frame_plain_image"]).max(1) > 1e-3).sum() >= 100


def test_brush_records_match_the_c_header(tmp_path):
    """`SdnSealBrush` and `SdnRenderCtx` (which reaches it through its last field) against include/sdn_hip.h: a C program prints
    sizeof and every field's offset."""
    import sdn_backend as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    records = {"SdnSealBrush": B.SdnSealBrush, "SdnRenderCtx": B.SdnRenderCtx}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sdn_hip.h"', 'int main(void) {',
             '  printf("kind brush %d\\n", SDN_SEAL_BRUSH);']
    for name, rec in records.items():
        lines.append(f'  printf("{name} size %zu\\n", sizeof({name}));')
        for field, _ in rec._fields_:
            lines.append(f'  printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        name, field, value = line.split()
        if name == "kind":
            assert int(value) == B.SEAL_BRUSH == 2
            continue
        rec = records[name]
        assert int(value) == (ctypes.sizeof(rec) if field == "size" else getattr(rec, field).offset), (name, field)
        seen += 1
    assert seen == sum(len(r._fields_) + 1 for r in records.values())
    assert B.SdnRenderCtx._fields_[-1][0] == "seal_brush" and B.SdnRenderCtx.seal_brush.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(B.SdnRenderCtx)
    assert B.BRUSH_TRI_FLOATS == 16 and (B.BRUSH_LINEAR, B.BRUSH_DRY) == (0, 1)
