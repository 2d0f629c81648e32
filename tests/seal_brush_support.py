"""Inputs shared by the brush seal mapper's fixture generator (tests/golden/gen_brush_fixture.py) and its tests: the seal
configs, the seeded point sets, a numpy restatement of the reference constructor's geometry (SealNeRF/seal_utils.py:304-383,
599-631 -- the generator builds the reference's mapper object from it), and float64 evaluations of `map_mask` and of
`SealBrushMapper.map_to_origin` (:132-153, :415-461, :638-693) that say where an fp32 evaluation may round either way."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caller_seald_brush.npz")

MARGIN = 1e-5          # every predicate threshold (t, u, v >= 0, u + v <= 1, the AABB sides) is moved in / out by this much in float64
MARGIN_CAP = 0.005     # ... and the points on which the two forms disagree may be at most this share of a point set
N_POINTS = 6000
BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def _frame(normal):
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    u = np.cross(n, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    return n, u, np.cross(n, u)


def disc_stroke(center, normal, radius, count=48, bump=0.002):
    """`count` points of a sunflower disc about `center` in the plane with `normal`, lifted off it by up to `bump` (a hand-drawn
    stroke is not planar)."""
    n, u, v = _frame(normal)
    k = np.arange(count)
    r = radius * np.sqrt((k + 0.5) / count)
    a = k * np.pi * (3.0 - np.sqrt(5.0))
    return (np.asarray(center, np.float64) + r[:, None] * (np.cos(a)[:, None] * u + np.sin(a)[:, None] * v)
            + (bump * np.sin(5.0 * a))[:, None] * n).tolist()


def ribbon_stroke(center, normal, length, sway, width, count=48, bump=0.002):
    """`count` points drawn densely along a swaying path of `length` about `center` in the plane with `normal`, zig-zagging over the
    brush's `width` (a curve stroke: the points are closer than the simplification's voxel, so the fitted mesh is clustered)."""
    n, u, v = _frame(normal)
    k = np.arange(count)
    s = (k / (count - 1) - 0.5) * length
    w = sway * np.sin(2.0 * np.pi * s / length) + np.where(k % 2 == 0, 0.5, -0.5) * width
    return (np.asarray(center, np.float64) + s[:, None] * u + w[:, None] * v + (bump * np.sin(0.7 * k))[:, None] * n).tolist()


def band_stroke(center, normal, length, width, count=14, bump=0.002):
    """`count` points zig-zagging along a band of `length` x `width` about `center` in the plane with `normal`."""
    n, u, v = _frame(normal)
    k = np.arange(count)
    s = (k / (count - 1) - 0.5) * length
    w = np.where(k % 2 == 0, 0.5, -0.5) * width
    return (np.asarray(center, np.float64) + s[:, None] * u + w[:, None] * v + (bump * np.cos(3.0 * k))[:, None] * n).tolist()


# (a) the point sets: strokes in a tilted plane
_PN = [0.3, 0.8, 0.52]
_PC = np.array([0.11, 0.17, -0.06])
_BRUSH = dict(type="brush", normal=_PN, brushDepth=0.5, brushPressure=0.04, attenuationDistance=0.03, attenuationMode="linear", simplifyVoxel=16)
CURVE_CONFIG = dict(_BRUSH, brushType="curve", raw=ribbon_stroke(_PC, _PN, 0.26, 0.03, 0.04))
CURVE_DRY_CONFIG = dict(CURVE_CONFIG, attenuationMode="dry")
LINE_CONFIG = dict(_BRUSH, brushType="line", raw=band_stroke(_PC, _PN, 0.22, 0.05))
TWO_STROKE_CONFIG = dict(_BRUSH, brushType=["line", "curve"],
                         raw=[band_stroke(_PC - 0.16 * _frame(_PN)[2], _PN, 0.22, 0.05), ribbon_stroke(_PC, _PN, 0.26, 0.03, 0.04)])
CURVE_CONFIG_HSV = dict(CURVE_CONFIG, hsv=[0.2, -0.1, 0.05])
CURVE_CONFIG_RGB = dict(CURVE_CONFIG, rgb=[0.2, 0.6, 0.9], rgbLightOffset=0.1)
POINT_CONFIGS = {"curve": CURVE_CONFIG, "curve_dry": CURVE_DRY_CONFIG, "two_stroke": TWO_STROKE_CONFIG}

# (b) the rendered frame: a curve stroke on the torso's surface at azimuth 300 degrees (the fixture camera, at azimuth 30, sees it from
# the side) plus a line stroke next to it, raised outwards and hue-shifted.  The strokes are large on purpose: the edit has to change at
# least 100 pixels of a 64 x 64 frame (the generator requires it).
_N = np.array([-0.8660254037844386, 0.0, 0.5])                # the torso capsule's outward normal there
_A = np.array([0.0, 0.08, 0.0]) + 0.11 * _N
FRAME_CONFIG = dict(type="brush", normal=_N.tolist(), brushDepth=0.5, brushPressure=0.22, attenuationDistance=0.08, attenuationMode="linear",
                    simplifyVoxel=16, brushType=["curve", "line"], hsv=[0.33, 0.0, 0.0],
                    raw=[disc_stroke(_A, _N, 0.22, bump=0.004), band_stroke(_A + np.array([0.0, -0.36, 0.0]), _N, 0.3, 0.12, bump=0.004)])
FRAME_CONFIG_RGB = dict({k: v for k, v in FRAME_CONFIG.items() if k != "hsv"}, rgb=[0.2, 0.6, 0.9], rgbLightOffset=0.1)


# ----------------------------------------------------------------------------------------------------------------------
# the constructor's geometry, restated (seal_utils.py:304-383 with get_trimesh_box :595-596 and get_trimesh_fit :599-631)
# ----------------------------------------------------------------------------------------------------------------------
def _pca_box(points):
    """bounding_box_oriented's stand-in: the PCA-aligned box (vertex k = lo / hi per PCA axis by bits k&1, k>>1&1, k>>2)."""
    c = points.mean(0)
    _, _, vt = np.linalg.svd(points - c, full_matrices=False)
    q = (points - c) @ vt.T
    lo, hi = q.min(0), q.max(0)
    return np.stack([c + np.array([(hi if (k >> a) & 1 else lo)[a] for a in range(3)]) @ vt for k in range(8)])


def _fit_mesh(points, normal, growth, simplify_voxel):
    """get_trimesh_fit: 10 nearest neighbours by brute force ((distance, index) order, the point first), four faces per neighbour
    pair, vertex clustering with averaging (voxel = largest extent / simplify_voxel, grid origin = min bound - voxel / 2)."""
    n, K = points.shape[0], 10
    indices = []
    for i in range(n):
        d = np.sum((points - points[i]) ** 2, axis=1)
        order = sorted(range(n), key=lambda j: (-1.0 if j == i else d[j], j))
        indices.append(order[:K])
    faces = []
    for i in range(n):
        for j in range(1, K):
            for k in range(j + 1, K):
                x, y, z = i, indices[i][j], indices[i][k]
                faces += [[x, y, z], [x + n, y + n, z + n], [x, y, x + n], [x + n, y, y + n]]
    verts = np.concatenate([points + normal * growth[0], points + normal * growth[1]])
    voxel = (verts.max(0) - verts.min(0)).max() / simplify_voxel
    origin = verts.min(0) - voxel * 0.5
    cells = {}
    for vi, vtx in enumerate(verts):
        cells.setdefault(tuple(np.floor((vtx - origin) / voxel).astype(np.int64)), []).append(vi)
    new_index, new_verts = {}, []
    for ci, key in enumerate(sorted(cells)):
        new_verts.append(verts[cells[key]].sum(0) / len(cells[key]))
        for vi in cells[key]:
            new_index[vi] = ci
    kept = set()
    for f in faces:
        a, b, c = (new_index[v] for v in f)
        if a == b or b == c or a == c:
            continue
        lo = min(a, b, c)
        kept.add((a, b, c) if a == lo else (b, c, a) if b == lo else (c, a, b))
    return np.array(new_verts), np.array(sorted(kept), dtype=np.int64).reshape(-1, 3)


def brush_construction(cfg, surface_points_mask):
    """-> (map_data as the reference's __init__ fills it, triangles [F,3,3] float64, test_dir [1,3]).  surface_points_mask(triangles
    fp32 tensor, points fp32 tensor) -> bool tensor: the reference's `mesh_surface_points_mask`, passed in by the generator."""
    import torch
    strokes = cfg["raw"]
    if np.asarray(strokes[0]).ndim == 1:
        strokes = [strokes]
    kinds = cfg["brushType"]
    if isinstance(kinds, str):
        kinds = [kinds] * len(strokes)
    tris, bounds, border = [], [], []
    for pts, kind in zip(strokes, kinds):
        pts = np.asarray(pts, np.float64)
        centroid = pts.mean(0)
        u, _, _ = np.linalg.svd((pts - centroid).T, full_matrices=False)
        normal = u[:, -1]
        if "normal" in cfg and normal @ np.array(cfg["normal"]) < 0:
            normal = normal * -1
        normal_expand = normal * cfg["brushPressure"]
        projected = pts - ((pts - centroid) @ normal)[:, None] / (normal @ normal) * normal
        if kind == "line":
            t = _pca_box(np.vstack([pts + 2 * normal_expand, pts - cfg["brushDepth"] * normal_expand]))[BOX_FACES]
        else:
            v, f = _fit_mesh(projected, normal_expand, [-cfg["brushDepth"], 2], cfg["simplifyVoxel"] if "simplifyVoxel" in cfg else 16)
            t = v[f]
        tris.append(t)
        bounds.append(np.stack([t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)]))
        mask = surface_points_mask(torch.from_numpy(t).to(torch.float32), torch.from_numpy(projected).to(torch.float32)).numpy()
        border.append(projected[mask])
    md = {"force_fill_bound": np.array(bounds), "map_bound": np.array(bounds), "normal_expand": normal_expand, "center": centroid,
          "border_points": torch.from_numpy(np.concatenate(border)), "attenuation_distance": cfg["attenuationDistance"],
          "attenuation_mode": cfg["attenuationMode"]}
    if "hsv" in cfg:
        md["hsv"] = cfg["hsv"]
    if "rgb" in cfg:
        md["rgb"] = cfg["rgb"]
        md["rgb_light_offset"] = cfg["rgbLightOffset"] if "rgbLightOffset" in cfg else 0
    return md, np.concatenate(tris), normal_expand[None]


# ----------------------------------------------------------------------------------------------------------------------
# point sets and float64 evaluations
# ----------------------------------------------------------------------------------------------------------------------
def draw_points(bounds, n=N_POINTS, seed=61, n_zero=8, n_zero_one=8):
    """`n` seeded fp32 points of the strokes' bounds +- 0.03 (drawn per stroke in turn); the first `n_zero` are all-zero, the next
    `n_zero_one` have one zero coordinate (the reference's map_mask drops both, `points.all(1)`)."""
    b = np.asarray(bounds, np.float64).reshape(-1, 2, 3)
    rng = np.random.default_rng(seed)
    which = np.arange(n) % b.shape[0]
    p = (b[which, 0] - 0.03 + rng.uniform(0.0, 1.0, (n, 3)) * (b[which, 1] - b[which, 0] + 0.06)).astype(np.float32)
    p[:n_zero] = 0.0
    for k in range(n_zero, n_zero + n_zero_one):
        p[k, k % 3] = 0.0
    return p


def geometry(triangles, bounds, test_dir, normal_expand, center, border_points, attenuation_distance, mode):
    """The fp32 values an evaluation is given, as float64 arrays: what the float64 forms below take for exact."""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    return dict(tri=f(triangles).reshape(-1, 3, 3), bounds=f(bounds).reshape(-1, 2, 3), d=f(test_dir).reshape(3), ne=f(normal_expand).reshape(3),
                center=f(center).reshape(3), border=f(border_points).reshape(-1, 3), att=float(np.float32(attenuation_distance)), mode=mode)


def mapper_geometry(m):
    md = m.map_data
    return geometry(m.map_triangles.cpu().numpy(), md["map_bound"].cpu().numpy(), m.map_test_dir.cpu().numpy(), md["normal_expand"].cpu().numpy(),
                    md["center"].cpu().numpy(), md["border_points"].cpu().numpy(), float(md["attenuation_distance"]), md["attenuation_mode"])


def map_mask64(g, points, margin=MARGIN, chunk=500):
    """-> (strict [n] bool, loose [n] bool): map_mask in float64 with every threshold moved IN by `margin` (t, u, v >= margin, u + v <=
    1 - margin, the AABBs shrunk) and moved OUT by it.  Where the two agree the mask does not depend on rounding."""
    p = np.asarray(points, np.float64)
    tri, d = g["tri"], g["d"]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = np.cross(e1, e2)
    nonzero = (p != 0).all(1)
    out = []
    for m in (margin, -margin):
        box = np.zeros(p.shape[0], bool)
        for lo, hi in g["bounds"]:
            box |= ((hi - m > p) & (p > lo + m)).all(1)
        cand = np.nonzero(nonzero & box)[0]
        inside = np.zeros(p.shape[0], bool)
        for s in range(0, cand.size, chunk):
            idx = cand[s:s + chunk]
            a0 = p[idx, None] - v0[None]
            both = np.ones(idx.size, bool)
            for dd in (d, -d):
                invdet = 1.0 / -(nrm @ dd + 1e-8)
                c = np.cross(a0, dd)
                u = (c * e2[None]).sum(-1) * invdet
                v = -(c * e1[None]).sum(-1) * invdet
                t = (a0 * nrm[None]).sum(-1) * invdet
                both &= ((t >= m) & (u >= m) & (v >= m) & (u + v <= 1.0 - m)).any(1)
            inside[idx] = both
        out.append(inside)
    return out[0], out[1]


def clear_of_boundaries(g, points):
    """-> (clear [n] bool, mask64 [n] bool): the points whose mask is decided beyond rounding, asserting the cap on the others' share;
    and the float64 mask (the strict form: on clear points it is the loose one too)."""
    strict, loose = map_mask64(g, points)
    clear = strict == loose
    assert (~clear).mean() <= MARGIN_CAP, f"{int((~clear).sum())} of {clear.size} points lie within {MARGIN} of a predicate boundary"
    return clear, strict


def map_to_origin64(g, points, mask):
    """seal_utils.py:424-452 in float64 on the masked points -> (points' [n,3] float64, dist [n]: the projected point's distance to
    the nearest border point, NaN where unmasked)."""
    p = np.asarray(points, np.float64)
    out, dist = p.copy(), np.full(p.shape[0], np.nan)
    inner = p[mask]
    ne = g["ne"]
    q = inner - ((inner - g["center"]) @ ne)[:, None] / (ne @ ne) * ne
    dd = np.sqrt(((q[:, None] - g["border"][None]) ** 2).sum(-1)).min(1)
    dist[mask] = dd
    if g["mode"] == "linear":
        moved = inner - ne
        near = g["att"] > dd
        moved[near] += (np.abs(g["att"] - dd[near]) / g["att"])[:, None] * ne
        out[mask] = moved
    return out, dist
