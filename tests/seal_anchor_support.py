"""Inputs shared by the anchor seal mapper's fixture generator (tests/golden/gen_anchor_fixture.py) and its tests: the seal
configs, the seeded point sets, and the float64 distances of a point from the three predicate boundaries of
`SealAnchorMapper.map_to_origin` (SealNeRF/seal_utils.py:545-551), which say where an fp32 evaluation may round either way."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caller_seald_anchor.npz")

# (a) the point sets: a tilted plane through four (not exactly coplanar) points, a generic translation
POINTS_CONFIG = dict(type="anchor", radius=0.12, translation=[0.05, 0.18, -0.04], scale=[1.0, 1.2, 0.9],
                     raw=[[0.16, 0.21, -0.02], [0.04, 0.23, -0.09], [0.05, 0.18, 0.01], [0.15, 0.17, -0.10]])
POINTS_CONFIG_HSV = dict(POINTS_CONFIG, hsv=[0.2, -0.1, 0.05])
POINTS_CONFIG_RGB = dict(POINTS_CONFIG, rgb=[0.2, 0.6, 0.9], rgbLightOffset=0.1)

# (b) the rendered frame: the anchor on the torso's surface at azimuth 300 degrees (the fixture camera, at azimuth 30, sees the cone
# from the side), pulled straight out, hue-shifted.  The cone is large on purpose: the edit has to show through the filled box
# around it in at least 100 pixels of a 64 x 64 frame (the generator requires it).
_N = np.array([-0.8660254037844386, 0.0, 0.5])                # the torso capsule's outward normal there
_A = np.array([0.0, 0.08, 0.0]) + 0.11 * _N
_U, _V = np.array([0.0, 1.0, 0.0]), np.cross(_N, [0.0, 1.0, 0.0])
FRAME_CONFIG = dict(type="anchor", radius=0.35, translation=(0.6 * _N).tolist(), scale=[1.0, 1.0, 1.0], hsv=[0.33, 0.0, 0.0],
                    raw=[(_A + 0.05 * a * _U + 0.05 * b * _V).tolist() for a, b in ((1, 0), (0, 1), (-1, 0), (0, -1))])

MARGIN = 1e-5          # points closer than this to a predicate boundary (in float64) may fall on either side in fp32
MARGIN_CAP = 0.005     # ... and they may be at most this share of a point set


def anchor_geometry(cfg):
    """The constructor's plane geometry (seal_utils.py:477-489) in float64 -> dict(v_anchor, v_offset, v_h, len_h)."""
    raw = np.asarray(cfg["raw"], np.float64)
    t = np.asarray(cfg["translation"], np.float64)
    v_anchor = raw.mean(0)
    u, _, _ = np.linalg.svd((raw - v_anchor).T, full_matrices=False)
    n = u[:, -1]
    projected = (v_anchor + t) - ((v_anchor + t - v_anchor) @ n) * n
    v_h = projected - (v_anchor + t)
    return dict(v_anchor=v_anchor, v_offset=projected - v_anchor, v_h=v_h, len_h=np.linalg.norm(v_h))


def draw_points(cfg, n, n_zero, seed, n_zero_y=0):
    """`n` seeded fp32 points of v_anchor +- 0.2 (about 4 % of them lie in the cone); the first `n_zero` are all-zero, the next
    `n_zero_y` have a zero y (the reference's map_mask drops points with a zero coordinate, `points.all(1)`)."""
    rng = np.random.default_rng(seed)
    p = (anchor_geometry(cfg)["v_anchor"] + rng.uniform(-0.2, 0.2, (n, 3))).astype(np.float32)
    p[:n_zero] = 0.0
    p[n_zero:n_zero + n_zero_y, 1] = 0.0
    return p


def predicates64(cfg, points):
    """-> (valid [n] bool, margin [n]): map_to_origin's valid_mask evaluated in float64, and each point's distance from the nearest of
    the three predicate boundaries: |pop - radius|, |d - 1.1 len_h / radius (radius - pop)| where pop < radius, and the distance d to
    the anchor plane."""
    g = anchor_geometry(cfg)
    p = np.asarray(points, np.float64)
    radius = float(cfg["radius"])
    h = g["v_h"]
    proj = p - ((p - g["v_anchor"]) @ h)[:, None] / (h @ h) * h
    to_plane = proj - p
    d = np.linalg.norm(to_plane, axis=1)
    pop = np.linalg.norm(proj - (d / g["len_h"])[:, None] * g["v_offset"] - g["v_anchor"], axis=1)
    slope = 1.1 * g["len_h"] / radius
    with np.errstate(divide="ignore", invalid="ignore"):
        cone = (pop <= radius) & (d / (radius - pop) < slope)
    valid = cone & (to_plane @ h > 0)
    margin = np.minimum(np.abs(pop - radius), d)
    margin = np.where(pop < radius, np.minimum(margin, np.abs(d - slope * (radius - pop))), margin)
    return valid, margin


def clear_of_boundaries(cfg, points):
    """-> bool [n]: the points whose mask is decided beyond rounding; asserts the cap on the others' share."""
    _, margin = predicates64(cfg, points)
    clear = margin > MARGIN
    assert (~clear).mean() <= MARGIN_CAP, f"{int((~clear).sum())} of {clear.size} points lie within {MARGIN} of a predicate boundary"
    return clear
