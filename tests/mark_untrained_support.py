"""Shared by the mark_untrained_grid tests and tests/golden/gen_mark_untrained_fixture.py: the fixture's inputs, its loader, and
the rule that decides which cells two fp32 evaluations of the frustum test may disagree on.

A camera sees a cell if min(cam.z, cx/fx*cam.z + 2*half - |cam.x|, cy/fy*cam.z + 2*half - |cam.y|) > 0.  torch's matmul and the kernel
may order the three products of cam = (p - t) @ R differently, so a cell whose margin is within fp32 rounding of zero can fall
either way.  A cell is BORDERLINE if, for any camera, |margin| < 1e-5 with the margin computed in float64: an order of magnitude
above the rounding of these expressions at scene scale <= 4 (|p - t| <= 8, ulp 1e-6, three products summed).  Every other cell must
agree exactly, and borderline cells may be at most 1e-3 of a cascade's cells -- the cap keeps the rule from hiding a failure."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "caller_mark_untrained.npz")
BORDER = 1e-5
CAP = 1e-3

# a deliberately narrow camera (half-angle atan(50 / 220) = 12.8 degrees): most of the grid is seen by nobody
INTRINSIC = (220.0, 220.0, 50.0, 50.0)
LOOK_AT = ((30.0, 30.0, 1.4), (150.0, 10.0, 1.6), (260.0, 50.0, 1.8))     # azimuth, elevation (degrees), radius
CASES = {"bound1": 1, "bound2": 2, "away": 1}                              # case -> bound


def look_at(azimuth_deg, elevation_deg, radius, away=False):
    """cam2world [4,4] float32 looking at the origin (columns right, down, forward, position); away: turned by 180 degrees."""
    az, el = np.radians(azimuth_deg), np.radians(elevation_deg)
    p = radius * np.array([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)])
    fwd = -p / np.linalg.norm(p)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, np.cross(fwd, right), fwd, p
    if away:
        pose[:3, 0], pose[:3, 2] = -pose[:3, 0], -pose[:3, 2]
    return pose.astype(np.float32)


def case_poses(name):
    if name == "away":          # one camera behind the grid with its back to it: every cell is marked
        return look_at(30.0, 30.0, 3.0, away=True)[None]
    return np.stack([look_at(*c) for c in LOOK_AT])


def morton_coords(H):
    """[H^3, 3] integer coordinates of the cells in Morton order (raymarching.cu:282-289)."""
    def compact(v):
        v = v & 0x49249249
        v = (v | (v >> 2)) & 0xc30c30c3
        v = (v | (v >> 4)) & 0x0f00f00f
        v = (v | (v >> 8)) & 0xff0000ff
        return (v | (v >> 16)) & 0x0000ffff
    i = np.arange(H ** 3, dtype=np.int64)
    return np.stack([compact(i), compact(i >> 1), compact(i >> 2)], axis=1)


def margins64(H, bound, cascade, poses, intrinsic):
    """[cascade, B, H^3] float64: each camera's deciding margin for every cell (Morton order); > 0 = the camera sees the cell."""
    fx, fy, cx, cy = (float(v) for v in intrinsic)
    poses = np.asarray(poses, np.float64)
    unit = 2.0 * morton_coords(H) / (H - 1) - 1.0
    out = np.empty((cascade, poses.shape[0], H ** 3))
    for cas in range(cascade):
        b = min(2 ** cas, bound)
        half = b / H
        for k, pose in enumerate(poses):
            cam = (unit * (b - half) - pose[:3, 3]) @ pose[:3, :3]
            z = cam[:, 2]
            out[cas, k] = np.minimum(z, np.minimum(cx / fx * z + 2 * half - np.abs(cam[:, 0]), cy / fy * z + 2 * half - np.abs(cam[:, 1])))
    return out


def borderline(H, bound, cascade, poses, intrinsic):
    """[cascade, H^3] bool; asserts the cap."""
    b = (np.abs(margins64(H, bound, cascade, poses, intrinsic)) < BORDER).any(axis=1)
    share = b.mean(axis=1)
    assert (share <= CAP).all(), f"borderline cells {share.tolist()} of a cascade exceed the cap {CAP}"
    return b


def assert_same_marks(got, want, border, what):
    """got / want [cascade, H^3] bool: equal on every cell that is not borderline; the counts agree within the borderline cells."""
    got, want = np.asarray(got, bool), np.asarray(want, bool)
    bad = (got != want) & ~border
    assert not bad.any(), (what, "cells off per cascade", bad.sum(axis=1).tolist(), "first", np.argwhere(bad)[:4].tolist())
    off = np.abs(got.sum(axis=1).astype(np.int64) - want.sum(axis=1).astype(np.int64))
    assert (off <= border.sum(axis=1)).all(), (what, "counts", got.sum(axis=1).tolist(), want.sum(axis=1).tolist())


def load_case(name):
    """One case of the fixture: poses, intrinsic, bound, cascade, grid_size, marked [cascade], unseen [cascade, H^3] bool (Morton
    order), border [cascade, H^3] bool (recomputed here; the share the generator recorded must match)."""
    fx = np.load(FIXTURE)
    g = lambda k: fx[f"{name}_{k}"]   # noqa: E731
    H, cascade, bound = int(g("grid_size")), int(g("cascade")), float(g("bound"))
    unseen = np.unpackbits(g("unseen_bits"), axis=1, bitorder="little").astype(bool)
    assert unseen.shape == (cascade, H ** 3) and (unseen.sum(axis=1) == g("marked")).all()
    border = borderline(H, bound, cascade, g("poses"), g("intrinsic"))
    assert np.allclose(border.mean(axis=1), g("borderline_share"), rtol=0, atol=1e-9)
    return dict(poses=g("poses"), intrinsic=tuple(float(v) for v in g("intrinsic")), bound=bound, cascade=cascade, grid_size=H,
                marked=g("marked").astype(np.int64), unseen=unseen, border=border)
