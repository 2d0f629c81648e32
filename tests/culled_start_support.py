"""Inputs and CPU reference for the tests of the device loop's culled start (k_cull_start, cull_scan_range, ray_may_hit, lattice_floor,
certified_jump and the per-ray t_end cache): engineered occupancies, adversarial ray families, the numpy restatement of the cull grid
and the whole-ray march of the CPU oracle.  Everything is generated from seeds; nothing here needs a GPU.

Configuration: H = 128, C = 1, bound = 1, dt_gamma = 0 (the one the culled start applies to).  `MIN_NEAR` is lowered from the
scene's 0.2 to 0.05 so that a ray starting inside the cube has [near, far] across t = 0.125.

A family is a dict {ro [n,3], rd [n,3], tag [n]} of at most MAX_RAYS float32 rays: finite directions of length in [0.5, 2], origins
within 64 of the centre, no NaN near / far (no origin coordinate exactly on a cube face under a zero direction component)."""
import numpy as np

from tests_support import O

H, C, BOUND = 128, 1, 1.0
MIN_NEAR = 0.05
MAX_RAYS = 2048
AABB = np.array([-1, -1, -1, 1, 1, 1], np.float32)
ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))
VOX = 2.0 / 128                  # fine voxel width
CW = 2.0 / 32                    # cull cell width
K_TEND_DEAD, K_TEND_UNSET = np.float32(-1.0), np.float32(-2.0)
FINE_CACHE_CELLS = 4096
CROSS_EDGES = (0.125, 0.25, 0.5, 1.0, 2.0, 8.0, 16.0, 32.0)      # tag of a crosser = index into this
ORDINARY_EDGES = (2, 3, 4, 5)                                     # 0.5 .. 8


def f32(x):
    return np.asarray(x, np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# occupancies
# ------------------------------------------------------------------------------------------------------------------------
def bitfield_of(occ3):
    """occ3 [128,128,128] bool in (ix, iy, iz) order -> the Morton bitfield the marchers read."""
    from dnerf_amd import scene
    ix, iy, iz = np.nonzero(occ3)
    bits = np.zeros(H ** 3, np.uint8)
    bits[scene.morton3d(ix, iy, iz)] = 1
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1)


def occupancy_of(bitfield):
    """Morton bitfield -> occ3 [128,128,128] bool in (ix, iy, iz) order."""
    from dnerf_amd import scene
    bits = np.unpackbits(np.ascontiguousarray(bitfield, np.uint8), bitorder="little")
    g = np.arange(H)
    ix, iy, iz = np.meshgrid(g, g, g, indexing="ij")
    return (bits[scene.morton3d(ix.reshape(-1), iy.reshape(-1), iz.reshape(-1))] > 0).reshape(H, H, H)


def _voxels(*vox):
    occ = np.zeros((H, H, H), bool)
    for v in vox:
        occ[v] = True
    return occ


def _figure():
    from dnerf_amd import scene
    return occupancy_of(scene.jumpingjacks_occupancy(0.5))


def _two_slabs():
    occ = np.zeros((H, H, H), bool)
    occ[40:42, 40:88, 40:88] = True          # cull cell x = 10
    occ[88:90, 40:88, 40:88] = True          # cull cell x = 22: unmarked cells 12 .. 20 in between
    return occ


def _column():
    occ = np.zeros((H, H, H), bool)
    occ[2:126, 60:68, 60:68] = True          # a ray along x meets 124 occupied voxels in a row
    return occ


# name -> (occupancy builder, target voxel the ray families aim at)
OCCUPANCIES = {
    "one_voxel": (lambda: _voxels((66, 61, 70)), (66, 61, 70)),
    "corners": (lambda: _voxels((0, 0, 0), (127, 127, 127)), (0, 0, 0)),
    "box16": (lambda: _voxels((38, 37, 39), (90, 89, 91)), (38, 37, 39)),        # cells 9 and 22: marked 8 .. 23 on every axis
    "box17": (lambda: _voxels((38, 37, 39), (90, 89, 95)), (38, 37, 39)),        # z: cells 9 and 23: marked 8 .. 24
    "two_slabs": (_two_slabs, (40, 64, 64)),
    "figure": (_figure, None),
    "column": (_column, (64, 64, 64)),
}
_occ_cache = {}


def occupancy(name):
    """-> dict(occ3, bitfield, target [3] world point (an occupied voxel's centre), vox (its index), grid (cull_grid_reference))."""
    if name not in _occ_cache:
        build, vox = OCCUPANCIES[name]
        occ3 = build()
        if vox is None:                       # the figure: the occupied voxel nearest the centroid of the occupied ones
            idx = np.argwhere(occ3)
            vox = tuple(int(v) for v in idx[np.argmin(((idx - idx.mean(0)) ** 2).sum(1))])
        assert occ3[vox]
        target = (np.array(vox, np.float64) + 0.5) * VOX - 1.0
        _occ_cache[name] = dict(name=name, occ3=occ3, bitfield=bitfield_of(occ3), vox=vox, target=target, grid=cull_grid_reference(occ3))
    return _occ_cache[name]


def cull_grid_reference(occ3):
    """The cull grid restated: marks = 3x3x3 dilation of the 4^3 blocks that hold an occupied voxel, bit c = (z*32 + y)*32 + x of 1024
    words; meta = the marks' inclusive bounding box {x0, y0, z0, x1, y1, z1}, then the flag `the packed fine image is present` (the box
    holds at most 4096 cells) and a zero; image = one 64-bit word per block of the box, x fastest, bit = 2-bit Morton code of the voxel
    in its block (= the block's 64 consecutive bits of the Morton bitfield)."""
    from dnerf_amd import scene
    coarse = occ3.reshape(32, 4, 32, 4, 32, 4).any(axis=(1, 3, 5))
    pad = np.pad(coarse, 1)
    dil = np.zeros_like(coarse)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                dil |= pad[a:a + 32, b:b + 32, c:c + 32]
    marks = np.packbits(dil.transpose(2, 1, 0).reshape(-1).astype(np.uint8), bitorder="little").view(np.uint32)
    if dil.any():
        xs, ys, zs = np.nonzero(dil)
        lo, hi = np.array([xs.min(), ys.min(), zs.min()]), np.array([xs.max(), ys.max(), zs.max()])
    else:
        lo, hi = np.array([32, 32, 32]), np.array([-1, -1, -1])
    ext = hi - lo + 1
    fits = bool((ext > 0).all() and int(ext.prod()) <= FINE_CACHE_CELLS)
    meta = np.array(list(lo) + list(hi) + [1 if fits else 0, 0], np.int32)
    image = np.zeros(0, np.uint64)
    if fits:
        words = bitfield_of(occ3).view(np.uint64)            # word m = the block with Morton code m
        cz, cy, cx = np.meshgrid(np.arange(lo[2], hi[2] + 1), np.arange(lo[1], hi[1] + 1), np.arange(lo[0], hi[0] + 1), indexing="ij")
        image = words[scene.morton3d(cx.reshape(-1), cy.reshape(-1), cz.reshape(-1))]
    return dict(marks=marks, meta=meta, image=image, dil=dil, lo=lo, hi=hi, fits=fits,
                box_lo=lo * CW - 1.0, box_hi=(hi + 1) * CW - 1.0)


# ------------------------------------------------------------------------------------------------------------------------
# ray families
# ------------------------------------------------------------------------------------------------------------------------
def _ulp_steps(x, k):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def _offsets(x):
    """x and its neighbours at -1e-4, -1 ulp, 0, +1 ulp, +1e-4 (float32)."""
    return [np.float32(np.float32(x) - np.float32(1e-4)), _ulp_steps(x, -1), np.float32(x), _ulp_steps(x, 1), np.float32(np.float32(x) + np.float32(1e-4))]


def _pack(ro, rd, tag=None):
    ro, rd = f32(ro).reshape(-1, 3), f32(rd).reshape(-1, 3)
    tag = np.zeros(ro.shape[0], np.int32) if tag is None else np.asarray(tag, np.int32)
    ro, rd, tag = ro[:MAX_RAYS], rd[:MAX_RAYS], tag[:MAX_RAYS]
    return dict(ro=np.ascontiguousarray(ro), rd=np.ascontiguousarray(rd), tag=tag)


def _lateral_coords(occ, a):
    """Coordinates along axis `a` of interest to a ray that runs parallel to that axis' slabs: inside the target voxel (centre, on its
    faces, 1 ulp / 1e-4 either side) and beside the marked box (half a cull cell, exactly one cell, one and a half cells outside)."""
    v, g = occ["vox"][a], occ["grid"]
    lo_face, hi_face = v * VOX - 1.0, (v + 1) * VOX - 1.0
    out = [np.float32(occ["target"][a])] * 6 + _offsets(lo_face) + _offsets(hi_face)
    for edge, sgn in ((g["box_lo"][a], -1.0), (g["box_hi"][a], 1.0)):
        out += _offsets(edge)
        out += [np.float32(edge + sgn * 0.5 * CW)] + _offsets(edge + sgn * CW) + [np.float32(edge + sgn * 1.5 * CW)]
    return [c for c in out if abs(float(c)) < 1.0]           # inside the cube, never on its faces (0 * inf is NaN in near_far_from_aabb)


def family_axis(occ, seed=11):
    """Axis-parallel (two zero components) and plane-parallel (one zero component) rays, the zeros as +0.0 and as -0.0."""
    rng = np.random.default_rng(seed)
    ro, rd, tag = [], [], []
    zeros = (np.float32(0.0), np.float32(-0.0))
    lat = [_lateral_coords(occ, a) for a in range(3)]
    for k in range(MAX_RAYS):
        a = k % 3
        b, c = (a + 1) % 3, (a + 2) % 3
        sgn = 1.0 if (k // 3) % 2 == 0 else -1.0
        d, o = np.zeros(3, np.float32), np.zeros(3, np.float32)
        if k % 2 == 0:                       # along axis a
            d[a] = sgn * (1.0, 0.5, 2.0)[(k // 6) % 3]
            d[b], d[c] = zeros[(k // 2) % 2], zeros[(k // 4) % 2]
            o[a] = -sgn * rng.uniform(1.3, 2.5)
            o[b], o[c] = lat[b][rng.integers(len(lat[b]))], lat[c][rng.integers(len(lat[c]))]
            tag.append(0)
        else:                                # in the plane normal to axis a, through the target's (b, c)
            ang = rng.uniform(0, 2 * np.pi)
            d[a] = zeros[(k // 2) % 2]
            d[b], d[c] = np.cos(ang), np.sin(ang)
            L = rng.uniform(1.5, 2.5)
            o[a] = lat[a][rng.integers(len(lat[a]))]
            o[b], o[c] = occ["target"][b] - L * d[b], occ["target"][c] - L * d[c]
            tag.append(1)
        ro.append(o); rd.append(d)
    return _pack(ro, rd, tag)


def family_grazing(occ, seed=12):
    """Rays tangent to the marked bounding box and to the target voxel: in the plane of a face (exactly: a zero direction component and
    the face's coordinate), across an edge and across a corner, the contact point offset by 0, +-1 ulp and +-1e-4."""
    rng = np.random.default_rng(seed)
    g = occ["grid"]
    v = np.array(occ["vox"])
    boxes = [(v * VOX - 1.0, (v + 1) * VOX - 1.0), (np.array(g["box_lo"], np.float64), np.array(g["box_hi"], np.float64))]
    ro, rd, tag = [], [], []
    k = 0
    while len(ro) < MAX_RAYS:
        lo, hi = boxes[k % 2]
        kind = (k // 2) % 3                  # 0 face, 1 edge, 2 corner
        side = rng.integers(0, 2, 3)         # which of lo / hi per axis
        p = np.where(side == 1, hi, lo).astype(np.float64)
        off = (k // 6) % 5
        d = np.zeros(3)
        if kind == 0:
            a = int(rng.integers(3))
            b, c = (a + 1) % 3, (a + 2) % 3
            p[b], p[c] = rng.uniform(lo[b], hi[b]), rng.uniform(lo[c], hi[c])      # a point of the face
            ang = rng.uniform(0, 2 * np.pi)
            d[b], d[c] = np.cos(ang), np.sin(ang)
            d[a] = (0.0, -0.0)[(k // 30) % 2]     # (k % 2 picks the box: both boxes see both signs)
            pa = _offsets(p[a])[off]
            o = p - d * rng.uniform(1.2, 2.2)
            o[a] = pa
        elif kind == 1:
            e = int(rng.integers(3))         # the edge runs along e
            a, b = (e + 1) % 3, (e + 2) % 3
            p[e] = rng.uniform(lo[e], hi[e])
            d[a], d[b] = (1.0 if side[a] == 0 else -1.0), (-1.0 if side[b] == 0 else 1.0)   # across the edge, outside the box
            d[e] = rng.uniform(-0.5, 0.5)
            d /= np.linalg.norm(d)
            p[a], p[b] = _offsets(p[a])[off], _offsets(p[b])[off]
            o = p - d * rng.uniform(1.2, 2.2)
        else:
            n = np.where(side == 1, 1.0, -1.0)                                      # outward diagonal of the corner
            d = np.cross(n, rng.standard_normal(3))
            d /= np.linalg.norm(d)
            p = np.array([_offsets(p[i])[off] for i in range(3)], np.float64)
            o = p - d * rng.uniform(1.2, 2.2)
        k += 1
        if np.abs(np.abs(o) - 1.0).min() < 1e-6 or np.abs(o).max() > 60:
            continue
        ro.append(o); rd.append(d); tag.append(kind + 3 * ((k - 1) % 2))
    return _pack(ro, rd, tag)


def _aim(rng, n, target, wide_every=9):
    """n aim points: the target voxel jittered by +-0.6 voxel (hits), +-3 voxels (mostly misses) and, every `wide_every`-th, anywhere."""
    j = np.where((np.arange(n) % 2 == 0)[:, None], rng.uniform(-0.6, 0.6, (n, 3)), rng.uniform(-3, 3, (n, 3))) * VOX
    p = target[None, :] + j
    wide = np.arange(n) % wide_every == wide_every - 1
    p[wide] = rng.uniform(-0.9, 0.9, (int(wide.sum()), 3))
    return p


def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def family_crossers(occ, seed=13):
    """Rays whose [near, far] holds a binade edge of t: the aim point lies at distance edge + U(0.1, 0.9) from the origin (the edge
    falls into the empty lead before it), far away for 8, 16, 32.  The edges below 1 come two ways, eight rays of each in turn:
    origins INSIDE the cube, 0.6 .. 1.4 before the aim point (near = MIN_NEAR: the chain starts below every such edge), and origins
    OUTSIDE it at a matching distance from the face the ray enters through -- near in [0.07, 0.12], [0.13, 0.24], [0.26, 0.49] for the
    edges 0.125, 0.25, 0.5 -- so that the chain starts in the binade just below the edge and the lead holds the crossing."""
    rng = np.random.default_rng(seed)
    n = MAX_RAYS
    p = _aim(rng, n, occ["target"])
    tag = (np.arange(n) // 2) % len(CROSS_EDGES)            # (aim points alternate hit / miss: every edge gets both)
    edge = np.array(CROSS_EDGES)[tag]
    d = _unit(rng, n)
    dist = edge + rng.uniform(0.1, 0.9, n)
    low = edge < 1.0
    outside = low & ((np.arange(n) // 16) % 2 == 1)
    dist[low] = rng.uniform(0.6, 1.4, int(low.sum()))        # inside (or just outside) the cube: the target behind a lead of >= 0.5
    o = p - d * dist[:, None]
    # origins meant to be inside the cube: turn the direction until they are (the target is within ~1 of every face)
    for i in np.nonzero(low & ~outside)[0]:
        for _ in range(64):
            if np.abs(o[i]).max() < 0.98:
                break
            d[i] = _unit(rng, 1)[0]
            o[i] = p[i] - d[i] * dist[i]
    near_range = {0.125: (0.07, 0.12), 0.25: (0.13, 0.24), 0.5: (0.26, 0.49)}
    for i in np.nonzero(outside)[0]:
        with np.errstate(divide="ignore"):
            ta, tb = (-1.0 - p[i]) / d[i], (1.0 - p[i]) / d[i]
        t_in = np.minimum(ta, tb).max()                      # (negative: the aim point is inside the cube) where the line enters it
        o[i] = p[i] + d[i] * (t_in - rng.uniform(*near_range[float(edge[i])]))
    return _pack(o, d, tag)


def family_unnormalised(occ, seed=14):
    """Directions of length 0.5 and 2 through (or just past) the target, from outside the cube."""
    rng = np.random.default_rng(seed)
    n = MAX_RAYS // 2
    p = _aim(rng, n, occ["target"])
    d = _unit(rng, n)
    o = p - d * rng.uniform(2.2, 3.5, n)[:, None]
    scale = np.where(np.arange(n) % 4 < 2, 0.5, 2.0)
    return _pack(o, d * scale[:, None], (scale > 1).astype(np.int32))


def family_degenerate(occ, seed=15):
    """Near-degenerate segments on the `corners` occupancy: rays that clip the cube's corner (0,0,0)-side through or just past the
    corner voxel (near within a few steps of far), rays that miss the cube by a hair or by far, and long rays that END in the
    opposite corner cell."""
    rng = np.random.default_rng(seed)
    ro, rd, tag = [], [], []
    n_diag = np.array([-1.0, -1.0, -1.0])
    for k in range(MAX_RAYS // 2):
        kind = k % 4
        d = np.cross(n_diag, rng.standard_normal(3))
        d /= np.linalg.norm(d)
        if kind == 0:                        # through the corner voxel: a chord of a few steps
            p = -1.0 + rng.uniform(0.001, 0.014, 3)
        elif kind == 1:                      # past the voxel, inside marked cells: listed, no sample
            p = -1.0 + rng.uniform(0.03, 0.1) + rng.uniform(0, 0.01, 3)
        elif kind == 2:                      # misses the cube: by 1e-6 .. 1e-2, or looking away
            p = -1.0 - 10 ** rng.uniform(-6, -2) * np.ones(3)
        else:                                # a long ray that ends in the corner cell (31,31,31)
            p = 1.0 - rng.uniform(0.001, 0.014, 3)
            d = np.abs(_unit(rng, 1)[0])         # every component positive: towards the corner (1,1,1)
        L = rng.uniform(1.0, 3.0)
        ro.append(p - d * L); rd.append(d * (1.0, 0.5, 2.0)[(k // 4) % 3]); tag.append(kind)
    return _pack(ro, rd, tag)


FAMILIES = {"axis": family_axis, "grazing": family_grazing, "crossers": family_crossers, "unnormalised": family_unnormalised,
            "degenerate": family_degenerate}
# (occupancy, family, meant to jump): the cases of the stage test and of the loop test
PAIRS = [
    ("one_voxel", "axis", True), ("corners", "axis", True), ("box16", "axis", True), ("box17", "axis", True), ("two_slabs", "axis", True),
    ("one_voxel", "grazing", True), ("two_slabs", "grazing", True), ("box16", "grazing", True),
    ("one_voxel", "crossers", True), ("two_slabs", "crossers", True), ("figure", "crossers", True),
    ("one_voxel", "unnormalised", True), ("figure", "unnormalised", True), ("box17", "unnormalised", True),
    ("corners", "degenerate", True),
]
NOISE_KINDS = ("none", "mixed")


def noises_for(n, kind, seed=21):
    """None, or [n] float32 offsets: 0, the largest float below 1 and random values, interleaved."""
    if kind == "none":
        return None
    z = np.random.default_rng(seed).random(n, dtype=np.float32)
    z[0::4] = 0.0
    z[1::4] = ONE_BELOW
    return z


# ------------------------------------------------------------------------------------------------------------------------
# CPU reference
# ------------------------------------------------------------------------------------------------------------------------
def step_of(max_steps=1024):
    """The constant step of dt_gamma = 0: clamp(0, dt_min, dt_max) as the marcher's float32 expressions give it."""
    sqrt3 = np.float32(1.7320508075688772)
    dt_min = np.float32(2) * sqrt3 / np.float32(max_steps)
    dt_max = np.float32(2) * sqrt3 * np.float32(1 << (C - 1)) / np.float32(H)
    return np.float32(min(dt_max, max(dt_min, np.float32(0))))


def chain_start(nears, noises, max_steps=1024, dt_gamma=0.0):
    """t0 = near + step(near) * noise, in float32 as k_march_rays and the oracle evaluate it."""
    nears = f32(nears)
    if noises is None:
        return nears.copy()
    sqrt3 = np.float32(1.7320508075688772)
    dt_min = np.float32(2) * sqrt3 / np.float32(max_steps)
    dt_max = np.float32(2) * sqrt3 * np.float32(1 << (C - 1)) / np.float32(H)
    with np.errstate(over="ignore", invalid="ignore"):
        dt = np.minimum(dt_max, np.maximum(dt_min, (nears * np.float32(dt_gamma)).astype(np.float32))).astype(np.float32)
        return (nears + (dt * f32(noises)).astype(np.float32)).astype(np.float32)


def near_far(ro, rd):
    return O.near_far_from_aabb(ro, rd, AABB, MIN_NEAR)


def march_whole(ro, rd, bitfield, starts, fars, max_steps=1024, dt_gamma=0.0, n_step=None):
    """Every ray marched to its end by the oracle in ONE call, from rays_t = starts -> (xyzs, dirs, deltas) [n, n_step, .] and the
    per-ray sample count."""
    n = ro.shape[0]
    n_step = int(max_steps if n_step is None else n_step)
    alive = np.arange(n, dtype=np.int32)
    x, d, l = O.march_rays(n, n_step, alive, f32(starts), ro, rd, BOUND, bitfield, C, H, f32(starts), f32(fars), dt_gamma=dt_gamma,
                           max_steps=max_steps)
    x, d, l = x[: n * n_step].reshape(n, n_step, 3), d[: n * n_step].reshape(n, n_step, 3), l[: n * n_step].reshape(n, n_step, 2)
    return x, d, l, (l[:, :, 0] > 0).sum(1)


_case_cache = {}


def case(occ_name, fam_name, noise_kind, max_steps=1024, dt_gamma=0.0):
    """One (occupancy, family, noises) case with its CPU reference, computed once and shared (treat it as read-only):
    ro, rd, tag, nears, fars, noises, t0, and the oracle's whole-ray march from t0 (x, d, l, count), first_t (the parameter of each
    ray's first sample, +inf without one) and eligible (first sample more than 0.5 beyond t0)."""
    key = (occ_name, fam_name, noise_kind, max_steps, dt_gamma)
    if key not in _case_cache:
        occ = occupancy(occ_name)
        fam = FAMILIES[fam_name](occ)
        ro, rd = fam["ro"], fam["rd"]
        n = ro.shape[0]
        nears, fars = near_far(ro, rd)
        noises = noises_for(n, noise_kind)
        t0 = chain_start(nears, noises, max_steps, dt_gamma)
        x, d, l, count = march_whole(ro, rd, occ["bitfield"], t0, fars, max_steps, dt_gamma, n_step=max_steps + 8)   # (+ 8: the last iteration may overshoot the budget)
        keep = min(int(count.max()) + 1, l.shape[1])          # one empty slot behind the longest ray: a longer march shows
        x, d, l = np.ascontiguousarray(x[:, :keep]), np.ascontiguousarray(d[:, :keep]), np.ascontiguousarray(l[:, :keep])
        # the first sample's parameter: its second delta is (t_first + dt) - t0
        with np.errstate(invalid="ignore", over="ignore"):
            first_t = np.where(count > 0, (t0.astype(np.float64) + l[:, 0, 1].astype(np.float64)) - l[:, 0, 0].astype(np.float64), np.inf)
            eligible = (count > 0) & (first_t - t0.astype(np.float64) > 0.5)
        _case_cache[key] = dict(occ=occ, ro=ro, rd=rd, tag=fam["tag"], n=n, nears=nears, fars=fars, noises=noises, t0=t0, x=x, d=d, l=l,
                                count=count, first_t=first_t, eligible=eligible, max_steps=max_steps, dt_gamma=dt_gamma)
    return _case_cache[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def walk_visits(c, rays, starts):
    """Does the oracle's walk from t0 VISIT the parameter starts[k] of ray rays[k]?  Asked of the oracle itself: with the voxel
    that holds the point at `start` marked occupied as well, the walk from t0 emits its first sample where it first stands in that
    voxel -- at `start`, bit for bit, if and only if it visits it (the lead before it holds no other occupied voxel).  -> bool [k]."""
    from dnerf_amd import scene
    bf = c["occ"]["bitfield"].copy()
    out = np.zeros(len(rays), bool)
    one = np.zeros(1, np.int32)
    for k, (i, start) in enumerate(zip(rays, starts)):
        o, d, start = c["ro"][i], c["rd"][i], np.float32(start)
        p = np.clip((o + (start * d).astype(np.float32)).astype(np.float32), np.float32(-1), np.float32(1))
        v = np.clip(((p + np.float32(1)) * np.float32(64)).astype(np.float32), 0, 127).astype(np.int64)      # exact: scaling by powers of two
        m = int(scene.morton3d(v[0:1], v[1:2], v[2:3])[0])
        keep = bf[m >> 3]
        bf[m >> 3] = keep | np.uint8(1 << (m & 7))
        args = (c["ro"][i:i + 1], c["rd"][i:i + 1], BOUND, bf, C, H)
        far = c["fars"][i:i + 1]
        x0, _, l0 = O.march_rays(1, 1, one, c["t0"][i:i + 1], *args, far, far, max_steps=c["max_steps"], dt_gamma=c["dt_gamma"])
        x1, _, l1 = O.march_rays(1, 1, one, np.array([start], np.float32), *args, far, far, max_steps=c["max_steps"], dt_gamma=c["dt_gamma"])
        bf[m >> 3] = keep
        stands = l1[0, 0] > 0 and np.array_equal(bits(x1[0]), bits(p))          # the march from `start` samples AT start: right voxel
        out[k] = bool(stands and l0[0, 0] > 0 and np.array_equal(bits(x0[0]), bits(x1[0])))
    return out


def reference_schedule(counts, N, max_steps):
    """The reference's loop (dnerf/renderer.py:350-376) for rays that compositing never ends (T_thresh = 0: a ray leaves when a march
    gives it fewer samples than n_step): the trace [(n_alive, n_step)] from the per-ray whole-ray sample counts."""
    trace, step, done = [], 0, 0
    n_alive = N
    while step < max_steps and n_alive > 0:
        n_step = max(min(N // n_alive, 8), 1)
        trace.append((n_alive, n_step))
        done += n_step
        step += n_step
        n_alive = int((counts >= done).sum())
    return trace


def reference_loop(c, max_steps):
    """The reference's loop (dnerf/renderer.py:350-376) stepped with the oracle's march_rays and composite_rays for rays that compositing
    never ends (sigma = 0, T_thresh = 0): a perturbed first march included -- compositing advances rays_t from `near` by the deltas, as
    the reference does.  -> (trace [(n_alive, n_step)], samples emitted)."""
    N = c["n"]
    ws, dp, im = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32)
    alive = np.arange(N, dtype=np.int32)
    t = c["nears"].copy()
    trace, step, samples = [], 0, 0
    while step < max_steps and alive.shape[0] > 0:
        n_alive = alive.shape[0]
        n_step = max(min(N // n_alive, 8), 1)
        noises = c["noises"] if step == 0 else None          # (iteration 0 walks arange(N): list position == ray)
        x, d, l = O.march_rays(n_alive, n_step, alive, t, c["ro"], c["rd"], BOUND, c["occ"]["bitfield"], C, H, c["nears"], c["fars"], align=128,
                               dt_gamma=c["dt_gamma"], max_steps=max_steps, noises=noises)
        samples += int((l[: n_alive * n_step, 0] > 0).sum())
        O.composite_rays(n_alive, n_step, alive, t, np.zeros(x.shape[0], np.float32), np.zeros((x.shape[0], 3), np.float32), l, ws, dp, im, 0.0)
        trace.append((n_alive, n_step))
        alive = np.ascontiguousarray(alive[alive >= 0])
        step += n_step
    return trace, samples
