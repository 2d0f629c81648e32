"""Inputs shared by the brush texture stamp's fixture generator (tests/golden/gen_image_fixture.py) and its tests: the procedural
textures, the stamp's rectangle over the brush fixture's curve stroke and over its frame's disc stroke, the seal configs, and the
float64 texel coordinates that say where an fp32 evaluation of the texel index may round either way."""
import os

import numpy as np

import seal_brush_support as BS

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caller_seald_image.npz")

W, H = 24, 16          # wider than high, so that a swapped index shows
CLEAR = 1e-3           # a point is clear if both float64 texel coordinates are this far from every integer 1..W-1 / 1..H-1
CLEAR_CAP = 0.02       # ... and at most this share of the masked points may be unclear (uniform points: 1 - (1 - 2e-3)^2 = 0.4 %)
LIGHT_OFFSET = 0.1
RGB = [0.2, 0.6, 0.9]


def stamp_texture():
    """-> uint8 [H, W, 4]: a distinct colour per texel -- a row of greys (delta 0: hue and saturation 0), the pure primaries, black and
    white among them --, columns 0..7 transparent (alpha 0), columns 8..11 a band of fractional alpha (every value distinct, 1..254),
    columns 12..23 opaque."""
    y, x = np.mgrid[0:H, 0:W]
    rgba = np.stack([(x * 10 + y + 7) % 256, (y * 15 + x * 3 + 20) % 256, (250 - x * 9 - y * 5) % 256, np.full_like(x, 255)], -1).astype(np.uint8)
    rgba[3, 2:8, :3] = (np.arange(6) * 40 + 15)[:, None]
    rgba[3, 14:20, :3] = (np.arange(6) * 40 + 25)[:, None]
    rgba[12, 14:17, :3] = [[255, 0, 0], [0, 255, 0], [0, 0, 255]]
    rgba[12, 4:7, :3] = [[0, 255, 255], [255, 0, 255], [255, 255, 0]]
    rgba[5, 20, :3], rgba[6, 20, :3] = 0, 255
    rgba[:, :8, 3] = 0
    rgba[:, 8:12, 3] = (8 + 15 * y + 3 * (x - 8))[:, 8:12]
    flat = rgba[..., :3].reshape(-1, 3)
    assert np.unique(flat, axis=0).shape[0] == flat.shape[0], "every texel has its own colour"
    band = rgba[:, 8:12, 3]
    assert band.min() >= 1 and band.max() <= 254 and np.unique(band).size == band.size
    return rgba


def index_texture():
    """-> uint8 [H, W, 3], no alpha: the column coded in the hue, the row in the saturation, every value 1 (brightest channel 255), so
    that the texel a sample was given can be read off its output colour (`decode_index`) whatever the sample's own colour was."""
    y, x = np.mgrid[0:H, 0:W]
    h6 = (x + 0.5) / W * 6.0
    s = 0.3 + 0.7 * y / (H - 1)
    c, m = s, 1.0 - s
    xx = c * (1.0 - np.abs(h6 % 2.0 - 1.0))
    k = h6.astype(np.int64) % 6
    z = np.zeros_like(c)
    table = [(c, xx, z), (xx, c, z), (z, c, xx), (z, xx, c), (xx, z, c), (c, z, xx)]
    rgb = np.zeros((H, W, 3))
    for q, (r, g, b) in enumerate(table):
        rgb = np.where((k == q)[..., None], np.stack([r, g, b], -1), rgb)
    return np.round((rgb + m[..., None]) * 255).astype(np.uint8)


def hue_saturation(rgb):
    """float64 (hue / 6, saturation) of colours [..., 3] with a positive value and delta."""
    rgb = np.asarray(rgb, np.float64)
    cmax, cmin = rgb.max(-1), rgb.min(-1)
    delta = cmax - cmin
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    safe = np.where(delta == 0, 1.0, delta)
    h = np.where(cmax == r, ((g - b) / safe) % 6.0, np.where(cmax == g, (b - r) / safe + 2.0, (r - g) / safe + 4.0))
    return h / 6.0, delta / np.where(cmax == 0, 1.0, cmax)


def decode_index(colors):
    """Output colours of a stamp with `index_texture` -> (idx_w, idx_h): the texel whose (hue, saturation) is nearest.  The output's
    value is 1 + (V - mean V) of the sample >= 0.2 for colours of [0, 1] with a mean V near 0.75, so hue and saturation survive; the
    texels' hues are 1/24 apart, their saturations 0.047, rounding to 8 bits moves either by < 0.004."""
    th, ts = hue_saturation(index_texture().astype(np.float64) / 255)
    h, s = hue_saturation(colors)
    dh = np.abs(h[:, None] - th.reshape(-1)[None])
    d = np.minimum(dh, 1.0 - dh) * 24.0 + np.abs(s[:, None] - ts.reshape(-1)[None]) / (0.7 / (H - 1))
    best = d.argmin(1)
    assert float(d.min(1).max()) < 0.25, "an output colour is not close to any texel's hue and saturation"
    return best % W, best // W


def write_png(path, array):
    from PIL import Image
    Image.fromarray(array, "RGBA" if array.shape[2] == 4 else "RGB").save(path)
    return str(path)


def rectangle(center, normal, along, across, turn_deg, lift=(0.08, -0.05)):
    """o, w, h of a `along` x `across` parallelogram about `center`: the frame of the plane with `normal` (seal_brush_support._frame)
    turned by `turn_deg` in the plane, each edge leaning out of it by `lift`: tilted against the axes and against the stroke's plane."""
    n, u, v = BS._frame(normal)
    a = np.deg2rad(turn_deg)
    e1 = np.cos(a) * u + np.sin(a) * v + lift[0] * n
    e2 = -np.sin(a) * u + np.cos(a) * v + lift[1] * n
    e1, e2 = e1 / np.linalg.norm(e1), e2 / np.linalg.norm(e2)
    o = np.asarray(center, np.float64) - 0.5 * along * e1 - 0.5 * across * e2
    return dict(o=o.tolist(), w=(o + along * e1).tolist(), h=(o + across * e2).tolist())


# (a) the point set: the brush fixture's curve stroke (0.26 long, ~0.1 across); the rectangle is smaller than its bounds on every side
RECT = rectangle(BS._PC, BS._PN, 0.17, 0.055, 12.0)
# (b) the frame: the brush fixture's frame strokes without their hue shift, the stamp over the disc (curve) stroke of radius 0.22
FRAME_RECT = rectangle(BS._A, BS._N, 0.3, 0.2, 20.0)


def point_config(path, rgb=False):
    cfg = dict(BS.CURVE_CONFIG, imageConfig=dict(RECT, path=path), rgbLightOffset=LIGHT_OFFSET)
    return dict(cfg, rgb=RGB) if rgb else cfg


def frame_config(path):
    return dict({k: v for k, v in BS.FRAME_CONFIG.items() if k != "hsv"}, imageConfig=dict(FRAME_RECT, path=path), rgbLightOffset=LIGHT_OFFSET)


def texel_coordinates64(points, rect=RECT):
    """The float64 texel coordinates (column, row, before floor and clamp) of fp32 points for the fp32-rounded rectangle: what an
    evaluation in exact arithmetic is given -> (u [n], v [n], clear [n] bool, idx_w, idx_h)."""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    p, o, w, h = f(points), f(rect["o"]), f(rect["w"]), f(rect["h"])
    c = np.stack([o, w, h]).mean(0)
    nrm = np.linalg.svd((np.stack([o, w, h]) - c).T, full_matrices=False)[0][:, -1]
    nrm = f(nrm)
    q = p - ((p - o) @ nrm)[:, None] / (nrm @ nrm) * nrm
    op, ow, oh = q - o, w - o, h - o
    u = op @ ow / (ow @ ow) * W
    v = op @ oh / (oh @ oh) * H
    clear = (np.abs(u[:, None] - np.arange(1, W)[None]).min(1) >= CLEAR) & (np.abs(v[:, None] - np.arange(1, H)[None]).min(1) >= CLEAR)
    return u, v, clear, np.clip(np.floor(u), 0, W - 1).astype(np.int64), np.clip(np.floor(v), 0, H - 1).astype(np.int64)
