"""Probe weights for the fused field kernels (csrc/field_f16_net.h, field.hip, field_pp.inc, field_f32*.hip): model weights under which the
kernels' own outputs are read-outs of ONE internal stage, the engineered point sets, the expected values from the CPU oracle and the bars.

Every layer of the field network is a bias-free Linear with ReLU, so a value v is carried through a ReLU stack exactly: a hidden layer
holds relu(+v) and relu(-v) in two units (weights +-1), the next layer keeps or subtracts them.  All products are by +-1 (or a power of
two) or 0 and one addend of every sum is zero: the result is exact on the fp16 MFMAs (fp32 accumulation, fp16 store of an fp16 value),
on the fp32 MFMAs and in oracle/field.py's `_mlp`.  Then
    sigma = density_scale * exp(fp16 logit)   (fp32)      and      rgb = fp16(sigmoid(fp16 logit))
read the logit back.  tests/test_field_probes_cpu.py checks all of this file against `FieldOracle` and shows that each bar rejects a
named wrong variant; tests/test_gpu_field_probes.py holds the kernels to it.

A "state" is a plain dict of numpy arrays with the model's state_dict keys (what `oracle.render.state_of` returns)."""
import ctypes
import itertools

import numpy as np

from oracle import oracle as O

f32 = np.float32
LEVELS, H_BASE, LOG2_T = 16, 16, 19
F_SMALL = 2.0 ** -6          # below this a feature is compared by distance, not bit for bit
# ---- the bar of the grid stage, fp16 kernel ---------------------------------------------------------------------------------------------
# The kernel computes sigma = density_scale * v_exp_f32(h * log2(e)), h the fp16 logit (field_f16_net.h: density).  The product
# h * log2(e) is rounded to fp32: relative 2^-24, i.e. |h| 2^-24 in the exponent (log2(e) itself is the fp32 constant: another
# |h| 2^-25); the hardware exp2 is documented at 1 ulp: relative 2^-23 of sigma = 2^-23 in the natural-log exponent; density_scale = 1
# multiplies exactly.  Decoding f = log(sigma / density_scale) in float64 therefore returns h within
#     2^-23 + 1.5 |h| 2^-24 * ln 2 ... < 1.2e-7 + 0.9e-7 |h|  <  1e-6   for |h| <= 1 (the table's magnitudes bound the features by 1).
# An fp16 value at or above 2^-6 has its neighbours at least 2^-17 = 7.6e-6 away (one ulp just below 2^-6), so float16(f) is the
# kernel's logit bit for bit; below 2^-6 the fp16 grid is finer than the decode error and the distance is held to DECODE_BAR instead.
DECODE_BAR = 2e-6
MAX_SMALL_SHARE = 0.10       # at most this share of (point, feature) pairs may fall under F_SMALL: the exact part must carry the test
# fp32 kernels.  field_f32_net.h:trilinear is written to BE the oracle's arithmetic: the same weights w = ((1 * a) * b) * c in corner
# order, results = results + w * val per corner in corner order, and csrc is built with -ffp-contract=off, so every operation rounds as
# oracle/sdn_oracle.c's does; the fp32-MFMA kernel passes the feature through +-1 weights exactly and the only error is the decode of
# expf (OCML, 1 ulp: the same term as above): DECODE_BAR.  The split kernel (field_f32x3.hip) carries activations as hi + lo fp16 pairs,
# 22 bits: it is not the oracle's arithmetic and keeps the project's bar for it (tests/test_gpu_field_f32.py: 2.5e-4 relative on
# sigma = 2.5e-4 absolute on the logit).
F32_BAR = {"mfma32": DECODE_BAR, "split": 2.5e-4}
# project's fp32 bars on an output (tests/test_gpu_field_f32.py): relative, with an absolute floor
F32_OUT_RTOL = {"mfma32": 1e-4, "split": 2.5e-4}
GAIN = 4.0                   # colour logit = GAIN * (one input of the colour net): inputs lie in about [-1.5, 1.5]
DEFORM_G = 0.25              # dx = DEFORM_G * (one input of the first deformation layer): |dx| <= 0.25 (0.5 for the raw coordinate at bound 2)


def ulp16(v):
    """Size of one fp16 ulp at |v| (the subnormal spacing below 2^-14)."""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    return np.exp2(np.floor(np.log2(a)) - 10)


def f16_step(h, up):
    """The fp16 neighbour of every element of the fp16 array h, one ulp up or down."""
    return np.nextafter(h, np.float16(np.inf if up else -np.inf))


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
class Geometry:
    """The model's grid: 16 levels x 2, base 16, finest 2048 bound, 2^19 rows at most, tiled (gridencoder/grid.py:100-128); per level the
    constants of kernel_grid (gridencoder.cu:66-84,138-139) from the oracle's own float32 expression."""

    def __init__(self, bound=1):
        self.bound = float(bound)
        self.offsets, self.pls = O.grid_offsets(3, LEVELS, 2, 2, H_BASE, LOG2_T, 2048 * bound, False)
        self.S = f32(np.log2(self.pls))
        self.rows = int(self.offsets[-1])
        self.levels = []
        for l in range(LEVELS):
            sc, res = ctypes.c_float(), ctypes.c_uint32()
            O.lib().orc_grid_level_params(O.u32(l), O.f32(float(self.S)), O.u32(H_BASE), ctypes.byref(sc), ctypes.byref(res))
            hs, res = int(self.offsets[l + 1] - self.offsets[l]), int(res.value)
            s1 = res + 1 if res + 1 <= hs else 0
            s2 = (res + 1) ** 2 if s1 and (res + 1) ** 2 <= hs else 0
            self.levels.append(dict(l=l, off=int(self.offsets[l]), hs=hs, scale=f32(sc.value), res=res, s1=s1, s2=s2,
                                    capped=(res + 1) ** 3 > hs))
        self.capped = [lv["l"] for lv in self.levels if lv["capped"]]
        assert all(self.levels[l]["hs"] == 2 ** LOG2_T for l in self.capped) and self.capped and self.capped[0] > 0

    def u_of(self, x):
        """GridEncoder.forward (grid.py:149) in float32."""
        return ((np.asarray(x, f32) + f32(self.bound)) / f32(2 * self.bound)).astype(f32)

    def cell_rows(self, x, l):
        """Index arithmetic of level l for undeformed points: (q = u scale + 0.5, low-corner cell, unwrapped low-corner row)."""
        lv = self.levels[l]
        q = (self.u_of(x) * lv["scale"] + f32(0.5)).astype(f32)
        cell = np.floor(q).astype(np.int64)
        return q, cell, cell[:, 0] + cell[:, 1] * lv["s1"] + cell[:, 2] * lv["s2"]


def random_table(geo, seed=0):
    """Seeded fp16 table, magnitudes in [0.25, 1], random sign: every row is distinct in practice and interpolated features are rarely tiny."""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.25, 1.0, (geo.rows, 2))
    return (mag * rng.choice([-1.0, 1.0], (geo.rows, 2))).astype(np.float16)


def ramp_table(geo, axis):
    """Level 0 (dense, 17^3 rows, row = i + 17 j + 289 k) channel 0 = the cell coordinate of `axis` / 16, everything else zero: trilinear
    interpolation of a linear function is linear, so feature 0 is (u_axis scale_0 + 0.5) / 16 to the rounding of the fp16 arithmetic."""
    lv = geo.levels[0]
    assert not lv["capped"] and lv["res"] == 16 and lv["s1"] == 17 and lv["s2"] == 289
    t = np.zeros((geo.rows, 2), np.float16)
    r = np.arange(17 ** 3)
    t[lv["off"] + r, 0] = ((r // 17 ** axis) % 17 / 16.0).astype(np.float16)
    return t


# ---- a numpy restatement of kernel_grid with named wrong variants ------------------------------------------------------------------------
def grid_features(geo, u, table, variant=None, vlevel=None):
    """kernel_grid (gridencoder.cu:87-245; oracle/sdn_oracle.c: orc_grid_encode_forward) for the tiled D = 3, C = 2 grid, vectorised:
    -> [N, 32] in the table's dtype.  An fp16 table runs the at::Half arithmetic (two roundings per corner), an fp32 one plain float32.
    variant (applied at level `vlevel`, or at every level when that is None) names one WRONG kernel, for the CPU test of the bars:
      swap_x        the corner order swapped in x (the weights keep theirs)
      clamp         the x + 1 corner's row clamped at hs - 1 instead of (index + 1) % hs
      no_zero       out-of-range points keep the features of the clamped position
      ge1           `>= 1` instead of `> 1` in the range test
      swap_ch       the level's two channels swapped
      one_round     Half(float(acc) + w * val): one rounding per corner
      scale_no_m1   scale = exp2(l S) H, without the - 1"""
    half = table.dtype == np.float16
    u = np.asarray(u, f32)
    N = u.shape[0]
    out = np.zeros((N, 2 * LEVELS), table.dtype)
    tab = table.astype(f32)
    for lv in geo.levels:
        on = variant if (vlevel is None or vlevel == lv["l"]) else None
        oob = ((u < 0) | ((u >= 1) if on == "ge1" else (u > 1))).any(1)
        scale = f32(lv["scale"] + f32(1)) if on == "scale_no_m1" else lv["scale"]
        uu = np.clip(u, 0, 1) if on == "no_zero" else u
        q = (uu * scale + f32(0.5)).astype(f32)
        pg = np.floor(q)
        fr = (q - pg.astype(f32)).astype(f32)
        pg = pg.astype(np.int64)
        acc = np.zeros((N, 2), f32)
        hs, s1, s2 = lv["hs"], lv["s1"], lv["s2"]
        for idx in range(8):
            w = np.ones(N, f32)
            for d in range(3):
                w = (w * (fr[:, d] if idx & (1 << d) else f32(1) - fr[:, d])).astype(f32)
            bx = (idx & 1) ^ 1 if on == "swap_x" else idx & 1
            rest = (pg[:, 1] + ((idx >> 1) & 1)) * s1 + (pg[:, 2] + ((idx >> 2) & 1)) * s2
            if on == "clamp" and bx:
                row = np.minimum((pg[:, 0] + rest) % hs + 1, hs - 1)
            else:
                row = (pg[:, 0] + bx + rest) % hs
            val = tab[lv["off"] + row]
            if on == "swap_ch":
                val = val[:, ::-1]
            t = (w[:, None] * val).astype(f32)
            if half and on != "one_round":
                t = t.astype(np.float16).astype(f32)
            acc = (acc + t).astype(f32)
            if half:
                acc = acc.astype(np.float16).astype(f32)
        if on != "no_zero":
            acc[oob] = 0
        out[:, 2 * lv["l"]:2 * lv["l"] + 2] = acc.astype(table.dtype)
    return out


def oracle_features(geo, x, table):
    """The expected features of undeformed points: the oracle's grid encoder on the table as it is (fp16: at::Half arithmetic)."""
    enc, _ = O.grid_encode_forward(geo.u_of(x), table, geo.offsets, geo.pls, H_BASE, False, 1, False, 0)
    return enc


# ---- point sets -------------------------------------------------------------------------------------------------------------------------------
def _cells_with_row(lv, target, rng, want=3):
    """Cells of a capped level whose low corner's row (index % hs) is `target`, every corner inside the level."""
    n1 = lv["res"] + 1
    total = n1 ** 3 if lv["s2"] else n1 ** 2
    ks = np.arange((total - target + lv["hs"] - 1) // lv["hs"])
    if ks.shape[0] > 4096:
        ks = rng.choice(ks, 4096, replace=False)
    T = target + ks * lv["hs"]
    p0, p1 = T % n1, (T // n1) % n1
    p2 = T // n1 ** 2 if lv["s2"] else rng.integers(1, lv["res"] - 1, T.shape[0])
    cells = np.stack([p0, p1, p2], 1)
    ok = ((cells >= 1) & (cells <= lv["res"] - 2)).all(1)
    if not ok.any():
        ok = ((cells >= 0) & (cells <= lv["res"] - 1)).all(1)
    return cells[ok][:want]


def point_sets(geo, seed=1, n_uniform=1536):
    """The engineered points of the grid stage, as one float32 array [N, 3] plus {name: index array}.  Each set is built here and
    ASSERTED from the index arithmetic by `assert_coverage` (the CPU test, and again the GPU test before it launches)."""
    rng = np.random.default_rng(seed)
    b = geo.bound
    parts, names = [], []

    def add(name, pts):
        parts.append(np.asarray(pts, np.float64).reshape(-1, 3).astype(f32))
        names.append(name)

    add("first", rng.uniform(-0.9 * b, 0.9 * b, (1, 3)))      # (a one-point launch evaluates an ordinary point)
    # u exactly 0 and 1: the eight corners and the six face centres; the box centre u = 0.5
    add("corners", [[sx, sy, sz] for sx in (-b, b) for sy in (-b, b) for sz in (-b, b)])
    add("faces", [np.eye(3)[a] * s * b for a in range(3) for s in (-1, 1)] + [[0, 0, 0]])
    # just outside on each axis (the other coordinates inside), and one point far outside
    # (nextafter(+bound) is NOT outside: x + bound rounds back to 2 bound in float32 and u == 1, in range -- kept as its own set; the
    #  first x above it whose u exceeds 1 is two steps out.  Below -bound the sum is exact and one step is outside.)
    out, edge = rng.uniform(-0.9 * b, 0.9 * b, (6, 3)).astype(f32), rng.uniform(-0.9 * b, 0.9 * b, (3, 3)).astype(f32)
    for a in range(3):
        edge[a, a] = np.nextafter(f32(b), f32(np.inf))
        out[2 * a, a] = np.nextafter(edge[a, a], f32(np.inf))
        out[2 * a + 1, a] = np.nextafter(f32(-b), f32(-np.inf))
    add("outside", np.concatenate([out, [[5.0 * b, 0.3 * b, -0.2 * b]]]))
    add("edge_in", edge)
    # wrap rows on every capped level: cells whose low corner is hs-1, hs-1-s1, hs-1-s2, hs-1-s1-s2
    for l in geo.capped:
        lv = geo.levels[l]
        pts = []
        for target in sorted({lv["hs"] - 1 - a * lv["s1"] - c * lv["s2"] for a in (0, 1) for c in (0, 1)}):
            for cell in _cells_with_row(lv, target, rng):
                for _ in range(3):           # q = u scale + 0.5 inside (cell + 0.1, cell + 0.9)
                    uq = (cell + rng.uniform(-0.4, 0.4, 3)) / np.float64(lv["scale"])
                    pts.append((2.0 * np.clip(uq, 0, 1) - 1.0) * b)
        add(f"wrap{l}", pts)
    # q = u scale + 0.5 an exact integer (fraction 0) on one, two and three axes, for levels 0, 7 and 15.  u >= 0.5: x = (2 u - 1) bound
    # and u = (x + bound) / (2 bound) are then exact, and so u is the float32 the search fixed
    for l in (0, 7, 15):
        sc = geo.levels[l]["scale"]
        good = []
        for m in rng.permutation(np.arange(int(sc) // 2 + 2, int(sc)))[:400]:
            for cand in (f32((m - 0.5) / np.float64(sc)), np.nextafter(f32((m - 0.5) / np.float64(sc)), f32(1)), np.nextafter(f32((m - 0.5) / np.float64(sc)), f32(0))):
                if f32(f32(cand * sc) + f32(0.5)) == f32(m) and 0.5 <= cand < 1:
                    good.append(cand)
                    break
            if len(good) == 24:
                break
        assert len(good) >= 3, (l, len(good))      # (level 0 has six such integers in the upper half)
        good = np.asarray(good, f32)
        pts = []
        for i in range(12):
            for k in (1, 2, 3):
                uq = rng.uniform(0.5, 0.999, 3).astype(f32)
                axes = rng.permutation(3)[:k]
                uq[axes] = good[(i + np.arange(k)) % good.shape[0]]
                pts.append((f32(2) * uq - f32(1)) * f32(b))
        add(f"intq{l}", pts)
    add("uniform", rng.uniform(-b, b, (n_uniform, 3)))
    x = np.concatenate(parts)
    sets, at = {}, 0
    for name, p in zip(names, parts):
        sets[name] = np.arange(at, at + p.shape[0])
        at += p.shape[0]
    return np.ascontiguousarray(x), sets


def assert_coverage(geo, x, sets, f_ref=None):
    """From index arithmetic alone: the sets hit what they are named for.  f_ref (the oracle's features): the share under F_SMALL."""
    u = geo.u_of(x)
    inside = ((u >= 0) & (u <= 1)).all(1)
    assert ((u[sets["corners"]] == 0) | (u[sets["corners"]] == 1)).all() and sets["corners"].shape[0] == 8
    assert all(((u[sets["faces"]][:, a] == 0).any() and (u[sets["faces"]][:, a] == 1).any()) for a in range(3))
    o = sets["outside"]
    assert not inside[o].any() and inside.sum() == x.shape[0] - o.shape[0]
    assert all(x[sets["edge_in"]][a, a] > geo.bound and u[sets["edge_in"]][a, a] == 1 for a in range(3))
    uo = u[o[:6]]
    assert all(uo[2 * a, a] > 1 and uo[2 * a + 1, a] < 0 and np.delete(uo[2 * a], a).max() <= 1 for a in range(3))
    report = {}
    for l in geo.capped:
        lv = geo.levels[l]
        _, cell, base = geo.cell_rows(x[inside], l)
        assert (cell >= 0).all() and (cell + 1 <= lv["res"]).all()
        wraps = np.stack([(base + (c & 1) * lv["s1"] + (c >> 1) * lv["s2"]) % lv["hs"] == lv["hs"] - 1 for c in range(4)], 1)
        assert wraps.any(0).all(), (l, wraps.sum(0))           # every corner pair has its x corner on the level's last row
        report[l] = wraps.sum(0).tolist()
    for l in (0, 7, 15):
        q, _, _ = geo.cell_rows(x[sets[f"intq{l}"]], l)
        n_int = (q == np.floor(q)).sum(1)
        assert all((n_int >= k).any() for k in (1, 2, 3)) and (n_int >= 1).all(), (l, n_int)
    if f_ref is not None:
        share = float((np.abs(f_ref.astype(np.float64)) < F_SMALL).mean())
        assert share <= MAX_SMALL_SHARE, share
        report["small_share"] = share
    return report


def unit_dirs(seed=2, n_random=160):
    """Directions for the SH stage: random unit vectors, the six axes, vectors with one and two zero components, and unnormalised ones
    (the SH encoder is a polynomial and takes them as they are: shencoder.cu:49-121)."""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((n_random, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    one_zero = np.array([[0, .6, .8], [.6, 0, -.8], [-.8, .6, 0]])
    raw = rng.uniform(-1, 1, (24, 3)) * rng.uniform(0.5, 1.5, (24, 1))
    return np.concatenate([axes, one_zero, r, raw]).astype(f32)


# ---- probe weights ------------------------------------------------------------------------------------------------------------------------------
SHAPES = {"deform_net": [(128, 76)] + [(128, 128)] * 6 + [(3, 128)], "sigma_net": [(64, 32), (16, 64)], "color_net": [(64, 31), (64, 64), (3, 64)]}


def blank_state(geo, table, seed=3):
    """All-zero deformation and sigma nets, a seeded random colour net (the grid probes leave it arbitrary), the table as float32."""
    rng = np.random.default_rng(seed)
    st = {f"{net}.{i}.weight": np.zeros(s, f32) for net, shapes in SHAPES.items() for i, s in enumerate(shapes)}
    for i, s in enumerate(SHAPES["color_net"]):
        st[f"color_net.{i}.weight"] = (rng.standard_normal(s) / np.sqrt(s[1])).astype(f32)
    st["encoder.embeddings"] = table.astype(f32)
    st["encoder.offsets"] = geo.offsets.copy()
    return st


def _pm(W, unit, col, scale=1.0):
    """Units `unit`, `unit + 1` of a layer = +-scale * (input col)."""
    W[unit, col], W[unit + 1, col] = scale, -scale


def set_grid_probe(st, j):
    """density logit = grid feature j (the deformation net stays zero)."""
    w0, w1 = np.zeros((64, 32), f32), np.zeros((16, 64), f32)
    _pm(w0, 0, j)
    w1[0, 0], w1[0, 1] = 1, -1
    st["sigma_net.0.weight"], st["sigma_net.1.weight"] = w0, w1
    return st


def set_wiring_probe(st, inputs, gain=GAIN):
    """sigma-net output k = grid feature k (k = 0..15: the logit and geo_feat[k - 1]); colour logit c = gain * (input inputs[c] of the
    colour net, whose 31 inputs are [SH(16), geo_feat(15)] in that order: dnerf/network.py:162-165)."""
    w0, w1 = np.zeros((64, 32), f32), np.zeros((16, 64), f32)
    for k in range(16):
        _pm(w0, 2 * k, k)
        w1[k, 2 * k], w1[k, 2 * k + 1] = 1, -1
    c0, c1, c2 = np.zeros((64, 31), f32), np.zeros((64, 64), f32), np.zeros((3, 64), f32)
    for c, m in enumerate(inputs):
        _pm(c0, 2 * c, m)
        c1[2 * c, 2 * c] = c1[2 * c + 1, 2 * c + 1] = 1
        c2[c, 2 * c], c2[c, 2 * c + 1] = gain, -gain
    st["sigma_net.0.weight"], st["sigma_net.1.weight"] = w0, w1
    st["color_net.0.weight"], st["color_net.1.weight"], st["color_net.2.weight"] = c0, c1, c2
    return st


def set_deform_probe(st, cols, g=DEFORM_G):
    """dx[a] = g * (input cols[a] of the first deformation layer: the 63 columns of freq(x, 10), then the 13 of freq(t, 6)), carried
    through the eight layers in +- pairs."""
    ws = [np.zeros(s, f32) for s in SHAPES["deform_net"]]
    for a, col in enumerate(cols):
        _pm(ws[0], 2 * a, col)
        for l in range(1, 7):
            ws[l][2 * a, 2 * a] = ws[l][2 * a + 1, 2 * a + 1] = 1
        ws[7][a, 2 * a], ws[7][a, 2 * a + 1] = g, -g
    for i, w in enumerate(ws):
        st[f"deform_net.{i}.weight"] = w
    return st


WIRING_LAUNCHES = [tuple(min(3 * i + c, 30) for c in range(3)) for i in range(10)] + [(30, 29, 28)]
DEFORM_LAUNCHES = [tuple((3 * i + c) % 76 for c in range(3)) for i in range(26)]
assert {m for t in WIRING_LAUNCHES for m in t} == set(range(31)) and {m for t in DEFORM_LAUNCHES for m in t} == set(range(76))


def variant_features(geo):
    """The fixed subset of 8 features that goes through every kernel variant: both channels of level 0, the last dense level, the
    coarsest capped level and level 15."""
    return tuple(2 * l + c for l in (0, geo.capped[0] - 1, geo.capped[0], 15) for c in (0, 1))


# ---- expected values --------------------------------------------------------------------------------------------------------------------------------
def colour_inputs(d, feats, half, variant=None):
    """The colour net's 31 inputs [SH(d, 4) (16), geo_feat = features 1..15] as the network sees them.  variants: swap_sh (SH components
    4 and 5 swapped), concat_reversed ([geo, SH])."""
    sh, _ = O.sh_encode_forward(np.asarray(d, f32), 4)
    if variant == "swap_sh":
        sh = sh.copy()
        sh[:, [4, 5]] = sh[:, [5, 4]]
    geo = np.asarray(feats)[:, 1:16].astype(f32)
    cin = np.concatenate([geo, sh] if variant == "concat_reversed" else [sh, geo], axis=1)
    return cin.astype(np.float16).astype(np.float64) if half else cin.astype(np.float64)


def expected_rgb(cin, inputs, half, gain=GAIN):
    """-> (rgb [N,3] float64, logit [N,3]): rgb = sigmoid(gain * input); half: the logit is an fp16 value, rgb rounded to fp16."""
    logit = gain * cin[:, list(inputs)]
    if half:
        logit = logit.astype(np.float16).astype(np.float64)
    rgb = 1.0 / (1.0 + np.exp(-logit))
    return (rgb.astype(np.float16).astype(np.float64) if half else rgb), logit


def rgb_bar_f16(rgb_ref, logit_ref, inputs, gain=GAIN):
    """Bar on |rgb - rgb_ref| for the fp16 kernel.  The kernel stores fp16(s~(l')) with s~ its fp32 sigmoid (v_exp_f32, v_rcp_f32: 1 ulp
    each, < 2^-20 in all) and l' the kernel's logit; the reference is fp16(s(l)).  Two fp16 roundings cost half an ulp each: one ulp of
    the output (taken at the largest value the result may have), plus |s(l') - s(l)| <= |l' - l| / 4.  A geo_feat input is a grid
    feature, bit-exact (stage 1): l' = l.  An SH input is an fp32 polynomial evaluated in another order than the oracle's float64 one, a
    few fp32 ulps apart, so its fp16 rounding may flip where the value lies next to a tie: |l' - l| <= gain * ulp16(input) = ulp16(logit)."""
    dl = np.where(np.asarray(inputs)[None, :] < 16, ulp16(logit_ref), 0.0)
    return ulp16(rgb_ref + 0.25 * dl) + 0.25 * dl + 2.0 ** -20


def deform_inputs(x, t):
    """[N, 76] float32: freq(x, 10) ++ freq(t, 6), the first deformation layer's input (dnerf/network.py:123-138)."""
    ex = O.freq_encode_forward(np.asarray(x, f32), 10)
    et = O.freq_encode_forward(np.asarray([[t]], f32), 6)
    return np.concatenate([ex, np.repeat(et, ex.shape[0], 0)], axis=1)


def deformed_points_f16(x, enc_col, g=DEFORM_G, step=0, variant=None):
    """x + dx as the fp16 network forms it for ONE axis set: dx = fp16(g * fp16(enc)) per axis, added in fp32 to the unrounded x
    (dnerf/network.py:139-145 under autocast: the deformation is an fp16 tensor, x float32, the sum float32).  enc_col [N,3]: the probed
    input per axis.  step = -1 / +1 (or one such value per axis): the fp16 neighbour of fp16(enc) instead (the bar's candidates).  variant after_add: the SUM is
    rounded to fp16."""
    e16 = np.asarray(enc_col, f32).astype(np.float16).copy()
    for a, sa in enumerate(np.broadcast_to(step, (3,))):
        if sa:
            e16[:, a] = f16_step(e16[:, a], sa > 0)
    dx = (f32(g) * e16.astype(f32)).astype(np.float16).astype(f32)
    xd = (np.asarray(x, f32) + dx).astype(f32)
    return xd.astype(np.float16).astype(f32) if variant == "after_add" else xd


def feature0_candidates(geo, x, enc_col, table, g=DEFORM_G, variant=None):
    """The deformation stage's bar, fp16 kernel: feature 0 of the ramp table at x + dx for fp16(enc) and its two fp16 neighbours, per
    axis independently -- ONE fp16 ulp of enc carried through g and the ramp, and the ramp's own fp16 resolution, both by evaluating the
    oracle there instead of bounding them.  The kernel's sine and cosine are polynomials ~1.3e-7 (x 2^4 after the angle doublings) from
    the exact values, the oracle's are sinf of the float32 argument (cosine: of the argument + float(pi/2), itself off by up to 3e-5 at
    2^9): both far below one fp16 ulp EXCEPT where the value lies next to an fp16 tie -- so the kernel's fp16(enc) is the reference's or
    its neighbour.  (For the cosine columns at high octaves the reference's own phase error reaches a fraction of an fp16 ulp of values
    near 1: still one neighbour.)  The ramp reads ONE axis, but the fp16 blend's roundings depend on the fractions of all three (measured
    on the CPU: a one-ulp step of ANOTHER axis' encoding moves feature 0 by up to two fp16 ulps), so every axis steps on its own: 27
    candidates per point, the unstepped one first.  -> [27, N] fp16."""
    steps = sorted(itertools.product((0, -1, 1), repeat=3), key=lambda s: sum(map(abs, s)))
    return np.stack([level0_feature(geo, deformed_points_f16(x, enc_col, g, s, variant), table) for s in steps])


def level0_feature(geo, x, table):
    """Feature 0 of `oracle_features` from level 0 alone (the ramp tables are zero elsewhere): the oracle's encoder on a one-level grid."""
    enc, _ = O.grid_encode_forward(geo.u_of(x), table[:geo.offsets[1]], geo.offsets[:2], geo.pls, H_BASE, False, 1, False, 0)
    return enc[:, 0]


def enc_error(cols):
    """Per probed column, how far the kernel's float32 encoding may lie from the oracle's, absolutely.  Raw coordinates and the raw time
    (columns 0..2, 63) are copied: 0.  Octave f of freq(x, 10): the oracle's cosine is sinf(2^f x + float(pi/2)), whose float32 argument
    (below 2^(f+1)) is rounded by up to 2^f 2^-23 -- 3e-5 at f = 9, as field_f16_net.h notes -- (taken for the sine too); the kernel's
    polynomial pair is within 1.3e-7 of the exact values and four angle doublings multiply that by at most 2^4: 2.1e-6; sinf itself 1
    ulp: 6e-8.  Time octaves: both sides evaluate the SAME float32 expression with a 1-ulp sinf each: 2.4e-7."""
    out = []
    for c in cols:
        if c < 3 or c == 63:
            out.append(0.0)
        elif c < 63:
            out.append(2.0 ** ((c - 3) // 6) * 2.0 ** -23 + 2.1e-6 + 6e-8)
        else:
            out.append(2.4e-7)
    return np.asarray(out)


# One fp16 trilinear evaluation is within 8 x 2^-11 of the exact blend of values of magnitude <= 1 (eight products and eight sums, each
# rounded by at most 2^-11 of a value <= 1; the weights sum to 1): two evaluations (kernel, oracle) at nearby points differ by twice that
# plus the exact ramp's slope (15 / 16 per unit of u) times the distance of the points.
RAMP_ROUNDING = 2 * 8 * 2.0 ** -11


def deform_bar_f16(geo, x, enc_col, cols, table, sigma, g=DEFORM_G):
    """The deformation stage's bar on the fp16 kernel's sigma (density logit = feature 0 of a ramp table).  -> (ok [N], stats).
    STRICT points (every probed input at least 2 enc_error away from being resolvable in fp16: ulp16(enc) >= 2 enc_error, so the
    kernel's fp16(enc) is the oracle's or its neighbour): float16(log sigma) must be one of `feature0_candidates` under the grid bar.
    The other points (an encoding near a zero crossing, where one fp16 ulp is smaller than the float32 encodings' own distance): the
    logit within RAMP_ROUNDING + (15 / 16) (g (enc_error + ulp16(enc)) + 2^-23) / (2 bound) of the oracle's, unless the reference point
    lies within 1e-4 of the range test (counted as `skipped`)."""
    E = enc_error(cols)[None, :]
    strict = (ulp16(np.asarray(enc_col, f32).astype(np.float16)) >= 2 * E).all(1)
    cands = feature0_candidates(geo, x, enc_col, table, g)
    first = grid_bar_f16(sigma, cands[0])
    ok_strict = np.logical_or.reduce([first[0]] + [grid_bar_f16(sigma, c)[0] for c in cands[1:]])
    u = geo.u_of(deformed_points_f16(x, enc_col, g))
    edge = ((np.abs(u) < 1e-4) | (np.abs(u - 1) < 1e-4)).any(1)
    du = (g * (E + ulp16(enc_col)) + 2.0 ** -23).max(1) / (2 * geo.bound)
    ok_loose = np.abs(decode(sigma) - cands[0].astype(np.float64)) <= RAMP_ROUNDING + 15.0 / 16.0 * du
    ok = np.where(strict, ok_strict, ok_loose | edge)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        print("deform bar, first failure: point", i, "x", x[i], "enc", np.asarray(enc_col)[i], "enc_error", E[0], "strict", bool(strict[i]),
              "log sigma", decode(sigma)[i], "candidates", cands[:, i].astype(np.float64), "u", u[i])
    return ok, {"worst_decode_err": first[1]["worst_decode_err"], "exact_pairs": int((strict & (np.abs(cands[0].astype(np.float64)) >= F_SMALL)).sum()),
                "strict_share": float(strict.mean()), "neighbour_candidate": int((strict & ~first[0] & ok_strict).sum()),
                "skipped": int((~strict & edge).sum()), "failed": int((~ok).sum())}


# ---- the bars as functions (the GPU test and the CPU test's wrong variants go through the same code) ---------------------------------------------
def decode(sigma, density_scale=1.0):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(sigma, np.float64) / float(density_scale))


def grid_bar_f16(sigma, f_ref, density_scale=1.0):
    """-> (ok [N] bool, stats).  f_ref: fp16 features from the oracle.  See DECODE_BAR."""
    f = decode(sigma, density_scale)
    ref = f_ref.astype(np.float64)
    big = np.abs(ref) >= F_SMALL
    with np.errstate(over="ignore", invalid="ignore"):
        exact = f.astype(np.float16).view(np.uint16) == np.asarray(f_ref, np.float16).view(np.uint16)
    err = np.abs(f - ref)
    ok = np.where(big, exact, err <= DECODE_BAR)
    fin = np.isfinite(err)
    return ok, {"worst_decode_err": float(err[ok & fin].max()) if (ok & fin).any() else float("nan"), "exact_pairs": int(big.sum()),
                "small_share": float(1 - big.mean()), "failed": int((~ok).sum()), "worst_err": float(np.nanmax(np.where(fin, err, np.inf)))}


def grid_bar_f32(sigma, f_ref, bar, density_scale=1.0):
    err = np.abs(decode(sigma, density_scale) - f_ref.astype(np.float64))
    ok = err <= bar
    return ok, {"worst_decode_err": float(np.nanmax(err)), "pairs": int(err.size), "failed": int((~ok).sum())}


def line(stage, variant, stats):
    return f"[field-probe] {stage:10s} {variant:22s} " + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in stats.items())
