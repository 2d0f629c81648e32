"""The fused field kernels at the edges of their OPERAND ranges (tests/test_gpu_field_ranges.py; validated without a GPU by
tests/test_field_ranges_cpu.py): probe states built with the machinery of tests/field_probe_support.py (bias-free ReLU layers that carry
one value as a +- pair), an exact rescaling that walks one operand across its range while the network's value stays put, a float64
restatement that also records the magnitude of the operand entering every layer, the subnormal table of a freshly initialised grid and
the logits of the output stage.  numpy only.

The rescaling.  A probe carries a value v into layer L.  A gain 2^k sits on what feeds L (the layer before it, and where one fp16-held
weight cannot take it -- the split kernel packs 2^8 w into fp16, so |w| <= 255 -- the layers before that: at most 2^7 each) and 2^-k on
L (and, for the same reason, on the layers behind it).  Every factor is a power of two: exact in fp16, fp32 and float64, so the float64
value of the network is the same for every k (tests/test_field_ranges_cpu.py: `np.array_equal`), and only the operand entering L --
v 2^k -- and L's weights move.

A "state" is a plain dict of numpy arrays with the model's state_dict keys, as in field_probe_support."""
import numpy as np

import field_probe_support as P
from oracle import oracle as O

f32, f64 = np.float32, np.float64
N = 513                      # two whole 256-point tiles + one lane (kinds 0, 3, 4) = four 128-point workgroups + one lane (kinds 1, 2, 5)
T = 0.5
LAYERS = tuple(f"D{i}" for i in range(8)) + ("S0", "S1", "C0", "C1", "C2")
KEY = {**{f"D{i}": f"deform_net.{i}.weight" for i in range(8)}, "S0": "sigma_net.0.weight", "S1": "sigma_net.1.weight",
       "C0": "color_net.0.weight", "C1": "color_net.1.weight", "C2": "color_net.2.weight"}

# ---- the split kernel's documented envelope (csrc/field_f32x3.hip, "Scaling") -------------------------------------------------------------
X_LO, X_HI = 2.0 ** -8, 1023.0          # activations: lo parts normal from 2^-8 (3.9e-3), hi parts finite up to 1023
W_LO, W_HI = 2.0 ** -10, 255.0          # weights
X_OVERFLOW = 1023.75                    # 2^6 x >= 65520 rounds to the fp16 infinity
CAP = 7                                 # log2 of the largest power of two one split-packed weight may carry next to a mantissa (2^7 < 255)
# the bar tests/test_gpu_field_f32.py applies to the split variant against float64: |got - ref| / (|ref| + 1e-2) < 2.5e-4, and the
# fp32-MFMA kernel's own: rtol 1e-4, atol 1e-6
SPLIT_REL, SPLIT_FLOOR = 2.5e-4, 1e-2
MFMA32_RTOL, MFMA32_ATOL = 1e-4, 1e-6
SUB_TERM = 2.0 ** -11                   # relative error of a term whose lo part is lost: hi alone carries 11 bits

A_STAGES = ("D1", "D4", "S1", "C1")
A_INSIDE = (2.0 ** -8, 2.0 ** -7, 2.0 ** -2, 1.0, 2.0 ** 9, 1023.0)     # (2^-7: the lowest point of the launch at 1.5 x 2^-8, all of them inside)
A_BELOW = (2.0 ** -12, 2.0 ** -16)
A_ABOVE = 1100.0
A_MFMA32 = (2.0 ** -16, 2.0 ** -12, 2.0 ** -8, 2.0 ** -2, 1.0, 2.0 ** 9, 1023.0, 1100.0, 2.0 ** 12)
A_WEIGHTS = (2.0 ** -10, 1.0, 255.0)
# S and C stages: density logit = READ_S v, colour logit = -READ_C v.  A relative error e of v moves sigma by 4 e relative, and rgb =
# sigmoid(-4 v) (0.02 .. 0.05) by about 4 e relative too: a term that lost its lo part (e = 2^-11) shows at 2e-3, eight times the bar.
READ_S, READ_C = 4.0, P.GAIN
READ_D = 16.0                           # D stages: both logits = READ_D x (feature 0 of the ramp table at x + dx), dx[1] = DEFORM_G v


def split_bar(ref):
    return SPLIT_REL * (np.abs(ref) + SPLIT_FLOOR)


def mfma32_bar(ref):
    return MFMA32_RTOL * np.abs(ref) + MFMA32_ATOL


def k_and_mantissa(a):
    """a = vm 2^k with vm in (0.5, 1]."""
    k = int(np.ceil(np.log2(abs(a))))
    return k, a / 2.0 ** k


# ---- tables and points -------------------------------------------------------------------------------------------------------------------
def a_table(geo):
    """fp32 table of section A: level 0 channel 0 = the ramp of axis 1 (field_probe_support.ramp_table: the D stages read x + dx through
    it), level 1 (dense) channel 0 = 16 on the vertices of the upper half in x, 12 on the others: a point whose level-1 cell does not
    straddle the step reads 16 or 12 (to fp32 rounding of the blend); everything else zero."""
    t = P.ramp_table(geo, 1).astype(f32)
    lv = geo.levels[1]
    assert not lv["capped"]
    n1 = lv["res"] + 1
    r = np.arange(n1 ** 3)
    t[lv["off"] + r, 0] = np.where(r % n1 >= n1 // 2, 16.0, 12.0).astype(f32)
    return t


def a_points(geo, seed=21):
    """513 points.  x0 takes the few-bit values {1, -1, -0.5, 0.25, -0.25} in turn (the D stages' value is vm (7 + x0) / 8: x0 = 1 carries
    the target magnitude, the others at most 0.91 of it; the S and C stages' is vm (x0 > 0: 16, else 12) / 16), every value at least
    0.2 from the level-1 step at x0 = 0; x1, x2 uniform in [-0.8, 0.6] (x1 + dx stays inside the box).  -> x [513,3] f32, d [513,3]."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.8, 0.6, (N, 3)).astype(f32)
    x[:, 0] = np.resize(np.array([1.0, -1.0, -0.5, 0.25, -0.25], f32), N)
    lv = geo.levels[1]
    q, cell, _ = geo.cell_rows(x, 1)
    half = (lv["res"] + 1) // 2
    assert ((cell[:, 0] + 1 < half) | (cell[:, 0] >= half)).all()             # no level-1 cell straddles the step
    return x, np.resize(P.unit_dirs(), (N, 3)).astype(f32)


# ---- probe states ------------------------------------------------------------------------------------------------------------------------------
def _zero_state():
    return {f"{net}.{i}.weight": np.zeros(s, f32) for net, shapes in P.SHAPES.items() for i, s in enumerate(shapes)}


def _spread(e, n, cap):
    """The exponent e over n layers, first layer first, at most `cap` each (cap None: all on the first)."""
    out = []
    for _ in range(n):
        step = e if cap is None else min(e, cap)
        out.append(step)
        e -= step
    assert e == 0, "the gain does not fit the layers"
    return out


def _carry(st, layer, w=1.0):
    W = st[KEY[layer]]
    W[0, 0] = W[1, 1] = w


def _pair(st, layer, col, w):
    W = st[KEY[layer]]
    W[0, col], W[1, col] = w, -w


def _read(st, layer, row, w):
    W = st[KEY[layer]]
    W[row, 0], W[row, 1] = w, -w


def _ramp_readout(st):
    """Both logits = READ_D x feature 0."""
    _pair(st, "S0", 0, 4.0)
    _read(st, "S1", 0, READ_D / 4.0)
    _read(st, "S1", 1, 1.0)
    _pair(st, "C0", 16, 1.0)
    _carry(st, "C1")
    _read(st, "C2", 0, READ_D / 4.0)


def reads_sigma(stage, a):
    """False for the sub-unit cases of S1 (a < 2^-5: 2^-k READ_S does not fit one weight of S1, and nothing lies between S1 and the
    exponential): those read the value through rgb only, the density logit is 0."""
    return stage != "S1" or 2.0 ** -k_and_mantissa(a)[0] * READ_S <= 2.0 ** CAP


def a_twin(stage, a, cap=CAP):
    """The same probe at k = 0: the mantissa alone, read out the same way."""
    return a_state(stage, k_and_mantissa(a)[1], cap, sigma=reads_sigma(stage, a))


def a_state(stage, a, cap=CAP, sigma=None):
    """The probe state whose operand entering `stage` has the magnitude a on the points with x0 = 1 (D stages) or x0 > 0 (S1, C1), and
    0.75 .. 0.94 a on the others.  -> (state, L) where L names the layer the operand enters.  sigma: see `reads_sigma`."""
    k, vm = k_and_mantissa(a)
    st = _zero_state()
    up = 2.0 ** k
    if stage in ("D1", "D4"):
        L = int(stage[1])
        first = vm if L > 1 else vm * up                       # D0: v = vm (7 + x0) / 8 from the raw x0 and the raw time (column 63, t = 0.5)
        _pair(st, "D0", 0, first / 8.0)
        _pair(st, "D0", 63, first * 7.0 / 4.0)
        if L > 1:                                              # the gain on D(L-1), D(L-2), ...
            back = _spread(k, L - 1, cap) if k > 0 else [k] + [0] * (L - 2)
            for i, e in enumerate(back):
                _carry(st, f"D{L - 1 - i}", 2.0 ** e)
        fwd = _spread(-k, 7 - L, cap) if k < 0 else [-k] + [0] * (6 - L)
        for i, e in enumerate(fwd):
            _carry(st, f"D{L + i}", 2.0 ** e)
        st[KEY["D7"]][1, 0], st[KEY["D7"]][1, 1] = P.DEFORM_G, -P.DEFORM_G
        _ramp_readout(st)
        return st, stage
    if stage == "S1":
        _pair(st, "S0", 2, vm * 2.0 ** (k - 4))                # feature 2 = 16 or 12
        if reads_sigma(stage, a) if sigma is None else sigma:
            _read(st, "S1", 0, 2.0 ** -k * READ_S)
            _read(st, "S1", 1, 2.0 ** -k)
            fwd = [0, 0]
        else:
            e = _spread(-k, 3, cap)
            _read(st, "S1", 1, 2.0 ** e[0])
            fwd = e[1:]
        _pair(st, "C0", 16, 2.0 ** fwd[0])
        _carry(st, "C1", 2.0 ** fwd[1])
        _read(st, "C2", 0, -READ_C)
        return st, stage
    assert stage == "C1"
    back = _spread(k, 3, cap) if k > 0 else [k, 0, 0]
    _pair(st, "S0", 2, 2.0 ** (back[2] - 4))
    _read(st, "S1", 0, READ_S)                                 # a density that no colour-side overflow may touch
    _read(st, "S1", 1, 2.0 ** back[1])
    _pair(st, "C0", 16, vm * 2.0 ** back[0])
    e1, e2 = _spread(-2 - k, 2, cap) if -2 - k > 0 else (-2 - k, 0)      # 16 pairs: 16 2^e1 2^e2 = READ_C 2^-k
    W1, W2 = st[KEY["C1"]], st[KEY["C2"]]
    for i in range(16):
        W1[2 * i, 0] = W1[2 * i + 1, 1] = 2.0 ** e1
        W2[0, 2 * i], W2[0, 2 * i + 1] = -(2.0 ** e2), 2.0 ** e2
    return st, stage


def weight_state(w):
    """Section A.4: the last sigma layer's weights have the magnitude w -- row 0 (the density logit) exactly w, a power of two or 255;
    row 1 (geo_feat 0 -> colour logit READ_C x) w (1 +- 5 2^-14), whose lo part is not empty -- and S0 scales feature 2 (16 or 12) so
    that the operand stays inside the activation envelope and the logits are of order 1."""
    st = _zero_state()
    k, _ = k_and_mantissa(w)
    _pair(st, "S0", 2, 2.0 ** min(-k - 3, 5))
    _read(st, "S1", 0, w)
    _read(st, "S1", 1, float(f32(w * (1 - 5 * 2.0 ** -14 if w >= W_HI else 1 + 5 * 2.0 ** -14))))
    _pair(st, "C0", 16, 1.0)
    _carry(st, "C1")
    _read(st, "C2", 0, -READ_C / 2)
    return st


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------------------
def forward64(st, geo, table, x, d, t=T, density_scale=1.0, perturb=None, half_table=False):
    """dnerf/network.py:123-169 in float64 on the oracle's encoders (float32 outputs, taken as they are).  -> dict: sigma (float64 exp,
    times the scale, cast to float32), rgb (float64), logit, rgb_logit, dx, and `operand`: {layer: per point, the largest |input| among
    the columns that layer's weights read}.  perturb = (layer, eps): that layer's output times (1 + eps), for the derived bounds."""
    x = np.asarray(x, f32)
    operand = {}

    def mlp(h, names):
        for i, name in enumerate(names):
            W = np.asarray(st[KEY[name]], f64)
            used = np.abs(W).max(0) > 0
            operand[name] = np.abs(h[:, used]).max(1) if used.any() else np.zeros(h.shape[0])
            h = h @ W.T
            if perturb is not None and perturb[0] == name:
                h = h * (1.0 + perturb[1])
            if i != len(names) - 1:
                h = np.maximum(h, 0)
        return h

    dx = mlp(P.deform_inputs(x, t).astype(f64), LAYERS[:8])
    if t == 0.0:
        dx = np.zeros_like(dx)
    xd = (x + dx.astype(f32)).astype(f32)
    feats = P.oracle_features(geo, xd, table.astype(np.float16) if half_table else table).astype(f64)
    h = mlp(feats, ("S0", "S1"))
    sh, _ = O.sh_encode_forward(np.asarray(d, f32), 4)
    c = mlp(np.concatenate([sh.astype(f64), h[:, 1:]], axis=1), ("C0", "C1", "C2"))
    with np.errstate(over="ignore", under="ignore"):
        sigma = (float(density_scale) * np.exp(h[:, 0])).astype(f32)
        rgb = 1.0 / (1.0 + np.exp(-c))
    return {"sigma": sigma, "rgb": rgb, "logit": h[:, 0], "rgb_logit": c, "dx": dx, "operand": operand, "features": feats}


def sub_envelope_terms(ref):
    """Per point, the number of layers whose (non-zero) operand lies below the split kernel's 2^-8."""
    return sum(((v > 0) & (v < X_LO * (1 - 1e-6))).astype(int) for v in ref["operand"].values())


def sub_envelope_bound(st, geo, table, x, d, L, ref):
    """Section A.2: below the envelope the lo part of the operand is lost and hi alone carries 11 bits -- the term entering L, and the
    term of every later layer that still lies below 2^-8 because one weight cannot take the whole gain back (`sub_envelope_terms` of
    them, per point), are each off by up to 2^-11 relative.  The outputs' distance under that error, from the restatement itself with
    L's output times (1 +- n 2^-11); the file's bar comes on top.  Zero for a point whose terms all lie inside.
    -> (d_sigma [N], d_rgb [N,3], n [N])."""
    n = sub_envelope_terms(ref)
    eps = (n * SUB_TERM)[:, None]
    hi, lo = (forward64(st, geo, table, x, d, perturb=(L, s * eps)) for s in (1, -1))
    ds = np.maximum(np.abs(hi["sigma"].astype(f64) - ref["sigma"]), np.abs(lo["sigma"].astype(f64) - ref["sigma"]))
    dc = np.maximum(np.abs(hi["rgb"] - ref["rgb"]), np.abs(lo["rgb"] - ref["rgb"]))
    return ds, dc, n


def overflowing(ref, L):
    """Section A.3, from the probe's construction: (points whose operand entering L converts to the fp16 infinity as 2^6 x, points that
    stay inside the envelope).  Every point is one or the other."""
    v = ref["operand"][L]
    over, inside = v >= 1024.0, v <= X_HI
    assert (over | inside).all() and over.any() and inside.any()
    return over, inside


# ---- section B: a freshly initialised table ----------------------------------------------------------------------------------------------------
SUBNORMAL_VALUES = (np.float16(1e-4), np.float16(2.0 ** -14), np.float16(2.0 ** -15), np.float16(2.0 ** -20), np.float16(2.0 ** -24))
B_GAIN = 2.0 ** 12
B_SLABS = (1, 4, 7, 10, 13)            # level-0 vertex planes (i, i + 1) in x that hold SUBNORMAL_VALUES[s]: channel 0 +, channel 1 -
B_FEATURES = (0, 1, 31)                # + value, - value, and a feature of the +-1e-4 fill (level 15)


def b_table(geo, seed=31, dim=3):
    """fp16 table as `GridEncoder` initialises it -- uniform in +-1e-4 (gridencoder/grid.py) -- with the level-0 vertices of five slabs in
    x set to the listed values: channel 0 the value, channel 1 its negative."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1e-4, 1e-4, (geo.rows, 2)).astype(np.float16)
    lv = geo.levels[0]
    assert lv["res"] == 16 and lv["hs"] >= 17 ** dim          # dense: row = ix + 17 iy + 289 iz (+ 4913 iw for the 4-D grid)
    r = np.arange(17 ** dim)
    for v, i in zip(SUBNORMAL_VALUES, B_SLABS):
        rows = lv["off"] + r[(r % 17 == i) | (r % 17 == i + 1)]
        t[rows, 0], t[rows, 1] = v, -v
    return t


def b_points(geo, seed=32):
    """513 points, point p inside level-0 cell column B_SLABS[p % 5] in x (all eight corners hold that slab's value): q = 15 u + 0.5 in
    (i + 0.1, i + 0.9).  -> (x, d, slab index per point)."""
    rng = np.random.default_rng(seed)
    slab = np.arange(N) % 5
    q = np.asarray(B_SLABS)[slab] + rng.uniform(0.1, 0.9, N)
    x = rng.uniform(-0.9, 0.9, (N, 3))
    x[:, 0] = 2.0 * (q - 0.5) / 15.0 - 1.0
    x = x.astype(f32)
    _, cell, _ = geo.cell_rows(x, 0)
    assert np.array_equal(cell[:, 0], np.asarray(B_SLABS)[slab])
    return x, np.resize(P.unit_dirs(), (N, 3)).astype(f32), slab


# The three models' sigma and colour nets: (shapes, row of the last sigma layer that is geo_feat 0, rows of the last colour layer per
# channel).  "dnerf": kinds 0-2; "basis": kinds 3 and 5 (64 coefficients = 32 density ++ 32 geo_feat, colour (3, 8) coefficients; with
# the constants row e_0 + e_32 the density logit is coefficient 0 and colour logit c is colour coefficient (c, 0)); "hyper": kind 4.
MODELS = {
    "dnerf": dict(sigma=[(64, 32), (16, 64)], color=[(64, 31), (64, 64), (3, 64)], geo_row=1, colour_rows=(0, 1, 2)),
    "basis": dict(sigma=[(64, 32), (64, 64)], color=[(64, 48), (64, 64), (24, 64)], geo_row=32, colour_rows=(0, 8, 16)),
    "hyper": dict(sigma=[(64, 32), (33, 64)], color=[(64, 48), (64, 64), (3, 64)], geo_row=1, colour_rows=(0, 1, 2)),
}


def head_state(model):
    """Zero sigma and colour nets of `model` (a key of MODELS); for "dnerf" a zero deformation net as well."""
    m = MODELS[model]
    st = {f"sigma_net.{i}.weight": np.zeros(s, f32) for i, s in enumerate(m["sigma"])}
    st.update({f"color_net.{i}.weight": np.zeros(s, f32) for i, s in enumerate(m["color"])})
    if model == "dnerf":
        st.update({f"deform_net.{i}.weight": np.zeros(s, f32) for i, s in enumerate(P.SHAPES["deform_net"])})
    return st


def basis_row():
    """The basis model's constants row for these probes: sigma_basis = e_0, color_basis = e_0."""
    r = np.zeros(128, f32)
    r[0] = r[32] = 1.0
    return r


def basis_net_probe(shapes, t=T):
    """basis_net weights under which the model itself produces `basis_row()` at time t: unit 0 of the first layer = (1 / t) x the raw time
    (column 0 of freq(t, 6)), carried to outputs 0 and 32; every product exact in fp16.  shapes: the layers' (out, in)."""
    ws = [np.zeros(s, f32) for s in shapes]
    assert (1.0 / t) * t == 1.0
    ws[0][0, 0] = 1.0 / t
    for w in ws[1:-1]:
        w[0, 0] = 1.0
    ws[-1][0, 0] = ws[-1][32, 0] = 1.0
    return ws


def b_state(j, model="dnerf"):
    """density logit = 2^12 x grid feature j: the gain on S0, identity behind it; the deformation and colour nets zero."""
    st = head_state(model)
    _pair(st, "S0", j, B_GAIN)
    _read(st, "S1", 0, 1.0)
    return st


def flush16(v):
    """fp16 subnormals -> 0 (what an operand port that flushes them sees)."""
    v = np.asarray(v, np.float16).copy()
    v[np.abs(v.astype(f32)) < 2.0 ** -14] = 0
    return v


def b_expected(feature, flush_subnormal_operands=False):
    """The fp16 restatement of the probe (oracle/field.py `_linear` in mode fp16): h = fp16(2^12 f) carried through the +- pair, logit
    = h, sigma = exp(fp32 h).  flush_subnormal_operands: the matrix unit reads a subnormal f as zero.  -> (sigma f32, logit fp16)."""
    f = flush16(feature) if flush_subnormal_operands else np.asarray(feature, np.float16)
    logit = (f.astype(f64) * B_GAIN).astype(f32).astype(np.float16)
    return np.exp(logit.astype(f64)).astype(f32), logit


# ---- section C: the output stage -------------------------------------------------------------------------------------------------------------------
C_DENSITY = (87.0, 88.5, 88.8, 100.0, -87.0, -104.0)
C_INFINITE = (False, False, True, True, False, False)          # at either density_scale
C_COLOUR = (20.0, -20.0, 90.0, -90.0, 0.0)
C_SCALES = (1.0, 2.0 ** -8)


def c_expected(dl, cl, density_scale, half):
    """sigma: float64 exp cast to float32 -- +inf above log(float32 max) = 88.7228 at EITHER density_scale, as the table of cases has
    it -- times the scale in float32, the network's own order (sigma = trunc_exp(h) in float32, then density_scale * sigma).  The other
    reading, float64 exp times the scale and one cast at the end, would keep exp(88.8) 2^-8 = 1.6e36 finite and contradict that table;
    `c_expected_one_cast` computes it for the record.  rgb: float64 sigmoid (rounded to fp16 for the fp16 kinds)."""
    with np.errstate(over="ignore", under="ignore"):
        sigma = (f32(density_scale) * np.exp(np.asarray(dl, f64)).astype(f32)).astype(f32)
        rgb = 1.0 / (1.0 + np.exp(-np.asarray(cl, f64)))
    return sigma, (rgb.astype(np.float16).astype(f64) if half else rgb)


def c_expected_one_cast(dl, density_scale):
    with np.errstate(over="ignore", under="ignore"):
        return (float(density_scale) * np.exp(np.asarray(dl, f64))).astype(f32)


def c_logits(features, channel):
    """The logits the probe (`c_state`) puts on the points, from the oracle's grid features of the table (fp16 table: the at::Half blend
    the fp16 kernels reproduce bit for bit, and the fp16 product by 128, exact): (density [N], colour [N,3]) float64."""
    f = np.asarray(features)
    dl, c1 = 128.0 * f[:, 0].astype(f64), 128.0 * f[:, 1].astype(f64)
    cl = np.zeros((f.shape[0], 3))
    cl[:, channel] = c1
    return dl, cl


def c_table(geo, half, dim=3):
    """The logits travel in the table, so that one launch holds all of them: level 0 (17^3 dense), the density logit varies with x (six slabs of two vertex planes, i = 0/1, 3/4, 6/7, 9/10, 12/13, 15/16 -> channel 0 = logit / 128),
    the colour logit with y (five slabs i = 1/2, 4/5, 7/8, 10/11, 13/14 -> channel 1 = logit / 128).  1/128 is exact; a value the fp16
    table cannot hold (88.8 / 128) is rounded here -- the nearest fp16 logit, 88.8125 -- and the expectation is computed from the
    table as it is (`c_logits`).  The fp16 blend of eight equal corners rounds at every corner: a point's logit lies an fp16 ulp or two
    (0.0625 at 88) from its slab's value, which `c_logits` reproduces and tests/test_field_ranges_cpu.py holds on the right side of
    the overflow."""
    t = np.zeros((geo.rows, 2), np.float16 if half else f32)
    lv = geo.levels[0]
    assert lv["res"] == 16 and lv["hs"] >= 17 ** dim
    r = np.arange(17 ** dim)
    ix, iy = r % 17, (r // 17) % 17
    for s, v in enumerate(C_DENSITY):
        t[lv["off"] + r[(ix == 3 * s) | (ix == 3 * s + 1)], 0] = v / 128.0
    for s, v in enumerate(C_COLOUR):
        t[lv["off"] + r[(iy == 3 * s + 1) | (iy == 3 * s + 2)], 1] = v / 128.0
    return t


def c_points(geo, seed=41):
    """Point p in x slab p % 6 and y slab (p // 6) % 5 of `c_table`; z uniform.  Cell column i in x <=> q = 15 u + 0.5 in (i, i + 1);
    column 0 needs q in [0.5, 1) and column 15 q in [15, 15.5] (u in [0, 1]): the first slab's points sit at q in (0.55, 0.95), the last
    one's at (15.05, 15.45), the others at (i + 0.1, i + 0.9)."""
    rng = np.random.default_rng(seed)
    p = np.arange(N)
    sx, sy = p % 6, (p // 6) % 5
    qx = 3 * sx + np.where(sx == 0, rng.uniform(0.55, 0.95, N), np.where(sx == 5, rng.uniform(0.05, 0.45, N), rng.uniform(0.1, 0.9, N)))
    qy = 3 * sy + 1 + rng.uniform(0.1, 0.9, N)
    x = rng.uniform(-0.9, 0.9, (N, 3))
    x[:, 0], x[:, 1] = 2.0 * (qx - 0.5) / 15.0 - 1.0, 2.0 * (qy - 0.5) / 15.0 - 1.0
    x = x.astype(f32)
    _, cell, _ = geo.cell_rows(x, 0)
    assert np.array_equal(cell[:, 0], 3 * sx) and np.array_equal(cell[:, 1], 3 * sy + 1)
    return x, np.resize(P.unit_dirs(), (N, 3)).astype(f32), sx, sy


def c_state(channel=0, model="dnerf"):
    """density logit = 128 x feature 0, colour logit `channel` = 128 x feature 1 (as geo_feat 0, through the colour net's +- pair)."""
    m = MODELS[model]
    st = head_state(model)
    _pair(st, "S0", 0, 1.0)
    st[KEY["S0"]][2, 1], st[KEY["S0"]][3, 1] = 1.0, -1.0
    _read(st, "S1", 0, 128.0)
    st[KEY["S1"]][m["geo_row"], 2], st[KEY["S1"]][m["geo_row"], 3] = 1.0, -1.0
    _pair(st, "C0", 16, 1.0)
    _carry(st, "C1")
    _read(st, "C2", m["colour_rows"][channel], 128.0)
    return st
