"""Shared by the ambient-dimension tests and the fixture generator (tests/golden/gen_hyper_fixture.py): the recipe behind
tests/golden/caller_hyper.npz, the 4-D grid's geometry and level classes from the oracle's offsets, a numpy restatement of kernel_grid
for D = 4 and of the model (dnerf/network_hyper.py:121-194 of the reference) in two precisions, the weight packing restated, named
wrong variants and the bars the GPU tests hold the fused kernel to (those of tests/basis_support.py, whose helpers are imported).

fp16 restatement -- the reference under `-O` (torch autocast), the roundings csrc/field_hyper.hip implements: every Linear with fp16
operands, wide accumulation and an fp16 result; the grid table and the encoder's output fp16 with kernel_grid's two roundings per
corner; SH, the frequency encoding and trunc_exp in fp32; the ambient coordinate an fp16 value (tanh of an fp16 tensor, times bound)
that `torch.cat` promotes to float32 before the encoder normalises it.
"""
import ctypes
import hashlib
import os

import numpy as np

import basis_support as BS
from basis_support import TIMES, dist3, field_bars, occupancy_bits, seeded_points, slice_of, state_of, ulp16  # noqa: F401
from oracle import oracle as O
from oracle.field import _mlp

f32 = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caller_hyper.npz")
MODEL_KW = dict(BS.MODEL_KW)
NETS = {"ambient_net": 5, "sigma_net": 2, "color_net": 3}
VARIANTS = ("w_indexed_where_dropped", "upper_corners_first", "ambient_unnormalised", "s1_off_by_one")
LEVELS, H_BASE, LOG2_T = 16, 16, 19


def load():
    return np.load(FIXTURE)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
class Geometry4:
    """The model's 4-D grid: 16 levels x 2, base 16, finest 2048 bound, 2^19 rows at most, tiled.  Per level the strides of
    get_grid_index (gridencoder.cu:66-84: a coordinate is indexed while the running stride does not exceed the level's size), from the
    oracle's offsets and its float32 level parameters; `classes` names what each level does with the upper two coordinates."""

    def __init__(self, bound=1):
        self.bound = float(bound)
        self.offsets, self.pls = O.grid_offsets(4, LEVELS, 2, 2, H_BASE, LOG2_T, 2048 * bound, False)
        self.S = f32(np.log2(self.pls))
        self.rows = int(self.offsets[-1])
        self.levels = []
        for l in range(LEVELS):
            sc, res = ctypes.c_float(), ctypes.c_uint32()
            O.lib().orc_grid_level_params(O.u32(l), O.f32(float(self.S)), O.u32(H_BASE), ctypes.byref(sc), ctypes.byref(res))
            hs, res = int(self.offsets[l + 1] - self.offsets[l]), int(res.value)
            strides, stride = [], 1
            for _ in range(4):
                strides.append(stride if stride <= hs else 0)
                if stride <= hs:
                    stride *= res + 1
            if strides[3] and (res + 1) ** 4 <= hs:
                kind = "dense"
            elif strides[3]:
                kind = "w_wraps"
            elif strides[2]:
                kind = "w_dropped"
            else:
                kind = "zw_dropped"
            self.levels.append(dict(l=l, off=int(self.offsets[l]), hs=hs, scale=f32(sc.value), res=res, s=strides, kind=kind))
        self.classes = {k: [lv["l"] for lv in self.levels if lv["kind"] == k] for k in ("dense", "w_wraps", "w_dropped", "zw_dropped")}

    def u_of(self, x):
        """GridEncoder.forward (grid.py:149) in float32."""
        return ((np.asarray(x, f32) + f32(self.bound)) / f32(2 * self.bound)).astype(f32)

    def u4(self, x, ambient, normalise=True):
        a = np.full((np.asarray(x).shape[0], 1), f32(ambient), f32)
        return np.concatenate([self.u_of(x), self.u_of(a) if normalise else a], axis=1)

    def cell_w(self, ambient, l):
        """The fourth coordinate's cell at level l."""
        q = f32(f32(self.u_of(f32(ambient)) * self.levels[l]["scale"]) + f32(0.5))
        return int(np.floor(q))


def random_table(geo, seed=0):
    """Seeded fp16 table, magnitudes in [0.25, 1], random sign (tests/field_probe_support.random_table for this geometry)."""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.25, 1.0, (geo.rows, 2)).astype(f32)
    return (mag * rng.choice(np.array([-1.0, 1.0], f32), (geo.rows, 2))).astype(np.float16)


def grid_features4(geo, u, table, variant=None):
    """kernel_grid (gridencoder.cu:87-245) for the tiled D = 4, C = 2 grid, vectorised: -> [N, 32] in the table's dtype; an fp16 table
    runs the at::Half arithmetic (two roundings per corner).  variant names one WRONG kernel:
      w_indexed_where_dropped   the fourth coordinate indexed (stride (res+1)^3, mod the level's size) at the levels that drop it
      upper_corners_first       corners idx 8..15 accumulated before 0..7"""
    half = table.dtype == np.float16
    u = np.asarray(u, f32)
    N = u.shape[0]
    out = np.zeros((N, 2 * LEVELS), table.dtype)
    tab = table.astype(f32)
    oob = ((u < 0) | (u > 1)).any(1)
    order = list(range(8, 16)) + list(range(8)) if variant == "upper_corners_first" else list(range(16))
    for lv in geo.levels:
        q = (u * lv["scale"] + f32(0.5)).astype(f32)
        pg = np.floor(q)
        fr = (q - pg.astype(f32)).astype(f32)
        pg = pg.astype(np.int64)
        s = list(lv["s"])
        if variant == "w_indexed_where_dropped" and lv["kind"] == "w_dropped":
            s[3] = (lv["res"] + 1) ** 3
        acc = np.zeros((N, 2), f32)
        for idx in order:
            w = np.ones(N, f32)
            row = np.zeros(N, np.int64)
            for d in range(4):
                bit = (idx >> d) & 1
                w = (w * (fr[:, d] if bit else f32(1) - fr[:, d])).astype(f32)
                row = row + (pg[:, d] + bit) * s[d]
            val = tab[lv["off"] + np.where(oob, 0, row % lv["hs"])]
            t = (w[:, None] * val).astype(f32)
            if half:
                t = t.astype(np.float16).astype(f32)
            acc = (acc + t).astype(f32)
            if half:
                acc = acc.astype(np.float16).astype(f32)
        acc[oob] = 0
        out[:, 2 * lv["l"]:2 * lv["l"] + 2] = acc.astype(table.dtype)
    return out


def oracle_features(geo, u4, table):
    """The oracle's D = 4 grid encoder on normalised coordinates (fp16 table: at::Half arithmetic)."""
    enc, _ = O.grid_encode_forward(np.ascontiguousarray(u4, f32), table, geo.offsets, geo.pls, H_BASE, False, 1, False, 0)
    return enc


# ---- the fixture's model -------------------------------------------------------------------------------------------------------------------
def scale_rows(model, sigma_scale, ambient_scale):
    """The calibration both sides apply: row 0 of the last sigma layer (the density logit) and the last ambient layer, each times one
    recorded float32 factor."""
    import torch
    with torch.no_grad():
        model.ambient_net[-1].weight.mul_(float(f32(ambient_scale)))
        model.sigma_net[-1].weight[0].mul_(float(f32(sigma_scale)))


def mirror_model(device="cpu", check=True):
    """The mirror network (dnerf_amd/network_hyper.py) built from the seed and the two recorded factors; with `check` every state-dict
    entry must hash to the digest the generator recorded from the REFERENCE's class.  -> (model, bits)."""
    import torch
    from dnerf_amd.network_hyper import NeRFNetwork
    fx = load()
    torch.manual_seed(int(fx["seed"]))
    model = NeRFNetwork(**MODEL_KW)
    with torch.no_grad():
        model.encoder.embeddings.mul_(1e3)
    model.eval()
    bits = occupancy_bits(model.time_size, model.grid_size)
    with torch.no_grad():
        model.density_bitfield.copy_(torch.from_numpy(bits))
    scale_rows(model, fx["sigma_scale"], fx["ambient_scale"])
    if check:
        want = dict(zip(fx["digest_keys"].tolist(), fx["digest_vals"].tolist()))
        got = {k: hashlib.sha256(np.ascontiguousarray(v.detach().numpy()).tobytes()).hexdigest() for k, v in model.state_dict().items()
               if not k.startswith("density_grid")}
        assert set(want) == set(got), sorted(set(want) ^ set(got))
        bad = [k for k in want if want[k] != got[k]]
        assert not bad, f"state differs from the reference-built network: {bad}"
    return model.to(device).eval(), bits


def boosted_colour(state, gain=4.0):
    """`basis_support.boosted_colour` for this model: the seeded colour logits are of the order 1e-3 here too."""
    out = dict(state)
    for i in range(NETS["color_net"]):
        out[f"color_net.{i}.weight"] = (np.asarray(state[f"color_net.{i}.weight"], f32) * f32(gain)).astype(f32)
    return out


# ---- the model, restated -------------------------------------------------------------------------------------------------------------------
class HyperOracle:
    """forward / density of the ambient-dimension model from a state dict of numpy arrays.  mode "fp32": float64 accumulation rounded
    once to float32; "fp16": the `-O` roundings listed at the top of this file.  variant: one named WRONG model (VARIANTS).
    numpy_grid: the grid through `grid_features4` instead of the oracle's operator (the variants of the grid need it)."""

    def __init__(self, state, bound=1.0, density_scale=1.0, mode="fp32", variant=None, numpy_grid=False):
        assert variant is None or variant in VARIANTS, variant
        self.w = {net: [np.asarray(state[f"{net}.{i}.weight"], f32) for i in range(n)] for net, n in NETS.items()}
        emb = np.asarray(state["encoder.embeddings"], f32)
        self.table = emb.astype(np.float16) if mode == "fp16" else emb
        self.geo = Geometry4(bound)
        assert np.array_equal(self.geo.offsets, np.asarray(state["encoder.offsets"]))
        self.bound, self.density_scale, self.mode, self.variant = float(bound), density_scale, mode, variant
        self.numpy_grid = numpy_grid or variant in ("w_indexed_where_dropped", "upper_corners_first")

    def ambient(self, t):
        """-> the float32 the encoder receives (network_hyper.py:126-137)."""
        enc_t = O.freq_encode_forward(np.asarray(t, f32).reshape(1, 1), 6)
        h = _mlp(enc_t, self.w["ambient_net"], self.mode)[0, 0]
        if self.mode == "fp16":
            a = np.tanh(np.float64(h)).astype(np.float16)
            return f32(np.float16(f32(a) * f32(self.bound)))
        return f32(f32(np.tanh(np.float64(h))) * f32(self.bound))

    def row(self, t):
        """The [128] float32 constants row the kernel takes."""
        r = np.zeros(128, f32)
        r[0] = self.ambient(t)
        return r

    def features(self, x, ambient):
        u4 = self.geo.u4(x, ambient, normalise=self.variant != "ambient_unnormalised")
        if self.numpy_grid:
            return grid_features4(self.geo, u4, self.table, self.variant)
        return oracle_features(self.geo, u4, self.table)

    def sigma_outputs(self, x, ambient):
        """-> h [N, 33]: the density logit ++ 32 geo_feat (network_hyper.py:139-148)."""
        h = _mlp(self.features(x, ambient), self.w["sigma_net"], self.mode)
        if self.variant == "s1_off_by_one":
            h = np.concatenate([h[:, 1:2], h[:, 1:]], axis=1)      # sigma read from geo_feat[0]
        return h

    def density(self, x, t, ambient=None):
        h = self.sigma_outputs(x, self.ambient(t) if ambient is None else ambient)
        return {"sigma": np.exp(h[:, 0].astype(f32)).astype(f32), "geo_feat": h[:, 1:], "logit": h[:, 0]}

    def forward(self, x, d, t, ambient=None):
        """-> sigma [M] f32 (times density_scale), rgb [M,3] f32, None."""
        dens = self.density(x, t, ambient)
        sh, _ = O.sh_encode_forward(np.asarray(d, f32), 4)
        logit = _mlp(np.concatenate([sh, dens["geo_feat"].astype(f32)], axis=1), self.w["color_net"], self.mode).astype(np.float64)
        rgb = (1.0 / (1.0 + np.exp(-logit))).astype(f32)
        if self.mode == "fp16":
            rgb = rgb.astype(np.float16).astype(f32)
        return (f32(self.density_scale) * dens["sigma"]).astype(f32), rgb, None


def expected_f16(oracle, x, d, t, ambient=None):
    """The fp16 restatement's logits and outputs with the carried rounding bound of each logit (tests/basis_support.py, "the bars of
    the fused kernel": e_out = ulp16(out) + |W| e_in per layer, the grid features exact) -- in `field_bars`' record."""
    assert oracle.mode == "fp16" and oracle.variant is None
    a = oracle.ambient(t) if ambient is None else ambient
    enc = oracle.features(x, a)
    h, e = BS._bounded_mlp(enc, np.zeros(enc.shape, np.float64), oracle.w["sigma_net"])
    sh, _ = O.sh_encode_forward(np.asarray(d, f32), 4)
    cin = np.concatenate([sh, h[:, 1:].astype(f32)], axis=1)
    ein = np.concatenate([ulp16(sh), e[:, 1:]], axis=1)
    C, eC = BS._bounded_mlp(cin, ein, oracle.w["color_net"])
    L = h[:, 0]
    rgb = (1.0 / (1.0 + np.exp(-C.astype(np.float64)))).astype(np.float16)
    return {"logit": L, "logit_bound": e[:, 0], "rgb_logit": C, "rgb_logit_bound": eC, "rgb": rgb, "sigma": np.exp(L.astype(f32)).astype(f32)}


# ---- the weight packing, restated -----------------------------------------------------------------------------------------------------------
def pack_numpy(weights):
    """weights: the five [out, in] float32 arrays as the model holds them -> [30, 64, 8] float16.  The k-maps and tile counts are the
    basis kernel's (`basis_support.kmaps`); the last sigma layer goes in with geo_feat (rows 1..32) in tile 0 and the density logit
    (row 0) in row 0 of tile 1."""
    s0, s1, c0, c1, c2 = [np.asarray(w, f32) for w in weights]
    perm = np.zeros((33, 64), f32)
    perm[:32], perm[32] = s1[1:33], s1[0]
    return BS.pack_numpy([s0, perm, c0, c1, c2])
