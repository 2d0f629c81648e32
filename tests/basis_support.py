"""Shared by the temporal-basis tests and the fixture generator (tests/golden/gen_basis_fixture.py): the recipe behind
tests/golden/caller_basis.npz, a numpy restatement of the model (dnerf/network_basis.py:123-195 of the reference) over the oracle's
grid, SH and frequency operators in two precisions, a numpy restatement of the weight packing, named wrong variants and the bars the
GPU tests hold the fused kernel to.

fp16 restatement -- the reference under `-O` (torch autocast), the roundings csrc/field_basis.hip implements:
  * every Linear: inputs and weights rounded to fp16, exact products accumulated wide, output rounded to fp16, ReLU on the fp16 value;
  * the grid table and the encoder's output are fp16 with kernel_grid's per-corner roundings (the oracle's at::Half arithmetic); SH,
    the frequency encoding and trunc_exp run in fp32;
  * both contractions with the basis (`h[:, :32] @ sigma_basis`, `h.view(-1, 3, 8) @ color_basis`) are fp16 matrix products: fp16
    operands, wide accumulation, fp16 result;  sigma = exp(fp32(logit)),  rgb = fp16(sigmoid(logit)).
"""
import hashlib
import math
import os

import numpy as np

from oracle import oracle as O
from oracle.field import _linear, _mlp

f32 = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caller_basis.npz")
TIMES = (0.0, 0.5, 0.93)            # slice 0, slice 32 (the calibrated one), slice 59
MODEL_KW = dict(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1)
POINT_SEED, N_POINTS = 13, 2048
VARIANTS = ("other_time", "geo_sh_swapped", "view_8_3")
NETS = {"basis_net": 5, "sigma_net": 2, "color_net": 3}


def load():
    return np.load(FIXTURE)


def slice_of(t, T):
    return int(min(max(math.floor(t * T), 0), T - 1))


def occupancy_bits(T, G, scene=None):
    """The bench scene's occupancy bits in the slices of TIMES (`scene`: dnerf_amd/scene.py as a module, the generator loads it by path)."""
    if scene is None:
        from dnerf_amd import scene
    return scene.density_bitfield_all_times(T, G, "jumpingjacks", times={slice_of(t, T) for t in TIMES})


def scale_density_rows(model, scale):
    """The calibration both sides apply: the first 32 rows of the last sigma layer (the density coefficients) times one float32 factor."""
    import torch
    with torch.no_grad():
        model.sigma_net[-1].weight[:32].mul_(float(f32(scale)))


def seeded_points():
    import torch
    g = torch.Generator().manual_seed(POINT_SEED)
    x = (torch.rand(N_POINTS, 3, generator=g) * 2 - 1) * torch.tensor([0.45, 0.7, 0.3])
    d = torch.nn.functional.normalize(torch.randn(N_POINTS, 3, generator=g), dim=-1)
    return x.numpy().astype(f32), d.numpy().astype(f32)


def mirror_model(device="cpu", check=True):
    """The mirror network (dnerf_amd/network_basis.py) built from the seed and the recorded calibration factor; with `check` every
    state-dict entry must hash to the digest the generator recorded from the REFERENCE's class.  -> (model, bits)."""
    import torch
    from dnerf_amd.network_basis import NeRFNetwork
    fx = load()
    torch.manual_seed(int(fx["seed"]))
    model = NeRFNetwork(**MODEL_KW)
    with torch.no_grad():
        model.encoder.embeddings.mul_(1e3)
    model.eval()
    bits = occupancy_bits(model.time_size, model.grid_size)
    with torch.no_grad():
        model.density_bitfield.copy_(torch.from_numpy(bits))
    scale_density_rows(model, fx["sigma_scale"])
    if check:
        want = dict(zip(fx["digest_keys"].tolist(), fx["digest_vals"].tolist()))
        got = {k: hashlib.sha256(np.ascontiguousarray(v.detach().numpy()).tobytes()).hexdigest() for k, v in model.state_dict().items()
               if not k.startswith("density_grid")}
        assert set(want) == set(got), sorted(set(want) ^ set(got))
        bad = [k for k in want if want[k] != got[k]]
        assert not bad, f"state differs from the reference-built network: {bad}"
    return model.to(device).eval(), bits


def state_of(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if not k.startswith("density_grid")}


def boosted_colour(state, gain=4.0):
    """The state with every colour layer times `gain` (a power of two: nothing but exponents changes).  The seeded network's colour
    logits are of the order 1e-3 -- every rgb lies within an fp16 ulp or two of 0.5, and a wrong wiring of the colour net would pass
    any bar that allows for the output's own rounding; with gain^3 on the logits they are of order 0.1 .. 1 and the wiring shows.  The
    field tests (CPU variants, GPU kernel against the restatement) run on this state."""
    out = dict(state)
    for i in range(NETS["color_net"]):
        out[f"color_net.{i}.weight"] = (np.asarray(state[f"color_net.{i}.weight"], f32) * f32(gain)).astype(f32)
    return out


# ---- the model, restated ---------------------------------------------------------------------------------------------------------------
def _contract(h, basis, mode):
    """`h @ basis` along the last axis: fp16 mode = an autocast matmul (fp16 operands, wide sum, fp16 result)."""
    if mode == "fp16":
        y = h.astype(np.float16).astype(np.float64) @ basis.astype(np.float16).astype(np.float64)
        return y.astype(f32).astype(np.float16)
    return (h.astype(np.float64) @ basis.astype(np.float64)).astype(f32)


class BasisOracle:
    """forward / density of the temporal-basis model from a state dict of numpy arrays.  mode "fp32": float64 accumulation rounded once
    to float32; "fp16": the `-O` roundings listed at the top of this file.  variant: one named WRONG model (VARIANTS), for the CPU test
    of the GPU tests' bars."""

    def __init__(self, state, bound=1.0, density_scale=1.0, mode="fp32", variant=None, other_time=0.93):
        assert variant is None or variant in VARIANTS, variant
        self.w = {net: [np.asarray(state[f"{net}.{i}.weight"], f32) for i in range(n)] for net, n in NETS.items()}
        self.emb = np.asarray(state["encoder.embeddings"], f32)
        self.table = self.emb.astype(np.float16) if mode == "fp16" else self.emb
        self.offsets = np.asarray(state["encoder.offsets"], np.int32)
        self.bound, self.density_scale, self.mode, self.variant, self.other_time = float(bound), density_scale, mode, variant, other_time
        self.pls = np.exp2(np.log2(2048 * bound / 16) / 15)

    def basis(self, t):
        """-> (sigma_basis [32], color_basis [8]), network_basis.py:128-137."""
        if self.variant == "other_time":
            t = self.other_time
        enc_t = O.freq_encode_forward(np.asarray(t, f32).reshape(1, 1), 6)
        h = _mlp(enc_t, self.w["basis_net"], self.mode)[0]
        return h[:32], h[32:]

    def row(self, t):
        """The [128] float32 constants row the kernel takes."""
        r = np.zeros(128, f32)
        sb, cb = self.basis(t)
        r[:32], r[32:40] = sb.astype(f32), cb.astype(f32)
        return r

    def coefficients(self, x):
        """-> h [N, 64]: 32 density coefficients ++ 32 geo_feat (network_basis.py:140-145)."""
        u = ((np.asarray(x, f32) + f32(self.bound)) / f32(2 * self.bound)).astype(f32)
        enc, _ = O.grid_encode_forward(u, self.table, self.offsets, self.pls, 16, False, 1, False, 0)
        return _mlp(enc, self.w["sigma_net"], self.mode)

    def density(self, x, t):
        sb, _ = self.basis(t)
        h = self.coefficients(x)
        logit = _contract(h[:, :32], sb, self.mode)
        return {"sigma": np.exp(logit.astype(f32)).astype(f32), "geo_feat": h[:, 32:], "logit": logit}

    def colour_logits(self, d, geo_feat, cb):
        sh, _ = O.sh_encode_forward(np.asarray(d, f32), 4)
        geo = geo_feat.astype(f32)
        cin = np.concatenate([geo, sh] if self.variant == "geo_sh_swapped" else [sh, geo], axis=1)
        h = _mlp(cin, self.w["color_net"], self.mode)
        if self.variant == "view_8_3":
            coef = h.reshape(-1, 8, 3).transpose(0, 2, 1)
        else:
            coef = h.reshape(-1, 3, 8)
        return _contract(coef, cb, self.mode)

    def forward(self, x, d, t):
        """-> sigma [M] f32 (times density_scale), rgb [M,3] f32, None."""
        _, cb = self.basis(t)
        dens = self.density(x, t)
        logit = self.colour_logits(d, dens["geo_feat"], cb).astype(np.float64)
        rgb = (1.0 / (1.0 + np.exp(-logit))).astype(f32)
        if self.mode == "fp16":
            rgb = rgb.astype(np.float16).astype(f32)
        return (f32(self.density_scale) * dens["sigma"]).astype(f32), rgb, None


# ---- the weight packing, restated ----------------------------------------------------------------------------------------------------------
# v_mfma_f32_32x32x16_f16, weights = A operand: block (layer, m-tile mt, k-step ks) is 64 lanes x 8 halves, lane l holds
# W[32 mt + (l & 31)][kmap(ks, l >> 5, j)], j = 0..7.
def _acc(tile, s, h, j):
    return 32 * tile + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)


def kmaps():
    """Per layer (S0 S1 C0 C1 C2): (m-tiles, [k-step][h][j] -> input column)."""
    hj = [(h, j) for h in range(2) for j in range(8)]
    tab = lambda fn, steps: [np.array([fn(s, h, j) for h, j in hj]).reshape(2, 8) for s in range(steps)]  # noqa: E731
    hidden = tab(lambda s, h, j: _acc(s >> 1, s & 1, h, j), 4)
    s0 = tab(lambda s, h, j: 2 * (8 * h + 4 * s + (j >> 1)) + (j & 1), 2)
    c0 = tab(lambda s, h, j: 8 * h + j if s == 0 else 16 + _acc(0, s - 1, h, j), 3)
    return [(2, s0), (2, hidden), (2, c0), (2, hidden), (1, hidden)]


def pack_numpy(weights):
    """weights: the five [out, in] float32 arrays -> [30, 64, 8] float16."""
    blocks = []
    for W, (n_mt, km) in zip(weights, kmaps()):
        Wh = np.asarray(W, f32).astype(np.float16)
        for mt in range(n_mt):
            for ks in range(len(km)):
                b = np.zeros((64, 8), np.float16)
                for l in range(64):
                    r = 32 * mt + (l & 31)
                    if r < Wh.shape[0]:
                        b[l] = Wh[r, km[ks][l >> 5]]
                blocks.append(b)
    return np.stack(blocks)


def unpack_numpy(blocks, shapes):
    """The inverse: every weight read back from the one block element that holds it; rows a tile pads must be zero."""
    out, at = [], 0
    for shape, (n_mt, km) in zip(shapes, kmaps()):
        W = np.full(shape, np.nan, np.float16)
        for mt in range(n_mt):
            for ks in range(len(km)):
                b = blocks[at]
                at += 1
                for l in range(64):
                    r = 32 * mt + (l & 31)
                    if r < shape[0]:
                        W[r, km[ks][l >> 5]] = b[l]
                    else:
                        assert not b[l].any()
        assert not np.isnan(W.astype(f32)).any()
        out.append(W)
    assert at == blocks.shape[0]
    return out


# ---- the bars of the fused kernel against the fp16 restatement ---------------------------------------------------------------------------
# Kernel and restatement perform the same roundings on the same operands (the grid features are bit-exact: tests/field_probe_support.py);
# they differ in
#   (a) the accumulation: the MFMA sums 16 exact products at a time into an fp32 accumulator, the restatement sums all of them in
#       float64 -- a result that lies within fp32 rounding of an fp16 tie rounds to the other neighbour: ONE fp16 ulp of that value;
#   (b) SH: an fp32 polynomial evaluated in another order than the oracle's: the same effect on an input of the colour net.
# So every rounded value v of the chain may be off by ulp16(v) on its own account, plus what its inputs' errors contribute through
# the layer: e_out = ulp16(out) + |W| e_in (ReLU does not increase an error).  `expected_f16` carries this bound along the restatement,
# from the values the restatement itself computes, down to both logits: eL for the density logit, eC for the colour logits.  The bars:
#   sigma:  |log sigma - L| <= eL + DECODE        (DECODE = 2e-6 + 1e-7 |L|: v_exp_f32 and the float64 log, field_probe_support.DECODE_BAR)
#   rgb:    |rgb - ref| <= 2^-11 + eC / 4 + 2^-20 (the output's own fp16 rounding below 1; sigmoid's slope is at most 1/4; the fp32
#           v_exp_f32 / v_rcp_f32 pair)
# on EVERY point.  This is a worst case (every value flipping at once, all errors aligned), a few per cent of a logit of magnitude 1; the
# three wrong variants move logits by tenths and more on most points (tests/test_basis_cpu.py requires them to fail these bars).


def ulp16(v):
    """One fp16 ulp at |v|, taken one step up so that a value at the top of a binade counts its upper neighbour's spacing."""
    a = np.maximum(np.abs(np.asarray(v, np.float64)) * (1 + 2.0 ** -10), 2.0 ** -14)
    return np.exp2(np.floor(np.log2(a)) - 10)


def _bounded_mlp(h, e, weights):
    """fp16 `_mlp` with the error bound carried along: -> (h_out fp16, e_out)."""
    for i, w in enumerate(weights):
        h = _linear(h, w, "fp16")
        e = ulp16(h) + e @ np.abs(w.astype(np.float16).astype(np.float64)).T
        if i != len(weights) - 1:
            h = np.maximum(h, 0)
    return h, e


def expected_f16(oracle, x, d, t):
    """The fp16 restatement's logits and outputs with the bound of each logit (see above).  `oracle`: a BasisOracle in mode "fp16"."""
    assert oracle.mode == "fp16"
    sb, cb = oracle.basis(t)
    u = ((np.asarray(x, f32) + f32(oracle.bound)) / f32(2 * oracle.bound)).astype(f32)
    enc, _ = O.grid_encode_forward(u, oracle.table, oracle.offsets, oracle.pls, 16, False, 1, False, 0)
    h, e = _bounded_mlp(enc, np.zeros(enc.shape, np.float64), oracle.w["sigma_net"])
    assert np.array_equal(h, oracle.coefficients(x))
    L = _contract(h[:, :32], sb, "fp16")
    eL = ulp16(L) + e[:, :32] @ np.abs(sb.astype(np.float64))
    sh, _ = O.sh_encode_forward(np.asarray(d, f32), 4)
    cin = np.concatenate([sh, h[:, 32:].astype(f32)], axis=1)
    ein = np.concatenate([ulp16(sh), e[:, 32:]], axis=1)
    hc, ec = _bounded_mlp(cin, ein, oracle.w["color_net"])
    C = _contract(hc.reshape(-1, 3, 8), cb, "fp16")
    eC = ulp16(C) + ec.reshape(-1, 3, 8) @ np.abs(cb.astype(np.float64))
    rgb = (1.0 / (1.0 + np.exp(-C.astype(np.float64)))).astype(np.float16)
    return {"logit": L, "logit_bound": eL, "rgb_logit": C, "rgb_logit_bound": eC, "rgb": rgb, "sigma": np.exp(L.astype(f32)).astype(f32)}


def field_bars(sigma, rgb, ref, density_scale=1.0):
    """-> (ok, stats): the kernel's (or a wrong variant's) sigma [N] and rgb [N,3] against `expected_f16`'s record."""
    with np.errstate(divide="ignore", invalid="ignore"):
        got = np.log(np.asarray(sigma, np.float64) / density_scale)
    L = ref["logit"].astype(np.float64)
    es = np.abs(got - L)
    bar_s = ref["logit_bound"] + 2e-6 + 1e-7 * np.abs(L)
    er = np.abs(np.asarray(rgb, np.float64) - ref["rgb"].astype(np.float64))
    bar_r = 2.0 ** -11 + ref["rgb_logit_bound"] / 4 + 2.0 ** -20
    with np.errstate(invalid="ignore"):
        bad_s, bad_r = ~(es <= bar_s), ~(er <= bar_r)
    stats = {"sigma_failed": int(bad_s.sum()), "rgb_failed": int(bad_r.sum()), "sigma_worst_of_bar": float(np.nanmax(es / bar_s)),
             "rgb_worst_of_bar": float(np.nanmax(er / bar_r)), "sigma_bit_exact_share": float((got.astype(np.float16) == ref["logit"]).mean()),
             "rgb_bit_exact_share": float((np.asarray(rgb, f32).astype(np.float16) == ref["rgb"]).mean()),
             "median_sigma_bar": float(np.median(bar_s)), "median_rgb_bar": float(np.median(bar_r))}
    return not bad_s.any() and not bad_r.any(), stats


def dist3(got, want, rel_floor=None):
    """(max, p99.9, mean) of |got - want| (relative with a floor, if given)."""
    e = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).ravel()
    if rel_floor is not None:
        e = e / np.maximum(np.abs(np.asarray(want, np.float64)).ravel(), rel_floor)
    return float(e.max()), float(np.quantile(e, 0.999)), float(e.mean())
