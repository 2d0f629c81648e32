"""MI355X-native fused field of the temporal-basis model (`network_basis.NeRFNetwork`, the reference's `--basis`): host side of
csrc/field_basis.hip.  Packs the five Linear layers of the sigma and colour nets into MFMA fragment order (30 blocks of 1 KiB, all
resident in LDS), computes the basis row of a time stamp with the model's own `basis_net`, and launches the kernel through the C ABI.

Fragment order: that of dnerf_amd/fused.py (`_pack_layer`).  The k-maps:
  * first sigma layer: lane-half h owns grid levels 8h..8h+7 (`fused._s0_kmap`);
  * hidden layers: the accumulator-as-operand order (`fused._acc_kmap`);
  * first colour layer: k-step 0 = SH coefficient 8h + j, k-steps 1 and 2 = geo_feat -- output tile 1 of the sigma net, raw -- in
    accumulator order, behind the 16 SH columns (the colour input is [SH(16), geo_feat(32)], network_basis.py:151-152).
The constants row of a frame is [128] f32: sigma_basis in 0..31, color_basis in 32..39, zeros behind -- the fp16 values autocast's
basis_net returns, which are exactly what the reference contracts with.
The density-grid query (`query_cells`, `time_bias`: the CELLS variant of the kernel behind `fused.DensityGridUpdater`) takes the same
packed weights and one such row per time slice.

`FusedBasisFieldF32` is the same model WITHOUT `-O` (csrc/field_basis_f32.hip): the fp32 weights in the A-operand order of
v_mfma_f32_32x32x2_f32 (`pack_weights_f32`: `fused_f32._pack_layer` blocks [pair][lane][m-tile], S0 | S1 | C0 | C1 | C2), the model's own
fp32 table in place, and the basis row of `basis_net` evaluated without autocast.
"""
import numpy as np
import torch

import sdn_backend
from sdn_backend import check, ptr, stream

from . import fused as F16
from . import fused_f32 as F32

SHAPES = {"sigma_net": [(64, 32), (64, 64)], "color_net": [(64, 48), (64, 64), (24, 64)]}
ROW = 128


def available():
    return hasattr(sdn_backend.lib, "sdn_field_basis_forward_f16")


def shapes_ok(model):
    """The architecture the kernel is built for: the defaults of dnerf/network_basis.py on the default tiled grid."""
    enc = model.encoder
    nets_ok = all([tuple(l.weight.shape) for l in getattr(model, name)] == shapes for name, shapes in SHAPES.items())
    return bool(nets_ok and model.sigma_basis_dim == 32 and model.color_basis_dim == 8 and enc.gridtype == "tiled" and not enc.align_corners
                and enc.interpolation == "linear" and enc.num_levels == 16 and enc.level_dim == 2)


def _c0_kmap(s):
    h = np.arange(2)[:, None]
    j = np.arange(8)[None, :]
    if s == 0:
        return 8 * h + j                           # SH coefficient
    return 16 + F16._acc_kmap(0, s - 1)            # geo_feat[i] = sigma-net output 32 + i, i in accumulator order


def layer_plan(weights):
    """(W [out, in] float32, m-tile count, k-maps) of the five Linear layers in the kernel's block order S0 S1 C0 C1 C2; `weights`: their
    arrays in that order."""
    s0, s1, c0, c1, c2 = weights
    hidden64 = [F16._acc_kmap(t, s) for t in range(2) for s in range(2)]
    yield s0, 2, [F16._s0_kmap(s) for s in range(2)]
    yield s1, 2, hidden64
    yield c0, 2, [_c0_kmap(s) for s in range(3)]
    yield c1, 2, hidden64
    yield c2, 1, hidden64


def pack_weights(model):
    """[30, 64, 8] float16."""
    g = lambda m: m.weight.detach().float().cpu().numpy()  # noqa: E731
    ws = [g(l) for l in model.sigma_net] + [g(l) for l in model.color_net]
    assert [w.shape for w in ws] == SHAPES["sigma_net"] + SHAPES["color_net"], "the fused kernel is built for the basis network's default shape"
    packed = np.concatenate([F16._pack_layer(*layer) for layer in layer_plan(ws)], axis=0)
    assert packed.shape[0] == int(sdn_backend.lib.sdn_field_basis_weight_blocks()), packed.shape
    return packed


class FusedBasisField(F16.Fp16Table, F16.FusedFieldBase):
    """Callable (xyzs [M,3], dirs [M,3]) -> (sigmas [M] f32, rgbs [M,3] f32) with the reference's -O numerics, for the frame drivers of
    dnerf_amd/frame_loops.py through `ctx_kind`.  `bias0` is the basis row of the selected time stamp (the name the drivers read);
    `zero_deform` is always 0: the model deforms nothing."""

    ctx_kind = 3

    def __init__(self, model, time, fp16=True, max_points=None, table_layout=None):
        if not fp16:
            raise NotImplementedError("the fused basis field implements the -O (fp16) configuration; use the op-by-op network for fp32, "
                                      "or fused_basis.FusedBasisFieldF32 for the fused fp32 kernel")
        if not available():
            raise sdn_backend.SdnError("libsdn_hip was built without the fused basis field kernel")
        self._choose_layout(table_layout)
        super().__init__(model, time, max_points)

    def _packed(self):
        return torch.from_numpy(pack_weights(self.model))

    def _time_row(self, t):
        """The basis of time stamp `t` from the model's own encoder_time and basis_net under fp16 autocast -> (row [128] f32, 0)."""
        m = self.model
        dev = self.weights.device
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sigma_basis, color_basis = m.basis(torch.tensor([[t]], dtype=torch.float32, device=dev))
        row = torch.zeros(ROW, dtype=torch.float32, device=dev)
        row[:32], row[32:40] = sigma_basis.float(), color_basis.float()
        return row, 0

    def invalidate_time_cache(self):
        """Call after basis_net's weights changed: cached rows were computed from the old weights."""
        self._time_cache.clear()
        self._group_cache.clear()

    def time_bias(self, times):
        """[K] (perturbed) times -> basis rows [K,128] for the slices of a density update; row k is `_time_row(times[k])[0]` bit for bit.
        One `basis()` call per stamp, as `density(cas_xyzs, time_perturb)` makes it: a batched fp16 GEMM of K rows need not accumulate in
        the order of the one-row product.  (`_time_row` opens its own autocast region: the trainer calls update_extra_state under one.)"""
        return torch.stack([self._time_row(self.time_value(t))[0] for t in times.reshape(-1).tolist()]).contiguous()

    def query_cells(self, out, bias0, zero_deform, cas_bound, cells=None, cell_count=None, n=None, noise=None, seed=0):
        """out[cell] = density_scale * sigma for the listed (or the first n) cells of one occupancy slice (CELLS variant of the kernel);
        bias0: the basis row of the slice's time.  zero_deform is accepted for the updater's sake and ignored: nothing deforms."""
        if cells is not None:
            n = cells.shape[0]
        with sdn_backend.timed("density_query_cells_basis_f16", n):
            check(sdn_backend.lib.sdn_density_query_cells_basis_f16(ptr(cells, torch.int32, "cells"), ptr(cell_count), n, ptr(noise, torch.float32, "noise"),
                                                                    int(seed) & 0xFFFFFFFF, self.model.grid_size, float(cas_bound), ptr(self.weights),
                                                                    ptr(bias0, torch.float32, "bias0"), ptr(self.table, torch.float16, "embeddings"),
                                                                    self.offsets_host.ctypes.data, self.S, self.H, self.bound, self.density_scale,
                                                                    ptr(out, torch.float32, "out"), stream()),
                  "density_query_cells_basis_f16")
        return out

    def __call__(self, xyzs, dirs, live_idx=None, live_count=None):
        M = xyzs.shape[0]
        sigmas, rgbs = self._outputs(M)
        with sdn_backend.timed("field_basis_forward_f16", M):
            check(sdn_backend.lib.sdn_field_basis_forward_f16(ptr(xyzs, torch.float32, "xyzs"), ptr(dirs, torch.float32, "dirs"),
                                                              ptr(live_idx), ptr(live_count), M, ptr(self.weights), ptr(self.bias0),
                                                              ptr(self.table), self.offsets_host.ctypes.data, self.S, self.H, self.bound,
                                                              self.density_scale, ptr(sigmas), ptr(rgbs), stream()),
                  "field_basis_forward_f16")
        return sigmas, rgbs


# ---- the same model without -O: csrc/field_basis_f32.hip ---------------------------------------------------------------------------
def available_f32():
    return hasattr(sdn_backend.lib, "sdn_field_basis_forward_f32")


def pair_plan_f32():
    """(k-pairs, m-tiles) of the five layers in stage order S0 S1 C0 C1 C2: which two input columns the lane halves of a k-pair mean."""
    s0 = [(2 * l, 2 * l + 1) for l in range(16)]                          # the two channels of grid level l
    c0 = [(2 * p, 2 * p + 1) for p in range(8)]                           # SH coefficients
    for v in range(16):                                                   # geo_feat: accumulator registers 0..15 of the sigma net's tile 1
        g = 8 * (v >> 2) + (v & 3)
        c0.append((16 + g, 16 + g + 4))
    acc = F32._acc_pairs(2)
    return [(s0, 2), (acc, 2), (c0, 2), (acc, 2), (acc, 1)]


def pack_weights_f32(model):
    """The five Linear weights in the kernel's stage order (S0 | S1 | C0 | C1 | C2), flat float32."""
    g = lambda lin: lin.weight.detach().float().cpu().numpy()   # noqa: E731
    ws = [g(l) for l in model.sigma_net] + [g(l) for l in model.color_net]
    assert [w.shape for w in ws] == SHAPES["sigma_net"] + SHAPES["color_net"], "the fused kernel is built for the basis network's default shape"
    flat = np.concatenate([F32._pack_layer(w, pairs, mt).reshape(-1) for w, (pairs, mt) in zip(ws, pair_plan_f32())]).astype(np.float32)
    assert flat.shape[0] == int(sdn_backend.lib.sdn_field_basis_weight_floats_f32()), flat.shape
    return flat


class FusedBasisFieldF32(F16.FusedFieldBase):
    """Callable (xyzs [M,3], dirs [M,3]) -> (sigmas [M] f32, rgbs [M,3] f32): the temporal-basis model without autocast
    (dnerf/network_basis.py:123-161 in float32) in one launch, within 1e-4 of the fp32 network.  Same interface as `FusedBasisField`;
    the table is the model's own fp32 tensor, read in place.  `zero_deform` is always 0: the model deforms nothing."""

    ctx_kind = 5

    def __init__(self, model, time, max_points=None):
        if not available_f32():
            raise sdn_backend.SdnError("libsdn_hip was built without the fp32 fused basis field kernel")
        if getattr(model, "bg_radius", 0) > 0:
            raise NotImplementedError("the fp32 fused basis field does not serve bg_radius > 0 (the background sphere)")
        if not shapes_ok(model):
            raise NotImplementedError("the fp32 fused basis field is built for the default architecture of dnerf/network_basis.py (sigma "
                                      "net 32-64-64, colour net 48-64-64-24, basis 32 + 8, 16 x 2 tiled grid)")
        if model.encoder.embeddings.dtype != torch.float32:
            raise sdn_backend.SdnError("the fp32 fused basis field reads the model's fp32 embedding table in place")
        super().__init__(model, time, max_points)

    def _packed(self):
        return torch.from_numpy(pack_weights_f32(self.model))

    _bind_table = F32.FusedFieldF32._bind_table
    load_table = F32.FusedFieldF32.load_table

    def _time_row(self, t):
        """The basis of time stamp `t` from the model's own encoder_time and basis_net without autocast -> (row [128] f32, 0)."""
        m = self.model
        dev = self.weights.device
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            sigma_basis, color_basis = m.basis(torch.tensor([[t]], dtype=torch.float32, device=dev))
        row = torch.zeros(ROW, dtype=torch.float32, device=dev)
        row[:32], row[32:40] = sigma_basis.float(), color_basis.float()
        return row, 0

    invalidate_time_cache = FusedBasisField.invalidate_time_cache

    def time_bias(self, times):
        """[K] (perturbed) times -> basis rows [K,128]; row k is `_time_row(times[k])[0]` bit for bit: one `basis()` call per stamp,
        as `density(cas_xyzs, time_perturb)` makes it (a batched GEMM of K rows need not accumulate in the order of the one-row product)."""
        return torch.stack([self._time_row(self.time_value(t))[0] for t in times.reshape(-1).tolist()]).contiguous()

    def query_cells(self, out, bias0, zero_deform, cas_bound, cells=None, cell_count=None, n=None, noise=None, seed=0):
        """out[cell] = density_scale * sigma for the listed (or the first n) cells of one occupancy slice (CELLS variant of the kernel);
        bias0: the basis row of the slice's time.  zero_deform is accepted for the updater's sake and ignored: nothing deforms."""
        if cells is not None:
            n = cells.shape[0]
        with sdn_backend.timed("density_query_cells_basis_f32", n):
            check(sdn_backend.lib.sdn_density_query_cells_basis_f32(ptr(cells, torch.int32, "cells"), ptr(cell_count), n, ptr(noise, torch.float32, "noise"),
                                                                    int(seed) & 0xFFFFFFFF, self.model.grid_size, float(cas_bound), ptr(self.weights),
                                                                    ptr(bias0, torch.float32, "bias0"), ptr(self.table, torch.float32, "embeddings"),
                                                                    self.offsets_host.ctypes.data, self.S, self.H, self.bound, self.density_scale,
                                                                    ptr(out, torch.float32, "out"), stream()),
                  "density_query_cells_basis_f32")
        return out

    def __call__(self, xyzs, dirs, live_idx=None, live_count=None):
        M = xyzs.shape[0]
        sigmas, rgbs = self._outputs(M)
        with sdn_backend.timed("field_basis_forward_f32", M):
            check(sdn_backend.lib.sdn_field_basis_forward_f32(ptr(xyzs, torch.float32, "xyzs"), ptr(dirs, torch.float32, "dirs"),
                                                              ptr(live_idx), ptr(live_count), M, ptr(self.weights), ptr(self.bias0),
                                                              ptr(self.table, torch.float32, "embeddings"), self.offsets_host.ctypes.data,
                                                              self.S, self.H, self.bound, self.density_scale, ptr(sigmas), ptr(rgbs), stream()),
                  "field_basis_forward_f32")
        return sigmas, rgbs
