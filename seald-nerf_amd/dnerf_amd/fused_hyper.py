"""MI355X-native fused field of the ambient-dimension model (`network_hyper.NeRFNetwork`, the reference's `--hyper`): host side of
csrc/field_hyper.hip.  Packs the five Linear layers of the sigma and colour nets into MFMA fragment order (30 blocks of 1 KiB, all
resident in LDS), computes the ambient coordinate of a time stamp with the model's own `ambient_net`, and launches the kernel through
the C ABI.

Fragment order: that of dnerf_amd/fused.py (`_pack_layer`).  The k-maps:
  * first sigma layer: lane-half h owns grid levels 8h..8h+7 (`fused._s0_kmap`);
  * hidden layers: the accumulator-as-operand order (`fused._acc_kmap`);
  * first colour layer: k-step 0 = SH coefficient 8h + j, k-steps 1 and 2 = geo_feat -- output tile 0 of the sigma net, raw -- in
    accumulator order, behind the 16 SH columns (the colour input is [SH(16), geo_feat(32)], network_hyper.py:151-152).
The last sigma layer (64 -> 33, output 0 the density logit, outputs 1..32 geo_feat: network_hyper.py:147-148) is packed with its rows
PERMUTED: geo_feat in tile 0 (rows 0..31), the logit in row 0 of tile 1, the rest of that tile zero (`permute_s1`).
The constants row of a frame is [128] f32: entry 0 = the ambient coordinate in [-bound, bound], zeros behind.  Under autocast the
reference's `tanh(ambient_net(.)) * bound` is an fp16 tensor and `torch.cat([x, ambient.repeat(..)])` promotes it to x's float32: the
encoder receives the fp16 value as float32, and that is the value stored.
The density-grid query (`query_cells`, `time_bias`: the CELLS variant of the kernel behind `fused.DensityGridUpdater`) takes the same
packed weights and one such row per time slice; a field offers it when it is built with `density_query=True`.
"""
import numpy as np
import torch

import sdn_backend
from sdn_backend import check, ptr, stream

from . import fused as F16

SHAPES = {"sigma_net": [(64, 32), (33, 64)], "color_net": [(64, 48), (64, 64), (3, 64)]}
ROW = 128
_NO_QUERY = ("this hyper field was built without density_query=True and has no density query (CELLS kernel): keep its grid with the "
             "op-by-op update_extra_state")


def available():
    return hasattr(sdn_backend.lib, "sdn_field_hyper_forward_f16")


def shapes_ok(model):
    """The architecture the kernel is built for: the defaults of dnerf/network_hyper.py on the default 4-D tiled grid."""
    enc = model.encoder
    nets_ok = all([tuple(l.weight.shape) for l in getattr(model, name)] == shapes for name, shapes in SHAPES.items())
    return bool(nets_ok and model.ambient_dim == 1 and enc.input_dim == 4 and enc.gridtype == "tiled" and not enc.align_corners
                and enc.interpolation == "linear" and enc.num_levels == 16 and enc.level_dim == 2 and not model.bg_radius > 0)


def permute_s1(w):
    """[33, 64] -> [33, 64]: rows 1..32 (geo_feat) first, row 0 (the density logit) last = row 0 of the second 32-row tile."""
    return np.concatenate([w[1:], w[:1]], axis=0)


def layer_plan(weights):
    """(W [out, in] float32, m-tile count, k-maps) of the five Linear layers in the kernel's block order S0 S1 C0 C1 C2; `weights`: their
    arrays in that order, as the model holds them."""
    s0, s1, c0, c1, c2 = weights
    hidden64 = [F16._acc_kmap(t, s) for t in range(2) for s in range(2)]
    c0_kmap = lambda s: 8 * np.arange(2)[:, None] + np.arange(8)[None, :] if s == 0 else 16 + F16._acc_kmap(0, s - 1)  # noqa: E731
    yield s0, 2, [F16._s0_kmap(s) for s in range(2)]
    yield permute_s1(s1), 2, hidden64
    yield c0, 2, [c0_kmap(s) for s in range(3)]
    yield c1, 2, hidden64
    yield c2, 1, hidden64


def pack_weights(model):
    """[30, 64, 8] float16."""
    g = lambda m: m.weight.detach().float().cpu().numpy()  # noqa: E731
    ws = [g(l) for l in model.sigma_net] + [g(l) for l in model.color_net]
    assert [w.shape for w in ws] == SHAPES["sigma_net"] + SHAPES["color_net"], "the fused kernel is built for the hyper network's default shape"
    packed = np.concatenate([F16._pack_layer(*layer) for layer in layer_plan(ws)], axis=0)
    assert packed.shape[0] == int(sdn_backend.lib.sdn_field_hyper_weight_blocks()), packed.shape
    return packed


class FusedHyperField(F16.Fp16Table, F16.FusedFieldBase):
    """Callable (xyzs [M,3], dirs [M,3]) -> (sigmas [M] f32, rgbs [M,3] f32) with the reference's -O numerics, for the frame drivers of
    dnerf_amd/frame_loops.py through `ctx_kind`.  `bias0` is the ambient row of the selected time stamp (the name the drivers read);
    `zero_deform` is always 0: the model deforms nothing."""

    ctx_kind = 4
    has_density_query = False    # an instance built with density_query=True sets it: `fused.DensityGridUpdater` reads it

    def __init__(self, model, time, fp16=True, max_points=None, table_layout=None, persistent=False, density_query=False):
        """density_query: also offer `time_bias` / `query_cells`, the density-grid query behind `fused.DensityGridUpdater` (the CELLS
        variant of the kernel, on the same packed weights and table).  Without it both raise NotImplementedError."""
        if not fp16:
            raise NotImplementedError("the fused hyper field implements the -O (fp16) configuration; use the op-by-op network for fp32")
        if persistent:
            raise NotImplementedError("the fused hyper field has no persistent two-set form: every launch is one tile per workgroup")
        if model.ambient_dim != 1:
            raise NotImplementedError("the fused hyper field is built for ambient_dim == 1 (a 4-D grid); use the op-by-op network")
        if model.bg_radius > 0:
            raise NotImplementedError("the fused hyper field does not serve the native drivers with a background model (bg_radius > 0)")
        if not available():
            raise sdn_backend.SdnError("libsdn_hip was built without the fused hyper field kernel")
        self.has_density_query = bool(density_query)
        self._choose_layout(table_layout)
        super().__init__(model, time, max_points)

    def _packed(self):
        return torch.from_numpy(pack_weights(self.model))

    def _time_row(self, t):
        """The ambient coordinate of time stamp `t` from the model's own encoder_time and ambient_net under fp16 autocast, as the
        float32 the grid encoder receives -> (row [128] f32, 0)."""
        dev = self.weights.device
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            a = self.model.ambient(torch.tensor([[t]], dtype=torch.float32, device=dev))
        row = torch.zeros(ROW, dtype=torch.float32, device=dev)
        row[0] = a.reshape(-1)[0].float()
        return row, 0

    def invalidate_time_cache(self):
        """Call after ambient_net's weights changed: cached rows were computed from the old weights."""
        self._time_cache.clear()
        self._group_cache.clear()

    def time_bias(self, times):
        """[K] (perturbed) times -> ambient rows [K,128] for the slices of a density update; row k is `_time_row(times[k])[0]` bit for
        bit.  One `ambient()` call per stamp, as `density(cas_xyzs, time_perturb)` makes it: a batched fp16 GEMM of K rows need not
        accumulate in the order of the one-row product.  Nothing is cached: perturbed times never repeat.  (`_time_row` opens its own
        autocast region: the trainer calls update_extra_state under one.)"""
        if not self.has_density_query:
            raise NotImplementedError(_NO_QUERY)
        return torch.stack([self._time_row(self.time_value(t))[0] for t in times.reshape(-1).tolist()]).contiguous()

    def query_cells(self, out, bias0, zero_deform, cas_bound, cells=None, cell_count=None, n=None, noise=None, seed=0):
        """out[cell] = density_scale * sigma for the listed (or the first n) cells of one occupancy slice (CELLS variant of the kernel);
        bias0: the ambient row of the slice's time.  zero_deform is accepted for the updater's sake and ignored: nothing deforms.
        Only a field built with `density_query=True` offers it."""
        if not self.has_density_query:
            raise NotImplementedError(_NO_QUERY)
        if cells is not None:
            n = cells.shape[0]
        with sdn_backend.timed("density_query_cells_hyper_f16", n):
            check(sdn_backend.lib.sdn_density_query_cells_hyper_f16(ptr(cells, torch.int32, "cells"), ptr(cell_count), n, ptr(noise, torch.float32, "noise"),
                                                                    int(seed) & 0xFFFFFFFF, self.model.grid_size, float(cas_bound), ptr(self.weights),
                                                                    ptr(bias0, torch.float32, "bias0"), ptr(self.table, torch.float16, "embeddings"),
                                                                    self.offsets_host.ctypes.data, self.S, self.H, self.bound, self.density_scale,
                                                                    ptr(out, torch.float32, "out"), stream()),
                  "density_query_cells_hyper_f16")
        return out

    def __call__(self, xyzs, dirs, live_idx=None, live_count=None):
        M = xyzs.shape[0]
        sigmas, rgbs = self._outputs(M)
        with sdn_backend.timed("field_hyper_forward_f16", M):
            check(sdn_backend.lib.sdn_field_hyper_forward_f16(ptr(xyzs, torch.float32, "xyzs"), ptr(dirs, torch.float32, "dirs"),
                                                              ptr(live_idx), ptr(live_count), M, ptr(self.weights), ptr(self.bias0),
                                                              ptr(self.table), self.offsets_host.ctypes.data, self.S, self.H, self.bound,
                                                              self.density_scale, ptr(sigmas), ptr(rgbs), stream()),
                  "field_hyper_forward_f16")
        return sigmas, rgbs
