"""Temporal-basis dynamic-NeRF field network (`main_dnerf.py --basis`): a static tiled-grid field whose outputs are coefficients, and a
small MLP of the time stamp alone whose outputs are the basis that contracts them.

Host-side mirror of the reference's dnerf/network_basis.py:10-262 (`NeRFNetwork`), the way dnerf_amd/network.py mirrors the
deformation model: the same constructor arguments, sub-module and parameter names (`encoder_time`, `basis_net.{l}.weight`,
`encoder.embeddings`, `encoder.offsets`, `sigma_net`, `encoder_dir`, `color_net`, `bg_net`) and `get_params`, so a reference
checkpoint's model state dict loads.  (The reference's `color` is commented out there -- its non-cuda-ray mode is broken for this
model, network_basis.py:214 -- and is kept here as its masked colour query with the basis passed in.)

Two evaluation paths, as in dnerf_amd/network.py:
  * `forward` / `density` / `background` / `color` -- the reference's op sequence on the drop-in operators; differentiable.
  * the fused dispatch inside `forward`: in eval mode, without autograd, under fp16 autocast (the reference's `-O`) and with the
    default geometry the whole network is ONE launch of csrc/field_basis.hip (`sdn_field_basis_forward_f16`) behind
    `fused_basis.FusedBasisField`; `model.fused_inference = False` switches it off.  Without autocast (the reference without `-O`)
    `forward` stays op by op unless `model.fused_inference_f32 = True`: then it is one launch of csrc/field_basis_f32.hip
    (`sdn_field_basis_forward_f32`) behind `fused_basis.FusedBasisFieldF32`, within 1e-4 of the op-by-op fp32 network.
"""
import torch

import sdn_backend
from freqencoder import FreqEncoder
from gridencoder import GridEncoder
from shencoder import SHEncoder

from .network import _mlp, _run_mlp, trunc_exp
from .network import NeRFNetwork as _DeformNetwork
from .renderer import NeRFRenderer


class NeRFNetwork(NeRFRenderer):
    def __init__(self, encoding="tiledgrid", encoding_dir="sphere_harmonics", encoding_time="frequency", encoding_bg="hashgrid",
                 num_layers=2, hidden_dim=64, geo_feat_dim=32, num_layers_color=3, hidden_dim_color=64, num_layers_bg=2, hidden_dim_bg=64,
                 sigma_basis_dim=32, color_basis_dim=8, num_layers_basis=5, hidden_dim_basis=128, bound=1, **kwargs):
        super().__init__(bound, **kwargs)
        if (encoding, encoding_dir, encoding_time, encoding_bg) != ("tiledgrid", "sphere_harmonics", "frequency", "hashgrid"):
            raise NotImplementedError("only the default encoders of dnerf/network_basis.py are mirrored")
        self.num_layers_basis, self.hidden_dim_basis = num_layers_basis, hidden_dim_basis
        self.sigma_basis_dim, self.color_basis_dim = sigma_basis_dim, color_basis_dim
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim
        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color

        # basis: freq(t, 6) -> 4 x 128 -> 32 + 8                                    (network_basis.py:32-53)
        self.encoder_time = FreqEncoder(input_dim=1, degree=6)
        self.in_dim_time = self.encoder_time.output_dim
        self.basis_net = _mlp([self.in_dim_time] + [hidden_dim_basis] * (num_layers_basis - 1) + [sigma_basis_dim + color_basis_dim])

        # density coefficients: tiled grid (16 levels x 2, 16 -> 2048*bound) -> 64 -> 32 + 32      (network_basis.py:55-75)
        self.encoder = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                                   desired_resolution=2048 * bound, gridtype="tiled", align_corners=False)
        self.in_dim = self.encoder.output_dim
        self.sigma_net = _mlp([self.in_dim] + [hidden_dim] * (num_layers - 1) + [sigma_basis_dim + geo_feat_dim])

        # colour coefficients: SH(dir, 4) ++ geo_feat -> 64 -> 64 -> 3 x 8                             (network_basis.py:77-96)
        self.encoder_dir = SHEncoder(input_dim=3, degree=4)
        self.in_dim_dir = self.encoder_dir.output_dim
        self.color_net = _mlp([self.in_dim_dir + geo_feat_dim] + [hidden_dim_color] * (num_layers_color - 1) + [3 * color_basis_dim])

        # background sphere (bg_radius > 0)                                                            (network_basis.py:98-120)
        if self.bg_radius > 0:
            self.num_layers_bg, self.hidden_dim_bg = num_layers_bg, hidden_dim_bg
            self.encoder_bg = GridEncoder(input_dim=2, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                                          desired_resolution=2048, gridtype="hash", align_corners=False)
            self.in_dim_bg = self.encoder_bg.output_dim
            self.bg_net = _mlp([self.in_dim_bg + self.in_dim_dir] + [hidden_dim_bg] * (num_layers_bg - 1) + [3])
        else:
            self.bg_net = None

    # ------------------------------------------------------------------------------------------
    def basis(self, t):
        """t [1,1] -> (sigma_basis [32], color_basis [8])   (network_basis.py:128-137)."""
        h = _run_mlp(self.basis_net, self.encoder_time(t))
        return h[0, :self.sigma_basis_dim], h[0, self.sigma_basis_dim:]

    def _sigma(self, x, sigma_basis):
        h = _run_mlp(self.sigma_net, self.encoder(x, bound=self.bound))
        return trunc_exp(h[..., :self.sigma_basis_dim] @ sigma_basis), h[..., self.sigma_basis_dim:]

    def _color(self, d, geo_feat, color_basis):
        h = _run_mlp(self.color_net, torch.cat([self.encoder_dir(d), geo_feat], dim=-1))
        return torch.sigmoid(h.view(-1, 3, self.color_basis_dim) @ color_basis)

    # -- fused inference dispatch -----------------------------------------------------------------
    fused_inference = True       # class default; set False on a model to keep `forward` on the op-by-op path in every mode

    fused_inference_f32 = False  # opt-in: without autocast (the reference without -O) dispatch to the fp32 fused kernel as well

    def _fused_inference_ok(self, x, d):
        """False, or the mode of the fused dispatch: 16 (-O: csrc/field_basis.hip) or 32 (no autocast, opt-in: csrc/field_basis_f32.hip)."""
        if not self.fused_inference or self.training or torch.is_grad_enabled() or not x.is_cuda or x.dim() != 2 or x.shape[0] == 0:
            return False
        if x.dtype != torch.float32 or d.dtype != torch.float32:
            return False
        if not torch.is_autocast_enabled("cuda"):
            if not self.fused_inference_f32:
                return False   # the default without -O stays the op-by-op network, what the fp32 fixture pins
            mode = 32
        elif torch.get_autocast_dtype("cuda") == torch.float16:
            mode = 16
        else:
            return False
        ok = self.__dict__.get("_fused_arch_ok")
        if ok is None:         # the architecture does not change after construction
            from . import fused_basis
            ok = bool(fused_basis.available() and fused_basis.shapes_ok(self))
            self.__dict__["_fused_arch_ok"] = ok
        if not ok:
            return False
        if mode == 32:
            ok32 = self.__dict__.get("_fused_f32_ok")
            if ok32 is None:
                from . import fused_basis
                ok32 = bool(fused_basis.available_f32() and not self.bg_radius > 0)
                self.__dict__["_fused_f32_ok"] = ok32
            if not ok32 or any(p.dtype != torch.float32 for p in (self.encoder.embeddings, self.sigma_net[0].weight, self.basis_net[0].weight)):
                return False
        return mode

    def _parameter_epoch(self):
        ps = self.__dict__.get("_fused_params")
        if ps is None:
            ps = tuple([self.encoder.embeddings] + [l.weight for net in (self.basis_net, self.sigma_net, self.color_net) for l in net])
            self.__dict__["_fused_params"] = ps
        return tuple([(p.data_ptr(), p._version) for p in ps])

    _fused_time_value = _DeformNetwork._fused_time_value

    def _forward_fused(self, x, d, t, mode=16):
        """The whole network in one launch: sigma [M] f32 (density_scale NOT applied: the caller multiplies), rgb [M,3].  mode 16 (-O):
        rgb holds the fp16 values of torch.sigmoid on the half logits in f32; mode 32: float32 throughout, within 1e-4 of the op-by-op
        evaluation (tests/test_gpu_basis_f32.py).  Each mode keeps its own field, built once per parameter version."""
        epoch = self._parameter_epoch()
        if mode == 16:
            cache = self.__dict__.get("_fused_cache")
            if cache is None or cache[0] != epoch[1:]:
                from . import fused_basis
                field = fused_basis.FusedBasisField(self, t, fp16=True)
                field.density_scale = 1.0
                cache = self.__dict__["_fused_cache"] = (epoch[1:], field, epoch[0])
            elif cache[2] != epoch[0]:      # only the embeddings moved
                cache[1].load_table(self.encoder.embeddings.detach())
                cache = self.__dict__["_fused_cache"] = (cache[0], cache[1], epoch[0])
        else:
            sdn_backend.await_pending_write(self.encoder.embeddings)     # (read in place below: a table pass still running elsewhere)
            cache = self.__dict__.get("_fused_cache32")
            if cache is None or cache[0] != epoch[1:] or cache[2][0] != epoch[0][0]:
                from . import fused_basis
                # (the table is read where it is: its in-place updates need nothing, only another tensor does)
                field = fused_basis.FusedBasisFieldF32(self, t)
                field.density_scale = 1.0
                cache = self.__dict__["_fused_cache32"] = (epoch[1:], field, epoch[0])
        field = cache[1]
        field.set_time_if_changed(self._fused_time_value(field, t))
        field._buf = None              # fresh output tensors per call: the caller owns them, as on the op-by-op path
        return field(x.contiguous(), d.contiguous())

    def use_native_density_update(self, field=None, fp32=False):
        """Route update_extra_state through the CELLS variant of csrc/field_basis.hip + csrc/density.hip (`-O` numerics;
        `fused.DensityGridUpdater`).  Opt-in: the op-by-op update stays the default.  The configurations the fused field refuses are
        refused here.  A model trained without -O: `field=fused_basis.FusedBasisFieldF32(model, t0)` (the CELLS variant of
        csrc/field_basis_f32.hip); `fp32=True` without a field stays refused."""
        from . import fused_basis
        if self.bg_radius > 0:
            raise NotImplementedError("native density update of the temporal-basis model: bg_radius > 0 (the background sphere) is not "
                                      "served by the fused basis field; keep the op-by-op update_extra_state")
        if not fused_basis.shapes_ok(self):
            raise NotImplementedError("native density update of the temporal-basis model: the fused basis field is built for the default "
                                      "architecture of dnerf/network_basis.py (sigma net 32-64-64, colour net 48-64-64-24, basis 32 + 8, "
                                      "16 x 2 tiled grid); keep the op-by-op update_extra_state")
        return super().use_native_density_update(field, fp32=fp32)

    def forward(self, x, d, t):
        """x [M,3] in [-bound,bound], d [M,3] unit, t [1,1] -> sigma [M], rgb [M,3], None  (network_basis.py:123-161)."""
        mode = self._fused_inference_ok(x, d)
        if mode:
            sigma, rgb = self._forward_fused(x, d, t, mode)
            return sigma, rgb, None
        sigma_basis, color_basis = self.basis(t)
        sigma, geo_feat = self._sigma(x, sigma_basis)
        return sigma, self._color(d, geo_feat, color_basis), None

    def density(self, x, t):
        """network_basis.py:163-195."""
        sigma_basis, _ = self.basis(t)
        sigma, geo_feat = self._sigma(x, sigma_basis)
        return {"sigma": sigma, "geo_feat": geo_feat}

    def background(self, x, d):
        """x [N,2] in [-1,1], d [N,3] -> rgb [N,3]   (network_basis.py:197-212)."""
        h = torch.cat([self.encoder_dir(d), self.encoder_bg(x)], dim=-1)
        return torch.sigmoid(_run_mlp(self.bg_net, h))

    def color(self, x, d, mask=None, geo_feat=None, color_basis=None, **kwargs):
        """The masked colour query the reference left commented out for want of the basis (network_basis.py:214-245): `color_basis` [8]
        is required here."""
        if color_basis is None:
            raise ValueError("the temporal-basis model's colour query needs color_basis (`model.basis(t)[1]`)")
        if mask is not None:
            rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            if not mask.any():
                return rgbs
            d, geo_feat = d[mask], geo_feat[mask]
        h = self._color(d, geo_feat, color_basis)
        if mask is not None:
            rgbs[mask] = h.to(rgbs.dtype)
            return rgbs
        return h

    def get_params(self, lr, lr_net):
        """network_basis.py:248-262."""
        return [
            {"params": self.encoder.parameters(), "lr": lr},
            {"params": self.sigma_net.parameters(), "lr": lr_net},
            {"params": self.encoder_dir.parameters(), "lr": lr},
            {"params": self.color_net.parameters(), "lr": lr_net},
            {"params": self.encoder_time.parameters(), "lr": lr},
            {"params": self.basis_net.parameters(), "lr": lr_net},
        ] + ([{"params": self.encoder_bg.parameters(), "lr": lr}, {"params": self.bg_net.parameters(), "lr": lr_net}] if self.bg_radius > 0 else [])
