"""Ambient-dimension dynamic-NeRF field network (`main_dnerf.py --hyper`): a small MLP of the time stamp alone gives an ambient
coordinate, and a static tiled grid over (x, y, z, ambient) -- 4-D for the default ambient_dim = 1 -- feeds the sigma and colour nets.

Host-side mirror of the reference's dnerf/network_hyper.py:10-262 (`NeRFNetwork`), the way dnerf_amd/network_basis.py mirrors the
temporal-basis model: the same constructor arguments, sub-module and parameter names (`encoder_time`, `ambient_net.{l}.weight`,
`encoder.embeddings`, `encoder.offsets`, `sigma_net`, `encoder_dir`, `color_net`, `bg_net`) and `get_params`, so a reference
checkpoint's model state dict loads with strict=True.

Two evaluation paths, as in dnerf_amd/network_basis.py:
  * `forward` / `density` / `background` / `color` -- the reference's op sequence on the drop-in operators; differentiable.
  * the fused dispatch inside `forward`: in eval mode, without autograd, under fp16 autocast (the reference's `-O`) and with the
    default geometry (ambient_dim 1, default widths, no background model) the whole network is ONE launch of csrc/field_hyper.hip
    (`sdn_field_hyper_forward_f16`) behind `fused_hyper.FusedHyperField`; `model.fused_inference = False` switches it off.  There is
    no fused fp32 configuration.
"""
import torch

from freqencoder import FreqEncoder
from gridencoder import GridEncoder
from shencoder import SHEncoder

from .network import _mlp, _run_mlp, trunc_exp
from .network import NeRFNetwork as _DeformNetwork
from .renderer import NeRFRenderer


class NeRFNetwork(NeRFRenderer):
    def __init__(self, encoding="tiledgrid", encoding_dir="sphere_harmonics", encoding_time="frequency", encoding_bg="hashgrid",
                 num_layers=2, hidden_dim=64, geo_feat_dim=32, num_layers_color=3, hidden_dim_color=64, num_layers_bg=2, hidden_dim_bg=64,
                 num_layers_ambient=5, hidden_dim_ambient=128, ambient_dim=1, bound=1, **kwargs):
        super().__init__(bound, **kwargs)
        if (encoding, encoding_dir, encoding_time, encoding_bg) != ("tiledgrid", "sphere_harmonics", "frequency", "hashgrid"):
            raise NotImplementedError("only the default encoders of dnerf/network_hyper.py are mirrored")
        self.num_layers_ambient, self.hidden_dim_ambient, self.ambient_dim = num_layers_ambient, hidden_dim_ambient, ambient_dim
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim
        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color

        # ambient: freq(t, 6) -> 4 x 128 -> ambient_dim                                 (network_hyper.py:31-51)
        self.encoder_time = FreqEncoder(input_dim=1, degree=6)
        self.in_dim_time = self.encoder_time.output_dim
        self.ambient_net = _mlp([self.in_dim_time] + [hidden_dim_ambient] * (num_layers_ambient - 1) + [ambient_dim])

        # sigma: tiled grid over (x, ambient) (16 levels x 2, 16 -> 2048*bound) -> 64 -> 1 + 32       (network_hyper.py:53-73)
        self.encoder = GridEncoder(input_dim=3 + ambient_dim, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                                   desired_resolution=2048 * bound, gridtype="tiled", align_corners=False)
        self.in_dim = self.encoder.output_dim
        self.sigma_net = _mlp([self.in_dim] + [hidden_dim] * (num_layers - 1) + [1 + geo_feat_dim])

        # colour: SH(dir, 4) ++ geo_feat -> 64 -> 64 -> 3                                              (network_hyper.py:75-94)
        self.encoder_dir = SHEncoder(input_dim=3, degree=4)
        self.in_dim_dir = self.encoder_dir.output_dim
        self.color_net = _mlp([self.in_dim_dir + geo_feat_dim] + [hidden_dim_color] * (num_layers_color - 1) + [3])

        # background sphere (bg_radius > 0)                                                            (network_hyper.py:96-118)
        if self.bg_radius > 0:
            self.num_layers_bg, self.hidden_dim_bg = num_layers_bg, hidden_dim_bg
            self.encoder_bg = GridEncoder(input_dim=2, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                                          desired_resolution=2048, gridtype="hash", align_corners=False)
            self.in_dim_bg = self.encoder_bg.output_dim
            self.bg_net = _mlp([self.in_dim_bg + self.in_dim_dir] + [hidden_dim_bg] * (num_layers_bg - 1) + [3])
        else:
            self.bg_net = None

    # ------------------------------------------------------------------------------------------
    def ambient(self, t):
        """t [1,1] -> the ambient coordinate [1, ambient_dim] in [-bound, bound]   (network_hyper.py:126-136)."""
        return torch.tanh(_run_mlp(self.ambient_net, self.encoder_time(t))) * self.bound

    def _sigma(self, x, t):
        x = torch.cat([x, self.ambient(t).repeat(x.shape[0], 1)], dim=1)
        h = _run_mlp(self.sigma_net, self.encoder(x, bound=self.bound))
        return trunc_exp(h[..., 0]), h[..., 1:]

    def _color(self, d, geo_feat):
        return torch.sigmoid(_run_mlp(self.color_net, torch.cat([self.encoder_dir(d), geo_feat], dim=-1)))

    # -- fused inference dispatch -----------------------------------------------------------------
    fused_inference = True       # class default; set False on a model to keep `forward` on the op-by-op path in every mode

    def _fused_inference_ok(self, x, d):
        if not self.fused_inference or self.training or torch.is_grad_enabled() or not x.is_cuda or x.dim() != 2 or x.shape[0] == 0:
            return False
        if x.dtype != torch.float32 or d.dtype != torch.float32:
            return False
        if not torch.is_autocast_enabled("cuda") or torch.get_autocast_dtype("cuda") != torch.float16:
            return False       # without -O the model stays op by op: there is no fused fp32 configuration of it
        ok = self.__dict__.get("_fused_arch_ok")
        if ok is None:         # the architecture does not change after construction
            from . import fused_hyper
            ok = bool(fused_hyper.available() and fused_hyper.shapes_ok(self))
            self.__dict__["_fused_arch_ok"] = ok
        return ok

    def _parameter_epoch(self):
        ps = self.__dict__.get("_fused_params")
        if ps is None:
            ps = tuple([self.encoder.embeddings] + [l.weight for net in (self.ambient_net, self.sigma_net, self.color_net) for l in net])
            self.__dict__["_fused_params"] = ps
        return tuple([(p.data_ptr(), p._version) for p in ps])

    _fused_time_value = _DeformNetwork._fused_time_value

    def _forward_fused(self, x, d, t):
        """The whole network in one launch: sigma [M] f32 (density_scale NOT applied: the caller multiplies), rgb [M,3] (the fp16 values
        of torch.sigmoid on the half logits, held in f32)."""
        epoch = self._parameter_epoch()
        cache = self.__dict__.get("_fused_cache")
        if cache is None or cache[0] != epoch[1:]:
            from . import fused_hyper
            field = fused_hyper.FusedHyperField(self, t, fp16=True)
            field.density_scale = 1.0
            cache = self.__dict__["_fused_cache"] = (epoch[1:], field, epoch[0])
        elif cache[2] != epoch[0]:      # only the embeddings moved
            cache[1].load_table(self.encoder.embeddings.detach())
            cache = self.__dict__["_fused_cache"] = (cache[0], cache[1], epoch[0])
        field = cache[1]
        field.set_time_if_changed(self._fused_time_value(field, t))
        field._buf = None              # fresh output tensors per call: the caller owns them, as on the op-by-op path
        return field(x.contiguous(), d.contiguous())

    def use_native_density_update(self, field=None, fp32=False):
        """Route update_extra_state through the CELLS variant of csrc/field_hyper.hip + csrc/density.hip (`-O` numerics;
        `fused.DensityGridUpdater`).  Opt-in: the op-by-op update stays the default.  The configurations the fused field refuses are
        refused here."""
        from . import fused_hyper
        if self.bg_radius > 0:
            raise NotImplementedError("native density update of the ambient-dimension model: bg_radius > 0 (the background sphere) is "
                                      "not served by the fused hyper field; keep the op-by-op update_extra_state")
        if self.ambient_dim != 1:
            raise NotImplementedError("native density update of the ambient-dimension model: the fused hyper field is built for "
                                      "ambient_dim == 1 (a 4-D grid); keep the op-by-op update_extra_state")
        if not fused_hyper.shapes_ok(self):
            raise NotImplementedError("native density update of the ambient-dimension model: the fused hyper field is built for the "
                                      "default architecture of dnerf/network_hyper.py (sigma net 32-64-33, colour net 48-64-64-3, "
                                      "16 x 2 tiled grid over 4 coordinates); keep the op-by-op update_extra_state")
        return super().use_native_density_update(field, fp32=fp32)

    def forward(self, x, d, t):
        """x [M,3] in [-bound,bound], d [M,3] unit, t [1,1] -> sigma [M], rgb [M,3], None  (network_hyper.py:121-161)."""
        if self._fused_inference_ok(x, d):
            sigma, rgb = self._forward_fused(x, d, t)
            return sigma, rgb, None
        sigma, geo_feat = self._sigma(x, t)
        return sigma, self._color(d, geo_feat), None

    def density(self, x, t):
        """network_hyper.py:163-194."""
        sigma, geo_feat = self._sigma(x, t)
        return {"sigma": sigma, "geo_feat": geo_feat}

    def background(self, x, d):
        """x [N,2] in [-1,1], d [N,3] -> rgb [N,3]   (network_hyper.py:196-211)."""
        h = torch.cat([self.encoder_dir(d), self.encoder_bg(x)], dim=-1)
        return torch.sigmoid(_run_mlp(self.bg_net, h))

    def color(self, x, d, mask=None, geo_feat=None, **kwargs):
        """The masked colour query (network_hyper.py:215-244)."""
        if mask is not None:
            rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            if not mask.any():
                return rgbs
            d, geo_feat = d[mask], geo_feat[mask]
        h = self._color(d, geo_feat)
        if mask is not None:
            rgbs[mask] = h.to(rgbs.dtype)
            return rgbs
        return h

    def get_params(self, lr, lr_net):
        """network_hyper.py:247-261."""
        return [
            {"params": self.encoder.parameters(), "lr": lr},
            {"params": self.sigma_net.parameters(), "lr": lr_net},
            {"params": self.encoder_dir.parameters(), "lr": lr},
            {"params": self.color_net.parameters(), "lr": lr_net},
            {"params": self.encoder_time.parameters(), "lr": lr},
            {"params": self.ambient_net.parameters(), "lr": lr_net},
        ] + ([{"params": self.encoder_bg.parameters(), "lr": lr}, {"params": self.bg_net.parameters(), "lr": lr_net}] if self.bg_radius > 0 else [])
