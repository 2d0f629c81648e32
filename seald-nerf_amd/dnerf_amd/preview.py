"""Native preview frames: the mirror of the reference's `Trainer.test_gui` (SealDNeRF/utils.py:174-240, dnerf/utils.py) and of the
GUI's accumulation over jittered frames (SealDNeRF/gui.py:241-267) on the device-driven loop.

`test_gui` never renders an unperturbed frame: it calls `test_step(..., perturb=spp)` with spp >= 1, so `run_cuda` jitters every ray's
start in iteration 0, and the GUI averages those frames while the camera rests.  It renders at `downscale`, blows the frame up with
`F.interpolate(mode='nearest')`, replaces NaN depths, converts a linear colour space to sRGB and, with `return_pos`, returns the 3D
point under every pixel.  Here the loop is `DeviceLoop.render(perturb / noises)` and everything after it is ONE launch,
`sdn_preview_finish` (csrc/preview.hip).  `accumulate_group` renders several of a resting view's jittered frames in one loop
(`DeviceLoop.render_samples`) and folds them with one launch, `sdn_preview_finish_group`."""
import ctypes

import numpy as np
import torch

from .renderer import DeviceLoop, first_march_noises
from .utils import get_rays


class PreviewRenderer:
    """`frame(...)` is `test_gui`; `accumulate(...)` adds the GUI's running mean, with the buffer on the device.

    model / field: as for `DeviceLoop` (the fused `-O` field or the fp32 one); W, H: the window; mapper: an optional SealD seal mapper
    (bbox, anchor, brush) -- the edit preview; loop_kw: further `DeviceLoop` arguments (T_thresh=1e-4 for the SealD teacher, ...).
    normalize_depth: True = dnerf's run_cuda (clamp(depth - near, 0) / (far - near)), False = the SealD teacher's raw depth."""

    def __init__(self, model, field, W, H, device, mapper=None, normalize_depth=True, **loop_kw):
        if int(loop_kw.get("frames", 1)) != 1:
            raise NotImplementedError("a preview frame is one frame per loop (frames == 1)")
        self.model, self.field, self.W, self.H, self.device = model, field, int(W), int(H), torch.device(device)
        self.mapper, self.normalize_depth, self.loop_kw = mapper, bool(normalize_depth), dict(loop_kw)
        self.loops = {}                       # rH * rW -> DeviceLoop: `downscale` changes rarely
        self.group_loops = {}                 # (rH * rW, samples) -> DeviceLoop(frames=samples): accumulate_group's
        f32 = torch.float32
        self.image = torch.empty(self.H, self.W, 3, dtype=f32, device=self.device)
        self.depth = torch.empty(self.H, self.W, dtype=f32, device=self.device)
        self.pos = None
        self.render_buffer = torch.empty(self.H, self.W, 3, dtype=f32, device=self.device)
        self.spp = 0                          # frames in render_buffer

    def loop_for(self, n_rays):
        loop = self.loops.get(n_rays)
        if loop is None:
            loop = self.loops[n_rays] = DeviceLoop(self.model, self.field, n_rays, self.device, mapper=self.mapper, **self.loop_kw)
        return loop

    def group_loop_for(self, n_rays, samples):
        """The loop of `samples` jittered copies of an n_rays view.  An edit a frame group cannot render (anchor, mapSource, tint, stamp)
        raises `DeviceLoop.set_mapper`'s NotImplementedError here."""
        loop = self.group_loops.get((n_rays, samples))
        if loop is None:
            kw = {k: v for k, v in self.loop_kw.items() if k != "frames"}
            loop = DeviceLoop(self.model, self.field, n_rays * samples, self.device, mapper=self.mapper, frames=samples, **kw)
            self.group_loops[(n_rays, samples)] = loop
        return loop

    def set_mapper(self, mapper):
        self.mapper = mapper
        for loop in self.loops.values():
            loop.set_mapper(mapper)
        for key, loop in list(self.group_loops.items()):
            try:
                loop.set_mapper(mapper)
            except NotImplementedError:       # not an edit for frame groups: accumulate_group raises it when it asks for the loop again
                del self.group_loops[key]

    def _view_rays(self, pose, intrinsics, downscale, return_pos):
        """-> rH, rW and the [rH * rW, 3] rays of the window rendered at `downscale`."""
        H, W = self.H, self.W
        rH, rW = int(H * downscale), int(W * downscale)
        if rH < 1 or rW < 1:
            raise ValueError(f"downscale {downscale} leaves no pixel of a {H} x {W} window")
        if return_pos and (rH != H or rW != W):
            raise ValueError("return_pos needs downscale == 1 (the reference's expression views the rays as [H, W, 3])")
        if isinstance(pose, np.ndarray):
            pose = torch.from_numpy(pose)
        pose = pose.to(self.device, torch.float32).reshape(1, 4, 4)
        intr = [float(v) * downscale for v in intrinsics]
        rays = get_rays(pose, intr, rH, rW, -1)
        return rH, rW, rays["rays_o"][0].contiguous(), rays["rays_d"][0].contiguous()

    @staticmethod
    def _background(bg_color):
        """bg_color (None, a number, one or three components) as three floats."""
        if bg_color is None:
            bg = (1.0, 1.0, 1.0)
        elif torch.is_tensor(bg_color) or isinstance(bg_color, (np.ndarray, list, tuple)):
            vals = [float(v) for v in (bg_color.reshape(-1).tolist() if hasattr(bg_color, "reshape") else bg_color)]
            bg = tuple(vals * 3) if len(vals) == 1 else tuple(vals)
        else:
            bg = (float(bg_color),) * 3
        if len(bg) != 3:
            raise ValueError("bg_color has one or three components")
        return bg

    def _outputs(self, return_pos):
        if return_pos and self.pos is None:
            self.pos = torch.empty(self.H, self.W, 3, dtype=torch.float32, device=self.device)
        out = {"image": self.image, "depth": self.depth}
        if return_pos:
            out["pos"] = self.pos
        return out

    @torch.no_grad()
    def frame(self, pose, intrinsics, time, bg_color=None, spp=1, downscale=1, return_pos=False, color_space="srgb", noises=None,
              _accum=None):
        """pose: [4,4] camera-to-world (numpy or torch); intrinsics: (fx, fy, cx, cy) of the H x W window; time: scalar in [0, 1].
        bg_color: None (white, as both run_cuda's do) or three components; spp truthy jitters the first march (`test_gui` passes it as
        `perturb`); noises: the [rH * rW] offsets to replay instead of drawing them.  color_space 'linear' converts to sRGB as
        `test_gui` does.  -> {'image' [H,W,3], 'depth' [H,W] (, 'pos' [H,W,3])}: device tensors owned by this object, overwritten by
        the next frame."""
        import sdn_backend as B
        H, W = self.H, self.W
        rH, rW, rays_o, rays_d = self._view_rays(pose, intrinsics, downscale, return_pos)
        loop = self.loop_for(rH * rW)
        t = time if torch.is_tensor(time) else torch.tensor([[float(time)]], dtype=torch.float32, device=self.device)
        if noises is None and spp:
            noises = first_march_noises(rH * rW, self.device, True)
        loop.render(rays_o, rays_d, t, want_stats=False, noises=noises, finish=False)
        bg_rays = None
        if getattr(self.model, "bg_radius", -1) > 0:          # the background-sphere model: one colour per ray, takes precedence
            bg_rays = self.model._bg(rays_o, rays_d, None).float().contiguous()
        bg = self._background(bg_color)
        out = self._outputs(return_pos)
        accum, n_acc = (None, 0) if _accum is None else _accum
        B.check(B.lib.sdn_preview_finish(ctypes.byref(loop.ctx), rH, rW, H, W, (ctypes.c_float * 3)(*bg), B.ptr(bg_rays), int(self.normalize_depth),
                                         int(color_space == "linear"), B.ptr(self.image), B.ptr(self.depth),
                                         B.ptr(self.pos) if return_pos else None, B.ptr(accum), int(n_acc), B.stream()), "preview_finish")
        self._refs = (rays_o, rays_d, bg_rays, noises)         # alive while the launch may still read them
        return out

    @torch.no_grad()
    def accumulate(self, pose, intrinsics, time, need_update=False, max_spp=64, **kw):
        """The GUI's loop body: `need_update` (the camera moved, the edit changed) restarts the mean with this frame;
        otherwise render_buffer = (render_buffer * spp + frame) / (spp + 1) until `max_spp` frames are in it.  The jitter's seed is
        the frame count, as the GUI passes it (`spp=self.spp` with spp >= 1).  -> the running mean [H,W,3] (device)."""
        if need_update:
            self.spp = 0
        if self.spp < max_spp:
            kw.setdefault("spp", max(self.spp, 1))
            self.frame(pose, intrinsics, time, _accum=(self.render_buffer, self.spp), **kw)
            self.spp += 1
        return self.render_buffer

    @torch.no_grad()
    def accumulate_group(self, pose, intrinsics, time, need_update=False, max_spp=64, samples=4, noises=None, bg_color=None, spp=1,
                         downscale=1, return_pos=False, color_space="srgb"):
        """`accumulate` for a resting camera, `samples` frames per call: the view's next `samples` jittered frames are rendered by ONE
        loop (`DeviceLoop.render_samples` -- they share camera, time, occupancy slice and cull grid, so the loop's chain of dependent
        launches is paid once) and the first min(samples, max_spp - spp) of them are folded into render_buffer by one launch,
        `sdn_preview_finish_group`, in order and with the roundings of as many `accumulate` calls; spp advances by that count.
        noises: the [samples, rH * rW] fp32 offsets to replay, row f for frame f; None draws them, one `torch.rand(rH * rW)` per frame
        in frame order (the draws `accumulate` makes; `spp` falsy, as in `frame`: no jitter, all offsets 0).  With the same offsets
        render_buffer is bit for bit `accumulate`'s.  `image`,
        `depth` (and `pos`) hold the last folded frame.  `need_update`, `max_spp` and the other arguments are `accumulate`'s /
        `frame`'s.  A bbox or brush edit (without tint or stamp) is previewed; the edits frame groups do not render (anchor,
        mapSource, tint, stamp) raise NotImplementedError: preview those with `accumulate`.  -> the running mean [H,W,3] (device)."""
        import sdn_backend as B
        samples = int(samples)
        if not 2 <= samples <= B.MAX_GROUP_FRAMES:
            raise ValueError(f"samples must be 2..{B.MAX_GROUP_FRAMES} (one frame per loop: accumulate)")
        if need_update:
            self.spp = 0
        n_fold = min(samples, int(max_spp) - self.spp)
        if n_fold <= 0:
            return self.render_buffer
        H, W = self.H, self.W
        rH, rW, rays_o, rays_d = self._view_rays(pose, intrinsics, downscale, return_pos)
        n = rH * rW
        loop = self.group_loop_for(n, samples)
        t = time if torch.is_tensor(time) else torch.tensor([[float(time)]], dtype=torch.float32, device=self.device)
        if noises is None and spp:
            noises = torch.stack([first_march_noises(n, self.device, True) for _ in range(samples)])
        elif noises is None:
            noises = torch.zeros(samples, n, dtype=torch.float32, device=self.device)
        loop.render_samples(rays_o, rays_d, t, noises, want_stats=False, finish=False)
        bg_rays = None
        if getattr(self.model, "bg_radius", -1) > 0:          # one colour per ray of the view, the same for every sample of it
            bg_rays = self.model._bg(rays_o, rays_d, None).float().repeat(samples, 1).contiguous()
        bg = self._background(bg_color)
        self._outputs(return_pos)
        B.check(B.lib.sdn_preview_finish_group(ctypes.byref(loop.ctx), rH, rW, H, W, (ctypes.c_float * 3)(*bg), B.ptr(bg_rays),
                                               int(self.normalize_depth), int(color_space == "linear"), B.ptr(self.image), B.ptr(self.depth),
                                               B.ptr(self.pos) if return_pos else None, B.ptr(self.render_buffer), int(self.spp), int(n_fold),
                                               B.stream()), "preview_finish_group")
        self._refs = (rays_o, rays_d, bg_rays, noises)         # alive while the launch may still read them
        self.spp += n_fold
        return self.render_buffer
