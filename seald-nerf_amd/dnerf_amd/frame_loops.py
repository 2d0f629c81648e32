"""MI355X-native frame drivers of the dynamic-NeRF path: the host side of csrc/render.hip and csrc/seal.hip.

Four drivers over the same operators and the same schedule (dnerf/renderer.py:333-381: n_step = clamp(N // n_alive, 1, 8), stop at
max_steps), each producing the frame `NeRFRenderer.run_cuda` produces:
  * `render_frame` (+ `FrameWorkspace`)   the loop in Python, one 4-byte read-back per iteration; any field, fused or op by op
  * `DeviceLoop`                          the device-driven loop (`sdn_render_frame_f16`): no host round trip inside an iteration
  * `PipelinedDeviceLoop`                 a stream of frames through several `DeviceLoop` contexts on their own HIP streams
  * `RayBatchRenderer` (+ `loop_schedule`) a small ray batch in one pass, without the iteration loop
The host steps they share -- buffer sizes, ray flattening, per-frame times, raw event handles, the frame finish -- are written once,
at the top.  `dnerf_amd.renderer` re-exports every public name of this module.
"""
import ctypes
import os
import sys
from time import perf_counter
from types import SimpleNamespace

import numpy as np
import torch

import raymarching
import sdn_backend
from sdn_backend import lib, check, ptr, stream
from .dist import InOrderHandOn


# ==================================================================================================
# host steps shared by the drivers
# ==================================================================================================
def sample_capacity(N):
    """Sample slots of a loop over N rays: >= n_alive * n_step + align for every schedule (n_alive * n_step <= N)."""
    return N + 128 + 8 * 128


def flat_rays(rays):
    """Rays of any prefix shape as one contiguous [N,3] tensor."""
    return rays.contiguous().view(-1, 3)


def per_frame_times(time, n, mismatch, spread_single=False):
    """`time` as a list of n entries: a list / tuple is one entry per frame, anything else stands for all n; `spread_single` lets a
    list of one do so too.  `mismatch`: the ValueError text for another length, formatted with `n` and `got`."""
    times = list(time) if isinstance(time, (list, tuple)) else [time] * n
    if spread_single and len(times) == 1:
        times = times * n
    if len(times) != n:
        raise ValueError(mismatch.format(n=n, got=len(times)))
    return times


def event_handles(events):
    """ctypes array of the raw `hipEvent_t` of torch events.  Torch creates the handle at the first record: each event is recorded once
    on the current stream here; the native call that is handed the array re-records it in place."""
    cur = torch.cuda.current_stream()
    for e in events:
        e.record(cur)
    return (ctypes.c_void_p * len(events))(*[e.cuda_event for e in events])


def sphere_background(model, rays_o, rays_d):
    """Colours [N,3] of the background-sphere model the rays end on (dnerf/renderer.py:277-279); None for a model without one."""
    return model._bg(rays_o, rays_d, None).float() if getattr(model, "bg_radius", -1) > 0 else None


def finish_frame(image, weights_sum, bg, depth=None, nears=None, fars=None, out=(None, None), fused=False):
    """The reference's frame finish (dnerf/renderer.py:378-379): image + (1 - weights_sum) * bg and, given `depth`, the clamped depth
    normalised to [near, far] -> (image, depth), written into the tensors `out` where given.  `fused`: the background mix in one
    multiply-add as the native finish kernel rounds it (bg a number or a tensor); otherwise the reference's two roundings."""
    mix = (1 - weights_sum).unsqueeze(-1)
    if fused:
        image = torch.addcmul(image, mix, bg if isinstance(bg, torch.Tensor) else torch.full((1, 3), float(bg), device=image.device), out=out[0])
    else:
        image = torch.add(image, mix * bg, out=out[0])
    if depth is not None:
        depth = torch.div(torch.clamp(depth - nears, min=0), fars - nears, out=out[1])
    return image, depth


# ==================================================================================================
# the loop in Python
# ==================================================================================================
class FrameWorkspace:
    """Per-(N) buffers of the native loop, allocated once and reused across frames: the reference
    re-allocates and memsets three M-sized sample buffers every iteration."""

    def __init__(self, N, device):
        self.N = N
        f32, i32 = torch.float32, torch.int32
        M = sample_capacity(N)
        self.xyzs = torch.empty(M, 3, dtype=f32, device=device)
        self.dirs = torch.empty(M, 3, dtype=f32, device=device)
        self.deltas = torch.empty(M, 2, dtype=f32, device=device)
        self.alive = [torch.empty(N, dtype=i32, device=device), torch.empty(N, dtype=i32, device=device)]
        self.rays_t = torch.empty(N, dtype=f32, device=device)
        self.weights_sum = torch.empty(N, dtype=f32, device=device)
        self.depth = torch.empty(N, dtype=f32, device=device)
        self.image = torch.empty(N, 3, dtype=f32, device=device)
        self.count = torch.zeros(1, dtype=i32, device=device)
        self.count_host = torch.zeros(1, dtype=i32).pin_memory()
        self.scratch = torch.empty(max(int(lib.sdn_compact_alive_scratch_bytes(N)), 4), dtype=torch.uint8, device=device)
        self.cull = torch.empty(int(lib.sdn_cull_grid_bytes()), dtype=torch.uint8, device=device)
        self.live_idx = torch.empty(M, dtype=i32, device=device)          # slots that received a sample, per iteration
        self.live_counts = torch.zeros(1024 + 8, dtype=i32, device=device)  # one counter per loop iteration (<= max_steps)


def first_march_noises(N, device, perturb=False, noises=None):
    """The per-ray offsets in [0, 1) of a perturbed first march, or None.  `noises`: an [N] fp32 device tensor, used as it is (what
    a recorded frame is replayed with).  Otherwise `perturb` truthy draws `torch.rand(N)` on the device -- the draw
    `raymarching.march_rays(perturb=True)` makes for iteration 0 of the reference-shaped loop, first in the generator's order, so
    that after `torch.manual_seed(s)` the op-by-op path and the native loops jitter every ray alike."""
    if noises is None:
        return torch.rand(N, dtype=torch.float32, device=device) if perturb else None
    if noises.dtype != torch.float32 or noises.numel() != N:
        raise ValueError(f"noises must be {N} fp32 offsets, one per ray (got {tuple(noises.shape)} {noises.dtype})")
    return noises.to(device).contiguous().view(-1)


@torch.no_grad()
def render_frame(model, rays_o, rays_d, time, fp16=False, dt_gamma=0.0, max_steps=1024, T_thresh=1e-2, bg_color=1.0,
                 workspace=None, field=None, count_samples=True, use_cull=True, mapper=None, perturb=False, noises=None):
    """One inference frame: rays [N,3] -> {'image' [N,3], 'depth' [N], 'weights_sum' [N], 'n_samples', 'trace'}.

    Same schedule as dnerf/renderer.py:340-381 (n_step = clamp(N // n_alive, 1, 8), stop at max_steps),
    same operators, but: buffers come from a reusable workspace, alive-ray compaction is the device-side
    `compact_alive` (one 4-byte count read back per iteration instead of a boolean-mask select), and the
    field network may be the fused MFMA kernel (`field`, see dnerf_amd/fused.py) instead of the op-by-op
    network.  `trace` lists (n_alive, n_step, padded_points) per iteration.

    With the fused field the marcher also appends the slots that received a sample to a compact list and the network is
    evaluated on those only (the reference evaluates every padded slot, including the ~94 % empty ones of the first
    iteration); rays whose remaining segment provably cannot produce a sample are retired by the marcher's exact
    cull-grid test instead of stepping through the empty volume voxel by voxel.

    `mapper`: an optional SealD seal mapper (`dnerf_amd.seal_mapper`), hooked exactly where `SealDNeRF/renderer.py:245-267` hooks
    it -- sample positions / directions are mapped back to their origin before the field is evaluated, colours of the mapped
    samples are re-mapped after it -- so an edited scene renders through the fused field as well.

    `perturb` / `noises`: the reference's preview (`run_cuda(perturb=True)`) -- the march of iteration 0 starts every ray at
    near + step * noise (see `first_march_noises`); later iterations are not perturbed.
    """
    device = rays_o.device
    rays_o, rays_d = flat_rays(rays_o), flat_rays(rays_d)
    N = rays_o.shape[0]
    noises = first_march_noises(N, device, perturb, noises)
    ws = workspace if workspace is not None and workspace.N == N else FrameWorkspace(N, device)
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, model.aabb_infer, model.min_near)
    bitfield = model.density_bitfield[model.time_slice(time)]
    ws.weights_sum.zero_(); ws.depth.zero_(); ws.image.zero_()
    ws.rays_t.copy_(nears)
    torch.arange(N, dtype=torch.int32, device=device, out=ws.alive[0])
    cur = 0
    n_alive = N
    step = 0
    trace = []
    use_list = field is not None
    n_samples = torch.zeros((), dtype=torch.int64, device=device) if (count_samples and not use_list) else None
    st = stream()
    evaluate = field if field is not None else _field_eval(model, time, fp16)
    cull = None
    if use_cull and model.grid_size == 128 and model.cascade == 1:
        check(lib.sdn_build_cull_grid(ptr(bitfield), 128, ptr(ws.cull), st), "build_cull_grid")
        cull = ptr(ws.cull)
    if use_list:
        ws.live_counts.zero_()
    it = 0
    while step < max_steps and n_alive > 0:
        n_step = max(min(N // n_alive, 8), 1)
        M0 = n_alive * n_step
        M = M0 + (128 - M0 % 128)
        xyzs, dirs, deltas = ws.xyzs[:M], ws.dirs[:M], ws.deltas[:M]
        alive = ws.alive[cur]
        live_count = ws.live_counts[it:it + 1] if use_list else None
        check(lib.sdn_march_rays_ex(n_alive, n_step, ptr(alive), ptr(ws.rays_t), ptr(rays_o), ptr(rays_d), float(model.bound),
                                    float(dt_gamma), int(max_steps), int(model.cascade), int(model.grid_size), ptr(bitfield), ptr(fars),
                                    ptr(xyzs), ptr(dirs), ptr(deltas), ptr(noises) if it == 0 else None, M, cull,
                                    ptr(ws.live_idx) if use_list else None, ptr(live_count), st), "march_rays_ex")   # (iteration 0 walks arange(N): list position == ray)
        if n_samples is not None:  # ops path: live samples = slots with a non-zero step (bookkeeping, off in the timed loop)
            n_samples += (deltas[:M0, 0] > 0).sum()
        q_xyzs, q_dirs, mapped = xyzs, dirs, None
        native_map = mapper is not None and hasattr(mapper, "map_to_origin_") and mapper._native_ok(xyzs, dirs)
        if native_map:      # in place on the sample buffers (the marcher rewrites them every iteration)
            mapper.map_data_conversion(xyzs)
            mapped = mapper.map_to_origin_(xyzs, dirs)
        elif mapper is not None:
            q_xyzs, q_dirs, mapped = mapper.map_to_origin(xyzs, dirs)
            q_xyzs, q_dirs = q_xyzs.contiguous(), q_dirs.contiguous()
        if use_list:
            sigmas, rgbs = evaluate(q_xyzs, q_dirs, ws.live_idx, live_count)
        else:
            sigmas, rgbs = evaluate(q_xyzs, q_dirs)
        if native_map:
            mapper.map_color_(rgbs, mapped, points=xyzs)      # (xyzs were mapped in place: the reference's `mapped_xyzs`, what a texture stamp looks up)
        elif mapped is not None and bool(mapped.any()):
            rgbs[mapped] = mapper.map_color(q_xyzs[mapped], q_dirs[mapped], rgbs[mapped]).to(rgbs.dtype)
        check(lib.sdn_composite_rays(n_alive, n_step, float(T_thresh), ptr(alive), ptr(ws.rays_t), ptr(sigmas), ptr(rgbs), ptr(deltas),
                                     ptr(ws.weights_sum), ptr(ws.depth), ptr(ws.image), st), "composite_rays")
        check(lib.sdn_compact_alive(ptr(alive), n_alive, ptr(ws.alive[1 - cur]), ptr(ws.count), ptr(ws.scratch), st), "compact_alive")
        ws.count_host.copy_(ws.count, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        trace.append((n_alive, n_step, M))
        n_alive = int(ws.count_host[0])
        cur = 1 - cur
        step += n_step
        it += 1
    sphere = sphere_background(model, rays_o, rays_d)
    image, depth = finish_frame(ws.image, ws.weights_sum, bg_color if sphere is None else sphere, ws.depth, nears, fars)
    if count_samples:
        total = int(ws.live_counts[:it].sum().item()) if use_list else int(n_samples.item())
    else:
        total = None
    return {"image": image, "depth": depth, "weights_sum": ws.weights_sum.clone(), "trace": trace, "nears": nears, "fars": fars,
            "n_samples": total}


def _field_eval(model, time, fp16):
    """Op-by-op field evaluation (the reference's network on the drop-in operators), fp32 outputs."""
    def run(xyzs, dirs):
        keep = model.__dict__.get("fused_inference")
        model.fused_inference = False          # this IS the op-by-op path: never the fused dispatch of NeRFNetwork.forward
        try:
            if fp16:
                with torch.autocast("cuda", dtype=torch.float16):
                    sigmas, rgbs, _ = model(xyzs, dirs, time)
            else:
                sigmas, rgbs, _ = model(xyzs, dirs, time)
        finally:
            if keep is None:
                del model.fused_inference
            else:
                model.fused_inference = keep
        return (model.density_scale * sigmas).float().contiguous(), rgbs.float().contiguous()
    return run


# ==================================================================================================
# device-driven loop (csrc/render.hip): no host round trip inside an iteration
# ==================================================================================================
class DeviceLoop:
    """Owns the buffers and the `SdnRenderCtx` of the device-driven inference loop for frames of N rays.

    The host enqueues iteration k+1 while iteration k runs; grids are sized with the survivor count read back (async,
    pinned memory) one iteration earlier, which is an upper bound of the current one.  Requires the fused field."""

    RING = 4
    MAX_TIMED = 24  # iterations whose fused-field launch can be timed in place (the headline frame has 11 + 1)

    def __init__(self, model, field, N, device, max_steps=1024, T_thresh=1e-2, dt_gamma=0.0, mailbox=True, mapper=None, frames=1,
                 keep_cull_grids=False):
        """frames > 1: a FRAME GROUP -- the N rays are `frames` equal, frame-major blocks (the shards of consecutive frames of a camera
        path / of successive time steps) rendered together by one loop, each at its own time (`bind(..., time=[t_0, ..., t_F-1])`):
        the chain of ~30 dependent launches of a loop is paid once per group instead of once per frame.  Per-ray results do not
        depend on which rays share a loop, so every frame of the group is bit-identical to the frame rendered alone."""
        f32, i32 = torch.float32, torch.int32
        self.model, self.field, self.N = model, field, N
        self.frames = int(frames)
        self.keep_cull_grids = bool(keep_cull_grids)
        if not 1 <= self.frames <= sdn_backend.MAX_GROUP_FRAMES or N % self.frames:
            raise ValueError(f"a frame group holds 1..{sdn_backend.MAX_GROUP_FRAMES} frames of equal ray count (N = {N}, frames = {frames})")
        M = sample_capacity(N)
        n_counters = max_steps + 8
        z = lambda *shape, dt=f32: torch.empty(*shape, dtype=dt, device=device)  # noqa: E731
        self.buf = dict(alive_a=z(N, dt=i32), alive_b=z(N, dt=i32), rays_t=z(N), weights_sum=z(N), depth=z(N), image=z(N, 3),
                        xyzs=z(M, 3), dirs=z(M, 3), deltas=z(M, 2), sigmas=z(M), rgbs=z(M, 3), live_idx=z(M, dt=i32),
                        live_counts=torch.zeros(n_counters, dtype=i32, device=device), state=torch.zeros(16, dtype=i32, device=device),
                        trace=torch.zeros(2 * n_counters + 16, dtype=i32, device=device), n_out=torch.zeros(1, dtype=i32, device=device),
                        block_totals=z((N + 255) // 256 + 1, dt=i32), nears=z(N), fars=z(N), rays_tend=z(N),
                        cull_bits=torch.empty(self.frames * int(lib.sdn_cull_grid_bytes()), dtype=torch.uint8, device=device))
        if self.frames > 1:
            self.buf["slot_frame"] = torch.zeros(M, dtype=torch.uint8, device=device)
        self.image_out, self.depth_out = z(N, 3), z(N)
        self.snap = self.buf["trace"][2 * n_counters: 2 * n_counters + 8].view(4, 2)  # device ring written by the advance
        # mailbox=True: coherent mapped host memory the loop kernels publish each iteration's survivor count into (the driver polls
        # it); False: ordinary pinned memory, which selects the driver's event + side-stream copy read-back
        self.host_state = sdn_backend.HostMailbox(1) if mailbox else torch.zeros(self.RING, 2, dtype=i32).pin_memory()
        self.events = [torch.cuda.Event() for _ in range(self.RING)]
        self.copy_events = [torch.cuda.Event() for _ in range(self.RING)]
        self.side = torch.cuda.Stream(device=device)
        self._handles = None
        self._timing_queue = []
        self._sample_rays = None              # render_samples: the one view's rays, replicated per sample
        c = sdn_backend.SdnRenderCtx()
        for k, v in self.buf.items():
            setattr(c, k, v.data_ptr())
        c.field_weights, c.field_bias0, c.grid_table = field.weights.data_ptr(), field.bias0.data_ptr(), field.table.data_ptr()
        c.grid_offsets = (ctypes.c_int32 * 17)(*[int(v) for v in field.offsets_host])
        c.grid_S, c.grid_H = field.S, field.H
        c.N, c.M_cap, c.n_counters, c.max_steps, c.C, c.H = N, M, n_counters, int(max_steps), int(model.cascade), int(model.grid_size)
        c.bound, c.dt_gamma, c.T_thresh, c.density_scale = float(model.bound), float(dt_gamma), float(T_thresh), float(model.density_scale)
        c.n_group_frames, c.rays_per_frame = (self.frames, N // self.frames) if self.frames > 1 else (0, 0)
        # the fp32 fused field (dnerf_amd.fused_f32.FusedFieldF32: the reference without -O) in the same loop: its packed floats, the
        # model's fp32 table in place, the reference's offsets
        c.field_f32 = field.ctx_kind
        self.ctx = c
        self.max_steps = int(max_steps)
        self.set_mapper(mapper)

    def set_mapper(self, mapper):
        """Hooks a SealD seal mapper (`dnerf_amd.seal_mapper.SealBBoxMapper` / `SealAnchorMapper` / `SealBrushMapper`, or None) into every iteration of the
        native loop: samples are mapped back to their origin before the field kernel, colours of the mapped samples re-mapped after it."""
        c = self.ctx
        self.mapper = mapper
        if mapper is None:
            c.seal, c.seal_mask, c.seal_brush, self._seal = None, None, None, None
            return
        dev = self.buf["xyzs"].device
        mapper.map_data_conversion(self.buf["xyzs"])
        a = mapper._native_args(dev)
        kind = getattr(sdn_backend, mapper.native_kind)
        if self.frames > 1 and (kind == sdn_backend.SEAL_ANCHOR or mapper.redirects_source or "rgb" in mapper.map_data or "image" in mapper.map_data):
            # these look at ALL samples of a loop iteration (the mean brightness of the masked ones -- the tint's and the texture stamp's --,
            # "does the call map anything" of mapSource and of the anchor mapper): in a frame group an iteration holds several frames'
            # samples, which the reference never mixes (the brush maps every sample on its own: without a tint or a stamp it runs on frame groups)
            raise NotImplementedError("mapSource / rgb tint / texture stamp / the anchor mapper depend on the set of samples of an iteration: "
                                      "render such edits one frame per loop")
        box = mapper._native_box_record(a)             # (`a`, which the records point into, is kept alive below)
        rec = mapper._native_brush_record(a)
        # the record's scratch bytes (modify_rgb's sum / count, the mapSource / anchor flag word, the texture stamp's sum / count in
        # [32..47]) belong to THIS loop, zeroed once: the loops of a PipelinedDeviceLoop share the mapper and run on their own streams, and
        # one buffer between them would let one loop's memset / sums land in another's mean brightness, and a later loop's mapSource tag
        # cancel an earlier one's redirect
        scratch = torch.zeros(48, dtype=torch.uint8, device=dev)
        box.scratch = scratch.data_ptr()
        mask = torch.empty(self.buf["sigmas"].shape[0], dtype=torch.uint8, device=dev)
        self._seal = (box, mask, a, scratch, rec)      # keep the records, the mask, the triangle / border tensors and the scratch alive
        c.seal, c.seal_mask = ctypes.addressof(box), mask.data_ptr()
        c.seal_brush = ctypes.addressof(rec) if rec is not None else None

    def prepare_timing(self, frames):
        """Pre-creates (outside any timed region) the HIP event pairs for `frames` timed renders: MAX_TIMED pairs per frame,
        recorded by the native loop around each fused-field launch."""
        self._timing_queue = []
        for _ in range(frames):
            recs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), 0) for _ in range(self.MAX_TIMED)]
            self._timing_queue.append((event_handles([ev for r in recs for ev in r[:2]]), recs))
        torch.cuda.synchronize()

    def frame_time(self, time):
        """`SdnFrameTime` record (+ the tensors it points into) for `time`: one time stamp, or -- for a frame group -- one per
        frame.  Everything is derived from the VALUE of the time stamp(s): the occupancy slice (dnerf/renderer.py:285), the
        time-encoding bias of the first deform layer and the canonical-frame rule t == 0 (dnerf/network.py:130-141)."""
        model = self.model
        times = per_frame_times(time, self.frames, "{n} frame(s) in this loop, {got} time stamp(s) given", spread_single=True)
        bias, mask, slices = self.field.group_constants(times)
        ft = sdn_backend.SdnFrameTime()
        bits = [model.density_bitfield[s_] for s_ in slices]          # views (no host sync: python int index)
        for f, b_ in enumerate(bits):
            ft.bitfield[f] = b_.data_ptr()
        ft.field_bias0, ft.zero_deform = bias.data_ptr(), mask
        culls = None
        if self.keep_cull_grids and int(model.grid_size) == 128 and int(model.cascade) == 1:
            culls = [self._cull_grid(s_) for s_ in slices]
            for f, g_ in enumerate(culls):
                ft.cull_grid[f] = g_.data_ptr()
        return ft, (bias, bits, culls)

    def _cull_grid(self, t_idx):
        """The marcher's coarse skip grid of one occupancy slice (`sdn_build_cull_grid`), kept until the density grid is updated
        (`model.iter_density` counts the updates) or `invalidate_cull_grids()` is called: a slice is rendered many times in between,
        and deriving its cull grid again is two launches at the head of every frame's latency chain (eight grids per frame group)."""
        # The kept grid carries the slice's occupancy bits themselves (the packed fine-bit image the marchers copy to LDS), so a stale
        # entry means marching on stale OCCUPANCY: the epoch includes the bitfield's version counter -- load_state_dict, fill_bitfield
        # and a direct `raymarching.packbits` into a slice rewrite the bitfield in place without a new iter_density -- and the cache
        # lives ON the model object (an id()-keyed table would hand a new model the entry of a collected one whose id Python reused).
        cache = self.model.__dict__.get("_sdn_cull_cache")
        if cache is None:
            cache = {"epoch": None, "grids": {}}
            self.model.__dict__["_sdn_cull_cache"] = cache
        bf = self.model.density_bitfield
        epoch = (self.model.iter_density, bf.data_ptr(), bf._version)
        if cache["epoch"] != epoch:
            cache["epoch"], cache["grids"] = epoch, {}
        hit = cache["grids"].get(t_idx)
        if hit is None:
            hit = torch.empty(int(lib.sdn_cull_grid_bytes()), dtype=torch.uint8, device=bf.device)
            check(lib.sdn_build_cull_grid(bf[t_idx].data_ptr(), 128, hit.data_ptr(), stream()), "build_cull_grid")
            cache["grids"][t_idx] = hit
        return hit

    @staticmethod
    def invalidate_cull_grids(model=None):
        """Forget the kept cull grids of `model`: only needed after writing `density_bitfield` behind torch's back (a raw pointer, DLPack,
        a custom kernel of the caller's) without moving its version counter (`torch.autograd.graph.increment_version`).  Torch-level
        writes (`fill_bitfield`, `load_state_dict`, `copy_`) move it by themselves, and this package's kernel writers (`packbits` with a
        bitfield, which `update_extra_state` calls; the native density update) move it after their launch: all of those are seen."""
        if model is not None:
            model.__dict__.pop("_sdn_cull_cache", None)

    def bind(self, rays_o, rays_d, time):
        """Points the context at this frame's rays and time constants (the native driver launches near_far_from_aabb itself)."""
        c, model = self.ctx, self.model
        rays_o, rays_d = flat_rays(rays_o), flat_rays(rays_d)
        assert rays_o.shape[0] == self.N
        nears, fars = self.buf["nears"], self.buf["fars"]  # filled by the native driver (ctx.aabb / ctx.min_near)
        c.aabb, c.min_near = ptr(model.aabb_infer, torch.float32, "aabb_infer"), float(model.min_near)
        ft, refs = self.frame_time(time)
        c.rays_o, c.rays_d = ptr(rays_o, torch.float32, "rays_o"), ptr(rays_d, torch.float32, "rays_d")
        c.bitfield, c.field_bias0, c.zero_deform = ft.bitfield[0], ft.field_bias0, int(ft.zero_deform)
        for f in range(self.frames):
            c.frame_bitfield[f] = ft.bitfield[f]
            c.frame_cull[f] = ft.cull_grid[f]
        self._frame_refs = (rays_o, rays_d, nears, fars, refs)  # keep the tensors alive while the frame is in flight
        if self._handles is None:  # raw hipEvent_t handles, once
            self._ev_main, self._ev_copy = event_handles(self.events), event_handles(self.copy_events)
            self._iters = ctypes.c_uint32(0)
            self._handles = True
        return nears, fars

    def collect(self, nears, fars, want_stats):
        out = {"image": self.image_out, "depth": self.depth_out, "weights_sum": self.buf["weights_sum"], "nears": nears, "fars": fars}
        if want_stats:
            iters = int(self.buf["state"][sdn_backend.LOOP_ITERATION].item())
            tr = self.buf["trace"][: 2 * iters].cpu().view(-1, 2).tolist()
            out["trace"] = [(a, s, a * s + (128 - (a * s) % 128)) for a, s in tr]
            out["n_samples"] = int(self.buf["live_counts"][:iters].sum().item())
        return out

    @torch.no_grad()
    def render(self, rays_o, rays_d, time, bg_color=1.0, want_stats=True, perturb=False, noises=None, finish=True):
        """`perturb` / `noises` (see `first_march_noises`): the first march of the reference's preview -- every ray starts iteration 0 at
        near + step * noises[ray]; with the culled start the jump is certified from that start.  `finish=False` runs the loop alone:
        the caller finishes the frame from the context's accumulators (`sdn_preview_finish`), `image_out` / `depth_out` are not written."""
        if (perturb or noises is not None) and self.frames > 1:
            raise NotImplementedError("a perturbed first march is built for one frame per loop (frames == 1)")
        nears, fars = self.bind(rays_o, rays_d, time)
        noises = first_march_noises(self.N, self.buf["rays_t"].device, perturb, noises)
        return self._run(nears, fars, noises, bg_color, want_stats, finish)

    @torch.no_grad()
    def render_samples(self, rays_o, rays_d, time, noises, bg_color=1.0, want_stats=True, finish=False):
        """F jittered samples of ONE frame in one loop, on a loop built with `frames = F` (N = F * n): what a resting preview
        accumulates.  rays_o / rays_d: the view's [n, 3] rays; time: its one time stamp; noises: [F, n] fp32 offsets in [0, 1), row f
        the first-march jitter of sample f (see `first_march_noises`).  The rays are replicated into buffers the loop owns, the time
        stamp is bound to all F frames and the loop runs once: the samples share the chain of dependent launches, and block f of
        every per-ray result (`buf['image']`, `buf['depth']`, `buf['weights_sum']`, frame-major) is bit for bit what
        `DeviceLoop(frames=1).render(noises=noises[f])` leaves.  `finish=False` (the default here) leaves the frames to the caller --
        `sdn_preview_finish_group` folds them into a running mean --, True writes `image_out` / `depth_out` for all F * n rays.
        Trace and sample count are the group's, not a frame's (see `__init__`)."""
        F = self.frames
        if F < 2:
            raise ValueError("render_samples needs a loop built with frames = F >= 2 (one frame per loop: render(noises=...))")
        if isinstance(time, (list, tuple)):
            raise ValueError("render_samples renders one frame: one time stamp")
        n = self.N // F
        rays_o, rays_d = flat_rays(rays_o), flat_rays(rays_d)
        if rays_o.shape[0] != n or rays_d.shape[0] != n:
            raise ValueError(f"this loop holds {F} samples of {n} rays, got {rays_o.shape[0]} rays")
        if not torch.is_tensor(noises) or noises.dtype != torch.float32 or tuple(noises.shape) != (F, n):
            got = (tuple(noises.shape), noises.dtype) if torch.is_tensor(noises) else type(noises).__name__
            raise ValueError(f"noises must be [{F}, {n}] fp32 offsets, one row per sample (got {got})")
        device = self.buf["rays_t"].device
        if self._sample_rays is None:
            self._sample_rays = (torch.empty(F, n, 3, dtype=torch.float32, device=device), torch.empty(F, n, 3, dtype=torch.float32, device=device))
        self._sample_rays[0].copy_(rays_o.unsqueeze(0).expand(F, n, 3))
        self._sample_rays[1].copy_(rays_d.unsqueeze(0).expand(F, n, 3))
        nears, fars = self.bind(self._sample_rays[0], self._sample_rays[1], time)
        return self._run(nears, fars, first_march_noises(self.N, device, noises=noises), bg_color, want_stats, finish)

    def _run(self, nears, fars, noises, bg_color, want_stats, finish):
        """The bound frame (group) through the native whole-frame driver, with `noises` (one per ray of the loop, or None)."""
        self.ctx.noises = ptr(noises, torch.float32, "noises")
        self._frame_refs += (noises,)
        bg_model = getattr(self.model, "bg_radius", -1) > 0 and finish
        if bg_model:         # the background-sphere colours are mixed in after the loop (the native finish takes one scalar colour)
            bg_color = 0.0
        cur = torch.cuda.current_stream()
        ev_field, n_ev, recs = None, 0, None
        if sdn_backend.timers is not None and self._timing_queue:  # bench: time the fused-field launches in place
            ev_field, recs = self._timing_queue.pop()
            n_ev = self.MAX_TIMED
        self.side.wait_stream(cur)
        check(lib.sdn_render_frame_f16(ctypes.byref(self.ctx), float(bg_color), ptr(self.image_out) if finish else None,
                                       ptr(self.depth_out) if finish else None, stream(),
                                       self.side.cuda_stream, self._ev_main, self._ev_copy, self.host_state.data_ptr(), ev_field, n_ev,
                                       ctypes.byref(self._iters)), "render_frame_f16")
        if recs is not None:  # keep the pairs of the iterations that ran
            sdn_backend.timers.records.setdefault("field_forward_f16", []).extend(recs[: min(n_ev, int(self._iters.value))])
        if bg_model:
            ro, rd = self._frame_refs[0], self._frame_refs[1]
            finish_frame(self.image_out, self.buf["weights_sum"], sphere_background(self.model, ro, rd), out=(self.image_out, None))
        return self.collect(nears, fars, want_stats)


def _context_streams(k, device):
    """One HIP stream per loop context, created here with `hipStreamCreateWithPriority` rather than taken from torch's pool: which
    hardware queue a pool stream lands on depends on how many of the pool's streams the process has touched before, and a context
    that shares its queue with another stream loses its overlap (measured, 4 contexts: 0.437 ms per frame with 5-6 hardware queues,
    0.52 with 7, 8 or 16, 0.49 with 3-4 from the pool; own streams: 0.435-0.439 for 5..9 queues -- profiles/r03_hw_queues.txt).  The
    process still needs GPU_MAX_HW_QUEUES >= contexts + 1 (set before the HIP runtime starts; bench.py does).
    SDN_CTX_PRIORITIES="p0,p1,..." (HIP priorities, -1 high / 0 normal / 1 low, used in turn; measured: no effect);
    SDN_CTX_STREAMS=torch falls back to the pool.
    One set of streams per (device, k, priorities) is created and REUSED by every later loop object of the process: raw HIP streams are
    never destroyed by torch's ExternalStream wrapper, and each leaked set would shift the queue assignment of the next -- the very
    sensitivity this function removes.  (Under rocprofv3 the profiler's preloaded library starts the HIP runtime before bench.py can set
    GPU_MAX_HW_QUEUES: export it in the environment of such a run.)"""
    if os.environ.get("SDN_CTX_STREAMS", "") == "torch":
        return [torch.cuda.Stream(device=device) for _ in range(k)]
    spec = os.environ.get("SDN_CTX_PRIORITIES", "").strip() or "0"
    try:
        prios = [int(x) for x in spec.split(",")]
    except ValueError:
        raise ValueError(f"SDN_CTX_PRIORITIES={spec!r}: expected comma-separated integers (HIP stream priorities, e.g. '-1,0,0,0')") from None
    if any(p < -1 or p > 1 for p in prios):
        raise ValueError(f"SDN_CTX_PRIORITIES={spec!r}: HIP stream priorities are -1 (high), 0, 1 (low)")
    key = (str(torch.device(device)), int(k), tuple(prios))
    if key in _CONTEXT_STREAMS:
        return _CONTEXT_STREAMS[key]
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        return [torch.cuda.Stream(device=device) for _ in range(k)]
    out = []
    with torch.cuda.device(device):
        for i in range(k):
            h = ctypes.c_void_p()
            rc = hip.hipStreamCreateWithPriority(ctypes.byref(h), ctypes.c_uint(1), ctypes.c_int(prios[i % len(prios)]))   # 1 = hipStreamNonBlocking
            if rc != 0:
                raise RuntimeError(f"hipStreamCreateWithPriority failed ({rc})")
            out.append(torch.cuda.ExternalStream(h.value, device=device))
    _CONTEXT_STREAMS[key] = out
    return out


_CONTEXT_STREAMS = {}


class PipelinedDeviceLoop:
    """A stream of frames (camera path / time steps of one model) through `contexts` `DeviceLoop` contexts used in turn, each on its
    own HIP stream, all driven by one host thread in `sdn_render_frames_pipelined_f16`: the next frame starts as soon as a
    context is free and the newest frame in flight is down to N / overlap_div alive rays (1 = at once), so the latency-bound
    parts of one frame (marching chains, tail iterations, launch gaps) run under the throughput-bound field kernels of another.
    Every frame is the one `DeviceLoop.render` produces, bit for bit; what changes is frames per second."""

    def __init__(self, model, field, N, device, overlap_div=1, contexts=2, mailbox=True, **kw):
        self.N, self.device, self.overlap_div, self.K = N, device, int(overlap_div), int(contexts)
        self.loops = [DeviceLoop(model, field, N, device, mailbox=mailbox, **kw) for _ in range(self.K)]
        self.streams = _context_streams(self.K, device)
        if self.K > 1:
            # several frames in flight: the persistent field launches leave an eighth of the CUs to the other frames' small kernels
            lib.sdn_field_persistent_workgroups(int(torch.cuda.get_device_properties(device).multi_processor_count) * 7 // 8)
        # mailbox=False: ordinary pinned memory -> the driver's event + side-stream copy read-back (see DeviceLoop)
        self.host_state = sdn_backend.HostMailbox(self.K) if mailbox else torch.zeros(self.K, 8, dtype=torch.int32).pin_memory()
        self._ctxs = (ctypes.POINTER(sdn_backend.SdnRenderCtx) * self.K)(*[ctypes.pointer(lp.ctx) for lp in self.loops])
        self._fixed = None

    @torch.no_grad()
    def render_frames(self, rays_o, rays_d, time, bg_color=1.0, outputs=None, timing=None, exclusive=None, on_done=None, perturb=False,
                      noises=None):
        """rays_o / rays_d: lists of [N,3] tensors, one per frame (entries may repeat).  time: ONE time stamp for the whole stream
        (number or the reference's [1,1] tensor), or a list with one entry per frame -- a D-NeRF test set carries its own time for
        every frame (dnerf/utils.py:151-161); with frame-group contexts (`frames=F`) an entry is itself a list of F times.
        outputs: optional list of (image [N,3],
        depth [N]) tensors per frame; by default frame f lands in the output buffers of context f % contexts.  timing: optional list
        (per frame, None allowed) of ctypes arrays of 2 * DeviceLoop.MAX_TIMED hipEvent_t for that frame's field launches.
        exclusive: optional list of bools per frame; a flagged frame is rendered with nothing else in flight.
        on_done: optional callable (frame index, image, depth) run on a helper thread, in frame order, as soon as a frame's last
        kernel has been enqueued -- with torch's current stream (of that thread) already ordered behind the frame -- while later
        frames still render: the hook for the per-frame all-gather of a ray-sharded job.
        Returns the list of (image, depth) per frame and the per-frame iteration counts."""
        t_entry = perf_counter()
        if perturb or noises is not None:
            raise NotImplementedError("a perturbed first march is not built for pipelined frames: render preview frames with DeviceLoop")
        n = len(rays_o)
        assert n == len(rays_d) and n >= 1
        cur = torch.cuda.current_stream()
        ro = [flat_rays(r) for r in rays_o]
        rd = [flat_rays(r) for r in rays_d]
        times = per_frame_times(time, n, "{n} frames, {got} time entries")     # a list is ALWAYS one entry per frame
        a_ft = (sdn_backend.SdnFrameTime * n)()
        ft_refs = []
        for f in range(n):
            a_ft[f], refs = self.loops[0].frame_time(times[f])
            ft_refs.append(refs)
        for s, lp in enumerate(self.loops):
            self.streams[s].wait_stream(cur)
            with torch.cuda.stream(self.streams[s]):
                lp.bind(ro[min(s, n - 1)], rd[min(s, n - 1)], times[min(s, n - 1)])     # aabb, handles; rays and time constants are set per frame
                lp.side.wait_stream(self.streams[s])
        if outputs is None:
            outputs = [(self.loops[f % self.K].image_out, self.loops[f % self.K].depth_out) for f in range(n)]
        vp = ctypes.c_void_p
        if self._fixed is None:
            K = self.K
            self._fixed = dict(streams=(vp * K)(*[s.cuda_stream for s in self.streams]),
                               sides=(vp * K)(*[lp.side.cuda_stream for lp in self.loops]),
                               ev_main=(vp * (4 * K))(*[e.cuda_event for lp in self.loops for e in lp.events]),
                               ev_copy=(vp * (4 * K))(*[e.cuda_event for lp in self.loops for e in lp.copy_events]))
        fx = self._fixed
        a_ro = (vp * n)(*[ptr(t, torch.float32, "rays_o") for t in ro])
        a_rd = (vp * n)(*[ptr(t, torch.float32, "rays_d") for t in rd])
        a_img = (vp * n)(*[ptr(o[0], torch.float32, "image_out") for o in outputs])
        a_dep = (vp * n)(*[ptr(o[1], torch.float32, "depth_out") for o in outputs])
        iters = (ctypes.c_uint32 * n)()
        a_ev, n_ev = None, 0
        if timing is not None:
            a_ev = (vp * n)(*[ctypes.cast(t, vp).value if t is not None else None for t in timing])
            n_ev = DeviceLoop.MAX_TIMED
        a_excl = (ctypes.c_uint8 * n)(*[1 if e else 0 for e in exclusive]) if exclusive is not None else None
        a_done, worker = None, None
        if on_done is not None:
            # (timing-enabled: bench.py reads the device-side span of the renders and of the gathers from them)
            done = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
            a_done = event_handles(done)
            dev_index = self.streams[0].device_index
            self._done_stream = getattr(self, "_done_stream", None) or torch.cuda.Stream()
            side = self._done_stream

            def in_side_stream():                # the helper thread's CUDA context: this device, its own stream
                torch.cuda.set_device(dev_index)
                return torch.cuda.stream(side)
            # loop f is finished once the driver has published its iteration count; its `done` event orders the helper's stream behind it
            worker = InOrderHandOn(n, lambda f: iters[f] != 0, on_done, outputs, before=lambda f: side.wait_event(done[f]),
                                   context=in_side_stream).start()
            self.last_done_events, self.last_hand_on = done, worker
        t_call = perf_counter()
        try:
            check(lib.sdn_render_frames_pipelined_f16(self._ctxs, self.K, n, a_ro, a_rd, a_img, a_dep, float(bg_color), self.overlap_div,
                                                      fx["streams"], fx["sides"], fx["ev_main"], fx["ev_copy"], self.host_state.data_ptr(),
                                                      a_ev, n_ev, a_excl, a_ft, a_done, iters), "render_frames_pipelined_f16")
        except BaseException:
            if worker is not None:
                worker.cancel()
                worker.thread.join()
            raise
        if worker is not None:
            worker.join()
            cur.wait_stream(self._done_stream)
        self._ft_refs = ft_refs    # the per-frame constants stay alive until the next stream of frames
        t_back = perf_counter()
        for s in self.streams:
            cur.wait_stream(s)
        if os.environ.get("SDN_DRIVER_STATS"):
            print(f"[sdn py] entry->call {1e3 * (t_call - t_entry):.2f} ms, driver call {1e3 * (t_back - t_call):.2f} ms, "
                  f"wait_stream {1e3 * (perf_counter() - t_back):.2f} ms", file=sys.stderr)
        return outputs, [int(v) for v in iters]


def loop_schedule(counts, stops, max_steps=1024):
    """The inference loop's schedule (dnerf/renderer.py:340-381) for rays whose samples are known up front: the specification of
    phase B of `sdn_whole_rays_schedule` (csrc/seal.hip), in Python.

    counts[r]: the number of samples of ray r; stops[r]: the index of the sample at which compositing kills it (the first one whose
    transmittance in front is < T_thresh; that sample is still composited), or counts[r] if there is none.  Per iteration the loop
    marches n_step = max(min(N // n_alive, 8), 1) samples of every alive ray -- all of the window that exist, also those behind a kill
    inside it --, and a ray leaves when its stop sample lies in the window (without one: when fewer than n_step samples were left; a
    ray without samples leaves in iteration 0).  It ends after max_steps steps or with no ray alive.

    -> (ids, trace): ids, int32, the iteration of every sample, rays packed one after the other (ray r's samples start at
    sum(counts[:r])), -1 for a sample the loop never marches; trace, the (n_alive, n_step) of every iteration."""
    counts, stops = np.asarray(counts, dtype=np.int64), np.asarray(stops, dtype=np.int64)
    N = counts.shape[0]
    first = np.concatenate([[0], np.cumsum(counts)])
    ids = np.full(int(first[-1]), -1, dtype=np.int32)
    pos, alive = np.zeros(N, dtype=np.int64), np.ones(N, dtype=bool)
    step, trace = 0, []
    while step < max_steps and alive.any():
        n_alive = int(alive.sum())
        n_step = max(min(N // n_alive, 8), 1)
        for r in np.nonzero(alive)[0]:
            ids[first[r] + pos[r]: first[r] + min(pos[r] + n_step, counts[r])] = len(trace)
        dies = alive & (stops < pos + n_step)
        alive &= ~dies
        pos[alive] += n_step
        trace.append((n_alive, n_step))
        step += n_step
    return ids, trace


class RayBatchRenderer:
    """A SMALL ray batch (a training batch's proxy render, SealDNeRF/utils.py:632-656; a preview; an error-map pass) rendered in one
    pass instead of through the iteration loop.

    The inference branch (dnerf/renderer.py:333-381) marches `n_step` samples per alive ray, evaluates, composites, compacts, ~12-16
    times: the point of the loop is to stop marching rays that have terminated, which pays for a frame of 640 000 rays.  For 4 096
    rays it is a chain of ~30 dependent launches of almost no work (0.96 ms on the MI355X).  Here every ray's samples are listed up
    front by the training marcher (same positions and step lengths as the inference marcher, no perturbation), the fused field
    kernel evaluates them in ONE launch (the count is read on the device), and `sdn_composite_whole_rays` composites each ray with
    the inference arithmetic: image and weights_sum are the loop's bit for bit, depth to fp32 rounding.  A seal mapper, if given,
    sits between marcher and field exactly as in the loop.  Cost: the samples behind a ray's termination point are evaluated too.

    The rgb tint (`modify_rgb`) re-centres brightness on the mean of the masked samples of one loop ITERATION.  Which samples share an
    iteration follows from the sample counts, the sigmas and the rule n_step = max(min(N // n_alive, 8), 1) -- colours never decide
    when a ray dies -- so after the field launch `sdn_seal_modify_rgb_whole_rays` replays the loop's schedule on the device
    (`loop_schedule` above states it in Python) and tints every masked sample by the mean of its own iteration: the loop's colours bit
    for bit, six more stream operations, no read-back.  A brush's texture stamp (`imageConfig`) re-centres on the same kind of mean and takes
    the same replay (`sdn_seal_modify_image_whole_rays`).  `mapSource` stays with the loops: its redirect moves samples, so it changes the
    sigmas that decide the schedule that decides which calls redirect.

    `samples_per_ray` sizes the sample buffer (N * samples_per_ray slots); a batch that needs more loses its last rays -- `render(...,
    check=True)` reads the count back and raises, `overflowed()` does the same on demand."""

    def __init__(self, model, field, N, device, max_steps=1024, T_thresh=1e-2, dt_gamma=0.0, mapper=None, samples_per_ray=96):
        sdn_backend.require_device()
        if mapper is not None and mapper.redirects_source:
            # (map_to_origin's early return looks at one loop iteration's samples, and the redirect it gates changes their sigmas, which
            #  decide the iterations: nothing to replay after the fact.  The tint is replayed, see above.  The anchor mapper's early return
            #  is no such case: its box contains its cone, so an iteration without a sample in the box holds no sample to map either)
            raise NotImplementedError("mapSource depends on the loop's iterations: use render_frame / DeviceLoop for such edits")
        tint = mapper is not None and ("rgb" in mapper.map_data or "image" in mapper.map_data)      # (the brush's texture stamp takes a mean per iteration too)
        if tint and int(N) > int(lib.sdn_whole_rays_schedule_max_rays()):
            raise NotImplementedError(f"the rgb tint's / texture stamp's schedule replay holds at most {int(lib.sdn_whole_rays_schedule_max_rays())} rays "
                                      f"(N = {N}): render larger batches with DeviceLoop")
        self.model, self.field, self.N, self.device, self.mapper = model, field, int(N), torch.device(device), mapper
        self.max_steps, self.T_thresh, self.dt_gamma = int(max_steps), float(T_thresh), float(dt_gamma)
        M = self.N * int(samples_per_ray)
        self.M = M + (128 - M % 128)
        f32, dev = torch.float32, self.device
        self.flat = torch.empty(self.M * 8, dtype=f32, device=dev)
        self.xyzs, self.dirs, self.deltas = self.flat[:3 * self.M].view(-1, 3), self.flat[3 * self.M:6 * self.M].view(-1, 3), self.flat[6 * self.M:].view(-1, 2)
        self.rays = torch.empty(self.N, 3, dtype=torch.int32, device=dev)
        self.counter = torch.zeros(2, dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.noises = torch.zeros(self.N, dtype=f32, device=dev)
        self.nears, self.fars = torch.empty(self.N, dtype=f32, device=dev), torch.empty(self.N, dtype=f32, device=dev)
        self.identity = torch.arange(self.M, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(int(lib.sdn_march_rays_train_scratch_bytes(self.N, self.max_steps)), dtype=torch.uint8, device=dev)
        self.weights_sum, self.depth = torch.empty(self.N, dtype=f32, device=dev), torch.empty(self.N, dtype=f32, device=dev)
        self.image = torch.empty(self.N, 3, dtype=f32, device=dev)
        self.image_out, self.depth_out = torch.empty(self.N, 3, dtype=f32, device=dev), torch.empty(self.N, dtype=f32, device=dev)
        self._aabb = model.aabb_infer.detach().to(dev, f32).contiguous()
        self._tint = None
        if tint:
            # the tint's work buffers belong to THIS renderer (as a DeviceLoop owns its 32 bytes): {sum, count} per loop iteration --
            # cleared on the stream by every render --, {stop sample, count} per ray, the iteration of every sample slot, the iteration count
            i32 = torch.int32
            self._tint = SimpleNamespace(rays=self.rays, sigmas=None, deltas=self.deltas, N=self.N, T_thresh=self.T_thresh, max_steps=self.max_steps,
                                         scratch=torch.zeros(16 * (self.max_steps + 8), dtype=torch.uint8, device=dev),
                                         image_scratch=torch.zeros(16 * (self.max_steps + 8), dtype=torch.uint8, device=dev),      # the stamp's own sums
                                         ray_stop=torch.zeros(self.N, 2, dtype=i32, device=dev),
                                         slot_iter=torch.full((self.M,), -1, dtype=i32, device=dev), n_iter=torch.zeros(1, dtype=i32, device=dev))

    @torch.no_grad()
    def render(self, rays_o, rays_d, time, bg_color=1.0, check=False, perturb=False, noises=None):
        if perturb or noises is not None:
            raise NotImplementedError("the one-pass renderer's marcher is unperturbed by design: render preview frames with DeviceLoop")
        m, st, ok = self.model, stream(), sdn_backend.check      # (`check` is this method's own flag)
        ro, rd = flat_rays(rays_o), flat_rays(rays_d)
        if ro.shape[0] != self.N:
            raise ValueError(f"RayBatchRenderer was built for {self.N} rays, got {ro.shape[0]}")
        self.field.set_time(time)                       # time bias, canonical-frame flag, occupancy slice -- by VALUE, cached
        bitfield = m.density_bitfield[self.field.t_idx]
        ok(lib.sdn_near_far_from_aabb(ptr(ro, torch.float32, "rays_o"), ptr(rd, torch.float32, "rays_d"), ptr(self._aabb), self.N,
                                      float(m.min_near), ptr(self.nears), ptr(self.fars), st), "near_far_from_aabb")
        self.flat.zero_()
        self.counter.zero_()
        ok(lib.sdn_march_rays_train(ptr(ro), ptr(rd), ptr(bitfield, torch.uint8, "density_bitfield"), float(m.bound), self.dt_gamma,
                                    self.max_steps, self.N, int(m.cascade), int(m.grid_size), self.M, ptr(self.nears), ptr(self.fars),
                                    ptr(self.xyzs), ptr(self.dirs), ptr(self.deltas), ptr(self.rays), ptr(self.counter),
                                    ptr(self.noises), ptr(self.scratch), st), "march_rays_train")
        torch.clamp(self.counter[:1], max=self.M, out=self.count)
        mask = self.mapper.map_to_origin_(self.xyzs, self.dirs) if self.mapper is not None else None
        sigmas, rgbs = self.field(self.xyzs, self.dirs, live_idx=self.identity, live_count=self.count)
        if self._tint is not None:
            self._tint.sigmas = sigmas
            self.mapper.map_color_(rgbs, mask, whole_rays=self._tint, points=self.xyzs)
        elif mask is not None:
            self.mapper.map_color_(rgbs, mask, points=self.xyzs)
        ok(lib.sdn_composite_whole_rays(ptr(sigmas), ptr(rgbs), ptr(self.deltas), ptr(self.rays), ptr(self.nears), self.M, self.N,
                                        self.T_thresh, ptr(self.weights_sum), ptr(self.depth), ptr(self.image), st), "composite_whole_rays")
        finish_frame(self.image, self.weights_sum, bg_color, self.depth, self.nears, self.fars, out=(self.image_out, self.depth_out), fused=True)
        if check and self.overflowed():
            raise RuntimeError(f"RayBatchRenderer: the batch needs {int(self.counter[0])} samples, the buffer holds {self.M} (raise samples_per_ray)")
        return {"image": self.image_out, "depth": self.depth_out, "weights_sum": self.weights_sum, "n_samples": self.counter[:1]}

    def overflowed(self):
        """One host read-back: did the last batch need more sample slots than the buffer has?"""
        return int(self.counter[0]) > self.M
