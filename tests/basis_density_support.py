"""Shared by tests/test_basis_density_cpu.py and tests/test_gpu_basis_density.py: the occupancy-grid cell -> jittered point construction
of update_extra_state (dnerf/renderer.py:480-490) restated in numpy with the reference's fp32 operation order, two named wrong variants
of it, and the sigma half of the bars tests/basis_support.py holds the fused basis field to."""
import numpy as np

import basis_support as BS

f32 = np.float32
G = 128
H3 = G ** 3
POINT_VARIANTS = ("xz_swapped", "centre")


def compact(v):
    """Morton code -> one coordinate (bits 0, 3, 6, ...), raymarching.cu:282-289."""
    v = np.asarray(v, np.uint32) & np.uint32(0x49249249)
    v = (v | (v >> np.uint32(2))) & np.uint32(0xc30c30c3)
    v = (v | (v >> np.uint32(4))) & np.uint32(0x0f00f00f)
    v = (v | (v >> np.uint32(8))) & np.uint32(0xff0000ff)
    return (v | (v >> np.uint32(16))) & np.uint32(0x0000ffff)


def cell_points(cells, noise, cas_bound=1.0, grid_size=G, variant=None):
    """xyzs = 2 * coords / (G - 1) - 1;  cas_xyzs = xyzs * (bound - half_grid);  cas_xyzs += (rand * 2 - 1) * half_grid, every operation
    rounded to fp32 on its own, `tensor / (G - 1)` as the multiplication by the fp32 reciprocal torch performs on the device.
    variant: one named WRONG construction (POINT_VARIANTS)."""
    assert variant is None or variant in POINT_VARIANTS, variant
    c = np.asarray(cells).astype(np.uint32)
    order = (2, 1, 0) if variant == "xz_swapped" else (0, 1, 2)
    coords = np.stack([compact(c >> np.uint32(s)) for s in order], axis=1).astype(f32)
    noise = np.full(coords.shape, 0.5, f32) if variant == "centre" else np.asarray(noise, f32)
    half_grid = f32(cas_bound / grid_size)
    span = f32(cas_bound - cas_bound / grid_size)
    xyzs = (f32(2) * coords) * (f32(1) / f32(grid_size - 1)) - f32(1)
    return (xyzs * span + (noise * f32(2) - f32(1)) * half_grid).astype(f32)


def sigma_bar(sigma, ref, density_scale=1.0):
    """The sigma half of BS.field_bars against `BS.expected_f16`'s record; the rgb half is fed the reference's own values.
    -> (ok, stats with `sigma_failed`, `sigma_worst_of_bar`, ...)."""
    ok, stats = BS.field_bars(sigma, ref["rgb"].astype(f32), ref, density_scale)
    assert stats["rgb_failed"] == 0
    return ok, stats


def update_times(model_times, time_noise, time_size):
    """The perturbed time of every slice, as DensityGridUpdater.update forms it from a [T, 1] draw (dnerf/renderer.py:486,492)."""
    return model_times.reshape(time_size, 1).cpu() + (time_noise.cpu().float() * 2 - 1) * (0.5 / time_size)


def torch_points(model, cells, noise, cas_bound=1.0):
    """dnerf/renderer.py:480-490 in torch on the device, for Morton indices `cells` (tests/test_gpu_density_update.py's `_points`)."""
    import raymarching
    import torch
    coords = raymarching.morton3D_invert(cells.to(torch.int32))
    xyzs = 2 * coords.float() / (model.grid_size - 1) - 1
    half_grid = cas_bound / model.grid_size
    cas = xyzs * (cas_bound - half_grid)
    cas += (noise * 2 - 1) * half_grid
    return cas.contiguous()
