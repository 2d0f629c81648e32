"""Shared by the frame-group preview tests (tests/test_gpu_preview_group.py, tests/test_preview_group_cpu.py): the noise rows a group
of F jittered samples is rendered with, the fake accumulators of a finished group, and the stubs of the CPU tests."""
import numpy as np

import preview_support as PS

ROW_NAMES = {2: ("below", "draw"), 3: ("draw", "zeros", "draw"), 4: ("draw", "zeros", "below", "draw")}


def noise_row(name, n, seed=3):
    """One frame's [n] fp32 offsets: 'draw' = the seeded draw with 0 and the largest float below 1 among its entries, 'zeros' = all 0
    (the unperturbed march), 'below' = all nextafter(1, 0)."""
    if name == "zeros":
        return np.zeros(n, np.float32)
    if name == "below":
        return np.full(n, PS.ONE_BELOW, np.float32)
    z = PS.draw_noises(n, seed)
    if n >= 35:
        z[n // 2], z[n // 2 + 1] = 0.0, PS.ONE_BELOW          # on rays through the middle of the frame: they hit the figure
    return z


def noise_rows(F, n):
    """[F, n]: F = 2 has the all-nextafter(1, 0) row, F = 3 and 4 the all-0 row and a row equal to row 0 (identical frames)."""
    return np.stack([noise_row(name, n) for name in ROW_NAMES[F]])


def fake_group(F, rH, rW, seed):
    """Accumulators of F finished frames of rH x rW rays, frame-major, as a group loop leaves them: NaN / inf depths among them, dark
    pixels on both sides of the sRGB edge, a ray that misses the box (0 / 0), and a NaN planted in frame 1's colour accumulator."""
    rng = np.random.default_rng(seed)
    n = rH * rW
    N = F * n
    f32 = np.float32
    acc = dict(image=rng.random((N, 3), dtype=f32) * f32(0.6), weights_sum=rng.random(N, dtype=f32), depth=rng.random(N, dtype=f32) * f32(2.0),
               nears=f32(0.2) + rng.random(N, dtype=f32) * f32(0.3), rays_o=rng.standard_normal((N, 3)).astype(f32),
               rays_d=rng.standard_normal((N, 3)).astype(f32))
    acc["fars"] = (acc["nears"] + f32(0.5) + rng.random(N, dtype=f32)).astype(f32)
    acc["image"][::5] *= f32(0.004)
    for f in range(F):
        for k, v in enumerate([np.nan, np.inf, -np.inf][:n]):
            acc["depth"][f * n + (k * 7 + f) % n] = v
        if n > 8:
            acc["fars"][f * n + 8] = acc["nears"][f * n + 8]
            acc["depth"][f * n + 8] = 0
    acc["image"][min(1, F - 1) * n + n // 3, 1] = np.nan
    return acc


class FakeGroupLoop:
    """What `PreviewRenderer.accumulate_group` needs of a group loop, without a device: records the `render_samples` calls."""

    def __init__(self, ctx):
        self.ctx, self.calls = ctx, []

    def render_samples(self, rays_o, rays_d, time, noises, **kw):
        self.calls.append((tuple(noises.shape), kw))
