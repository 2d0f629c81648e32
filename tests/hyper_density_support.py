"""Shared by tests/test_hyper_density_cpu.py and tests/test_gpu_hyper_density.py: the occupancy-grid cell -> jittered point construction
of update_extra_state (dnerf/renderer.py:480-490) and the perturbed slice times, both imported from tests/basis_density_support.py, and
the sigma half of the bars tests/hyper_support.py holds the fused hyper field to."""
import numpy as np

import hyper_support as HS
from basis_density_support import G, H3, POINT_VARIANTS, cell_points, compact, torch_points, update_times  # noqa: F401

f32 = np.float32
# the `hyper_support.VARIANTS` that change sigma through the network (the two grid variants change single features: test_hyper_cpu.py)
SIGMA_VARIANTS = ("ambient_unnormalised", "s1_off_by_one")


def sigma_bar(sigma, ref, density_scale=1.0):
    """The sigma half of HS.field_bars against `HS.expected_f16`'s record; the rgb half is fed the reference's own values.
    -> (ok, stats with `sigma_failed`, `sigma_worst_of_bar`, ...)."""
    ok, stats = HS.field_bars(sigma, ref["rgb"].astype(f32), ref, density_scale)
    assert stats["rgb_failed"] == 0
    return ok, stats


def ambient_row(a):
    """The [128] float32 constants row with ambient coordinate `a` in entry 0."""
    r = np.zeros(128, f32)
    r[0] = f32(a)
    return r
