"""The temporal-basis model's density-grid query without a GPU: the numpy cell -> point restatement the GPU test uses
(tests/basis_density_support.py) against the oracle's Morton decode and the reference's expressions written out, the sigma bar against
three named wrong variants, and the library's new entry point (exported, declared, argument checks in front of the launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

import basis_density_support as DS
import basis_support as BS
from oracle import oracle as O

f32 = np.float32
T = 0.5


@pytest.fixture(scope="module")
def cells_and_noise():
    rng = np.random.default_rng(7)
    corners = [O.morton3D(np.array([[x, y, z]], np.int32))[0] for x in (0, DS.G - 1) for y in (0, DS.G - 1) for z in (0, DS.G - 1)]
    cells = np.concatenate([np.array(corners, np.int64), rng.choice(DS.H3, 1000, replace=False)]).astype(np.int32)
    noise = rng.random((cells.shape[0], 3), dtype=np.float32)
    noise[:4], noise[4:8] = 0.0, 1.0         # the outermost cells at the jitter's extremes: centres on -bound / +bound
    return cells, noise


def test_numpy_cell_points_equal_the_reference_expressions(cells_and_noise):
    cells, noise = cells_and_noise
    assert {0, DS.H3 - 1} <= set(cells[:8].tolist())
    coords = np.asarray(O.morton3D_invert(cells.astype(np.uint32))).astype(f32)         # the oracle's decode
    assert np.array_equal(coords, np.stack([DS.compact(cells.astype(np.uint32) >> np.uint32(d)) for d in range(3)], axis=1).astype(f32))
    for cas_bound in (1.0, 2.0, 0.5):
        half_grid = f32(cas_bound / DS.G)
        # dnerf/renderer.py:480-490, every fp32 operation on its own, `/ (G - 1)` as the device's reciprocal multiplication
        xyzs = (f32(2) * coords) * (f32(1) / f32(DS.G - 1)) - f32(1)
        want = xyzs * f32(cas_bound - cas_bound / DS.G) + (noise * f32(2) - f32(1)) * half_grid
        got = DS.cell_points(cells, noise, cas_bound)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.astype(f32).view(np.uint32)), cas_bound
        assert np.abs(got).max() <= cas_bound
    edge = DS.cell_points(cells[:8], noise[:8])
    assert (np.abs(edge[:4]).max(axis=1) == 1.0).all() and (np.abs(edge[4:8]).max(axis=1) == 1.0).all()      # centres exactly on +- bound
    for v in DS.POINT_VARIANTS:
        assert (DS.cell_points(cells, noise, variant=v) != DS.cell_points(cells, noise)).any(axis=1).mean() > 0.9, v


@pytest.mark.parametrize("variant", ("other_time",) + DS.POINT_VARIANTS)
def test_sigma_bar_rejects_wrong_variants(cells_and_noise, variant):
    """The restatement passes the bar the GPU test applies (zero distance), and each named wrong construction -- the basis row of
    another time, x and z swapped in the Morton decode, the jitter ignored -- fails it on most cells."""
    cells, noise = cells_and_noise
    cells, noise = cells[8:520], noise[8:520]
    model, _ = BS.mirror_model("cpu")
    state = BS.state_of(model)
    good = BS.BasisOracle(state, mode="fp16")
    pts = DS.cell_points(cells, noise)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], f32), (pts.shape[0], 1))
    ref = BS.expected_f16(good, pts, d, T)
    ok, stats = DS.sigma_bar(good.density(pts, T)["sigma"], ref)
    assert ok and stats["sigma_bit_exact_share"] == 1.0, stats
    if variant == "other_time":
        sigma = BS.BasisOracle(state, mode="fp16", variant="other_time", other_time=0.0).density(pts, T)["sigma"]
    else:
        sigma = good.density(DS.cell_points(cells, noise, variant=variant), T)["sigma"]
    ok, stats = DS.sigma_bar(sigma, ref)
    print(variant, stats)
    assert not ok and stats["sigma_failed"] > pts.shape[0] // 2, stats


def test_library_exports_and_header_declares_the_entry():
    import sdn_backend as B
    assert hasattr(B.lib, "sdn_density_query_cells_basis_f16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sdn_hip.h")).read()
    m = re.search(r"int sdn_density_query_cells_basis_f16\(([^;]*)\);", header)
    assert m, "include/sdn_hip.h does not declare sdn_density_query_cells_basis_f16"
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["cells", "cell_count", "n", "noise", "seed", "grid_size", "cas_bound", "weights", "basis_row", "table", "offsets_host",
                    "S", "H", "bound", "density_scale", "tmp_slice", "stream"], args
    assert len(B.lib.sdn_density_query_cells_basis_f16.argtypes) == len(args)


def test_argument_checks_come_before_the_launch():
    """Null buffers, a list without a count, a bad grid size, a bad cascade bound and n > grid_size^3 are SDN_E_BADARG (-1) before anything
    touches a device; n == 0 is a successful no-op."""
    import sdn_backend as B
    entry = B.lib.sdn_density_query_cells_basis_f16
    keep = [np.zeros(64, np.float32) for _ in range(4)]
    offs = np.zeros(17, np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731  (host addresses: the checks never dereference them)
    good = dict(cells=None, cell_count=None, n=8, noise=None, seed=0, grid_size=128, cas_bound=1.0, weights=p(keep[0]), basis_row=p(keep[1]),
                table=p(keep[2]), offsets_host=p(offs), S=0.5, H=16, bound=1.0, density_scale=1.0, tmp_slice=p(keep[3]), stream=None)
    call = lambda **kw: entry(*{**good, **kw}.values())  # noqa: E731
    assert call(n=0) == 0
    for name in ("weights", "basis_row", "table", "offsets_host", "tmp_slice"):
        assert call(**{name: None}) == -1, name
    assert call(cells=p(keep[0]), cell_count=None) == -1
    assert call(cells=None, cell_count=p(keep[0])) == -1
    assert call(grid_size=1) == -1 and call(grid_size=1025) == -1
    assert call(cas_bound=0.0) == -1 and call(cas_bound=float("nan")) == -1
    assert call(n=128 ** 3 + 1) == -1
    assert call(grid_size=2, n=9) == -1
    assert ctypes.sizeof(ctypes.c_void_p) == 8
