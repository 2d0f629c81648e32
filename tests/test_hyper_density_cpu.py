"""The ambient-dimension model's density-grid query without a GPU: the library's new entry point (exported, declared, bound with as many
argtypes as the header has parameters, argument checks in front of the launch), the sigma bar of the GPU test on cell points of a 128^3
slice against named wrong variants, and the parts of `DensityGridUpdater` / `use_native_density_update` that raise before they touch a
device."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import hyper_density_support as DS
import hyper_support as HS
from oracle import oracle as O

f32 = np.float32
T = 0.5


@pytest.fixture(scope="module")
def rig():
    model, _ = HS.mirror_model("cpu")
    state = HS.state_of(model)
    rng = np.random.default_rng(7)
    corners = [O.morton3D(np.array([[x, y, z]], np.int32))[0] for x in (0, DS.G - 1) for y in (0, DS.G - 1) for z in (0, DS.G - 1)]
    cells = np.concatenate([np.array(corners, np.int64), rng.choice(DS.H3, 504, replace=False)]).astype(np.int32)
    noise = rng.random((cells.shape[0], 3), dtype=np.float32)
    noise[:4], noise[4:8] = 0.0, 1.0         # the outermost cells at the jitter's extremes: centres on -bound / +bound
    good = HS.HyperOracle(state, mode="fp16")
    pts = DS.cell_points(cells, noise)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], f32), (pts.shape[0], 1))
    return SimpleNamespace(model=model, state=state, cells=cells, noise=noise, good=good, pts=pts, d=d, ref=HS.expected_f16(good, pts, d, T))


def test_library_exports_and_header_declares_the_entry():
    import sdn_backend as B
    assert hasattr(B.lib, "sdn_density_query_cells_hyper_f16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sdn_hip.h")).read()
    m = re.search(r"int sdn_density_query_cells_hyper_f16\(([^;]*)\);", header)
    assert m, "include/sdn_hip.h does not declare sdn_density_query_cells_hyper_f16"
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["cells", "cell_count", "n", "noise", "seed", "grid_size", "cas_bound", "weights", "ambient_row", "table", "offsets_host",
                    "S", "H", "bound", "density_scale", "tmp_slice", "stream"], args
    assert len(B.lib.sdn_density_query_cells_hyper_f16.argtypes) == len(args)
    basis = re.search(r"int sdn_density_query_cells_basis_f16\(([^;]*)\);", header).group(1)
    assert [a.split()[:-1] for a in m.group(1).replace("\n", " ").split(",")] == [a.split()[:-1] for a in basis.replace("\n", " ").split(",")]


def test_argument_checks_come_before_the_launch():
    """Null buffers, a list without a count, a bad grid size, a bad cascade bound and n > grid_size^3 are SDN_E_BADARG (-1) before anything
    touches a device; n == 0 is a successful no-op.  (tests/test_basis_density_cpu.py's checks: kind 4 goes through the same ones.)"""
    import sdn_backend as B
    entry = B.lib.sdn_density_query_cells_hyper_f16
    keep = [np.zeros(64, np.float32) for _ in range(4)]
    offs = np.zeros(17, np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731  (host addresses: the checks never dereference them)
    good = dict(cells=None, cell_count=None, n=8, noise=None, seed=0, grid_size=128, cas_bound=1.0, weights=p(keep[0]), ambient_row=p(keep[1]),
                table=p(keep[2]), offsets_host=p(offs), S=0.5, H=16, bound=1.0, density_scale=1.0, tmp_slice=p(keep[3]), stream=None)
    call = lambda **kw: entry(*{**good, **kw}.values())  # noqa: E731
    assert call(n=0) == 0
    for name in ("weights", "ambient_row", "table", "offsets_host", "tmp_slice"):
        assert call(**{name: None}) == -1, name
    assert call(cells=p(keep[0]), cell_count=None) == -1
    assert call(cells=None, cell_count=p(keep[0])) == -1
    assert call(grid_size=1) == -1 and call(grid_size=1025) == -1
    assert call(cas_bound=0.0) == -1 and call(cas_bound=float("nan")) == -1
    assert call(n=128 ** 3 + 1) == -1
    assert call(grid_size=2, n=9) == -1


def test_sigma_bar_accepts_the_restatement_on_cell_points(rig):
    """512 cells of a 128^3 slice, the eight corner cells at the jitter's extremes among them (centres exactly on +-bound)."""
    assert (np.abs(rig.pts[:8]).max(axis=1) == 1.0).all()
    ok, stats = DS.sigma_bar(rig.good.density(rig.pts, T)["sigma"], rig.ref)
    assert ok and stats["sigma_bit_exact_share"] == 1.0, stats
    sigma = HS.HyperOracle(rig.state, mode="fp16", numpy_grid=True).density(rig.pts, T)["sigma"]     # (the grid variants' grid, unvaried)
    assert DS.sigma_bar(sigma, rig.ref)[0]
    assert float(np.std(rig.ref["sigma"])) > 0


@pytest.mark.parametrize("variant", DS.POINT_VARIANTS + HS.VARIANTS)
def test_sigma_bar_rejects_wrong_variants(rig, variant):
    """Each named wrong construction -- x and z swapped in the Morton decode, the jitter ignored, the ambient coordinate not normalised,
    sigma read from geo_feat[0], the fourth coordinate indexed where the level drops it -- fails the sigma bar on many cells.
    `upper_corners_first` sums the same sixteen products in another order, which the carried worst-case bound allows for by construction
    (tests/test_hyper_cpu.py): it is rejected with the bit-exact feature comparison on the cell points, as there."""
    assert set(DS.SIGMA_VARIANTS) <= set(HS.VARIANTS)
    if variant in DS.POINT_VARIANTS:
        sigma = rig.good.density(DS.cell_points(rig.cells, rig.noise, variant=variant), T)["sigma"]
    elif variant == "upper_corners_first":
        import field_probe_support as P
        a = rig.good.ambient(T)
        u4 = rig.good.geo.u4(rig.pts, a)
        want = HS.oracle_features(rig.good.geo, u4, rig.good.table)
        got = HS.grid_features4(rig.good.geo, u4, rig.good.table, variant)
        for j in (0, 9, 15, 31):
            okj, st = P.grid_bar_f16(np.exp(got[:, j].astype(np.float64)), want[:, j])
            assert (~okj).sum() >= 16, (j, st)
        return
    else:
        sigma = HS.HyperOracle(rig.state, mode="fp16", variant=variant).density(rig.pts, T)["sigma"]
    ok, stats = DS.sigma_bar(sigma, rig.ref)
    print(variant, stats)
    floor = rig.pts.shape[0] // 2 if variant in DS.POINT_VARIANTS else 16
    assert not ok and stats["sigma_failed"] >= floor, stats


def test_updater_detects_the_model_and_refuses_before_touching_a_device(rig):
    from dnerf_amd import fused, fused_hyper
    from dnerf_amd.network_hyper import NeRFNetwork
    import basis_support as BS
    assert fused_hyper.FusedHyperField.has_density_query is False and fused_hyper.FusedHyperField.ctx_kind == 4
    with pytest.raises(NotImplementedError, match="ambient-dimension model has no fp32"):
        fused.DensityGridUpdater(rig.model, fp32=True)
    with pytest.raises(NotImplementedError, match="temporal-basis model has no fp32"):
        fused.DensityGridUpdater(BS.mirror_model("cpu", check=False)[0], fp32=True)
    with pytest.raises(NotImplementedError, match="no density query"):
        fused.DensityGridUpdater(rig.model, field=SimpleNamespace(ctx_kind=4))                       # as a field built without density_query
    with pytest.raises(NotImplementedError, match="no density query"):
        fused.DensityGridUpdater(rig.model, field=SimpleNamespace(ctx_kind=4, has_density_query=False))
    with pytest.raises(NotImplementedError, match="bg_radius"):
        NeRFNetwork(**{**HS.MODEL_KW, "bg_radius": 1.0}).use_native_density_update()
    with pytest.raises(NotImplementedError, match="ambient_dim"):
        NeRFNetwork(**{**HS.MODEL_KW, "ambient_dim": 2}).use_native_density_update()
    with pytest.raises(NotImplementedError, match="architecture"):
        NeRFNetwork(**{**HS.MODEL_KW, "hidden_dim": 32}).use_native_density_update()
    assert getattr(rig.model, "_density_updater", None) is None
