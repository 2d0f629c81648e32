"""The ambient-dimension model without a GPU: tests/golden/caller_hyper.npz (the reference's own dnerf/network_hyper.py executed over the
oracle's operators, tests/golden/gen_hyper_fixture.py) against the numpy restatement of tests/hyper_support.py, the mirror's state, the
4-D grid's level classes, the weight packing of dnerf_amd/fused_hyper.py, and the GPU tests' bars against four named wrong variants."""
from types import SimpleNamespace

import numpy as np
import pytest

import basis_support as BS
import hyper_support as HS


@pytest.fixture(scope="module")
def rig():
    model, bits = HS.mirror_model("cpu")             # (asserts every digest)
    return SimpleNamespace(model=model, bits=bits, state=HS.state_of(model), fx=HS.load())


def test_mirror_state_is_the_reference_networks_state(rig):
    keys = set(rig.fx["digest_keys"].tolist())
    assert {"ambient_net.4.weight", "sigma_net.1.weight", "color_net.2.weight", "encoder.embeddings", "encoder.offsets", "density_bitfield"} <= keys
    assert keys == {k for k in rig.model.state_dict() if not k.startswith("density_grid")}
    assert tuple(rig.model.sigma_net[1].weight.shape) == (33, 64) and tuple(rig.model.color_net[2].weight.shape) == (3, 64)
    assert rig.model.encoder.input_dim == 4 and tuple(rig.model.ambient_net[4].weight.shape) == (1, 128)
    groups = rig.model.get_params(1e-2, 1e-3)
    assert len(groups) == 6 and [g["lr"] for g in groups] == [1e-2, 1e-3] * 3


def test_level_classes_from_the_oracles_offsets_and_index():
    """The classes come from the oracle's offsets and the stride rule of get_grid_index; that the rule IS the oracle's index is shown
    by the numpy restatement built on it reproducing the oracle's D = 4 forward bit for bit, across cell boundaries of the fourth
    coordinate.  Each class is non-empty for the default geometry."""
    geo = HS.Geometry4(1)
    print({k: v for k, v in geo.classes.items()})
    assert all(geo.classes[k] for k in ("dense", "w_wraps", "w_dropped", "zw_dropped"))
    assert sorted(sum(geo.classes.values(), [])) == list(range(16))
    assert all(geo.levels[l]["s"][3] == 0 and geo.levels[l]["s"][2] > 0 for l in geo.classes["w_dropped"])
    assert all(geo.levels[l]["hs"] == 2 ** 19 for l in geo.classes["w_wraps"] + geo.classes["w_dropped"] + geo.classes["zw_dropped"])
    table = HS.random_table(geo)
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, (96, 3)).astype(np.float32)
    for a in (-1.0, -0.3, 0.1333, 0.6, 1.0, 1.5):
        u4 = geo.u4(x, a)
        assert np.array_equal(HS.grid_features4(geo, u4, table).view(np.uint16), HS.oracle_features(geo, u4, table).view(np.uint16)), a


@pytest.mark.parametrize("t", HS.TIMES)
def test_fp32_restatement_reproduces_reference_forward_and_density(rig, t):
    fx = rig.fx
    f = HS.HyperOracle(rig.state, mode="fp32")
    assert abs(float(f.ambient(t)) - float(fx[f"t{t}_ambient"][0])) < 2e-6
    a = np.float32(fx[f"t{t}_ambient"][0])           # (the reference's own value: the grid is discontinuous in nothing, but keep the cells)
    sigma, rgb, _ = f.forward(fx["x"], fx["d"], t, ambient=a)
    np.testing.assert_allclose(sigma, fx[f"t{t}_sigma"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(rgb, fx[f"t{t}_rgb"], rtol=0, atol=2e-5)
    d = f.density(fx["x"], t, ambient=a)
    np.testing.assert_allclose(d["sigma"], fx[f"t{t}_density_sigma"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(d["geo_feat"], fx[f"t{t}_density_geo"], rtol=0, atol=2e-5)


def test_pack_restatement_matches_the_package(rig):
    from dnerf_amd import fused_hyper as FH
    ws = [rig.state[f"{net}.{i}.weight"] for net in ("sigma_net", "color_net") for i in range(HS.NETS[net])]
    blocks = HS.pack_numpy(ws)
    assert blocks.shape == (30, 64, 8)
    ours = np.concatenate([FH.F16._pack_layer(*layer) for layer in FH.layer_plan(ws)], axis=0)       # (pack_weights without the library call)
    assert np.array_equal(ours.view(np.uint16), blocks.view(np.uint16))
    # the permutation, read back: S1 is blocks 4..11 (2 m-tiles x 4 k-steps); lane l of tile mt holds output row 32 mt + l
    s1 = ws[1].astype(np.float16)
    km = BS.kmaps()[1][1]
    assert np.array_equal(blocks[4][5], s1[1 + 5, km[0][0]])                  # tile 0, row 5 = geo_feat[5] = output 6
    assert np.array_equal(blocks[8][0], s1[0, km[0][0]])                      # tile 1, row 0 = the density logit
    assert not blocks[8:12, 1:32].any() and not blocks[8:12, 33:].any()       # the rest of tile 1 is zero


def test_fp16_restatement_is_at_fp16_distance_of_the_fixture(rig):
    fx = rig.fx
    f = HS.HyperOracle(rig.state, mode="fp16")
    for t in HS.TIMES:
        a = f.ambient(t)
        assert a == np.float32(np.float16(a)) and abs(float(a) - float(fx[f"t{t}_ambient"][0])) < 4e-3
        sigma, rgb, _ = f.forward(fx["x"], fx["d"], t)
        rel = np.abs(sigma - fx[f"t{t}_sigma"]) / np.maximum(fx[f"t{t}_sigma"], 1e-3)
        print(t, float(np.quantile(rel, 0.5)), float(np.quantile(np.abs(rgb - fx[f"t{t}_rgb"]), 0.99)))
        assert np.quantile(rel, 0.5) < 5e-2, (t, float(np.quantile(rel, 0.5)))      # (the fp16 ambient moves every level-0..4 feature a little)
        assert np.quantile(np.abs(rgb - fx[f"t{t}_rgb"]), 0.99) < 5e-3, t


@pytest.mark.parametrize("variant", HS.VARIANTS)
def test_bars_of_the_gpu_tests_reject_wrong_variants(rig, variant):
    """The restatement itself passes the GPU tests' bars and each named wrong model fails them on many values -- on the state the GPU
    test uses (`boosted_colour`: the seeded colour logits are too small to show a wrong wiring)."""
    fx, state = rig.fx, HS.boosted_colour(rig.state)
    x, d, t = fx["x"][:512], fx["d"][:512], 0.5
    good = HS.HyperOracle(state, mode="fp16")
    ref = HS.expected_f16(good, x, d, t)
    s, c, _ = good.forward(x, d, t)
    ok, stats = HS.field_bars(s, c, ref)
    assert ok and stats["sigma_bit_exact_share"] == 1.0, stats
    s, c, _ = HS.HyperOracle(state, mode="fp16", numpy_grid=True).forward(x, d, t)       # (the variants' grid, unvaried: the same bits)
    assert HS.field_bars(s, c, ref)[0]
    bad = HS.HyperOracle(state, mode="fp16", variant=variant)
    s, c, _ = bad.forward(x, d, t)
    ok, stats = HS.field_bars(s, c, ref)
    print(variant, stats)
    if variant == "upper_corners_first":
        # The same sixteen products summed in another order: a difference of fp16 roundings of single features, which the carried
        # worst-case bound of the full network allows for by construction (measured here: 0 of 512 points fail, 20 % of the logits keep
        # their bits).  The bar that rejects it is the probe-weight test's, which reads each feature out bit for bit
        # (field_probe_support.grid_bar_f16 on exp(feature)): many features of every level fail it.
        import field_probe_support as P
        a = good.ambient(t)
        want = HS.oracle_features(good.geo, good.geo.u4(x, a), good.table)
        got = HS.grid_features4(good.geo, good.geo.u4(x, a), good.table, variant)
        for j in (0, 9, 15, 31):
            okj, st = P.grid_bar_f16(np.exp(got[:, j].astype(np.float64)), want[:, j])
            assert (~okj).sum() >= 16, (j, st)
        return
    assert not ok and stats["sigma_failed"] >= 16, stats      # not one marginal value
