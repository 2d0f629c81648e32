"""The temporal-basis model without a GPU: tests/golden/caller_basis.npz (the reference's own dnerf/network_basis.py executed over the
oracle's operators, tests/golden/gen_basis_fixture.py) against the numpy restatement of tests/basis_support.py, the mirror's state, the
weight packing of dnerf_amd/fused_basis.py, the basis row, and the GPU tests' bars against three named wrong variants."""
import numpy as np
import pytest
import torch

import basis_support as BS
from oracle.render import render_frame_oracle
from types import SimpleNamespace


@pytest.fixture(scope="module")
def rig():
    model, bits = BS.mirror_model("cpu")             # (asserts every digest)
    return SimpleNamespace(model=model, bits=bits, state=BS.state_of(model), fx=BS.load())


def test_mirror_state_is_the_reference_networks_state(rig):
    keys = set(rig.fx["digest_keys"].tolist())
    assert {"basis_net.4.weight", "sigma_net.1.weight", "color_net.2.weight", "encoder.embeddings", "density_bitfield"} <= keys
    assert not any(k.startswith("deform_net") for k in keys)
    assert tuple(rig.model.sigma_net[1].weight.shape) == (64, 64) and tuple(rig.model.color_net[2].weight.shape) == (24, 64)
    groups = rig.model.get_params(1e-2, 1e-3)
    assert len(groups) == 6 and [g["lr"] for g in groups] == [1e-2, 1e-3] * 3


@pytest.mark.parametrize("t", BS.TIMES)
def test_fp32_restatement_reproduces_reference_forward_and_density(rig, t):
    fx = rig.fx
    f = BS.BasisOracle(rig.state, mode="fp32")
    sigma, rgb, _ = f.forward(fx["x"], fx["d"], t)
    np.testing.assert_allclose(sigma, fx[f"t{t}_sigma"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(rgb, fx[f"t{t}_rgb"], rtol=0, atol=2e-5)
    d = f.density(fx["x"], t)
    np.testing.assert_allclose(d["sigma"], fx[f"t{t}_density_sigma"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(d["geo_feat"], fx[f"t{t}_density_geo"], rtol=0, atol=2e-5)


@pytest.mark.parametrize("t", BS.TIMES)
def test_fp32_restatement_reproduces_reference_frames(rig, t):
    from dnerf_amd import scene
    fx, model = rig.fx, rig.model
    ro, rd = scene.get_rays(scene.look_at_pose(30.0, 30.0), scene.intrinsics(64, 64), 64, 64)
    sc = SimpleNamespace(model=model, rays_o=torch.from_numpy(ro), rays_d=torch.from_numpy(rd), time=torch.tensor([[t]]),
                         bitfield=rig.bits[BS.slice_of(t, model.time_size)])
    out = render_frame_oracle(sc, field=BS.BasisOracle(rig.state, mode="fp32"))
    assert np.array_equal(np.array(out["trace"], np.int32), fx[f"t{t}_trace"])
    np.testing.assert_allclose(out["image"], fx[f"t{t}_image"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(out["weights_sum"], fx[f"t{t}_weights_sum"], rtol=0, atol=2e-5)
    miss = np.isnan(fx[f"t{t}_depth"])
    assert np.array_equal(np.isnan(out["depth"]), miss)
    np.testing.assert_allclose(out["depth"][~miss], fx[f"t{t}_depth"][~miss], rtol=0, atol=2e-5)


def test_pack_then_unpack_is_the_identity_and_matches_the_package(rig):
    from dnerf_amd import fused_basis as FB
    ws = [rig.state[f"{net}.{i}.weight"] for net in ("sigma_net", "color_net") for i in range(BS.NETS[net])]
    blocks = BS.pack_numpy(ws)
    assert blocks.shape == (30, 64, 8)
    back = BS.unpack_numpy(blocks, [w.shape for w in ws])
    for w, b in zip(ws, back):
        assert np.array_equal(w.astype(np.float16), b)
    ours = np.concatenate([FB.F16._pack_layer(*layer) for layer in FB.layer_plan(ws)], axis=0)       # (pack_weights without the library call)
    assert np.array_equal(ours.view(np.uint16), blocks.view(np.uint16))


@pytest.mark.parametrize("t", BS.TIMES)
def test_basis_row_equals_the_fixture(rig, t):
    row = BS.BasisOracle(rig.state, mode="fp32").row(t)
    np.testing.assert_allclose(row[:40], rig.fx[f"t{t}_basis"], rtol=0, atol=2e-6)
    assert not row[40:].any() and row.shape == (128,)
    # the fp16 row (what FusedBasisField._time_row computes with the mirror's own layers under autocast: tests/test_gpu_basis_field.py) holds fp16 values, within fp16 distance of the fp32 one
    r16 = BS.BasisOracle(rig.state, mode="fp16").row(t)
    assert np.array_equal(r16, r16.astype(np.float16).astype(np.float32))
    assert np.abs(r16[:40] - row[:40]).max() <= 16 * BS.ulp16(np.abs(row[:40]).max())


def test_fp16_restatement_is_at_fp16_distance_of_the_fixture(rig):
    """The expected value of the GPU tests is the model, not something else: sigma within 2 % and rgb within 5e-3 of the fp32 fixture at
    p99 (the spread of fp16 Linear layers on these magnitudes, as for the deformation model's fp16 oracle)."""
    fx = rig.fx
    f = BS.BasisOracle(rig.state, mode="fp16")
    for t in BS.TIMES:
        sigma, rgb, _ = f.forward(fx["x"], fx["d"], t)
        rel = np.abs(sigma - fx[f"t{t}_sigma"]) / np.maximum(fx[f"t{t}_sigma"], 1e-3)
        assert np.quantile(rel, 0.99) < 2e-2, (t, float(np.quantile(rel, 0.99)))
        assert np.quantile(np.abs(rgb - fx[f"t{t}_rgb"]), 0.99) < 5e-3, t


@pytest.mark.parametrize("variant", BS.VARIANTS)
def test_bars_of_the_gpu_tests_reject_wrong_variants(rig, variant):
    """The restatement itself passes the GPU tests' bars (it is the expected value: zero distance) and each named wrong model fails them,
    on many values -- on the state the GPU test uses (`boosted_colour`: see there why)."""
    fx, state = rig.fx, BS.boosted_colour(rig.state)
    x, d, t = fx["x"][:512], fx["d"][:512], 0.5
    good = BS.BasisOracle(state, mode="fp16")
    ref = BS.expected_f16(good, x, d, t)
    s, c, _ = good.forward(x, d, t)
    ok, stats = BS.field_bars(s, c, ref)
    assert ok and stats["sigma_bit_exact_share"] == 1.0, stats
    bad = BS.BasisOracle(state, mode="fp16", variant=variant, other_time=0.0)
    s, c, _ = bad.forward(x, d, t)
    ok, stats = BS.field_bars(s, c, ref)
    print(variant, stats)
    assert not ok
    assert (stats["rgb_failed"] if variant != "other_time" else stats["sigma_failed"]) >= 16, stats      # not one marginal value
