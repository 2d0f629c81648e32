"""The temporal-basis model's fp32 fused field without a GPU: the library's three new entries (exported, declared, argument checks in
front of the launch), the weight packing of `fused_basis.pack_weights_f32` against a numpy restatement, the fp32 bar of
tests/basis_f32_support.py against three named wrong variants of the model, and what `DensityGridUpdater` accepts and refuses."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import basis_f32_support as FS
import basis_support as BS

T = 0.5
ENTRIES = {
    "sdn_field_basis_forward_f32": ["xyzs", "dirs", "live_idx", "live_count", "M", "weights", "basis_row", "table", "offsets_host", "S", "H", "bound",
                                    "density_scale", "sigmas", "rgbs", "stream"],
    "sdn_density_query_cells_basis_f32": ["cells", "cell_count", "n", "noise", "seed", "grid_size", "cas_bound", "weights", "basis_row", "table",
                                          "offsets_host", "S", "H", "bound", "density_scale", "tmp_slice", "stream"],
}


@pytest.fixture(scope="module")
def rig():
    model, _ = BS.mirror_model("cpu")
    return SimpleNamespace(model=model, state=BS.state_of(model), fx=BS.load())


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "sdn_hip.h")).read()


def _declared_args(header, name, ret="int"):
    m = re.search(ret + r" " + name + r"\(([^;]*)\);", header)
    assert m, f"include/sdn_hip.h does not declare {name}"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1).replace("\n", " "))
    return [a.strip().split()[-1].lstrip("*") for a in body.split(",")]


def test_header_declares_the_entries_and_ctypes_agrees():
    import sdn_backend as B
    header = _header()
    assert _declared_args(header, "sdn_field_basis_weight_floats_f32", "uint32_t") == ["void"]
    assert int(B.lib.sdn_field_basis_weight_floats_f32()) == FS.STAGE_FLOATS
    for name, want in ENTRIES.items():
        assert hasattr(B.lib, name), name
        args = _declared_args(header, name)
        assert args == want, (name, args)
        assert len(getattr(B.lib, name).argtypes) == len(args), name
    # the argument list of the fp16 entries
    assert _declared_args(header, "sdn_field_basis_forward_f16") == ENTRIES["sdn_field_basis_forward_f32"]
    assert _declared_args(header, "sdn_density_query_cells_basis_f16") == ENTRIES["sdn_density_query_cells_basis_f32"]


def test_argument_checks_come_before_the_launch():
    """Null buffers, a list without a count, n > grid_size^3: SDN_E_BADARG (-1); a table in one of the fp16 kernels' own layouts (level
    sizes == 1 or 2 mod 8): SDN_E_UNSUPPORTED (-2); M == 0 a successful no-op -- all before anything touches a device."""
    import sdn_backend as B
    keep = [np.zeros(64, np.float32) for _ in range(6)]
    ref = (np.arange(17) * 8).astype(np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731  (host addresses: the checks never dereference them)
    fwd = dict(xyzs=p(keep[0]), dirs=p(keep[1]), live_idx=None, live_count=None, M=8, weights=p(keep[2]), basis_row=p(keep[3]), table=p(keep[4]),
               offsets_host=p(ref), S=0.5, H=16, bound=1.0, density_scale=1.0, sigmas=p(keep[5]), rgbs=p(keep[5]), stream=None)
    call = lambda **kw: B.lib.sdn_field_basis_forward_f32(*{**fwd, **kw}.values())  # noqa: E731
    assert call(M=0) == 0
    for name in ("xyzs", "dirs", "weights", "basis_row", "table", "offsets_host", "sigmas", "rgbs"):
        assert call(**{name: None}) == -1, name
    assert call(live_idx=p(keep[0])) == -1 and call(live_count=p(keep[0])) == -1
    cel = dict(cells=None, cell_count=None, n=8, noise=None, seed=0, grid_size=128, cas_bound=1.0, weights=p(keep[2]), basis_row=p(keep[3]),
               table=p(keep[4]), offsets_host=p(ref), S=0.5, H=16, bound=1.0, density_scale=1.0, tmp_slice=p(keep[5]), stream=None)
    qcall = lambda **kw: B.lib.sdn_density_query_cells_basis_f32(*{**cel, **kw}.values())  # noqa: E731
    assert qcall(n=0) == 0
    for name in ("weights", "basis_row", "table", "offsets_host", "tmp_slice"):
        assert qcall(**{name: None}) == -1, name
    assert qcall(cells=p(keep[0]), cell_count=None) == -1 and qcall(n=128 ** 3 + 1) == -1 and qcall(grid_size=1) == -1
    for step in (1, 2):        # PADDED / QUAD offsets
        derived = (ref + step * np.arange(17)).astype(np.int32)
        assert call(offsets_host=p(derived)) == -2 and qcall(offsets_host=p(derived)) == -2, step


def test_pack_then_unpack_is_the_identity_and_matches_the_package(rig):
    from dnerf_amd import fused_basis as FB
    ws = [rig.state[f"{net}.{i}.weight"] for net in ("sigma_net", "color_net") for i in range(BS.NETS[net])]
    flat = FS.pack_numpy(ws)
    assert flat.shape == (FS.STAGE_FLOATS,) and flat.dtype == np.float32
    back = FS.unpack_numpy(flat, [w.shape for w in ws])       # (asserts that padded rows are zero)
    for w, b in zip(ws, back):
        assert np.array_equal(w.view(np.uint32), b.view(np.uint32))
    ours = FB.pack_weights_f32(rig.model)
    assert ours.dtype == np.float32 and np.array_equal(ours.view(np.uint32), flat.view(np.uint32))
    # C2's rows 24..31: zero lanes
    c2 = flat[-32 * 64:].reshape(32, 64)
    assert not c2[:, 24:32].any() and not c2[:, 56:64].any() and c2[:, :24].any()


@pytest.mark.parametrize("variant", BS.VARIANTS)
def test_the_fp32_bar_rejects_wrong_variants(rig, variant):
    """On the state the GPU tests use (`BS.boosted_colour`): the restatement passes its own bar, and each named wrong model fails it on at
    least half of 513 points -- the basis of another time on sigma and on rgb, the two wrong colour wirings on rgb."""
    fx, state = rig.fx, BS.boosted_colour(rig.state)
    x, d = fx["x"][:513], fx["d"][:513]
    good = BS.BasisOracle(state, mode="fp32")
    ws, wc, _ = good.forward(x, d, T)
    ok, stats = FS.field_bar(ws, wc, ws, wc)
    assert ok and stats["points_failed"] == 0
    bad = BS.BasisOracle(state, mode="fp32", variant=variant, other_time=0.0)
    s, c, _ = bad.forward(x, d, T)
    ok, stats = FS.field_bar(s, c, ws, wc)
    print(variant, stats)
    assert not ok and stats["points_failed"] >= 257, stats
    assert stats["rgb_failed"] >= 257, stats
    if variant == "other_time":
        assert stats["sigma_failed"] >= 257, stats


def test_updater_accepts_the_fp32_field_and_keeps_its_refusals(rig):
    from dnerf_amd import fused, fused_basis
    assert fused_basis.FusedBasisFieldF32.ctx_kind == 5
    with pytest.raises(NotImplementedError, match="temporal-basis model has no fp32.*field="):
        fused.DensityGridUpdater(rig.model, fp32=True)
    with pytest.raises(NotImplementedError, match="FusedBasisFieldF32"):
        fused_basis.FusedBasisField(rig.model, T, fp16=False)
    up = fused.DensityGridUpdater(rig.model, field=SimpleNamespace(ctx_kind=5))          # as far as the constructor goes without a device
    assert up.fp32 and up.field.ctx_kind == 5
    with pytest.raises(NotImplementedError, match="no density query"):
        fused.DensityGridUpdater(rig.model, field=SimpleNamespace(ctx_kind=6))


def test_field_refuses_what_the_kernel_is_not_built_for(rig):
    import sdn_backend
    from dnerf_amd import fused_basis
    from dnerf_amd.network_basis import NeRFNetwork
    with pytest.raises(NotImplementedError, match="bg_radius"):
        fused_basis.FusedBasisFieldF32(NeRFNetwork(**{**BS.MODEL_KW, "bg_radius": 1.0}), T)
    with pytest.raises(NotImplementedError, match="architecture"):
        fused_basis.FusedBasisFieldF32(NeRFNetwork(**{**BS.MODEL_KW, "hidden_dim": 32}), T)
    half = NeRFNetwork(**BS.MODEL_KW)
    half.encoder.embeddings.data = half.encoder.embeddings.data.half()
    with pytest.raises(sdn_backend.SdnError, match="fp32 embedding table"):
        fused_basis.FusedBasisFieldF32(half, T)
    assert NeRFNetwork.fused_inference_f32 is False
