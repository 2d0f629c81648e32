"""tests/field_range_support.py without a GPU: the rescaling is exact, the float64 reference is finite where the GPU tests hold a bar and
non-finite only where the cases say so, every set of points the GPU tests name comes from the probes' construction, the split packer
refuses a weight it cannot hold, the subnormal table is what it claims to be, and each bar rejects the wrong kernel it exists for."""
import types

import numpy as np
import pytest
import torch

import field_probe_support as P
import field_range_support as R


@pytest.fixture(scope="module")
def rig():
    geo = P.Geometry(1)
    x, d = R.a_points(geo)
    return dict(geo=geo, table=R.a_table(geo), x=x, d=d)


ALL_A = sorted(set(R.A_INSIDE + R.A_BELOW + (R.A_ABOVE,)))


@pytest.mark.parametrize("stage", R.A_STAGES)
def test_the_rescaling_leaves_the_float64_network_unchanged(rig, stage):
    """Every probe state and every k used (the split kernel's cases with at most 2^7 per weight, the fp32-MFMA kernel's without a cap):
    identical outputs to the same probe at k = 0, and the operand entering the stage has the magnitude the case names on the target
    points (x0 = 1 for the D stages, x0 > 0 for S1 and C1) and 0.75 .. 0.94 of it elsewhere."""
    g = rig
    for cap, values in ((R.CAP, ALL_A), (None, R.A_MFMA32)):
        for a in values:
            st, L = R.a_state(stage, a, cap)
            ref = R.forward64(st, g["geo"], g["table"], g["x"], g["d"])
            twin = R.forward64(R.a_twin(stage, a, cap)[0], g["geo"], g["table"], g["x"], g["d"])
            assert np.array_equal(ref["sigma"], twin["sigma"]) and np.array_equal(ref["rgb"], twin["rgb"]), (stage, a)
            assert np.isfinite(ref["sigma"]).all() and np.isfinite(ref["rgb"]).all(), (stage, a)
            op = ref["operand"][L]
            target = g["x"][:, 0] == 1 if stage[0] == "D" else g["x"][:, 0] > 0
            assert np.allclose(op[target], a, rtol=2e-7, atol=0) and (op[~target] <= 0.95 * a).all() and (op[~target] >= 0.74 * a).all(), (stage, a)
            k = R.k_and_mantissa(a)[0]
            if k:                                      # the twin's operand is the mantissa: the cases differ in the operand alone
                assert np.allclose(twin["operand"][L] * 2.0 ** k, op, rtol=1e-12, atol=0)
            if cap is not None:                        # every packed weight inside what 2^8 w in fp16 can hold
                top = max(float(np.abs(st[R.KEY[l]][:, :63] if l == "D0" else st[R.KEY[l]]).max()) for l in R.LAYERS)
                assert top <= R.W_HI, (stage, a, top)
            if R.reads_sigma(stage, a):
                assert ref["sigma"].max() > 5.0 and np.ptp(ref["sigma"]) > 1.0, (stage, a)
            assert np.ptp(ref["rgb"][:, 0]) > 0.01 or stage[0] == "D", (stage, a)


@pytest.mark.parametrize("stage", R.A_STAGES)
def test_overflowing_and_sub_envelope_points_come_from_the_construction(rig, stage):
    g = rig
    st, L = R.a_state(stage, R.A_ABOVE)
    ref = R.forward64(st, g["geo"], g["table"], g["x"], g["d"])
    over, inside = R.overflowing(ref, L)
    target = g["x"][:, 0] == 1 if stage[0] == "D" else g["x"][:, 0] > 0
    assert np.array_equal(over, target) and np.array_equal(inside, ~target)
    assert all((v <= R.X_HI).all() for name, v in ref["operand"].items() if name != L)       # nothing else leaves the envelope
    for a in R.A_INSIDE + R.A_BELOW:
        st, L = R.a_state(stage, a)
        ref = R.forward64(st, g["geo"], g["table"], g["x"], g["d"])
        n = R.sub_envelope_terms(ref)
        assert all((v <= R.X_HI * (1 + 1e-6)).all() for v in ref["operand"].values())      # (1023 through an fp32 blend: 1023.0001)
        if a >= 2.0 ** -7:
            assert not n.any(), (stage, a)
        elif a == 2.0 ** -8:                            # the target points just inside, the others (0.75 a) just below: one term
            assert not n[target].any() and (n[~target] == 1).all(), (stage, a)
        else:
            assert (n >= 1).all() and n.max() <= 2, (stage, a, n.max())
        ds, dc, _ = R.sub_envelope_bound(st, g["geo"], g["table"], g["x"], g["d"], L, ref)
        assert (ds[n == 0] == 0).all() and (dc[n == 0] == 0).all()


@pytest.mark.parametrize("stage", R.A_STAGES)
def test_the_split_bar_rejects_a_lost_lo_part_inside_the_envelope(rig, stage):
    """A kernel that drops the lo part of the operand entering the stage (2^-11 relative on that term) while inside the envelope fails
    the bar of section A.1 on sigma or rgb; and a clamp at the fp16 maximum instead of the overflow (1100 -> 1023.5) is far outside it."""
    g = rig
    st, L = R.a_state(stage, 1.0)
    ref = R.forward64(st, g["geo"], g["table"], g["x"], g["d"])
    bad = R.forward64(st, g["geo"], g["table"], g["x"], g["d"], perturb=(L, R.SUB_TERM))
    fail_s = np.abs(bad["sigma"].astype(np.float64) - ref["sigma"]) > R.split_bar(ref["sigma"])
    fail_c = np.abs(bad["rgb"] - ref["rgb"]) > R.split_bar(ref["rgb"])
    assert fail_s.any() or fail_c.any(), stage
    clamp = R.forward64(st, g["geo"], g["table"], g["x"], g["d"], perturb=(L, 1023.5 / 1100.0 - 1))
    assert (np.abs(clamp["sigma"].astype(np.float64) - ref["sigma"]) > R.split_bar(ref["sigma"])).any() or \
        (np.abs(clamp["rgb"] - ref["rgb"]) > R.split_bar(ref["rgb"])).any()


def test_weight_cases_stay_inside_both_envelopes(rig):
    g = rig
    for w in R.A_WEIGHTS + (256.0,):
        st = R.weight_state(w)
        ref = R.forward64(st, g["geo"], g["table"], g["x"], g["d"])
        assert np.abs(st[R.KEY["S1"]][0]).max() == w and abs(np.abs(st[R.KEY["S1"]][1]).max() / w - 1) == 5 * 2.0 ** -14
        assert all(((v == 0) | ((v >= R.X_LO) & (v <= R.X_HI))).all() for v in ref["operand"].values()), w
        assert np.isfinite(ref["sigma"]).all() and ref["sigma"].max() > 1.5 and 0.01 < ref["rgb"][:, 0].min() < ref["rgb"][:, 0].max() < 0.5


# ---- the packer -------------------------------------------------------------------------------------------------------------------------------
def _stub(state):
    m = types.SimpleNamespace()
    for net, shapes in P.SHAPES.items():
        setattr(m, net, [types.SimpleNamespace(weight=torch.from_numpy(np.ascontiguousarray(state[f"{net}.{i}.weight"]))) for i in range(len(shapes))])
    return m


def test_split_packer_accepts_255_and_refuses_256():
    """2^8 x 255 = 65280 is an fp16 value; 2^8 x 256 is not: it used to be packed as an infinity.  The refusal names the layer; the
    fp16 packer and the fp32-MFMA packer take the same weights as they are."""
    import sdn_backend
    from dnerf_amd import fused_f32
    for sign in (1.0, -1.0):
        packed = fused_f32.pack_weights_f32_split(_stub(R.weight_state(sign * 255.0)))
        assert np.isfinite(packed.view(np.float16).astype(np.float32)).all()
        assert (np.abs(packed.view(np.float16).astype(np.float32)) == 65280.0).sum() == 2
        with pytest.raises(sdn_backend.SdnError, match="S1"):
            fused_f32.pack_weights_f32_split(_stub(R.weight_state(sign * 256.0)))
    st = R._zero_state()
    st[R.KEY["D3"]][5, 7] = -300.0
    with pytest.raises(sdn_backend.SdnError, match="D3"):
        fused_f32.pack_weights_f32_split(_stub(st))
    st[R.KEY["D3"]][5, 7] = np.inf
    with pytest.raises(sdn_backend.SdnError, match="D3"):
        fused_f32.pack_weights_f32_split(_stub(st))
    assert np.isfinite(fused_f32.pack_weights_f32(_stub(R.weight_state(256.0)))).all()


# ---- section B ------------------------------------------------------------------------------------------------------------------------------------
def test_subnormal_table_values_are_what_they_claim():
    v = np.asarray(R.SUBNORMAL_VALUES, np.float16)
    assert np.array_equal(v.astype(np.float32).astype(np.float16).view(np.uint16), v.view(np.uint16))
    expo = (v.view(np.uint16) >> 10) & 0x1F
    assert expo.tolist() == [1, 1, 0, 0, 0]                      # 1e-4 and 2^-14 normal (the smallest binade), the rest subnormal
    assert v.view(np.uint16).tolist()[1:] == [0x0400, 0x0200, 0x0010, 0x0001]
    assert float(v[0]) == float(np.float16(1e-4)) and 2.0 ** -14 < float(v[0]) < 2.0 ** -13
    assert np.array_equal(R.flush16(v).view(np.uint16), np.where(expo == 0, 0, v.view(np.uint16)))
    geo = P.Geometry(1)
    table = R.b_table(geo)
    assert np.abs(table.astype(np.float32)).max() <= float(np.float16(1e-4))                 # the initialisation's range
    assert float((np.abs(table.astype(np.float32)) < 2.0 ** -14).mean()) > 0.5    # most of a fresh table is subnormal
    x, d, slab = R.b_points(geo)
    f = P.oracle_features(geo, x, table)
    want = v[slab].astype(np.float64)
    # eight equal corners blended in fp16: the value itself to a subnormal ulp or two per rounding
    assert np.abs(f[:, 0].astype(np.float64) - want).max() <= 8 * 2.0 ** -24 + 2.0 ** -10 * want.max()
    assert np.array_equal(f[:, 1], -f[:, 0])
    assert np.isin(f[slab == 4, 0].astype(np.float64), (0.0, 2.0 ** -24)).all() and (f[slab == 4, 0] == 0).any()
    # (2^-24: a corner's product w x 2^-24 rounds to zero in the fp16 blend itself unless its weight exceeds one half)
    assert (np.abs(f[slab == 3, 0].astype(np.float64)) > 0).all()
    for j in R.B_FEATURES:
        kept, _ = R.b_expected(f[:, j])
        flushed, _ = R.b_expected(f[:, j], flush_subnormal_operands=True)
        assert np.isfinite(kept).all() and np.isfinite(flushed).all()
        sub = np.abs(f[:, j].astype(np.float32)) < 2.0 ** -14
        assert (flushed[sub] == 1.0).all() and np.array_equal(flushed[~sub], kept[~sub])
        # "kept" and "flushed" are far apart where it matters: 2^-15 -> exp(0.125) against 1
        big = sub & (np.abs(f[:, j].astype(np.float32)) >= 2.0 ** -16)
        if j < 2:
            assert big.sum() > 50 and (np.abs(kept[big] / flushed[big] - 1) > 0.05).all()


# ---- section C ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
def test_output_stage_reference_overflows_exactly_on_the_named_slabs(half):
    geo = P.Geometry(1)
    table = R.c_table(geo, half)
    x, d, sx, sy = R.c_points(geo)
    dl, cl = R.c_logits(P.oracle_features(geo, x, table), 0)
    want_d = np.asarray(R.C_DENSITY)[sx]
    assert np.abs(dl - want_d).max() <= (0.25 if half else 2e-5)           # fp16: the blend's roundings, two or three ulps of 0.0625
    assert np.abs(cl[:, 0] - np.asarray(R.C_COLOUR)[sy]).max() <= (0.25 if half else 2e-5)
    for scale in R.C_SCALES:
        sigma, rgb = R.c_expected(dl, cl, scale, half)
        inf = np.isinf(sigma)
        named = np.asarray(R.C_INFINITE)[sx]
        if scale == 1.0 and not half:
            assert np.array_equal(inf, named)
        elif scale == 1.0:
            # the fp16 blend leaves a point of the 88.8125 slab up to two fp16 ulps away: 88.6875 is below log(float32 max) = 88.7228,
            # so that point is finite in the fp16 network -- in the reference, and in the kernel that reproduces the blend bit for bit
            odd = inf != named
            assert (want_d[odd] == 88.8).all() and (dl[odd] == 88.6875).all() and odd.mean() < 0.05 and inf[want_d == 88.8].mean() > 0.8
        else:                                   # the same set at 2^-8: the float32 exponential overflows before the scale is applied ...
            assert np.array_equal(inf, np.isinf(R.c_expected(dl, cl, 1.0, half)[0]))
            one_cast = R.c_expected_one_cast(dl, scale)      # ... where one cast at the end would keep 88.8 finite: not the table's reading
            assert np.array_equal(np.isinf(one_cast), want_d == 100.0) and np.allclose(one_cast[~inf], sigma[~inf], rtol=1e-6, atol=1e-44)
        assert np.isfinite(sigma[~inf]).all() and (sigma[want_d == -104.0] < 2.0 ** -126).all() and (sigma[want_d == -87.0] > 0).all()
        assert np.isfinite(rgb).all() and rgb.min() >= 0 and rgb.max() <= 1 and (rgb[:, 1:] == 0.5).all()
        assert rgb[:, 0].min() < 1e-8 and rgb[:, 0].max() > 1 - 1e-8


# ---- the basis and ambient models' probes -------------------------------------------------------------------------------------------------------
def test_four_dimensional_tables_hold_the_same_slabs():
    """The ambient model's 4-D grid: level 0 is dense (17^4 rows), the slabs in x (and y) hold for every ambient coordinate -- the
    subnormal table's feature is its slab's value and the output-stage table's logits are the listed ones."""
    import hyper_support as HS
    geo, g4 = P.Geometry(1), HS.Geometry4(1)
    x, d, slab = R.b_points(geo)
    table = R.b_table(g4, dim=4)
    want = np.asarray(R.SUBNORMAL_VALUES, np.float16)[slab].astype(np.float64)
    for ambient in (0.3, -0.71, 1.0):
        f = HS.oracle_features(g4, g4.u4(x, ambient), table)
        assert np.abs(f[:, 0].astype(np.float64) - want).max() <= 8 * 2.0 ** -24 + 2.0 ** -10 * want.max() and np.array_equal(f[:, 1], -f[:, 0])
        assert float((np.abs(f[:, 31].astype(np.float32)) < 2.0 ** -14).mean()) > 0.5
    x, d, sx, sy = R.c_points(geo)
    dl, cl = R.c_logits(HS.oracle_features(g4, g4.u4(x, 0.3), R.c_table(g4, True, 4)), 2)
    assert np.abs(dl - np.asarray(R.C_DENSITY)[sx]).max() <= 0.25 and np.abs(cl[:, 2] - np.asarray(R.C_COLOUR)[sy]).max() <= 0.25
    assert not cl[:, :2].any()


def test_basis_probes_put_the_logits_on_coefficient_zero():
    """`basis_net_probe` makes the basis model's own row e_0 + e_32 (fp16 and fp32 alike), under which `b_state` / `c_state` of the basis
    model give the logits of the deformation model's probes: the restated model (basis_support.BasisOracle) on both."""
    import basis_support as BS
    geo = P.Geometry(1)
    x, d, sx, sy = R.c_points(geo)
    for half in (True, False):
        table = R.c_table(geo, half)
        st = R.c_state(1, "basis")
        st["encoder.embeddings"], st["encoder.offsets"] = table.astype(np.float32), geo.offsets
        for i, w in enumerate(R.basis_net_probe([(64, 13)] + [(64, 64)] * 3 + [(40, 64)])):
            st[f"basis_net.{i}.weight"] = w
        o = BS.BasisOracle(st, mode="fp16" if half else "fp32")
        assert np.array_equal(o.row(R.T), R.basis_row())
        dl, cl = R.c_logits(P.oracle_features(geo, x, table), 1)
        dens = o.density(x, R.T)
        assert np.array_equal(dens["logit"].astype(np.float64), dl)
        _, cb = o.basis(R.T)
        assert np.array_equal(o.colour_logits(d, dens["geo_feat"], cb).astype(np.float64), cl)
