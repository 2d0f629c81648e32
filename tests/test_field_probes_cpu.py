"""tests/field_probe_support.py proves its method without a GPU: under the probe weights the CPU oracle's field network returns exactly
the stage value the probe claims to read (so the pass-through is exact through `_mlp`'s roundings and every builder addresses the
column it names), the point sets hit what they are built for (index arithmetic alone), and every bar rejects a named wrong variant of
the stage it guards.  The full 6.1 M-row table is used; the tests sample fewer points than the GPU file instead."""
import numpy as np
import pytest

from oracle.field import FieldOracle

import field_probe_support as P


@pytest.fixture(scope="module")
def kit():
    geo = P.Geometry(1)
    table = P.random_table(geo)
    x, sets = P.point_sets(geo, n_uniform=384)
    return dict(geo=geo, table=table, x=x, sets=sets, f_ref=P.oracle_features(geo, x, table), dirs=P.unit_dirs(n_random=48))


def _bits(a):
    return np.asarray(a, np.float16).view(np.uint16)


def test_restatement_is_the_oracle_and_point_sets_cover_what_they_name(kit):
    geo, x, table = kit["geo"], kit["x"], kit["table"]
    assert np.array_equal(_bits(P.grid_features(geo, geo.u_of(x), table)), _bits(kit["f_ref"]))
    t32 = table.astype(np.float32)
    assert np.array_equal(P.grid_features(geo, geo.u_of(x), t32), P.oracle_features(geo, x, t32))
    rep = P.assert_coverage(geo, x, kit["sets"], kit["f_ref"])
    assert set(geo.capped) <= set(rep) and rep["small_share"] <= P.MAX_SMALL_SHARE
    # out-of-range points read the zero-feature value; the point one float32 step above +bound is in range (u == 1)
    assert not kit["f_ref"][kit["sets"]["outside"]].any() and kit["f_ref"][kit["sets"]["edge_in"]].all(1).all()
    feats = P.variant_features(geo)
    assert len(feats) == 8 and {f & 1 for f in feats} == {0, 1} and {f >> 1 for f in feats} >= {0, geo.capped[0], 15}
    # a second geometry: bound = 2
    g2 = P.Geometry(2)
    x2, s2 = P.point_sets(g2, n_uniform=128)
    P.assert_coverage(g2, x2, s2, P.oracle_features(g2, x2, P.random_table(g2)))
    assert (g2.u_of(x2) != ((x2 + 1) / 2).astype(np.float32)).any()


@pytest.mark.parametrize("mode", ["fp16", "fp32"])
def test_grid_probe_reads_out_exactly_the_feature(kit, mode):
    geo, x = kit["geo"], kit["x"]
    table = kit["table"] if mode == "fp16" else kit["table"].astype(np.float32)
    f_ref = P.oracle_features(geo, x, table)
    st = P.blank_state(geo, kit["table"])
    d = np.tile(np.array([[0, 0, 1]], np.float32), (x.shape[0], 1))
    for j in (0, 1, 2 * geo.capped[0] + 1, 17, 31):
        P.set_grid_probe(st, j)
        for t in (0.0, 0.5):
            sigma, _, deform = FieldOracle(st, mode=mode).forward(x, d, t)
            assert not deform.any()
            assert np.array_equal(sigma, np.exp(f_ref[:, j].astype(np.float32)).astype(np.float32)), (j, t)
            if mode == "fp16":
                ok, stats = P.grid_bar_f16(sigma, f_ref[:, j])      # (float32 exp of the oracle: inside the decode bar as well)
            else:
                ok, stats = P.grid_bar_f32(sigma, f_ref[:, j], P.F32_BAR["mfma32"])
            assert ok.all(), stats


@pytest.mark.parametrize("mode", ["fp16", "fp32"])
def test_wiring_probe_reads_out_the_colour_nets_inputs(kit, mode):
    geo, sets, half = kit["geo"], kit["sets"], mode == "fp16"
    x = kit["x"][sets["uniform"][:kit["dirs"].shape[0]]]
    d = kit["dirs"]
    table = kit["table"] if half else kit["table"].astype(np.float32)
    cin = P.colour_inputs(d, P.oracle_features(geo, x, table), half)
    assert cin.shape == (d.shape[0], 31)
    st = P.blank_state(geo, kit["table"])
    for inputs in P.WIRING_LAUNCHES:
        P.set_wiring_probe(st, inputs)
        _, rgb, _ = FieldOracle(st, mode=mode).forward(x, d, 0.0)
        want, logit = P.expected_rgb(cin, inputs, half)
        assert np.array_equal(rgb, want.astype(np.float32)), inputs
        if half:
            assert (np.abs(rgb - want) <= P.rgb_bar_f16(want, logit, inputs)).all()


def _deform_case(kit, cols, t):
    geo, x = kit["geo"], kit["x"][kit["sets"]["uniform"]]
    enc = P.deform_inputs(x, t)[:, list(cols)]
    st = P.set_deform_probe(P.set_grid_probe(P.blank_state(geo, P.ramp_table(geo, 0)), 0), cols)
    return geo, x, enc, st


@pytest.mark.parametrize("cols,t", [((0, 1, 2), 0.5), ((3, 7, 62), 0.5), ((63, 64, 75), 0.37), ((4, 69, 30), 0.0)])
def test_deform_probe_reads_out_the_deformed_coordinate(kit, cols, t):
    geo, x, enc, st = _deform_case(kit, cols, t)
    d = np.tile(np.array([[0, 0, 1]], np.float32), (x.shape[0], 1))
    for axis in range(3):
        table = P.ramp_table(geo, axis)
        st["encoder.embeddings"] = table.astype(np.float32)
        sigma, _, deform = FieldOracle(st, mode="fp16").forward(x, d, t)
        xd = x if t == 0.0 else P.deformed_points_f16(x, enc)
        if t != 0.0:
            assert np.array_equal(deform.astype(np.float32), (np.float32(P.DEFORM_G) * enc.astype(np.float16).astype(np.float32)).astype(np.float16).astype(np.float32))
        want = P.oracle_features(geo, xd, table)[:, 0]
        assert np.array_equal(sigma, np.exp(want.astype(np.float32)).astype(np.float32)), (cols, axis)
        # the ramp reads the coordinate: feature 0 = (u scale + 0.5) / 16 within the fp16 trilinear arithmetic's 8 x 2^-11
        u = geo.u_of(xd)[:, axis]
        inside = ((geo.u_of(xd) >= 0) & (geo.u_of(xd) <= 1)).all(1)
        assert np.abs(want.astype(np.float64) - (u * 15.0 + 0.5) / 16.0)[inside].max() <= 8 * 2.0 ** -11
        if t != 0.0 and axis == 0:
            assert (~inside).any() and not want[~inside].any()       # the deformation alone carries some points out: zero features
    # fp32 network: deform is g * enc in float32
    st["encoder.embeddings"] = P.ramp_table(geo, 0).astype(np.float32)
    _, _, deform = FieldOracle(st, mode="fp32").forward(x, d, t)
    assert np.array_equal(deform, np.zeros_like(x) if t == 0.0 else (np.float32(P.DEFORM_G) * enc).astype(np.float32))


# ---- every bar rejects its named wrong variants ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["swap_x", "clamp", "no_zero", "ge1", "swap_ch", "one_round", "scale_no_m1"])
def test_grid_bar_rejects_a_wrong_grid_stage(kit, variant):
    """The wrong kernel's features as an exact sigma = exp(feature) (no decode error at all in its favour), at ONE level only, read through
    that level's two probes: the bar must fail -- for the coarsest capped level, level 15 and (where the variant exists there) level 0."""
    geo, x, f_ref = kit["geo"], kit["x"], kit["f_ref"]
    for l in (0, geo.capped[0], 15):
        if variant == "clamp" and not geo.levels[l]["capped"]:
            continue                  # a dense level never wraps
        wrong = P.grid_features(geo, geo.u_of(x), kit["table"], variant, l)
        for bar in ("f16", "mfma32", "split"):
            failed = 0
            for j in (2 * l, 2 * l + 1):
                if bar == "f16":
                    ok, _ = P.grid_bar_f16(np.exp(wrong[:, j].astype(np.float64)), f_ref[:, j])
                else:
                    t32 = kit["table"].astype(np.float32)
                    w32 = P.grid_features(geo, geo.u_of(x), t32, variant, l)
                    ok, _ = P.grid_bar_f32(np.exp(w32[:, j].astype(np.float64)), P.oracle_features(geo, x, t32)[:, j], P.F32_BAR[bar])
                failed += int((~ok).sum())
            if variant == "one_round" and bar != "f16":
                assert failed == 0    # (the fp32 arithmetic has one rounding per operation: the variant does not exist there)
            else:
                assert failed > 0, (variant, l, bar)
    # ... and the other levels' probes do not see it
    other = P.grid_features(geo, geo.u_of(x), kit["table"], variant, 15)
    assert np.array_equal(_bits(other[:, :30]), _bits(f_ref[:, :30]))


@pytest.mark.parametrize("variant", ["swap_sh", "concat_reversed"])
def test_rgb_bar_rejects_wrong_wiring(kit, variant):
    geo, sets = kit["geo"], kit["sets"]
    d = kit["dirs"]
    x = kit["x"][sets["uniform"][:d.shape[0]]]
    feats = P.oracle_features(geo, x, kit["table"])
    cin, wrong = P.colour_inputs(d, feats, True), P.colour_inputs(d, feats, True, variant)
    cin32, wrong32 = P.colour_inputs(d, feats.astype(np.float32), False), P.colour_inputs(d, feats.astype(np.float32), False, variant)
    hit = 0
    for inputs in P.WIRING_LAUNCHES:
        want, logit = P.expected_rgb(cin, inputs, True)
        got, _ = P.expected_rgb(wrong, inputs, True)
        bad = np.abs(got - want) > P.rgb_bar_f16(want, logit, inputs)
        want32, _ = P.expected_rgb(cin32, inputs, False)
        got32, _ = P.expected_rgb(wrong32, inputs, False)
        bad32 = np.abs(got32 - want32) > 2.5e-4 * np.abs(want32) + 1e-6
        moved = [m for m in inputs if variant == "concat_reversed" or m in (4, 5)]
        assert bad.any() == bool(moved) and bad32.any() == bool(moved), (inputs, int(bad.sum()))
        hit += bool(moved)
    assert hit >= 1


@pytest.mark.parametrize("variant", ["after_add", "swap_freq"])
def test_deform_bar_rejects_a_wrong_hand_off(kit, variant):
    """dx rounded after the add instead of before; two frequency columns (sin x0 and cos x0: columns 3 and 6) swapped."""
    cols, t = (3, 7, 62), 0.5
    geo, x, enc, _ = _deform_case(kit, cols, t)
    enc_wrong = P.deform_inputs(x, t)[:, [6, 7, 62]] if variant == "swap_freq" else enc
    failed = 0
    for axis in range(3):
        table = P.ramp_table(geo, axis)
        got = P.oracle_features(geo, P.deformed_points_f16(x, enc_wrong, variant="after_add" if variant == "after_add" else None), table)[:, 0]
        ok, stat = P.deform_bar_f16(geo, x, enc, cols, table, np.exp(got.astype(np.float64)))
        assert not ok.all() or (variant == "swap_freq" and axis != 0), axis      # (a wrong dx on x still zeroes points seen through y and z)
        failed += stat["failed"]
    assert failed > 0
    # and the reference itself passes, also with every rounding of enc moved by one fp16 ulp; most points are held bit for bit
    table = P.ramp_table(geo, 0)
    for step in (0, 1, -1):
        near = P.oracle_features(geo, P.deformed_points_f16(x, enc, step=step), table)[:, 0]
        ok, stat = P.deform_bar_f16(geo, x, enc, cols, table, np.exp(near.astype(np.float64)))
        assert ok.all() and stat["strict_share"] > 0.8, stat
