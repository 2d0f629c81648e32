"""tests/ffmlp_probe_support.py validated without a GPU: (i) every exact case is certified exact at the MI355X's 256 CUs, and every
LDS tile of every weight-gradient split holds a row with a non-zero gradient; (ii) the float32 evaluation of every case in three
summation orders (forward, reversed, pairwise inside blocks of 16 k: the MFMA's shape) gives the reference's bits; (iii) the bitwise
comparison has teeth: six deliberately wrong restatements each change at least one bit on every case family that exercises them;
the launch rule's boundaries and the coverage table hold at several CU counts; the activation references and bars are sane.

The term-by-term float32 evaluation costs B x K x M element operations per layer in numpy, so (ii) and (iii) build the cases at 4 CUs
(every batch rule scales with the CU count) and cap the one rule that does not (`unbatched`, B = 28 929 x 512 inputs) at 2 100 rows;
(i) runs at full size."""
import numpy as np
import pytest

import ffmlp_probe_support as P

SMALL_CUS = 4
NAMES = [s["name"] for s in P.SPECS]


def _small(name):
    s = P.resolve(P.SPEC_BY_NAME[name], SMALL_CUS)
    if s["B"] > 4200:
        s["B"] = 2100
    return s


@pytest.mark.parametrize("name", NAMES)
def test_every_case_is_certified_exact_at_256_cus(name):
    s = P.resolve(P.SPEC_BY_NAME[name], 256)
    c = P.make_case(s)
    r = P.reference(s, c)
    assert r["cert"] < 2.0 ** 24, (name, r["cert"])
    assert all(np.isfinite(r[k].astype(np.float64)).all() for k in ("out", "fwd", "bwd", "gw")), name
    assert P.live_rows_reach_every_tile(s, c), name
    share = float(c["live"].mean())
    assert share >= 1.0 / 64 and np.abs(r["gw"].astype(np.float64)).max() > 0 and np.abs(r["out"].astype(np.float64)).max() > 0, (name, share)
    print(f"[ffmlp-probe] {P.describe(s)} | certificate {r['cert'] / 2.0 ** 24:.2e} of 2^24, live rows {share:.3f}")


@pytest.mark.parametrize("name", NAMES)
def test_three_summation_orders_give_the_reference_bits(name):
    s = _small(name)
    c = P.make_case(s)
    ref = P.reference(s, c)
    assert ref["cert"] < 2.0 ** 24
    for order in ("forward", "reversed", "mfma"):
        got = P.reference(s, c, lin=lambda a, b: P.lin32(a, b, order))
        assert P.results_equal(got, ref), (name, order)


def _exercises(wrong, s):
    """Does the case reach the code the wrong restatement is about?"""
    if wrong == "drop_ragged_tile":
        return s["B"] % P.launch_variant(s["W"], s["in_dim"], s["L"], 1, "forward", s["B"], s["cus"])["points"] != 0
    if wrong == "transpose_dw_block":
        return s["W"] >= 32
    return True


@pytest.mark.parametrize("name", NAMES)
def test_wrong_restatements_fail_the_bitwise_comparison(name):
    s = _small(name)
    c = P.make_case(s)
    ref = P.reference(s, c)
    field = dict(swap_runs="fwd", k_order="out", shift_layers="fwd", drop_ragged_tile="out", drop_split_tail="gw", transpose_dw_block="gw")
    for wrong in P.WRONG:
        if not _exercises(wrong, s):
            continue
        bad = P.reference(s, c, wrong=wrong)
        assert not P.results_equal(bad, ref), (name, wrong)
        assert not P.same_bits(bad[field[wrong]], ref[field[wrong]]), (name, wrong, field[wrong])


@pytest.mark.parametrize("cus", [4, 80, 256, 304])
def test_launch_rule_boundaries_and_coverage(cus):
    for W, L in ((64, 9), (128, 3)):
        kinds = {}
        for rule in ("lat2_max", "lat4_min", "lat4_max", "thr_min"):
            B = P.BATCH_RULES[rule](dict(W=W, in_dim=32, L=L), cus)
            for direction in ("forward", "backward"):
                kinds[rule, direction] = P.launch_variant(W, 32, L, 1, direction, B, cus)["kind"]
        for d in ("forward", "backward"):
            assert [kinds[r, d] for r in ("lat2_max", "lat4_min", "lat4_max", "thr_min")] == ["latency-2", "latency-4", "latency-4", "throughput"], (W, d, kinds)
    v = P.launch_variant(16, 16, 2, 1, "forward", P.resident_capacity(16, 16, 2, cus), cus)
    assert v["kind"] == "resident" and not v["tile_loop"]
    assert P.launch_variant(16, 16, 2, 1, "forward", P.resident_capacity(16, 16, 2, cus) + 1, cus)["tile_loop"]
    missing = P.required() - P.coverage(cus)
    assert not missing, sorted(missing)
    assert P.unreachable(cus) == ["latency-sw-w64", "latency-sw-w128"]       # at every CU count: see P.unreachable


def test_weight_gradient_plan_restates_the_split_sizes():
    assert P.dw_blocks(128, 288) == 3 and P.dw_blocks(16, 256) == 2 and P.dw_blocks(256, 256) == 4
    assert P.dw_splits(257, 1) == 2 and P.dw_splits(1 << 20, 4) == 128 and P.dw_splits(1, 1) == 1
    batched, jobs = P.dw_plan(64, 32, 3, 257)
    assert batched and all(j["used"] == 2 and j["last_rows"] == 65 and j["rows_per_split"] == 192 for j in jobs)
    assert all(j["used"] == 4 and j["last_rows"] == 1 and j["rows_per_split"] == 256 for j in P.dw_plan(64, 32, 2, 769)[1])
    B = P.first_unbatched_batch(256, 512, 2)
    assert P.dw_batched(B - 1, 512, 256, 2) and not P.dw_batched(B, 512, 256, 2)
    assert not P.dw_batched(300, 32, 64, 17)                                  # 18 jobs: layer by layer (and refused by backward)


def test_relu_follows_the_reference_products():
    h = np.array([np.nan, -np.inf, np.inf, -0.0, -3.0, 0.0, 2.0], np.float16)
    y = P.relu_forward(h)
    assert np.isnan(y[0]) and np.isnan(y[1]) and y[2] == np.inf and (y[3:6] == 0).all() and y[6] == 2
    f = np.array([-1.0, 0.0, -1.0, -1.0, np.nan, np.nan, 2.0, 2.0], np.float16)
    g = np.array([5.0, 5.0, np.inf, np.nan, 5.0, np.inf, 5.0, np.inf], np.float16)
    d = P.relu_backward(g, f)
    assert (d[:2] == 0).all() and np.isnan(d[2]) and np.isnan(d[3]) and d[4] == 0 and np.isnan(d[5]) and d[6] == 5 and d[7] == np.inf


def test_non_finite_cases_are_certified_and_carry_every_situation():
    for name in P.NONFINITE:
        s = P.resolve(P.SPEC_BY_NAME[name], 256)
        c = P.make_nonfinite_case(s)
        r = P.reference(s, c)
        assert r["cert"] < 2.0 ** 24
        f0 = r["fwd"][0].astype(np.float64)
        assert np.isnan(f0).any() and np.isposinf(f0).any() and np.isfinite(f0).all(axis=1).sum() > s["B"] // 2
        assert np.isnan(r["bwd"].astype(np.float64)).any() and np.isnan(r["out"].astype(np.float64)).any()
        if s["act"] == "relu":
            assert not np.isneginf(r["fwd"].astype(np.float64)).any()               # -inf never survives a ReLU: it is NaN
            # what a select-ReLU (x > 0 ? x : 0) would store instead differs
            sel = np.where(np.nan_to_num(f0, nan=-1.0) > 0, f0, 0.0)
            assert not np.array_equal(np.isnan(sel), np.isnan(f0))


def test_activation_references_and_bars():
    x = P.all_finite_halves()
    assert x.shape == (3968, 16) and np.unique(x.view(np.uint16)).size == 63488
    for act in ("exponential", "sine", "sigmoid", "squareplus", "softplus"):
        y64, y32 = P.act_forward64(act, x), P.act_forward32(act, x)
        bar = P.forward_bar(act, x, y64)
        assert (bar >= 2.0 ** -24).all()
        if act == "exponential":
            assert np.array_equal(np.isinf(y32), x.astype(np.float64) > np.log(65520.0))
            assert (y32[x.astype(np.float64) < -17.4] == 0).all()
        if act == "softplus":
            assert np.array_equal(np.isinf(y32), x.astype(np.float32) * np.float32(10) > np.float32(88.72284))
    assert P.ulp16(1.0) == 2.0 ** -10 and P.ulp16(0.0) == 2.0 ** -24 and P.ulp16(65504.0) == 32.0
