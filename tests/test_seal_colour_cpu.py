"""The yardsticks of the seal colour kernels' GPU test (tests/seal_colour_support.py) against what the reference's own modify_hsv,
rgb2hsv_torch and modify_rgb produced on the CPU (tests/golden/seal_colour_edges.npz, data only), without a GPU: the fp32 statement of
csrc/seal.hip's rgb_to_hsv / hsv_to_rgb / k_seal_hsv and the torch restatement of dnerf_amd/seal_mapper.py equal the reference BIT FOR
BIT on every colour and modification; the tint statement fed with the exact fixed-point mean stays within the project's 5e-6 of the
reference's torch.mean form and equals it where brightness minus mean is exactly zero; the fixture holds the edges it is for; and three
mutations of the statement each fail an assertion made here."""
import numpy as np
import pytest
import torch

import seal_colour_support as CS


@pytest.fixture(scope="module")
def fx():
    return CS.load()


def _hsv_equals_the_fixture(fx, **mutation):
    return all(CS.bits_equal(CS.modify_hsv(fx["colours"], mod, **mutation), fx["modify_hsv"][k]) for k, mod in enumerate(CS.MODS))


def _branch_is_the_first_maximum(colours, **mutation):
    """rgb2hsv_torch picks its hue statement by torch.max's index, which is that of the FIRST maximum (3: delta == 0)."""
    t = torch.from_numpy(colours)
    first = torch.max(t, dim=1).indices.numpy()
    first = np.where(colours.max(1) == colours.min(1), 3, first)
    return np.array_equal(CS.hue_branch(colours, **mutation), first)


def _negative_hue_lands_in_sextant_3(fx, **mutation):
    """Under (-0.3, 0, 0) some colour has h * 6 in (-2, -1]: truncated to -1, wrapped to 255, 255 % 6 = 3."""
    h, _, _ = CS.rgb_to_hsv(fx["colours"])
    h6 = (h + CS.MODS[2][0]) * CS.F(6)
    there = (h6 > -2) & (h6 <= -1)
    return bool(there.any()) and bool((CS.sextant(h + CS.MODS[2][0], **mutation)[there] == 3).all())


def _halves_round_up(**mutation):
    """0.5, 1.5, 2.5 and 0.75 steps of 2^-40 (the dark edge colours) become 1, 2, 3 and 1 steps."""
    return CS.fixed_v(CS.edge_colours()[-4:], **mutation) == [1, 2, 3, 1]


def test_statement_equals_the_reference_bit_for_bit(fx):
    assert _hsv_equals_the_fixture(fx)
    assert CS.bits_equal(np.stack(CS.rgb_to_hsv(fx["colours"]), -1), fx["rgb2hsv"])
    assert _branch_is_the_first_maximum(fx["colours"])
    # at a tie the two hue statements that could serve give the same bits ((g - b) and delta are one and the same subtraction, so the
    # quotient is exactly +-1): WHICH maximum wins shows in the branch, never in a colour -- of this statement, the reference or the kernel
    assert _hsv_equals_the_fixture(fx, first_max_wins=False)


def test_torch_restatement_equals_the_reference_bit_for_bit(fx):
    from dnerf_amd import seal_mapper as SM
    t = torch.from_numpy(fx["colours"])
    assert CS.bits_equal(SM.rgb2hsv(t).numpy(), fx["rgb2hsv"])
    for k, mod in enumerate(CS.MODS):
        assert CS.bits_equal(SM.modify_hsv(t.clone(), torch.from_numpy(mod.copy())).numpy(), fx["modify_hsv"][k]), mod
        hsv = SM.rgb2hsv(t) + torch.from_numpy(mod.copy()).view(1, 3)
        assert CS.bits_equal(SM.hsv2rgb(hsv).numpy(), fx["modify_hsv"][k]), mod


def test_fixture_holds_its_edges(fx):
    colours = fx["colours"]
    h, _, _ = CS.rgb_to_hsv(colours)
    seen = set()
    for k in CS.NEGATIVE_HUE_MODS:
        moved = h + CS.MODS[k][0]
        seen |= set(CS.sextant(moved)[moved < 0].tolist())
    assert seen == {0, 1, 2, 3, 4, 5}, seen
    assert _negative_hue_lands_in_sextant_3(fx)
    assert bool((((h + CS.MODS[9][0]) * CS.F(6)) >= 256).any())
    # every tie pattern and every hue statement occur, and reds whose hue is negative before `% 6`
    r, g, b = colours[:, 0], colours[:, 1], colours[:, 2]
    assert ((r == g) & (g > b)).any() and ((g == b) & (b > r)).any() and ((r == b) & (b > g)).any() and ((r == g) & (g == b)).any()
    assert set(CS.hue_branch(colours).tolist()) == {0, 1, 2, 3} and ((CS.hue_branch(colours) == 0) & (g < b)).any()
    # both brightness clamps, by the light offsets -2 and +2, on every sample; offsets 0 and 0.1 leave samples between them
    rnd = CS.random_block(colours)
    mean = CS.fixed_mean(*CS.fixed_sum(rnd))
    assert CS.LIGHT_OFFSETS[0] == -2 and CS.LIGHT_OFFSETS[-1] == 2
    assert (CS.tint_brightness(rnd, CS.TARGETS[0], -2.0, mean) < 0).all() and (CS.tint_brightness(rnd, CS.TARGETS[0], 2.0, mean) > 1).all()
    inside = CS.tint_brightness(rnd, CS.TARGETS[0], 0.1, mean)
    assert ((inside > 0) & (inside < 1)).any() and (inside > 1).any()
    assert (CS.tint_brightness(rnd, CS.TARGETS[2], 0.0, mean) < 0).any()
    assert bool((fx["constant_v"].max(1) == CS.F(0.25)).all())


def test_fixed_point_sum_is_exact_and_rounds_halves_up(fx):
    assert _halves_round_up()
    rnd = CS.random_block(fx["colours"])
    total, count = CS.fixed_sum(rnd)
    assert count == CS.N_RANDOM and abs(float(CS.fixed_mean(total, count)) - float(rnd.max(1).astype(np.float64).mean())) < 2.0 ** -24
    order = np.random.default_rng(3).permutation(count)
    assert CS.fixed_sum(rnd[order]) == (total, count)
    assert CS.fixed_sum(fx["constant_v"]) == (CS.N_RANDOM * 2 ** 38, CS.N_RANDOM) and CS.fixed_mean(CS.N_RANDOM * 2 ** 38, CS.N_RANDOM) == CS.F(0.25)
    assert CS.fixed_sum(rnd, np.zeros(count, bool)) == (0, 0)
    one = CS.fixed_sum(rnd[7:8])
    assert CS.fixed_mean(*one) == rnd[7].max()                      # count 1: the mean is the sample's own V
    assert CS.fixed_v(np.array([[9.0, 0, 0], [-1.0, -2.0, -3.0]], dtype=CS.F)) == [4 * 2 ** 40, 0]   # the clamp to [0, 4]


def test_tint_statement_against_the_reference(fx):
    """Fed with the fixed-point mean, within 5e-6 of the reference (whose mean is torch.mean's); on the constant-V set bit-equal."""
    rnd, flat = CS.random_block(fx["colours"]), fx["constant_v"]
    mean_rnd, mean_flat = CS.fixed_mean(*CS.fixed_sum(rnd)), CS.fixed_mean(*CS.fixed_sum(flat))
    worst = 0.0
    for t, target in enumerate(CS.TARGETS):
        for o, off in enumerate(CS.LIGHT_OFFSETS):
            got = CS.tint(rnd, target, off, mean_rnd)
            worst = max(worst, float(np.abs(got.astype(np.float64) - fx["modify_rgb_random"][t, o]).max()))
            assert CS.bits_equal(CS.tint(flat, target, off, mean_flat), fx["modify_rgb_constant_v"][t, o]), (target, off)
            # every sample: hsv_to_rgb of the target with the offset applied
            mh, ms, mv = CS.rgb_to_hsv(target.reshape(1, 3))
            want = CS.hsv_to_rgb(mh, ms, np.minimum(CS.F(1), np.maximum(CS.F(0), mv + CS.F(off))))
            assert CS.bits_equal(fx["modify_rgb_constant_v"][t, o], np.broadcast_to(want, flat.shape))
    print("tint statement with the fixed-point mean against the reference: largest difference", worst)
    assert worst <= CS.RGB_BAR


def test_mutations_of_the_statement_are_caught(fx):
    # the tie rule flipped to `r > g`: fails `_branch_is_the_first_maximum` of test_statement_equals_the_reference_bit_for_bit
    assert not _branch_is_the_first_maximum(fx["colours"], first_max_wins=False)
    # the uint8 wrap replaced by int(h6) % 6: fails `_hsv_equals_the_fixture` there and `_negative_hue_lands_in_sextant_3` of
    # test_fixture_holds_its_edges
    assert not _hsv_equals_the_fixture(fx, wrap_uint8=False)
    assert not _negative_hue_lands_in_sextant_3(fx, wrap_uint8=False)
    # the + 0.5 of the fixed-point rounding dropped: fails `_halves_round_up` of test_fixed_point_sum_is_exact_and_rounds_halves_up
    assert not _halves_round_up(round_half=False)
    tinted = CS.tint_colours(fx["colours"], 65)
    assert CS.fixed_sum(tinted, round_half=False) != CS.fixed_sum(tinted)          # ... and shows in the sums the GPU test reads back
