"""The per-sample colour kernels of csrc/seal.hip on the GPU -- k_seal_hsv (`sdn_seal_modify_hsv`), k_seal_image_texels
(`sdn_seal_image_texels`), k_seal_rgb_sum and k_seal_apply<false, SealTint> (`sdn_seal_modify_rgb`), and the rgb_to_hsv / hsv_to_rgb
helpers they share -- against what the reference's own modify_hsv, rgb2hsv_torch and modify_rgb produced on the CPU
(tests/golden/seal_colour_edges.npz, data only) and against the fp32 and integer statements of tests/seal_colour_support.py, which
tests/test_seal_colour_cpu.py holds to that fixture.

Bars.  The library is built with -ffp-contract=off and every operation of these kernels is one correctly rounded fp32 operation, so
hue shifts and texel conversions equal the reference BIT FOR BIT: ties between channels, greys, black, subnormal channels, hues made
negative (truncated towards zero, wrapped modulo 256, then modulo 6) and hues with h * 6 >= 256 included.  The tint's {sum, count}
pair read back from the scratch equals the integer statement exactly, its colours equal the fp32 statement fed with that mean bit for
bit, and they stay within the project's 5e-6 of the reference, whose mean is torch.mean's.  Unmasked slots and slots beyond the call hold
NaN and 3e38: they keep their bits, and a sum that read one would not equal the integer statement."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import seal_colour_support as CS  # noqa: E402

SDN_E_BADARG = -1
GUARD = 4                       # slots beyond the call's M: poisoned, their mask bytes SET -- a lane that ran past M would recolour them
SENTINEL = 0x5A5A5A5A5A5A5A5A   # what the scratch holds before a call: a call that runs clears it


@pytest.fixture(scope="module")
def fx():
    return CS.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _buffers(colours, masked):
    """colours [M,3] and a bool mask [M] -> device colours [M + GUARD, 3] (poison outside the mask and beyond M), device mask bytes
    [M + GUARD] (set beyond M), and the host copy of the colours as uploaded."""
    M = masked.shape[0]
    full = np.concatenate([masked, np.zeros(GUARD, bool)])
    host = CS.poisoned(np.concatenate([colours, np.zeros((GUARD, 3), CS.F)]), full)
    mask = np.concatenate([masked, np.ones(GUARD, bool)]).astype(np.uint8)
    assert host.shape[0] == M + GUARD
    return _dev(host), _dev(mask), host


def _scratch():
    return torch.full((2,), SENTINEL, dtype=torch.int64, device="cuda")


def _hsv(cols, mask, M, mod):
    from sdn_backend import lib, ptr, stream
    return lib.sdn_seal_modify_hsv(ptr(cols), ptr(mask), M, float(mod[0]), float(mod[1]), float(mod[2]), stream())


def _tint(cols, mask, M, target, offset, scratch, live_idx=None, live_count=None):
    from sdn_backend import lib, ptr, stream
    return lib.sdn_seal_modify_rgb(ptr(cols), ptr(mask), M, float(target[0]), float(target[1]), float(target[2]), float(offset), ptr(scratch),
                                   ptr(live_idx), ptr(live_count), None, stream())


def _assert_bits(got, want, inputs, what):
    """Bit equality; on a difference, the count, the largest distance and the input where it occurs."""
    if CS.bits_equal(got, want):
        return
    bad = np.nonzero((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(-1))[0]
    dist = np.abs(got[bad].astype(np.float64) - want[bad].astype(np.float64)).max(-1)
    worst = bad[int(np.nanargmax(dist))] if not np.isnan(dist).all() else bad[0]
    raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} rows differ in their bits; largest distance {np.nanmax(dist) if not np.isnan(dist).all() else np.nan} "
                         f"at row {worst}: input {inputs[worst].tolist()} got {got[worst].tolist()} want {want[worst].tolist()}")


# ---- sdn_seal_modify_hsv ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CS.MODS)))
def test_hue_shift_equals_the_reference_bit_for_bit(fx, k):
    colours = fx["colours"]
    N = colours.shape[0]
    cols, mask, _ = _buffers(colours, np.ones(N, bool))
    assert _hsv(cols, mask, N, CS.MODS[k]) == 0
    got = cols.cpu().numpy()
    _assert_bits(got[:N], fx["modify_hsv"][k], colours, f"modify_hsv {CS.MODS[k].tolist()}")
    assert CS.bits_equal(got[:N], CS.modify_hsv(colours, CS.MODS[k]))


def _spread(N, M):
    """M rows of the colour set: from the edge colours on, every second one, wrapping into the lattice."""
    return (len(CS.LATTICE_VALUES) ** 3 + 9 + 2 * np.arange(M)) % N


@pytest.mark.parametrize("M", CS.LAUNCH_SIZES)
def test_hue_shift_launch_sizes_and_masks(fx, M):
    rows = _spread(fx["colours"].shape[0], M)
    colours = fx["colours"][rows]
    for j, (name, masked) in enumerate(CS.masks(M).items()):
        k = (1, 2, 7, 9)[j % 4]
        cols, mask, host = _buffers(colours, masked)
        assert _hsv(cols, mask, M, CS.MODS[k]) == 0
        got = cols.cpu().numpy()
        _assert_bits(got[:M][masked], fx["modify_hsv"][k][rows][masked], colours[masked], f"M {M} mask {name}")
        keep = np.concatenate([~masked, np.ones(GUARD, bool)])
        assert CS.bits_equal(got[keep], host[keep]), (M, name)           # unmasked slots and the slots beyond M keep their bits


def test_hue_shift_of_no_slots_touches_nothing(fx):
    cols, mask, host = _buffers(fx["colours"][:64], np.ones(64, bool))
    assert _hsv(cols, mask, 0, CS.MODS[1]) == 0
    torch.cuda.synchronize()
    assert CS.bits_equal(cols.cpu().numpy(), host)


# ---- sdn_seal_image_texels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, None])
def test_texel_conversion_equals_the_reference_bit_for_bit(fx, n):
    from sdn_backend import lib, ptr, stream
    N = fx["colours"].shape[0]
    rows = np.arange(N) if n is None else _spread(N, n)
    n = rows.shape[0]
    alpha = (np.arange(n) / max(n - 1, 1)).astype(CS.F)                  # distinct, 0 first, 1 last
    assert np.unique(alpha).size == n and alpha[0] == 0 and (n == 1 or alpha[-1] == 1)
    host = np.concatenate([np.concatenate([fx["colours"][rows], alpha[:, None]], 1), np.array([[0.3, 0.6, 0.9, 0.5]], dtype=CS.F)])
    texels = _dev(host)
    assert lib.sdn_seal_image_texels(ptr(texels), n, stream()) == 0
    got = texels.cpu().numpy()
    _assert_bits(got[:n, :3], fx["rgb2hsv"][rows], fx["colours"][rows], f"texels n {n}")
    assert CS.bits_equal(got[:n, 3], alpha)
    assert CS.bits_equal(got[n], host[n])                                # the slot after the last one
    assert lib.sdn_seal_image_texels(ptr(texels), 0, stream()) == 0


# ---- sdn_seal_modify_rgb ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", range(len(CS.TARGETS)))
def test_tint_equals_the_statements_and_stays_near_the_reference(fx, t):
    """Every pairing of target and light offset, on the seeded colours and on the constant-V set.  The bar against the reference is
    5e-6 (the fixed-point mean against torch.mean); measured on an MI355X: 1.2e-7 for the target (0.2, 0.6, 0.9), 6.0e-8 for the grey,
    black, white and tied targets -- one ulp of the mean carried into a colour."""
    worst = 0.0
    for name, colours in (("random", CS.random_block(fx["colours"])), ("constant_v", fx["constant_v"])):
        M = colours.shape[0]
        total, count = CS.fixed_sum(colours)
        mean = CS.fixed_mean(total, count)
        for o, off in enumerate(CS.LIGHT_OFFSETS):
            cols, mask, host = _buffers(colours, np.ones(M, bool))
            scratch = _scratch()
            assert _tint(cols, mask, M, CS.TARGETS[t], off, scratch) == 0
            got = cols.cpu().numpy()
            assert scratch.cpu().tolist() == [total, count], (name, off)
            _assert_bits(got[:M], CS.tint(colours, CS.TARGETS[t], off, mean), colours, f"tint {name} target {CS.TARGETS[t].tolist()} offset {off}")
            assert CS.bits_equal(got[M:], host[M:])
            want = fx[f"modify_rgb_{name}"][t, o]
            err = float(np.abs(got[:M].astype(np.float64) - want).max())
            worst = max(worst, err)
            assert err <= CS.RGB_BAR, (name, off, err)
            if name == "constant_v":                                     # brightness minus mean is exactly zero: the reference's bits
                assert CS.bits_equal(got[:M], want), off
    print("tint target", CS.TARGETS[t].tolist(), "largest distance from the reference", worst)


@pytest.mark.parametrize("M", CS.LAUNCH_SIZES)
def test_tint_masks_and_tails(fx, M):
    colours = CS.tint_colours(fx["colours"], M)
    for j, (name, masked) in enumerate(CS.masks(M).items()):
        target, off = CS.TARGETS[j % len(CS.TARGETS)], CS.LIGHT_OFFSETS[1 + j % 2]
        cols, mask, host = _buffers(colours, masked)
        scratch = _scratch()
        assert _tint(cols, mask, M, target, off, scratch) == 0
        got = cols.cpu().numpy()
        total, count = CS.fixed_sum(colours, masked)
        assert scratch.cpu().tolist() == [total, count], (M, name)       # poison outside the mask and beyond M never enters the sum
        assert count == int(masked.sum())
        if name == "none" or count == 0:
            assert (total, count) == (0, 0) and CS.bits_equal(got, host), (M, name)
            continue
        if name == "lane63":
            assert count == M // 64                                      # one sample per whole wave, each carried from lane 63 to lane 0
        mean = CS.fixed_mean(total, count)
        if name in ("first", "last", "ragged"):
            assert count == 1 and mean == colours[masked][0].max()       # the sample's own V
        _assert_bits(got[:M][masked], CS.tint(colours[masked], target, off, mean), colours[masked], f"M {M} mask {name}")
        keep = np.concatenate([~masked, np.ones(GUARD, bool)])
        assert CS.bits_equal(got[keep], host[keep]), (M, name)


def test_tint_of_no_slots_touches_nothing(fx):
    cols, mask, host = _buffers(fx["colours"][:64], np.ones(64, bool))
    scratch = _scratch()
    assert _tint(cols, mask, 0, CS.TARGETS[0], 0.1, scratch) == 0
    torch.cuda.synchronize()
    assert CS.bits_equal(cols.cpu().numpy(), host) and scratch.cpu().tolist() == [SENTINEL, SENTINEL]


def _spread_slots(colours, n_slots, extra_listed, seed):
    """The colours spread over n_slots slots, poison between them -> (colours [n_slots,3], mask, the slot of every colour (unsorted), a
    list of those slots and of `extra_listed` unmasked ones, shuffled)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n_slots)
    slots, idle = order[:colours.shape[0]], order[colours.shape[0]:colours.shape[0] + extra_listed]
    masked = np.zeros(n_slots, bool)
    masked[slots] = True
    spread = np.zeros((n_slots, 3), CS.F)
    spread[slots] = colours
    listed = np.concatenate([slots, idle])
    return spread, masked, slots, listed[rng.permutation(listed.shape[0])] if extra_listed else slots


def test_tint_does_not_depend_on_the_order_of_the_samples(fx):
    colours = CS.tint_colours(fx["colours"], 513)
    target, off = CS.TARGETS[0], 0.1
    total, count = CS.fixed_sum(colours)
    assert CS.fixed_sum(colours, round_half=False) != (total, count)     # the set holds colours the fixed-point conversion has to round
    # slot order
    cols, mask, _ = _buffers(colours, np.ones(513, bool))
    s0 = _scratch()
    assert _tint(cols, mask, 513, target, off, s0) == 0
    in_order = cols.cpu().numpy()[:513]
    # a seeded permutation
    perm = np.random.default_rng(9).permutation(513)
    cols, mask, _ = _buffers(colours[perm], np.ones(513, bool))
    s1 = _scratch()
    assert _tint(cols, mask, 513, target, off, s1) == 0
    permuted = cols.cpu().numpy()[:513]
    # spread over 1024 slots, listed unsorted, the count on the device
    spread, masked, slots, listed = _spread_slots(colours, 1024, 0, 10)
    assert (np.diff(listed) < 0).any()
    cols, mask, host = _buffers(spread, masked)
    s2 = _scratch()
    assert _tint(cols, mask, 1024, target, off, s2, _dev(listed.astype(np.int32)), _dev(np.array([513], np.int32))) == 0
    listed_out = cols.cpu().numpy()
    assert s0.cpu().tolist() == s1.cpu().tolist() == s2.cpu().tolist() == [total, count]
    assert CS.bits_equal(permuted, in_order[perm]) and CS.bits_equal(listed_out[slots], in_order)
    keep = np.concatenate([~masked, np.ones(GUARD, bool)])
    assert CS.bits_equal(listed_out[keep], host[keep])
    _assert_bits(in_order, CS.tint(colours, target, off, CS.fixed_mean(total, count)), colours, "tint in slot order")


@pytest.mark.parametrize("live", [300, 513])
def test_tint_takes_its_mean_over_the_live_list_only(fx, live):
    """The mean is that of the first `live` listed slots (the masked ones among them).  Nothing is claimed about masked slots outside
    the list: k_seal_apply tints them, by design, by the same mean."""
    colours = CS.tint_colours(fx["colours"], 513)
    target, off = CS.TARGETS[4], 0.0
    spread, masked, slots, listed = _spread_slots(colours, 1024, 64, 11)
    head = listed[:live]
    in_list = np.zeros(1024, bool)
    in_list[head] = True
    assert 0 < int((in_list & ~masked).sum()) and int((in_list & masked).sum()) < 513    # poisoned slots are listed; masked ones are left out
    total, count = CS.fixed_sum(spread, in_list & masked)
    assert (total, count) != CS.fixed_sum(colours)
    cols, mask, host = _buffers(spread, masked)
    scratch = _scratch()
    assert _tint(cols, mask, 1024, target, off, scratch, _dev(listed.astype(np.int32)), _dev(np.array([live], np.int32))) == 0
    got = cols.cpu().numpy()
    assert scratch.cpu().tolist() == [total, count]
    sel = in_list & masked
    _assert_bits(got[:1024][sel], CS.tint(spread[sel], target, off, CS.fixed_mean(total, count)), spread[sel], f"live count {live}")
    keep = np.concatenate([~masked, np.ones(GUARD, bool)])
    assert CS.bits_equal(got[keep], host[keep])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_tint_refuses_an_unaligned_scratch_and_a_list_without_its_count(fx):
    from sdn_backend import lib, ptr, stream
    colours = CS.tint_colours(fx["colours"], 65)
    cols, mask, host = _buffers(colours, np.ones(65, bool))
    scratch = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
    live_idx = _dev(np.arange(65, dtype=np.int32))
    t = [float(v) for v in CS.TARGETS[0]]
    for off in (1, 4):
        assert lib.sdn_seal_modify_rgb(ptr(cols), ptr(mask), 65, t[0], t[1], t[2], 0.1, scratch.data_ptr() + off, None, None, None, stream()) == SDN_E_BADARG
    assert lib.sdn_seal_modify_rgb(ptr(cols), ptr(mask), 65, t[0], t[1], t[2], 0.1, ptr(scratch), ptr(live_idx), None, None, stream()) == SDN_E_BADARG
    torch.cuda.synchronize()
    # nothing ran: the colours keep their bits, the scratch was not cleared
    assert CS.bits_equal(cols.cpu().numpy(), host) and scratch.cpu().tolist() == [SENTINEL] * 4
    # (8 bytes into the same buffer is aligned: the call runs)
    assert lib.sdn_seal_modify_rgb(ptr(cols), ptr(mask), 65, t[0], t[1], t[2], 0.1, scratch.data_ptr() + 8, None, None, None, stream()) == 0
    total, count = CS.fixed_sum(colours)
    assert scratch.cpu().tolist() == [SENTINEL, total, count, SENTINEL]


# ---- dispatch ----------------------------------------------------------------------------------------------------------------------------
def test_map_color_on_the_device_and_on_the_cpu_agree(fx):
    from dnerf_amd.seal_mapper import SealBBoxMapper
    from test_caller_fixtures_cpu import SEAL_CONFIG
    box = {k: v for k, v in SEAL_CONFIG.items() if k != "hsv"}
    head = fx["colours"][:64]
    masked = np.arange(64) % 5 != 3
    host = CS.poisoned(head, masked)
    # an `hsv` mapper: bit for bit, and the reference's bits
    hsv = SealBBoxMapper(dict(box, hsv=[-0.3, 0.0, 0.0]))
    assert CS.bits_equal(np.array([-0.3, 0.0, 0.0], dtype=CS.F), CS.MODS[2])
    gpu = hsv.map_color_(_dev(host), _dev(masked)).cpu().numpy()
    cpu = SealBBoxMapper(dict(box, hsv=[-0.3, 0.0, 0.0])).map_color_(torch.from_numpy(host.copy()), torch.from_numpy(masked)).numpy()
    _assert_bits(gpu, cpu, host, "map_color_ hsv, device against cpu")
    assert CS.bits_equal(gpu[masked], fx["modify_hsv"][2][:64][masked]) and CS.bits_equal(gpu[~masked], host[~masked])
    # an `rgb` mapper: the fixed-point mean against torch.mean
    cfg = dict(box, rgb=[0.2, 0.6, 0.9], rgbLightOffset=0.1)
    gpu = SealBBoxMapper(cfg).map_color_(_dev(host), _dev(masked)).cpu().numpy()
    cpu = SealBBoxMapper(cfg).map_color_(torch.from_numpy(host.copy()), torch.from_numpy(masked)).numpy()
    err = float(np.abs(gpu[masked].astype(np.float64) - cpu[masked]).max())
    print("map_color_ rgb, device against cpu: largest difference", err)
    assert err <= CS.RGB_BAR and CS.bits_equal(gpu[~masked], host[~masked]) and CS.bits_equal(cpu[~masked], host[~masked])
    mean = CS.fixed_mean(*CS.fixed_sum(head, masked))
    _assert_bits(gpu[masked], CS.tint(head[masked], CS.TARGETS[0], 0.1, mean), head[masked], "map_color_ rgb against the statement")
