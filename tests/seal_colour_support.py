"""Inputs and yardsticks shared by the seal colour kernels' fixture generator (tests/golden/gen_seal_colour_fixture.py) and their tests
(test_seal_colour_cpu.py, test_gpu_seal_colour.py): the colour sets, modifications and tint targets of seal_colour_edges.npz, its loader,
a step-by-step fp32 statement of csrc/seal.hip's rgb_to_hsv / hsv_to_rgb / k_seal_hsv / SealTint in the kernel's statement order, an
exact integer statement of k_seal_rgb_sum's 2^-40 fixed-point sum, and the masks the launches are tried under.

Everything is vectorised numpy on float32 arrays: every operation below is one correctly rounded fp32 add, multiply, divide, floor or
compare, as in the kernels (the library is built with -ffp-contract=off), so the statement is the kernels' result bit for bit."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seal_colour_edges.npz")

F = np.float32
FIXED_ONE = 2 ** 40            # kSealFixedOne: 1.0 in 2^-40 fixed point
POISON = (np.nan, 3e38)        # what unmasked slots hold: a sum that read one would be NaN or far above any count of colours
RGB_BAR = 5e-6                 # the project's bar for the fixed-point mean against torch.mean (test_gpu_caller_fixtures.py)

LATTICE_VALUES = np.array([0.0, 1e-40, 2.0 ** -126, 1e-7, 0.25, 0.5, 0.99999994, 1.0], dtype=F)
# hue, saturation, value modifications of modify_hsv.  Rows 2, 3, 7, 10 make hues negative; 8, 9 push h * 6 to 256 and beyond.
MODS = np.array([[0, 0, 0], [0.2, -0.1, 0.05], [-0.3, 0, 0], [-1 / 6, 0, 0], [1 / 6, 0, 0], [0.5, 0, 0], [1, 0, 0], [-0.999, 0.5, 0.5], [5, -2, 0.3],
                 [42.6, 0, 0], [-43, 0, 0]], dtype=F)
NEGATIVE_HUE_MODS = (2, 3, 7, 10)
# modify_rgb's target colours (a colour, a grey, black, white, a tie) and light offsets (-2 and +2 drive the brightness to either clamp)
TARGETS = np.array([[0.2, 0.6, 0.9], [0.5, 0.5, 0.5], [0, 0, 0], [1, 1, 1], [1, 1, 0]], dtype=F)
LIGHT_OFFSETS = (-2.0, 0.0, 0.1, 2.0)
N_RANDOM = 512
LAUNCH_SIZES = (1, 63, 64, 65, 255, 256, 257, 513)


def edge_colours():
    """The sextant boundaries; reds whose green is below their blue by an ulp-scale step (a negative hue before `% 6`) and above it;
    the same around the other two maxima; and colours so dark that their V is no whole number of 2^-40 steps (0.5, 1.5, 2.5, 0.75 of
    one: the fixed-point conversion has to round them, halves upwards)."""
    one_m = F(0.99999994)
    return np.array([[1, 1, 0], [0, 1, 0], [0, 1, 1], [0, 0, 1], [1, 0, 1],
                     [1, 0, 1e-7], [1, 0, 1e-40], [1, 0, 2.0 ** -126], [1, one_m, 1], [0.5, 0.25, 0.25000003], [1, 1e-7, 0], [1, 1e-40, 0],
                     [one_m, 1, 1], [0, 1, 1e-40], [1e-40, 1, 0], [1e-7, 0, 1], [0, 1e-40, 1], [0.25, 0.25000003, 0.25],
                     [2.0 ** -41, 0, 0], [0, 3 * 2.0 ** -41, 2.0 ** -41], [2.0 ** -42, 0, 5 * 2.0 ** -41], [3 * 2.0 ** -42, 3 * 2.0 ** -42, 0]], dtype=F)


def colour_set():
    """-> float32 [N, 3]: the lattice of all 512 triples over LATTICE_VALUES (red slowest: every tie pattern, the greys, black, white, the
    primaries), `edge_colours`, N_RANDOM seeded uniform colours."""
    v = LATTICE_VALUES
    lattice = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    rnd = np.random.default_rng(20).random((N_RANDOM, 3), dtype=F)
    return np.ascontiguousarray(np.concatenate([lattice, edge_colours(), rnd]).astype(F))


def random_block(colours):
    return colours[-N_RANDOM:]


def constant_v_set():
    """-> float32 [N_RANDOM, 3]: seeded colours whose V = max(r, g, b) is 0.25 on every sample (the maximum moves through the channels)."""
    c = np.random.default_rng(21).random((N_RANDOM, 3), dtype=F) * F(0.25)
    c[np.arange(N_RANDOM), np.arange(N_RANDOM) % 3] = F(0.25)
    return np.ascontiguousarray(c)


def tint_colours(colours, M):
    """The M colours the mask, tail and order tests tint: the edge colours (the dark ones among them) ahead of the random block."""
    return np.ascontiguousarray(colours[len(LATTICE_VALUES) ** 3:][:M])


def load():
    """The fixture as a dict; its inputs must be the ones this module states."""
    fx = dict(np.load(FIXTURE))
    assert bits_equal(fx["colours"], colour_set()) and bits_equal(fx["constant_v"], constant_v_set())
    assert bits_equal(fx["mods"], MODS) and bits_equal(fx["targets"], TARGETS) and bits_equal(fx["light_offsets"], np.array(LIGHT_OFFSETS, dtype=F))
    return fx


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the fp32 statement (csrc/seal.hip) -------------------------------------------------------------------------------------------
def hue_branch(rgb, first_max_wins=True):
    """-> int [N]: which statement of rgb_to_hsv gives the hue: 0 red, 1 green, 2 blue, 3 none (delta == 0).  first_max_wins=False is
    the mutation `r > g`."""
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    delta = np.maximum(r, np.maximum(g, b)) - np.minimum(r, np.minimum(g, b))
    is_r = ((r >= g) if first_max_wins else (r > g)) & (r >= b)
    return np.where(delta == 0, 3, np.where(is_r, 0, np.where(g >= b, 1, 2)))


def rgb_to_hsv(rgb, first_max_wins=True):
    """rgb_to_hsv of float32 [N, 3] -> (h / 6, s, v), each float32 [N]."""
    rgb = np.asarray(rgb, dtype=F)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    cmax, cmin = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    delta = cmax - cmin
    branch = hue_branch(rgb, first_max_wins)
    with np.errstate(divide="ignore", invalid="ignore"):
        hr = (g - b) / delta
        hr = hr - F(6) * np.floor(hr / F(6))
        hg = (b - r) / delta + F(2)
        hb = (r - g) / delta + F(4)
        h = np.where(branch == 3, F(0), np.where(branch == 0, hr, np.where(branch == 1, hg, hb))).astype(F)
        h = h / F(6)
        s = np.where(cmax == 0, F(0), delta / cmax).astype(F)
    return h, s, cmax


def sextant(h, wrap_uint8=True):
    """The table index of hsv_to_rgb for hues h (h / 6 form): ((uint32_t)(uint8_t)(int)(h * 6)) % 6 -- truncation towards zero, then
    modulo 256, then modulo 6.  wrap_uint8=False is the mutation int(h6) % 6."""
    h6 = np.asarray(h, dtype=F) * F(6)
    i = np.trunc(h6).astype(np.int64)
    return ((i & 0xFF) if wrap_uint8 else i) % 6


def hsv_to_rgb(h, s, v, wrap_uint8=True):
    h, s, v = (np.asarray(a, dtype=F) for a in (h, s, v))
    c = v * s
    h6 = h * F(6)
    xx = c * (-np.abs((h6 - F(2) * np.floor(h6 / F(2))) - F(1)) + F(1))
    m = v - c
    idx = sextant(h, wrap_uint8)
    o = np.zeros_like(c)
    table = [(c, xx, o), (xx, c, o), (o, c, xx), (o, xx, c), (xx, o, c), (c, o, xx)]
    out = np.stack([np.choose(idx, [t[k] for t in table]) for k in range(3)], -1).astype(F)
    return out + m[:, None]


def modify_hsv(rgb, mod, **mutation):
    """k_seal_hsv on every colour: rgb -> hsv, + (mh, ms, mv), -> rgb."""
    mod = np.asarray(mod, dtype=F)
    h, s, v = rgb_to_hsv(rgb, mutation.get("first_max_wins", True))
    return hsv_to_rgb(h + mod[0], s + mod[1], v + mod[2], mutation.get("wrap_uint8", True))


def tint(rgb, target, light_offset, mean, **mutation):
    """SealTint on every colour: hue and saturation of the target, brightness min(1, max(0, (mv + (v - mean)) + light_offset))."""
    _, _, v = rgb_to_hsv(rgb, mutation.get("first_max_wins", True))
    mh, ms, mv = rgb_to_hsv(np.asarray(target, dtype=F).reshape(1, 3), mutation.get("first_max_wins", True))
    nv = np.minimum(F(1), np.maximum(F(0), (mv + (v - F(mean))) + F(light_offset)))
    n = nv.shape[0]
    return hsv_to_rgb(np.broadcast_to(mh, n), np.broadcast_to(ms, n), nv, mutation.get("wrap_uint8", True))


def tint_brightness(rgb, target, light_offset, mean):
    """The brightness SealTint hands hsv_to_rgb, before the clamp."""
    _, _, v = rgb_to_hsv(rgb)
    mv = rgb_to_hsv(np.asarray(target, dtype=F).reshape(1, 3))[2]
    return (mv + (v - F(mean))) + F(light_offset)


# ---- the fixed-point sum (k_seal_rgb_sum, seal_mean_v), exact ---------------------------------------------------------------------------
def fixed_v(rgb, round_half=True):
    """seal_rgb_fixed_v of every colour -> Python integers: int(clamp(V, 0, 4) * 2^40 + 0.5), the product and the sum taken in float64
    (both exact there: V has 24 bits, and the result stays below 2^53).  round_half=False is the mutation without the + 0.5."""
    v = np.asarray(rgb, dtype=F).max(1)
    x = np.minimum(np.maximum(v, F(0)), F(4)).astype(np.float64) * float(FIXED_ONE) + (0.5 if round_half else 0.0)
    return np.trunc(x).astype(np.uint64).tolist()


def fixed_sum(rgb, masked=None, round_half=True):
    """-> (sum, count) as Python integers over the colours `masked` selects (all without it)."""
    rgb = np.asarray(rgb, dtype=F)
    if masked is not None:
        rgb = rgb[np.asarray(masked, dtype=bool)]
    if rgb.shape[0] == 0:
        return 0, 0
    return sum(fixed_v(rgb, round_half)), int(rgb.shape[0])


def fixed_mean(total, count):
    """seal_mean_v: float32((sum / 2^40) / count), both divisions in float64 (sum < 2^53 converts exactly)."""
    return F((float(total) / float(FIXED_ONE)) / float(count))


# ---- masks --------------------------------------------------------------------------------------------------------------------------
def masks(M):
    """-> {name: bool [M]} of the launch-shape tests.  `ragged`: one masked slot, in the last wave of the launch (lane (M - 1) % 64
    of a wave whose tail lanes lie beyond M when M is no multiple of 64)."""
    i = np.arange(M)
    return {"all": np.ones(M, bool), "none": np.zeros(M, bool), "every_second": i % 2 == 0, "first": i == 0, "last": i == M - 1,
            "lane0": i % 64 == 0, "lane63": i % 64 == 63, "ragged": i == (M - 1) // 64 * 64 + ((M - 1) % 64) // 2}


def poisoned(colours, masked):
    """colours [M, 3] with NaN and 3e38 by turns in the slots that are not masked -> float32 [M, 3]."""
    out = np.array(colours, dtype=F)
    hole = np.nonzero(~masked)[0]
    out[hole] = np.array(POISON, dtype=F)[hole % 2][:, None]
    return out
