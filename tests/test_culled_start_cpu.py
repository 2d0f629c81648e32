"""CPU-only checks of the inputs of tests/test_gpu_culled_start.py, on the oracle alone: every ray family is what it claims to be
(finite, direction lengths, zero components of both signs, binade edges inside [near, far]) and holds, on every occupancy it is paired
with, rays that emit samples, rays that emit none and rays whose first sample lies far enough behind the chain's start for the
certified jump to be attempted; the engineered occupancies have the marked boxes they were built for; the numpy restatement of the
cull grid agrees with a brute-force one.  Prints the per-family counts (pytest -s)."""
import numpy as np
import pytest

import culled_start_support as S

PAIRS = [(o, f) for o, f, _ in S.PAIRS]


@pytest.mark.parametrize("noise", S.NOISE_KINDS)
@pytest.mark.parametrize("occ,fam", PAIRS)
def test_family_holds_both_kinds_of_ray_and_jump_candidates(occ, fam, noise):
    c = S.case(occ, fam, noise)
    emits, none = int((c["count"] > 0).sum()), int((c["count"] == 0).sum())
    eligible = int(c["eligible"].sum())
    print(f"{occ:10s} {fam:13s} noises={noise:5s} rays {c['n']:5d}  emit {emits:5d}  none {none:5d}  jump-eligible {eligible:5d}  "
          f"miss-the-cube {int((c['nears'] >= c['fars']).sum()):5d}  max samples {int(c['count'].max())}")
    assert c["n"] <= S.MAX_RAYS
    assert emits >= 16 and none >= 16 and eligible >= 16
    assert int(c["count"].max()) < c["max_steps"]            # the whole ray fits the one oracle call


@pytest.mark.parametrize("occ_name,fam", PAIRS)
def test_family_respects_the_input_contract(occ_name, fam):
    c = S.case(occ_name, fam, "none")
    ro, rd = c["ro"], c["rd"]
    assert ro.dtype == np.float32 and rd.dtype == np.float32 and np.isfinite(ro).all() and np.isfinite(rd).all()
    length = np.linalg.norm(rd.astype(np.float64), axis=1)
    assert length.min() >= 0.5 - 1e-6 and length.max() <= 2 + 1e-6
    assert np.linalg.norm(ro.astype(np.float64), axis=1).max() <= 64
    assert np.isfinite(c["nears"]).all() and np.isfinite(c["fars"]).all()       # FLT_MAX for a miss, never NaN / inf
    if fam == "axis":
        zero = rd == 0
        neg = np.signbit(rd) & zero
        assert int((zero.sum(1) == 2).sum()) >= 256 and int((zero.sum(1) == 1).sum()) >= 256
        assert int(neg.any(1).sum()) >= 256 and int((zero & ~neg).any(1).sum()) >= 256       # -0.0 and +0.0
        # parallel to the marked box within one cull cell outside it, and beyond: both are present among the along-axis rays
        g = c["occ"]["grid"]
        if occ_name != "corners":             # (its marked box is the whole cube: nothing inside the cube lies beside it)
            along = zero.sum(1) == 2
            out = np.maximum(g["box_lo"][None, :] - ro, ro - g["box_hi"][None, :])
            out = np.where(zero, out, -np.inf).max(1)[along]
            assert int(((out > 0) & (out < S.CW)).sum()) >= 16 and int((out > S.CW).sum()) >= 16
    if fam == "grazing":
        zero = rd == 0
        for box in (0, 1):                    # tag = kind + 3 * box; kind 0 = in the plane of a face: both signs of the zero per box
            face = c["tag"] == 3 * box
            assert int((face & (zero & np.signbit(rd)).any(1)).sum()) >= 16 and int((face & (zero & ~np.signbit(rd)).any(1)).sum()) >= 16
    if fam == "unnormalised":
        assert int((np.abs(length - 0.5) < 1e-6).sum()) >= 256 and int((np.abs(length - 2) < 1e-6).sum()) >= 256
    if fam == "crossers":
        for k, edge in enumerate(S.CROSS_EDGES):
            sel = c["tag"] == k
            crosses = sel & (c["nears"] < edge) & (c["fars"] > edge) & (c["nears"] < c["fars"])
            assert int(crosses.sum()) >= 16, (edge, int(crosses.sum()))
            # ... and the edge lies in the empty lead of rays that go on to emit
            assert int((crosses & c["eligible"] & (c["first_t"] > edge)).sum()) >= 4, edge
        inside = np.abs(ro).max(1) < 1
        assert int(inside.sum()) >= 256
        # the edges below 1 from INSIDE the cube (the chain starts at MIN_NEAR) and from outside it at a matching distance: the chain
        # starts in the binade just below the edge, behind it a lead that holds the crossing
        for k in (0, 1, 2):
            edge, sel = S.CROSS_EDGES[k], c["tag"] == k
            assert int((sel & inside).sum()) >= 64
            below = sel & ~inside & (c["nears"] >= edge / 2) & (c["nears"] < edge)
            assert int(below.sum()) >= 64 and int((below & c["eligible"] & (c["first_t"] > edge)).sum()) >= 4, (edge, int(below.sum()))
    if fam == "degenerate":
        dt = float(S.step_of())
        hit = c["nears"] < c["fars"]
        span = c["fars"].astype(np.float64) - c["nears"]
        assert int((hit & (span < 8 * dt)).sum()) >= 16 and int((~hit).sum()) >= 16


def test_noises_hold_zero_the_largest_float_below_one_and_random_values():
    z = S.noises_for(2048, "mixed")
    assert z.dtype == np.float32 and int((z == 0).sum()) >= 512 and int((z == S.ONE_BELOW).sum()) >= 512
    assert float(z.max()) < 1 and len(np.unique(z)) > 512
    assert S.noises_for(7, "none") is None
    near = np.array([0.05, 0.5, 33.0], np.float32)
    assert np.array_equal(S.chain_start(near, None), near)
    t0 = S.chain_start(near, np.array([0, S.ONE_BELOW, 0.5], np.float32))
    assert t0[0] == near[0] and near[1] < t0[1] <= near[1] + S.step_of() and t0[2] > near[2]


def test_engineered_occupancies_have_the_boxes_they_were_built_for():
    ext = {k: tuple(int(v) for v in S.occupancy(k)["grid"]["hi"] - S.occupancy(k)["grid"]["lo"] + 1) for k in S.OCCUPANCIES}
    assert ext["one_voxel"] == (3, 3, 3)
    g = S.occupancy("corners")["grid"]
    assert tuple(g["lo"]) == (0, 0, 0) and tuple(g["hi"]) == (31, 31, 31) and int(g["dil"].sum()) == 16 and not g["fits"]
    assert ext["box16"] == (16, 16, 16) and S.occupancy("box16")["grid"]["fits"] and len(S.occupancy("box16")["grid"]["image"]) == 4096
    assert ext["box17"] == (16, 16, 17) and not S.occupancy("box17")["grid"]["fits"]
    g = S.occupancy("two_slabs")["grid"]
    marked_x = g["dil"].any(axis=(1, 2))
    gap = np.nonzero(~marked_x[g["lo"][0]: g["hi"][0] + 1])[0]
    assert len(gap) >= 8 and g["fits"]
    assert S.occupancy("figure")["grid"]["fits"] and S.occupancy("column")["grid"]["fits"]


@pytest.mark.parametrize("name", ["one_voxel", "corners", "two_slabs"])
def test_cull_grid_restatement_against_brute_force(name):
    o = S.occupancy(name)
    g, occ3 = o["grid"], o["occ3"]
    cells = np.argwhere(occ3) // 4
    want = np.zeros((32, 32, 32), bool)
    for c in np.unique(cells, axis=0):
        lo, hi = np.maximum(c - 1, 0), np.minimum(c + 1, 31)
        want[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    assert np.array_equal(want, g["dil"])
    for cx, cy, cz in np.argwhere(want)[:: max(1, int(want.sum()) // 64)]:
        cell = (cz * 32 + cy) * 32 + cx
        assert (int(g["marks"][cell >> 5]) >> (cell & 31)) & 1
    assert int(sum(bin(int(w)).count("1") for w in g["marks"])) == int(want.sum())
    if g["fits"]:
        nx, ny = g["hi"][0] - g["lo"][0] + 1, g["hi"][1] - g["lo"][1] + 1
        for x, y, z in np.argwhere(occ3)[:: max(1, int(occ3.sum()) // 64)]:
            b = ((z // 4 - g["lo"][2]) * ny + (y // 4 - g["lo"][1])) * nx + (x // 4 - g["lo"][0])
            m2 = lambda v: (v & 1) | ((v & 2) << 2)  # noqa: E731
            bit = m2(x & 3) | (m2(y & 3) << 1) | (m2(z & 3) << 2)
            assert (int(g["image"][b]) >> int(bit)) & 1
        assert int(sum(bin(int(w)).count("1") for w in g["image"])) == int(occ3.sum())


def test_reference_schedule_restatement():
    # 8 rays: 3 never emit, the others hold 1, 2, 9, 40 and 100 samples
    counts = np.array([0, 0, 0, 1, 2, 9, 40, 100])
    tr = S.reference_schedule(counts, 8, 16)
    assert tr[0] == (8, 1) and tr[1] == (5, 1) and tr[2] == (4, 2)
    assert sum(s for _, s in tr) >= 16 or tr[-1][0] == 0
    # ... and stepped with the oracle's own march and compositing on the column's rays: the same trace where nothing is perturbed
    c = _column_case()
    assert S.reference_loop(c, 64)[0] == S.reference_schedule(c["count"], c["n"], 64)
    steps = 0
    for n_alive, n_step in tr:
        assert n_step == max(min(8 // n_alive, 8), 1) and steps < 16
        steps += n_step


def test_long_column_keeps_rays_alive_to_a_64_step_budget():
    c = _column_case()
    assert int((c["count"] >= 64).sum()) >= 16 and int((c["count"] == 0).sum()) >= 16


def _column_case():
    return S.case("column", "axis", "none", max_steps=64)


def test_walk_visits_tells_a_visited_parameter_from_a_neighbouring_lattice_point():
    """The probe the GPU test asks the oracle with: the chain's start is visited; the lattice point one step behind a ray's first sample
    lies in the occupied voxel the walk has already sampled at its first point there -- the walk, asked again, does not stand on it."""
    c = S.case("one_voxel", "crossers", "none")
    rays = np.nonzero(c["eligible"])[0][:32]
    assert S.walk_visits(c, rays, c["t0"][rays]).all()
    first = (c["t0"][rays].astype(np.float64) + c["l"][rays, 0, 1] - c["l"][rays, 0, 0]).astype(np.float32)
    assert not S.walk_visits(c, rays, (first + S.step_of()).astype(np.float32)).any()
