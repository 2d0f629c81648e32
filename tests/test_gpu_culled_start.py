"""The device loop's culled start, stage by stage and per ray, against the CPU oracle on adversarial rays (tests/culled_start_support.py:
axis- and plane-parallel rays with +0.0 / -0.0 components, rays grazing the marked box and the occupied voxel, [near, far] across the
binade edges 0.125 .. 32, near-degenerate segments, unnormalised directions, all with and without a perturbed first march) and on
engineered occupancies (one voxel, the cube's corner cells, a marked box of exactly 16^3 cells and one of 16 x 16 x 17, two slabs
with an empty gap, the figure).

Stage test: after `sdn_render_begin` the cull grid and its packed fine image equal the numpy restatement word for word; a ray left off
the list has no oracle sample; the list, its count and the loop record agree; the oracle marched with `far` cut to the cached t_end
returns the same samples bit for bit; the oracle marched from the certified start returns the samples of the march from t0 bit for
bit (the first sample's second delta excepted: it is measured from the chain's start, which the loop tests cover), and the oracle's
walk from t0 stands on the certified start (asked of up to 48 jumped rays per case).  Loop test: the
device loop with the t_end cache, without it, and the host-stepped loop agree bit for bit on the same rays -- also with
dt_gamma = 1/128 (no jump may be taken) and with a 64-step budget that ends rays which are still alive.

SDN_CULLED_START_RECORD=<path>: the per-case counts of listed / culled / jumped rays are written there as JSON (information only)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import culled_start_support as S  # noqa: E402

DEV = "cuda"
PAIRS = [(o, f) for o, f, _ in S.PAIRS]
_record = {}


class Rig:
    def __init__(self):
        from dnerf_amd import fused
        from dnerf_amd.bench_scene import build_scene
        self.sc = build_scene(H=32, W=32, device=DEV, seed=0)
        self.model = self.sc.model.eval()
        assert self.model.grid_size == S.H and self.model.cascade == S.C and self.model.bound == S.BOUND
        self.model.min_near = S.MIN_NEAR
        self.field = fused.FusedField(self.model, self.sc.time, fp16=True)
        self.saved = self.model.density_bitfield.clone()
        self.current = None
        self.loops = {}
        self.rays = {}

    def set_occupancy(self, name):
        if self.current != name:
            with torch.no_grad():   # in place: whatever is derived from the slice follows the tensor's version counter
                self.model.density_bitfield[self.sc.t_idx].copy_(torch.from_numpy(S.occupancy(name)["bitfield"]).to(DEV))
            self.current = name

    def loop(self, n, cached=True, **kw):
        from dnerf_amd.renderer import DeviceLoop
        key = (n, cached, tuple(sorted(kw.items())))
        if key not in self.loops:
            lp = DeviceLoop(self.model, self.field, n, DEV, **kw)
            if not cached:
                lp.ctx.rays_tend = None          # no t_end cache: no culled start, no jump
            self.loops[key] = lp
        return self.loops[key]

    def tensors(self, c):
        key = id(c)
        if key not in self.rays:
            z = None if c["noises"] is None else torch.from_numpy(c["noises"]).to(DEV)
            self.rays[key] = (torch.from_numpy(c["ro"]).to(DEV), torch.from_numpy(c["rd"]).to(DEV), z, c)
        return self.rays[key][:3]


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    with torch.no_grad():
        r.model.density_bitfield.copy_(r.saved)
    path = os.environ.get("SDN_CULLED_START_RECORD")
    if path and _record:
        with open(path, "w") as fh:
            json.dump(_record, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _begin(rig, c, **kw):
    """bind -> noises -> sdn_render_begin -> synchronise; what the first stage left, on the host."""
    import sdn_backend
    from sdn_backend import check, lib, ptr, stream
    rig.set_occupancy(c["occ"]["name"])
    ro, rd, z = rig.tensors(c)
    lp = rig.loop(c["n"], **kw)
    lp.bind(ro, rd, rig.sc.time)
    lp.ctx.noises = ptr(z, torch.float32, "noises")
    check(lib.sdn_render_begin(ctypes.byref(lp.ctx), stream()), "render_begin")
    torch.cuda.synchronize()
    n = c["n"]
    state = lp.buf["state"].cpu().numpy()
    n_counters = lp.max_steps + 8
    return dict(tend=lp.buf["rays_tend"].cpu().numpy(), start=lp.buf["sigmas"][:n].cpu().numpy(), alive_b=lp.buf["alive_b"].cpu().numpy(),
                n_out=int(lp.buf["trace"][2 * n_counters + 8].item()), nears=lp.buf["nears"].cpu().numpy(), fars=lp.buf["fars"].cpu().numpy(),
                rec={w: int(state[i]) for i, w in enumerate(sdn_backend.LOOP_WORDS)}, cull=lp.buf["cull_bits"].cpu().numpy(), loop=lp)


def _evidence(c, g, i):
    s = slice(0, min(int(c["count"][i]), 4))
    return (f"ray {i} (tag {int(c['tag'][i])}): o {c['ro'][i].tolist()} d {c['rd'][i].tolist()} near {c['nears'][i]!r} far {c['fars'][i]!r} "
            f"t0 {c['t0'][i]!r} start {g['start'][i]!r} t_end {g['tend'][i]!r} oracle samples {int(c['count'][i])} first at {c['first_t'][i]!r} "
            f"deltas {c['l'][i][s].tolist()}")


def _first_bad(mask):
    return int(np.nonzero(mask)[0][0])


def _check_cull_grid(raw, g):
    words = raw.view(np.uint32)
    assert np.array_equal(words[:1024], g["marks"]), "cull marks"
    assert words[1024:1032].view(np.int32).tolist() == g["meta"].tolist(), "bounding box meta and the image flag"
    if g["fits"]:
        n = len(g["image"])
        assert np.array_equal(raw[1032 * 4: 1032 * 4 + 8 * n].view(np.uint64), g["image"]), "packed fine image"


def _check_stage(c, g, jump_allowed=True):
    """Cull soundness, list / count / record, t_end soundness, jump soundness.  -> (listed, jumped) masks."""
    n, occ = c["n"], c["occ"]
    assert np.array_equal(S.bits(g["nears"]), S.bits(c["nears"])) and np.array_equal(S.bits(g["fars"]), S.bits(c["fars"]))
    has_segment = c["nears"] < c["fars"]
    listed = has_segment & (g["tend"] != S.K_TEND_DEAD)
    assert (g["tend"][~has_segment] == S.K_TEND_UNSET).all()                      # never scanned
    # cull soundness: a ray off the list has no oracle sample
    bad = ~listed & (c["count"] > 0)
    assert not bad.any(), "culled, but the oracle emits: " + _evidence(c, g, _first_bad(bad))
    ids = np.nonzero(listed)[0]
    assert g["n_out"] == len(ids) and np.array_equal(g["alive_b"][: len(ids)], ids.astype(np.int32))
    rec = g["rec"]
    assert rec["side"] == 1 and rec["culled_start"] == 1 and rec["n_step"] == 1 and rec["N"] == n
    assert rec["n_alive"] == len(ids) and rec["iteration"] == (0 if len(ids) else 1)
    # t_end soundness: nothing is emitted at or beyond the cached bound
    tend = g["tend"]
    fars_cut = np.where(listed, np.minimum(c["fars"], tend), c["fars"]).astype(np.float32)
    x, d, l, count = S.march_whole(c["ro"], c["rd"], occ["bitfield"], c["t0"], fars_cut, c["max_steps"], c["dt_gamma"], n_step=c["l"].shape[1])
    bad = (count != c["count"]) | (S.bits(x) != S.bits(c["x"])).any((1, 2)) | (S.bits(l) != S.bits(c["l"])).any((1, 2))
    assert not bad.any(), "t_end cuts samples: " + _evidence(c, g, _first_bad(bad)) + f" (with t_end: {int(count[_first_bad(bad)])} samples)"
    assert np.array_equal(S.bits(d), S.bits(c["d"]))
    # jump soundness
    start = g["start"]
    bad = listed & ~(start >= c["t0"])
    assert not bad.any(), "start before t0: " + _evidence(c, g, _first_bad(bad))
    jumped = listed & (start > c["t0"])
    assert np.array_equal(S.bits(start[listed & ~jumped]), S.bits(c["t0"][listed & ~jumped]))
    if not jump_allowed:
        assert not jumped.any(), "jumped with a variable step: " + _evidence(c, g, _first_bad(jumped))
    starts = np.where(listed, start, c["t0"]).astype(np.float32)
    x, d, l, count = S.march_whole(c["ro"], c["rd"], occ["bitfield"], starts, c["fars"], c["max_steps"], c["dt_gamma"], n_step=c["l"].shape[1])
    l2, want2 = l.copy(), c["l"].copy()
    l2[:, 0, 1], want2[:, 0, 1] = 0, 0        # the first sample's second delta is measured from the chain's start: the loop tests cover it
    bad = (count != c["count"]) | (S.bits(x) != S.bits(c["x"])).any((1, 2)) | (S.bits(l2) != S.bits(want2)).any((1, 2)) | \
          (S.bits(d) != S.bits(c["d"])).any((1, 2))
    assert not bad.any(), "the march from the certified start differs: " + _evidence(c, g, _first_bad(bad)) + \
        f" (from start: {int(count[_first_bad(bad)])} samples, deltas {l[_first_bad(bad)][:4].tolist()})"
    # ... and the certified start is a point the walk from t0 stands on (certified_jump's claim itself: two walks that differ in the
    # empty lead fall into step again at the next voxel, so the samples alone rarely show a start the walk never visits)
    pick = np.nonzero(jumped)[0]
    pick = pick[:: max(1, len(pick) // 48)][:48]
    seen = S.walk_visits(c, pick, start[pick])
    assert seen.all(), "the walk from t0 never stands on the certified start: " + _evidence(c, g, int(pick[_first_bad(~seen)]))
    return listed, jumped


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.OCCUPANCIES))
def test_cull_grid_and_fine_image_equal_the_restatement(rig, name):
    fam = "crossers" if name == "figure" else "axis"
    g = _begin(rig, S.case(name, fam, "none"))
    _check_cull_grid(g["cull"], S.occupancy(name)["grid"])


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", S.NOISE_KINDS)
@pytest.mark.parametrize("occ,fam", PAIRS)
def test_culled_start_stage_against_the_oracle(rig, occ, fam, noise):
    c = S.case(occ, fam, noise)
    g = _begin(rig, c)
    _check_cull_grid(g["cull"], c["occ"]["grid"])
    listed, jumped = _check_stage(c, g)
    eligible = c["eligible"]
    counts = dict(rays=c["n"], listed=int(listed.sum()), culled=int((~listed).sum()), jumped=int(jumped.sum()),
                  declined=int((listed & ~jumped).sum()), jump_eligible=int(eligible.sum()), eligible_jumped=int((eligible & jumped).sum()),
                  emitting=int((c["count"] > 0).sum()))
    if fam == "crossers":
        for k, edge in enumerate(S.CROSS_EDGES):
            sel = c["tag"] == k
            counts[f"edge_{edge}"] = dict(listed=int((listed & sel).sum()), jumped=int((jumped & sel).sum()),
                                          eligible=int((eligible & sel).sum()))
    _record[f"{occ}/{fam}/{noise}"] = counts
    print(f"{occ}/{fam}/{noise}: {counts}")
    # not vacuous
    assert counts["culled"] >= 1                                  # the CPU test found >= 16 rays without a sample in every case
    if fam == "crossers":                                         # per edge, 0.5 .. 8 (0.25 and 0.125 are recorded, not required)
        for k in S.ORDINARY_EDGES:
            assert int((eligible & jumped & (c["tag"] == k)).sum()) >= 1, S.CROSS_EDGES[k]
    elif fam == "unnormalised" or occ == "figure":
        assert int((eligible & jumped).sum()) >= 1


# 3 --------------------------------------------------------------------------------------------------------------------
def _three_loops(rig, c, **kw):
    """DeviceLoop with the t_end cache, DeviceLoop without it, the host-stepped loop: bit-identical frames."""
    from dnerf_amd.frame_loops import FrameWorkspace
    from dnerf_amd.renderer import render_frame
    rig.set_occupancy(c["occ"]["name"])
    ro, rd, z = rig.tensors(c)
    keep = lambda o: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()}  # noqa: E731
    culled, plain = rig.loop(c["n"], True, **kw), rig.loop(c["n"], False, **kw)
    a = keep(culled.render(ro, rd, rig.sc.time, noises=z))
    a_raw = culled.buf["depth"].clone()
    b = keep(plain.render(ro, rd, rig.sc.time, noises=z))
    b_raw = plain.buf["depth"].clone()
    ws = FrameWorkspace(c["n"], DEV)                                # the host-stepped loop's accumulators: its raw depth stays in ws.depth
    h = render_frame(rig.model, ro, rd, rig.sc.time, fp16=True, field=rig.field, noises=z, dt_gamma=kw.get("dt_gamma", 0.0),
                     max_steps=kw.get("max_steps", 1024), T_thresh=kw.get("T_thresh", 1e-2), workspace=ws)
    tr = lambda o: [tuple(r) for r in o["trace"]]  # noqa: E731
    for other, what in ((b, "no t_end cache"), (h, "host-stepped")):
        assert tr(a) == tr(other), what
        assert a["n_samples"] == other["n_samples"], what
        assert torch.equal(a["image"], other["image"]) and torch.equal(a["weights_sum"], other["weights_sum"]), what
        assert torch.equal(torch.isnan(a["depth"]), torch.isnan(other["depth"])), what
        assert torch.equal(torch.nan_to_num(a["depth"]), torch.nan_to_num(other["depth"])), what
    assert torch.equal(a_raw, b_raw) and torch.equal(a_raw, ws.depth)             # the raw depth accumulators of all three
    assert a["trace"][0][0] == c["n"]                             # iteration 0 logs all N rays, culled start or not
    return a


@pytest.mark.parametrize("noise", S.NOISE_KINDS)
@pytest.mark.parametrize("occ,fam", PAIRS)
def test_whole_loop_on_the_same_rays(rig, occ, fam, noise):
    c = S.case(occ, fam, noise)
    out = _three_loops(rig, c)
    assert out["n_samples"] > 0
    if noise == "none":
        # compositing ends rays early and adds no sample.  (Not so after a perturbed first march: compositing advances rays_t from
        # `near` by the first sample's second delta, as the reference does, so iteration 1 resumes step * noise before the chain's point.)
        assert out["n_samples"] <= int(c["count"].sum())


# 4 --------------------------------------------------------------------------------------------------------------------
DT_GAMMA = 1.0 / 128


@pytest.mark.parametrize("occ,fam", [("figure", "crossers"), ("one_voxel", "axis")])
def test_variable_step_culls_and_caches_but_never_jumps(rig, occ, fam):
    c = S.case(occ, fam, "mixed", dt_gamma=DT_GAMMA)
    assert int((c["count"] > 0).sum()) >= 16 and int((c["count"] == 0).sum()) >= 16
    g = _begin(rig, c, dt_gamma=DT_GAMMA)
    listed, jumped = _check_stage(c, g, jump_allowed=False)
    assert np.array_equal(S.bits(g["start"][c["nears"] < c["fars"]]), S.bits(c["t0"][c["nears"] < c["fars"]]))     # start == t0 for EVERY ray
    assert int((~listed).sum()) >= 1 and int(listed.sum()) >= 16
    _three_loops(rig, c, dt_gamma=DT_GAMMA)


@pytest.mark.parametrize("noise", S.NOISE_KINDS)
def test_step_budget_of_64_ends_rays_that_are_still_alive(rig, noise):
    """max_steps = 64 (the step is dt_max then), T_thresh = 0: compositing ends no ray, so a ray leaves the loop only when a march gives
    it fewer samples than n_step -- the whole trace follows from the oracle alone, stepped through the reference's schedule
    n_step = max(min(N // n_alive, 8), 1), `while step < max_steps`.  The rays along the long column are alive when the budget ends."""
    c = S.case("column", "axis", noise, max_steps=64)
    g = _begin(rig, c, max_steps=64, T_thresh=0.0)
    _check_stage(c, g)
    out = _three_loops(rig, c, max_steps=64, T_thresh=0.0)
    got = [(a, s) for a, s, _ in out["trace"]]
    steps = 0
    for n_alive, n_step in got:                                           # the reference's schedule, row by row
        assert steps < 64 and n_alive > 0 and n_step == max(min(c["n"] // n_alive, 8), 1)
        steps += n_step
    assert steps >= 64 and got[-1][0] >= 16                               # cut by the budget with rays alive ...
    assert got[-1][1] == 8 and got[-1][0] <= c["n"] // 8                  # ... in the steady mode (composite + march in one kernel)
    # the whole trace and the sample count from the reference loop stepped with the oracle's march and compositing (sigma = 0), the
    # perturbed first march included: compositing advances rays_t from `near`, as the reference does
    want, samples = S.reference_loop(c, 64)
    assert got == want, (got, want)
    assert out["n_samples"] == samples
    if noise == "none":
        # ... where the chain is the whole-ray march from t0: also from the per-ray counts alone
        assert got == S.reference_schedule(c["count"], c["n"], 64)
        assert int((c["count"] >= steps).sum()) >= 16
        assert out["n_samples"] == int(np.minimum(c["count"], steps).sum())
