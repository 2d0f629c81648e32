"""Density-grid maintenance of the ambient-dimension model on the device: the CELLS variant of csrc/field_hyper.hip
(`sdn_density_query_cells_hyper_f16` behind `FusedHyperField.query_cells` of a field built with `density_query=True`) and
`DensityGridUpdater` on a `network_hyper.NeRFNetwork`.

Pinned at three levels, as tests/test_gpu_basis_density.py pins the temporal-basis model's: the in-kernel cell -> point construction, the
four-coordinate range test and the density are BIT-EXACT against the forward kernel fed with points built by the reference's torch
expressions; the values pass the bar the forward kernel is held to against the fp16 restatement of tests/hyper_support.py (validated
without a GPU, with wrong variants, by tests/test_hyper_density_cpu.py); and a whole update agrees with the mirror's op-by-op
update_extra_state in structure.  Run with -s for the measured figures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hyper_density_support as DS  # noqa: E402
import hyper_support as HS  # noqa: E402

H3, G, T_SLICES = DS.H3, DS.G, 64


def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _row(a):
    return torch.from_numpy(DS.ambient_row(a)).cuda()


def _forward(field, row, x):
    """sigma of the forward kernel on points x with the constants row `row` (the `_set_ambient` technique of tests/test_gpu_hyper_field.py)."""
    field.bias0 = row
    return field(x, torch.zeros_like(x))[0].clone()


def _fresh_model(density_scale=None):
    model, _ = HS.mirror_model("cuda", check=False)
    if density_scale is not None:
        model.density_scale = density_scale
    assert model.iter_density == 0 and not bool(model.density_grid.any())
    return model


def _field(model, layout="quad", time=0.5):
    from dnerf_amd import fused_hyper
    return fused_hyper.FusedHyperField(model, time, table_layout=layout, density_query=True)


@pytest.fixture(scope="module")
def rig():
    model, _ = HS.mirror_model("cuda")
    oracle = HS.HyperOracle(HS.state_of(model), mode="fp16")
    g = torch.Generator(device="cuda").manual_seed(3)
    noise = torch.rand(H3, 3, device="cuda", generator=g)
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    fields = {"quad": _field(model, "quad"), "pad": _field(model, "pad")}
    assert all(f.has_density_query and f.ctx_kind == 4 for f in fields.values())
    return dict(model=model, oracle=oracle, noise=noise, cells=cells, x=DS.torch_points(model, cells, noise), fields=fields, field=fields["quad"])


# The range test sees u = (a + bound) / (2 bound) in float32 (GridEncoder.forward, grid.py:149): 1 + 2^-23 + 1 is a tie that rounds to 2,
# so the float32 next above +bound still normalises to exactly 1 (inside); 1 + 2^-22 is the first value whose u exceeds 1.
ROUNDS_INSIDE, JUST_OUTSIDE = float(np.float32(1 + 2.0 ** -23)), float(np.float32(1 + 2.0 ** -22))


@pytest.mark.parametrize("ambient", ["t0.0", "t0.93", 1.0, -1.0, ROUNDS_INSIDE, JUST_OUTSIDE])
def test_unlisted_launches_are_bit_exact_against_the_forward_kernel(rig, ambient):
    """n = 1 (one lane), 255, 256 (one tile), 257, 513 (a ragged third tile) and a whole slice; both table layouts, which also agree with
    each other; out[n:] keeps its fill.  The ambient rows of two ordinary time stamps, then three synthetic ones: exactly +bound and
    -bound (inside the range test, as in the forward), the float32 next above +bound (its normalised coordinate rounds to exactly 1: inside)
    and the first value whose normalised coordinate exceeds 1 (outside: every cell is density_scale * exp(0)).  Which side a value is on is
    worked out here in float32 with the encoder's expression, not read from the kernel."""
    r = rig
    a = float(r["oracle"].ambient(float(ambient[1:]))) if isinstance(ambient, str) else ambient
    row = _row(a)
    u3 = float(r["oracle"].geo.u_of(np.float32(a)))
    inside = 0.0 <= u3 <= 1.0
    assert inside == (ambient != JUST_OUTSIDE)
    whole = {}
    for layout, f in r["fields"].items():
        assert f.layout == layout
        for n in (1, 255, 256, 257, 513, H3):
            out = torch.full((H3,), -1.0, device="cuda")
            f.query_cells(out, row, 0, 1.0, n=n, noise=r["noise"][:n].contiguous())
            want = _forward(f, row, r["x"][:n].contiguous())
            assert torch.equal(out[:n], want), (layout, n, int((out[:n] != want).sum()))
            assert bool((out[n:] == -1).all()), (layout, n)
            assert bool(torch.isfinite(out[:n]).all()) and float(out[:n].min()) >= 0
        whole[layout] = out
    assert torch.equal(whole["quad"], whole["pad"])
    if inside:
        assert float(whole["quad"].std()) > 0
    else:
        assert bool((whole["quad"] == float(r["model"].density_scale)).all())


def test_listed_cells_with_the_live_count_on_the_device(rig):
    """513 listed cells -- cell 0 and the last cell among them, unsorted, one cell twice with the same noise -- at live counts 300, 513 and
    0: the listed live cells carry the forward kernel's value, every other entry of `out` keeps its fill."""
    r = rig
    f, row = r["field"], _row(r["oracle"].ambient(0.37))
    rng = np.random.default_rng(9)
    lst = rng.choice(np.arange(1, H3 - 1), 513, replace=False)
    lst[5], lst[7] = 0, H3 - 1
    lst[200] = lst[11]                              # the duplicate pair, both inside the first 300
    assert not (np.diff(lst) >= 0).all()
    cells = torch.from_numpy(lst.astype(np.int32)).cuda()
    nz = torch.rand(513, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    nz[200] = nz[11]
    for live in (300, 513, 0):
        count = torch.tensor([live], dtype=torch.int32, device="cuda")
        out = torch.full((H3,), -1.0, device="cuda")
        f.query_cells(out, row, 0, 1.0, cells=cells, cell_count=count, noise=nz)
        rest = torch.ones(H3, dtype=torch.bool, device="cuda")
        if live:
            idx = cells[:live].long()
            want = _forward(f, row, DS.torch_points(r["model"], cells[:live], nz[:live]))
            assert torch.equal(out[idx], want), live
            rest[idx] = False
            assert int((~rest).sum()) == live - (1 if live > 200 else 0)
        assert bool((out[rest] == -1).all()), live


def test_jitter_extremes_and_the_in_kernel_generator(rig):
    """Noise all 0 and all 1: the outermost cells' centres land exactly on -bound / +bound; whichever side of the grid's domain test
    they fall on, the query and the forward kernel share it.  Without a noise tensor: the counter-based generator on the seed."""
    r = rig
    f, row = r["field"], _row(r["oracle"].ambient(0.5))
    outs = []
    for v in (0.0, 1.0):
        nz = torch.full((H3, 3), v, device="cuda")
        out = torch.full((H3,), -1.0, device="cuda")
        f.query_cells(out, row, 0, 1.0, n=H3, noise=nz)
        x = DS.torch_points(r["model"], r["cells"], nz)
        assert float(x.abs().max()) == 1.0
        assert bool(torch.isfinite(out).all()) and torch.equal(out, _forward(f, row, x)), v
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])
    a, b, c = (torch.full((H3,), -1.0, device="cuda") for _ in range(3))
    f.query_cells(a, row, 0, 1.0, n=H3, seed=1)
    f.query_cells(b, row, 0, 1.0, n=H3, seed=2)
    f.query_cells(c, row, 0, 1.0, n=H3, seed=1)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and float(a.min()) >= 0 and float(b.min()) >= 0
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_cascades_of_a_bound_2_model():
    """bound = 2: two cascades per slice, cas_bound 1 and 2, one slice each, against the forward kernel on torch-built points.  The
    ambient coordinate is normalised by the MODEL's bound in both cascades: 1.5 and exactly 2 are inside the grid (they would be outside
    one normalised by cas_bound = 1), 2.5 is outside."""
    from dnerf_amd.network_hyper import NeRFNetwork
    torch.manual_seed(2)
    model = NeRFNetwork(**{**HS.MODEL_KW, "bound": 2})
    with torch.no_grad():
        model.encoder.embeddings.mul_(1e3)
    model = model.cuda().eval()
    assert model.cascade == 2
    f = _field(model)
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    noise = torch.rand(H3, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    own = float(f.time_constants(0.5)[0][0])
    assert abs(own) <= 2
    for a in (own, 1.5, 2.0, 2.5):
        row, outs = _row(a), []
        for cas_bound in (1.0, 2.0):
            out = torch.full((H3,), -1.0, device="cuda")
            f.query_cells(out, row, 0, cas_bound, n=H3, noise=noise)
            x = DS.torch_points(model, cells, noise, cas_bound)
            assert torch.equal(out, _forward(f, row, x)), (a, cas_bound)
            assert bool(torch.isfinite(out).all())
            outs.append(out)
        if a <= 2:
            assert float(outs[0].std()) > 0 and float(outs[1].std()) > 0 and not torch.equal(outs[0], outs[1]), a
        else:
            assert bool((outs[0] == float(model.density_scale)).all()) and bool((outs[1] == float(model.density_scale)).all())


@pytest.mark.parametrize("t", HS.TIMES)
def test_query_against_the_fp16_restatement(rig, t):
    """4096 sorted random cells of one slice, points built in numpy with the reference's fp32 operation order: the sigma bar the forward
    kernel is held to (tests/hyper_support.py), no new number."""
    r = rig
    rng = np.random.default_rng(5 + int(1000 * t))
    cells = np.sort(rng.choice(H3, 4096, replace=False)).astype(np.int32)
    noise = rng.random((4096, 3), dtype=np.float32)
    out = torch.full((H3,), -1.0, device="cuda")
    cnt = torch.tensor([4096], dtype=torch.int32, device="cuda")
    a = r["oracle"].ambient(t)
    r["field"].query_cells(out, _row(a), 0, 1.0, cells=torch.from_numpy(cells).cuda(), cell_count=cnt, noise=torch.from_numpy(noise).cuda())
    got = _np(out[torch.from_numpy(cells).long().cuda()])
    pts = DS.cell_points(cells, noise)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (4096, 1))
    ok, stats = DS.sigma_bar(got, HS.expected_f16(r["oracle"], pts, d, t), r["model"].density_scale)
    print(t, stats)
    assert ok, (t, stats)


def test_time_bias_rows_are_the_one_stamp_rows(rig):
    """The 64 perturbed times of an update: every row of `time_bias` equals `_time_row(t)[0]` -- the model's own `ambient()` under fp16
    autocast on a [1,1] stamp -- bit for bit, called outside and inside an autocast region; `_time_cache` keeps its size."""
    r = rig
    f, m = r["field"], r["model"]
    tn = torch.rand(T_SLICES, 1, generator=torch.Generator().manual_seed(8))
    times = DS.update_times(m.times, tn, T_SLICES).reshape(-1)
    cached = len(f._time_cache)
    outside = f.time_bias(times.cuda())
    with torch.autocast("cuda", dtype=torch.float16):
        inside = f.time_bias(times.cuda())
    assert len(f._time_cache) == cached
    assert tuple(outside.shape) == (T_SLICES, 128) and outside.dtype == torch.float32 and outside.is_contiguous()
    for k, t in enumerate(times.tolist()):
        want = f._time_row(f.time_value(t))[0]
        assert torch.equal(outside[k], want) and torch.equal(inside[k], want), k
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            a = m.ambient(torch.tensor([[t]], dtype=torch.float32, device="cuda"))
        assert float(want[0]) == float(a.float()) and not bool(want[1:].any()), k
    assert len(f._time_cache) == cached


def test_full_update_is_the_forward_kernel_plus_the_reference_ema():
    """A whole first update with supplied draws, bit for bit: per slice the forward kernel on torch-built points with the row of the
    perturbed time, then the reference's EMA expressions in torch; the mean within 1e-6 of the float64 mean (k_density_ema's sums: the
    basis test's bar), the bitfield exactly packbits of the native grid at the native threshold.  Cells marked -1 stay -1."""
    import raymarching
    from dnerf_amd import fused
    m = _fresh_model()
    m.density_grid[:, :, ::5] = -1
    want_grid = m.density_grid.clone()
    g = torch.Generator(device="cuda").manual_seed(21)
    noise = torch.rand(T_SLICES, 1, H3, 3, device="cuda", generator=g)
    tn = torch.rand(T_SLICES, 1, generator=torch.Generator().manual_seed(22))
    up = fused.DensityGridUpdater(m)
    assert up.field.ctx_kind == 4 and up.field.has_density_query and not up.fp32 and (T_SLICES, G) == (m.time_size, m.grid_size)
    versions = (m.density_grid._version, m.density_bitfield._version)
    mean = up.update(0.95, noise=noise, time_noise=tn)
    assert m.iter_density == 1
    assert m.density_grid._version > versions[0] and m.density_bitfield._version > versions[1]
    ref_field = _field(m)
    times = DS.update_times(m.times, tn, T_SLICES).reshape(-1).tolist()
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    for t in range(T_SLICES):
        tmp = _forward(ref_field, ref_field._time_row(ref_field.time_value(times[t]))[0], DS.torch_points(m, cells, noise[t, 0]))
        grid = want_grid[t, 0]
        valid = (grid >= 0) & (tmp >= 0)
        grid[valid] = torch.maximum(grid[valid] * 0.95, tmp[valid])
    assert torch.equal(m.density_grid, want_grid), int((m.density_grid != want_grid).sum())
    assert bool((m.density_grid[:, :, ::5] == -1).all()) and float(m.density_grid[:, :, 1::5].max()) > 0
    want_mean = float(m.density_grid.clamp(min=0).double().mean())
    print("mean", float(mean[0]), want_mean, "threshold", float(mean[1]))
    assert abs(float(mean[0]) - want_mean) <= 1e-6 * want_mean
    assert float(mean[1]) == min(float(mean[0]), np.float32(m.density_thresh))
    assert torch.equal(m.density_bitfield, torch.stack([raymarching.packbits(m.density_grid[t], float(mean[1])) for t in range(T_SLICES)]))


def test_partial_update_invariants():
    """tests/test_gpu_basis_density.py::test_partial_update_invariants on the hyper model."""
    import raymarching
    m = _fresh_model()
    up = m.use_native_density_update()
    m.update_extra_state()                       # full pass through the hook (in-kernel noise)
    assert m.iter_density == 1 and float(m.density_grid.min()) >= 0 and float((m.density_grid > 0).float().mean()) > 0.99
    m.density_grid[:, :, ::3] = 0                # make "occupied" a proper subset
    m.density_grid[5] = 0                        # and one slice with nothing occupied at all
    m.iter_density = 16
    before = m.density_grid.clone()
    torch.manual_seed(5)
    cells, counts = up.partial_cells()
    N = H3 // 4
    assert cells.shape == (T_SLICES, 1, 2 * N) and cells.dtype == torch.int32
    assert int(counts[5, 0]) == N and bool((counts[torch.arange(T_SLICES) != 5] == 2 * N).all())
    for t in (5, 9):
        live = cells[t, 0, :int(counts[t, 0])].long()
        assert 0 <= int(live.min()) and int(live.max()) < H3 and bool((live[1:] >= live[:-1]).all())   # valid, sorted by Morton index
    assert bool((cells[5, 0, N:] == 0x7FFFFFFF).all())                     # nothing occupied in slice 5: sentinels past the live count
    torch.manual_seed(5)                         # same lists inside update()
    mean = up.update(0.95)
    after = m.density_grid
    for t in (0, 5, 9, 63):
        touched = torch.zeros(H3, dtype=torch.bool, device="cuda")
        touched[cells[t, 0, :int(counts[t, 0])].long()] = True
        assert torch.equal(after[t, 0][~touched], before[t, 0][~touched])  # tmp = -1 there: no decay either
        assert bool((after[t, 0][touched] >= before[t, 0][touched] * 0.95).all())
        assert bool((after[t, 0][touched] >= 0).all())
    want = after.clamp(min=0).double().mean()
    assert abs(float(mean[0]) - float(want)) < 1e-6 * float(want)
    assert abs(m.mean_density - float(want)) < 1e-6 * float(want)
    assert torch.equal(m.density_bitfield, torch.stack([raymarching.packbits(after[t], float(mean[1])) for t in range(T_SLICES)]))
    m.iter_density = 100                         # no network queries any more: grid unchanged, bitfield re-packed
    frozen = after.clone()
    m.update_extra_state()
    assert torch.equal(m.density_grid, frozen) and m.iter_density == 101


class _ModelRowOracle(HS.HyperOracle):
    """The restatement with the ambient coordinate the MODEL computes (torch, fp16 autocast) in place of its own numpy ambient_net."""

    def __init__(self, state, model):
        super().__init__(state, mode="fp16")
        self._model = model

    def ambient(self, t):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            a = self._model.ambient(torch.tensor([[float(t)]], dtype=torch.float32, device="cuda"))
        return np.float32(float(a.float()))


def test_full_update_against_the_op_by_op_mirror():
    """Model A: the mirror's update_extra_state op by op under fp16 autocast.  Model B: the same torch.rand draws replayed into the native
    update (the mirror draws rand_like(points) then rand_like(time) per slice and enumerates cells in meshgrid order).  Both models carry
    density_scale = 2^-8 (a power of two: exact): at 1 the restatement's mean density over a slice is 30..50, above density_thresh = 10,
    and the threshold would not depend on the grid at all (the factor was chosen from the fp32 restatement on the host, not from either
    side under test; the condition itself is asserted on A below).
    On 4096 cells of each of three slices both A's and B's values pass the sigma bar at the slice's perturbed time -- against the
    restatement fed the ambient coordinate the model's own ambient_net gives for that time: the coordinate selects grid cells, so the
    restatement's numpy ambient_net, which may round the fp16 coordinate the other way, describes another point (both are printed).
    Over the whole grid a bitfield bit differs only where the threshold separates, or nearly separates, the two values: the basis
    test's comparison and bars."""
    import raymarching
    scale = 2.0 ** -8
    a, b = _fresh_model(scale), _fresh_model(scale)
    torch.manual_seed(11)
    with torch.autocast("cuda", dtype=torch.float16):
        a.update_extra_state()
    assert getattr(a, "_density_updater", None) is None
    assert 0 < a.mean_density < a.density_thresh, a.mean_density          # the threshold used is the mean: not vacuous
    set_a = float((a.density_grid > a.mean_density).float().mean())
    print("A: mean density", a.mean_density, "share of cells above the threshold", set_a)
    assert 0 < set_a < 1                                                  # the op-by-op bitfield is neither all set nor all clear
    assert bool((a.density_bitfield != 0).any()) and bool((a.density_bitfield != 255).any())
    torch.manual_seed(11)
    noise = torch.empty(T_SLICES, 1, H3, 3, device="cuda")
    tn = torch.empty(T_SLICES, 1)
    for t in range(T_SLICES):
        noise[t, 0] = torch.rand(H3, 3, device="cuda")
        tn[t, 0] = float(torch.rand(1, 1, device="cuda"))
    ax = torch.arange(G, dtype=torch.int32, device="cuda")
    xx, yy, zz = torch.meshgrid(ax, ax, ax, indexing="ij")
    morton_of_mesh = raymarching.morton3D(torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=-1).contiguous()).long()
    by_cell = torch.empty_like(noise)
    by_cell[:, :, morton_of_mesh] = noise
    del noise
    up = b.use_native_density_update()
    mean = up.update(0.95, noise=by_cell, time_noise=tn)
    assert a.iter_density == b.iter_density == 1
    assert bool((b.density_bitfield != 0).any()) and bool((b.density_bitfield != 255).any())
    da, db = a.density_grid, b.density_grid
    times = DS.update_times(b.times, tn, T_SLICES).reshape(-1).tolist()
    state = HS.state_of(b)
    oracle, model_rows = HS.HyperOracle(state, mode="fp16"), _ModelRowOracle(state, b)
    rng = np.random.default_rng(12)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (4096, 1))
    verdicts = []
    for t_idx in sorted({HS.slice_of(t, T_SLICES) for t in HS.TIMES}):
        cells = np.sort(rng.choice(H3, 4096, replace=False))
        ci = torch.from_numpy(cells).cuda()
        pts = DS.cell_points(cells, _np(by_cell[t_idx, 0][ci]))
        am, an = model_rows.ambient(times[t_idx]), oracle.ambient(times[t_idx])
        ref_m = HS.expected_f16(oracle, pts, d, times[t_idx], ambient=am)
        ref_n = HS.expected_f16(oracle, pts, d, times[t_idx], ambient=an)
        for name, grid in (("A op-by-op", da), ("B native", db)):
            ok, stats = DS.sigma_bar(_np(grid[t_idx, 0][ci]), ref_m, scale)
            _, stats_n = DS.sigma_bar(_np(grid[t_idx, 0][ci]), ref_n, scale)
            print(f"slice {t_idx} t={times[t_idx]:.6f} ambient model {am!r} numpy {an!r} {name}: failed {stats['sigma_failed']} worst/bar "
                  f"{stats['sigma_worst_of_bar']:.3f} | with the numpy ambient: failed {stats_n['sigma_failed']} worst/bar {stats_n['sigma_worst_of_bar']:.3f}")
            verdicts.append((t_idx, name, ok, stats))
    rel = (da - db).abs() / torch.maximum(da.abs(), db.abs()).clamp(min=1e-30)
    print("whole grid, |A - B| / max(|A|, |B|): max", float(rel.max()), "p99.9", float(torch.quantile(rel.view(-1)[::64], 0.999)), "median",
          float(rel.view(-1)[::64].median()), "| mean A", a.mean_density, "B", float(mean[0]))
    for t_idx, name, ok, stats in verdicts:
        assert ok, (t_idx, name, stats)
    # the structural part.  bit A = da > thr_a, bit B = db > thr_b: they can differ only if a threshold lies in [min, max] of the two
    # values, widened by the cell's own relative difference and by the distance of the two thresholds (the two means are sums in
    # different orders of grids that differ by `rel`)
    thr_a, thr_b = min(a.mean_density, a.density_thresh), float(mean[1])
    assert torch.equal(b.density_bitfield, torch.stack([raymarching.packbits(db[t], thr_b) for t in range(T_SLICES)]))
    diff = a.density_bitfield ^ b.density_bitfield
    n_diff = int(diff.count_nonzero())
    print("bitfield bytes that differ:", n_diff, "thresholds", thr_a, thr_b)
    if n_diff:
        bit = torch.arange(8, device="cuda", dtype=torch.uint8)
        cells = ((diff.view(T_SLICES, -1, 1) >> bit) & 1).bool().view(T_SLICES, 1, H3)
        va, vb, rr = da[cells].double(), db[cells].double(), rel[cells].double()
        slack = abs(thr_a - thr_b)
        lo = torch.minimum(va, vb) * (1 - rr) - slack
        hi = torch.maximum(va, vb) * (1 + rr) + slack
        inside = ((lo <= thr_a) & (thr_a <= hi)) | ((lo <= thr_b) & (thr_b <= hi))
        assert bool(inside.all()), int((~inside).sum())


def test_refusals_that_remain(rig):
    import sdn_backend
    from sdn_backend import ptr, stream
    from dnerf_amd import fused, fused_hyper
    from dnerf_amd.network_hyper import NeRFNetwork
    m, f = rig["model"], rig["field"]
    with pytest.raises(NotImplementedError):
        fused.DensityGridUpdater(m, fp32=True)
    with pytest.raises(NotImplementedError, match="bg_radius"):
        NeRFNetwork(**{**HS.MODEL_KW, "bg_radius": 1.0}).use_native_density_update()
    with pytest.raises(NotImplementedError, match="ambient_dim"):
        NeRFNetwork(**{**HS.MODEL_KW, "ambient_dim": 2}).use_native_density_update()
    with pytest.raises(NotImplementedError, match="architecture"):
        NeRFNetwork(**{**HS.MODEL_KW, "hidden_dim": 32}).use_native_density_update()
    out = torch.full((H3,), -1.0, device="cuda")
    row = _row(rig["oracle"].ambient(0.5))
    plain = fused_hyper.FusedHyperField(m, 0.5)                              # today's constructor arguments: no density query
    assert not plain.has_density_query
    with pytest.raises(NotImplementedError):
        plain.query_cells(out, row, 0, 1.0, n=8)
    with pytest.raises(NotImplementedError):
        plain.time_bias(torch.tensor([0.5]))
    with pytest.raises(NotImplementedError):
        fused.DensityGridUpdater(m, field=plain)
    assert fused.DensityGridUpdater(m, field=f).field is f                   # and the one built with density_query=True is accepted
    with pytest.raises(sdn_backend.SdnError, match="bad argument"):
        f.query_cells(out, row, 0, 1.0, cells=rig["cells"][:64].contiguous(), cell_count=None)
    with pytest.raises(sdn_backend.SdnError, match="bad argument"):
        f.query_cells(out, row, 0, 1.0, n=H3 + 1)
    # a reference-layout table (the model's own offsets) through the C entry: SDN_E_UNSUPPORTED, nothing launched
    ref_offsets = np.ascontiguousarray(m.encoder.offsets.cpu().numpy().astype(np.int32))
    table = m.encoder.embeddings.detach().to(torch.float16).contiguous()
    rc = sdn_backend.lib.sdn_density_query_cells_hyper_f16(None, None, 256, None, 1, G, 1.0, ptr(f.weights), ptr(row), ptr(table),
                                                           ref_offsets.ctypes.data, f.S, f.H, f.bound, f.density_scale, ptr(out), stream())
    assert rc == -2, rc                                                      # SDN_E_UNSUPPORTED
    with pytest.raises(sdn_backend.SdnError, match="unsupported"):
        sdn_backend.check(rc, "density_query_cells_hyper_f16")
    torch.cuda.synchronize()
    assert bool((out == -1).all())


def test_update_through_the_hook_after_training_steps():
    """Two op-by-op training steps of the mirror under autocast, then update_extra_state through the hook: the updater's field has the
    new weights, the new table and the new ambient rows (one slice of its query equals the forward kernel of a freshly built field on
    the trained model), iter_density and the step counter advance, the version counters of grid and bitfield move, and a frame rendered
    natively with the new bitfield -- whose cull grids are cached by those versions -- is finite and hits something."""
    from dnerf_amd import scene
    from dnerf_amd.renderer import DeviceLoop
    m = _fresh_model().train()
    up = m.use_native_density_update()
    assert up.field.has_density_query
    ro, rd = scene.get_rays(scene.look_at_pose(30.0, 30.0), scene.intrinsics(64, 64), 64, 64)
    ro, rd = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    time = torch.tensor([[0.5]], dtype=torch.float32, device="cuda")
    target = torch.rand(1024, 3, generator=torch.Generator().manual_seed(1)).cuda()
    opt = torch.optim.Adam(m.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")
    watched = lambda: (m.sigma_net[0].weight, m.ambient_net[0].weight, m.encoder.embeddings)  # noqa: E731
    before = [p.detach().clone() for p in watched()]
    row_before = up.time_bias(time.reshape(-1)).clone()
    table_before = up.field.table.clone()
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = m.render(ro[None, ::4].contiguous(), rd[None, ::4].contiguous(), time, staged=False, perturb=True, bg_color=1, force_all_rays=False)
            loss = ((out["image"][0] - target) ** 2).mean()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    assert all(not torch.equal(p, q) for p, q in zip(before, watched()))
    import raymarching
    steps_before = int(m.local_step)
    versions = (m.density_grid._version, m.density_bitfield._version)
    cull_before = raymarching._cull_grid_of(m.density_bitfield[32], m.cascade, m.grid_size)
    assert cull_before is not None and raymarching._cull_grid_of(m.density_bitfield[32], m.cascade, m.grid_size) is cull_before   # cached
    bits_before = m.density_bitfield[32].clone()
    with torch.autocast("cuda", dtype=torch.float16):
        m.update_extra_state()                   # the hook: refresh() + update()
    assert m.iter_density == 1 and m.mean_density > 0
    assert int(m.local_step) == 0 and steps_before == 2                     # _update_step_counter ran
    assert m.density_grid._version > versions[0] and m.density_bitfield._version > versions[1]
    # the drop-in marcher's cull-grid cache, keyed by the bitfield's version, misses and rebuilds from the new bits
    assert not torch.equal(m.density_bitfield[32], bits_before)
    cull_after = raymarching._cull_grid_of(m.density_bitfield[32], m.cascade, m.grid_size)
    assert cull_after is not None and cull_after is not cull_before
    assert raymarching._cull_grid_of(m.density_bitfield[32], m.cascade, m.grid_size) is cull_after
    fresh = _field(m, time=time)
    row = up.time_bias(time.reshape(-1))
    assert torch.equal(row[0], fresh.bias0) and not torch.equal(row, row_before)
    assert torch.equal(up.field.weights, fresh.weights) and torch.equal(up.field.table, fresh.table) and not torch.equal(up.field.table, table_before)
    noise = torch.rand(H3, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    got = up.query_cells(torch.full((H3,), -1.0, device="cuda"), row[0], 0, 1.0, n=H3, noise=noise)
    assert torch.equal(got, _forward(fresh, fresh.bias0, DS.torch_points(m, cells, noise)))
    m.eval()
    fresh.set_time(time)
    frame = DeviceLoop(m, fresh, ro.shape[0], "cuda").render(ro, rd, 0.5)
    torch.cuda.synchronize()
    depth_valid = torch.isfinite(frame["depth"]) & (frame["depth"] > 0)
    assert bool(torch.isfinite(frame["image"]).all()) and bool(depth_valid.any())
