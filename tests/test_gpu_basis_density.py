"""Density-grid maintenance of the temporal-basis model on the device: the CELLS variant of csrc/field_basis.hip
(`sdn_density_query_cells_basis_f16` behind `FusedBasisField.query_cells`) and `DensityGridUpdater` on a `network_basis.NeRFNetwork`.

Pinned at three levels, as tests/test_gpu_density_update.py pins the deformation model's: the in-kernel cell -> point construction and
the density are BIT-EXACT against the forward kernel fed with points built by the reference's torch expressions; the values pass the
bar the forward kernel is held to against the fp16 restatement of tests/basis_support.py (validated without a GPU, with wrong variants,
by tests/test_basis_density_cpu.py); and a whole update agrees with the mirror's op-by-op update_extra_state in structure.
Run with -s for the measured figures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import basis_density_support as DS  # noqa: E402
import basis_support as BS  # noqa: E402

H3, G, T_SLICES = DS.H3, DS.G, 64


def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _row(oracle, t):
    return torch.from_numpy(oracle.row(t)).cuda()


def _forward(field, row, x):
    """sigma of the forward kernel on points x with the constants row `row` (the `_set_row` technique of tests/test_gpu_basis_field.py)."""
    field.bias0 = row
    return field(x, torch.zeros_like(x))[0].clone()


def _fresh_model(density_scale=None):
    model, _ = BS.mirror_model("cuda", check=False)
    if density_scale is not None:
        model.density_scale = density_scale
    assert model.iter_density == 0 and not bool(model.density_grid.any())
    return model


@pytest.fixture(scope="module")
def rig():
    from dnerf_amd import fused_basis
    model, _ = BS.mirror_model("cuda")
    oracle = BS.BasisOracle(BS.state_of(model), mode="fp16")
    g = torch.Generator(device="cuda").manual_seed(3)
    noise = torch.rand(H3, 3, device="cuda", generator=g)
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    fields = {"quad": fused_basis.FusedBasisField(model, 0.5, table_layout="quad"), "pad": fused_basis.FusedBasisField(model, 0.5, table_layout="pad")}
    return dict(model=model, oracle=oracle, noise=noise, cells=cells, x=DS.torch_points(model, cells, noise), fields=fields, field=fields["quad"])


@pytest.mark.parametrize("t", [0.0, 0.93])
def test_unlisted_launches_are_bit_exact_against_the_forward_kernel(rig, t):
    """n = 1 (one lane), 255, 256 (one tile), 257, 513 (a ragged third tile) and a whole slice; both table layouts, which also agree with
    each other; out[n:] keeps its fill.  t = 0 is a time like any other: the model has no canonical frame."""
    r = rig
    row = _row(r["oracle"], t)
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
    assert float(whole["quad"].std()) > 0


def test_listed_cells_with_the_live_count_on_the_device(rig):
    """513 listed cells -- cell 0 and the last cell among them, unsorted, one cell twice with the same noise -- at live counts 300, 513 and
    0: the listed live cells carry the forward kernel's value, every other entry of `out` keeps its fill."""
    r = rig
    f, row = r["field"], _row(r["oracle"], 0.37)
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
    f, row = r["field"], _row(r["oracle"], 0.5)
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
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and float(a.min()) >= 0
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_cascades_of_a_bound_2_model():
    """bound = 2: two cascades per slice, cas_bound 1 and 2, one slice each, against the forward kernel on torch-built points."""
    from dnerf_amd import fused_basis
    from dnerf_amd.network_basis import NeRFNetwork
    torch.manual_seed(2)
    model = NeRFNetwork(**{**BS.MODEL_KW, "bound": 2})
    with torch.no_grad():
        model.encoder.embeddings.mul_(1e3)
    model = model.cuda().eval()
    assert model.cascade == 2
    f = fused_basis.FusedBasisField(model, 0.5)
    row = f.time_constants(0.5)[0]
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    noise = torch.rand(H3, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    outs = []
    for cas_bound in (1.0, 2.0):
        out = torch.full((H3,), -1.0, device="cuda")
        f.query_cells(out, row, 0, cas_bound, n=H3, noise=noise)
        x = DS.torch_points(model, cells, noise, cas_bound)
        assert torch.equal(out, _forward(f, row, x)), cas_bound
        assert bool(torch.isfinite(out).all()) and float(out.std()) > 0
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("t", BS.TIMES)
def test_query_against_the_fp16_restatement(rig, t):
    """4096 sorted random cells of one slice, points built in numpy with the reference's fp32 operation order: the sigma bar the forward
    kernel is held to (tests/basis_support.py), no new number."""
    r = rig
    rng = np.random.default_rng(5 + int(1000 * t))
    cells = np.sort(rng.choice(H3, 4096, replace=False)).astype(np.int32)
    noise = rng.random((4096, 3), dtype=np.float32)
    out = torch.full((H3,), -1.0, device="cuda")
    cnt = torch.tensor([4096], dtype=torch.int32, device="cuda")
    r["field"].query_cells(out, _row(r["oracle"], t), 0, 1.0, cells=torch.from_numpy(cells).cuda(), cell_count=cnt, noise=torch.from_numpy(noise).cuda())
    got = _np(out[torch.from_numpy(cells).long().cuda()])
    pts = DS.cell_points(cells, noise)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (4096, 1))
    ok, stats = DS.sigma_bar(got, BS.expected_f16(r["oracle"], pts, d, t), r["model"].density_scale)
    print(t, stats)
    assert ok, (t, stats)


def test_time_bias_rows_are_the_one_stamp_rows(rig):
    """The 64 perturbed times of an update: every row of `time_bias` equals `_time_row(t)[0]` -- the model's own `basis()` under fp16
    autocast on a [1,1] stamp -- bit for bit, called outside and inside an autocast region."""
    r = rig
    f, m = r["field"], r["model"]
    tn = torch.rand(T_SLICES, 1, generator=torch.Generator().manual_seed(8))
    times = DS.update_times(m.times, tn, T_SLICES).reshape(-1)
    outside = f.time_bias(times.cuda())
    with torch.autocast("cuda", dtype=torch.float16):
        inside = f.time_bias(times.cuda())
    assert tuple(outside.shape) == (T_SLICES, 128) and outside.dtype == torch.float32 and outside.is_contiguous()
    for k, t in enumerate(times.tolist()):
        want = f._time_row(float(t))[0]
        assert torch.equal(outside[k], want) and torch.equal(inside[k], want), k
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sb, cb = m.basis(torch.tensor([[t]], dtype=torch.float32, device="cuda"))
        assert torch.equal(want[:32], sb.float()) and torch.equal(want[32:40], cb.float()) and not bool(want[40:].any()), k
    assert len({tuple(row.tolist()) for row in outside[:8].cpu()}) == 8          # the rows do depend on the time


def test_full_update_is_the_forward_kernel_plus_the_reference_ema():
    """A whole first update with supplied draws, bit for bit: per slice the forward kernel on torch-built points with the row of the
    perturbed time, then the reference's EMA expressions in torch; the mean within 1e-6 of the float64 mean (k_density_ema's sums), the
    bitfield exactly packbits of the native grid at the native threshold.  Cells marked -1 stay -1."""
    import raymarching
    from dnerf_amd import fused, fused_basis
    m = _fresh_model()
    m.density_grid[:, :, ::5] = -1
    want_grid = m.density_grid.clone()
    g = torch.Generator(device="cuda").manual_seed(21)
    noise = torch.rand(T_SLICES, 1, H3, 3, device="cuda", generator=g)
    tn = torch.rand(T_SLICES, 1, generator=torch.Generator().manual_seed(22))
    up = fused.DensityGridUpdater(m)
    assert up.field.ctx_kind == 3 and not up.fp32 and (T_SLICES, G) == (m.time_size, m.grid_size)
    versions = (m.density_grid._version, m.density_bitfield._version)
    mean = up.update(0.95, noise=noise, time_noise=tn)
    assert m.iter_density == 1
    assert m.density_grid._version > versions[0] and m.density_bitfield._version > versions[1]
    ref_field = fused_basis.FusedBasisField(m, 0.5)
    times = DS.update_times(m.times, tn, T_SLICES).reshape(-1).tolist()
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    for t in range(T_SLICES):
        tmp = _forward(ref_field, ref_field._time_row(float(times[t]))[0], DS.torch_points(m, cells, noise[t, 0]))
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
    """tests/test_gpu_density_update.py::test_partial_update_invariants on the basis model."""
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


class _ModelRowOracle(BS.BasisOracle):
    """The restatement with the basis the MODEL computes (torch, fp16 autocast) in place of its own numpy basis_net: printed next to the
    asserted figures, never asserted on."""

    def __init__(self, state, model):
        super().__init__(state, mode="fp16")
        self._model = model

    def basis(self, t):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sb, cb = self._model.basis(torch.tensor([[float(t)]], dtype=torch.float32, device="cuda"))
        return sb.cpu().numpy(), cb.cpu().numpy()


def test_full_update_against_the_op_by_op_mirror(rig):
    """Model A: the mirror's update_extra_state op by op under fp16 autocast.  Model B: the same torch.rand draws replayed into the native
    update (the mirror draws rand_like(points) then rand_like(time) per slice and enumerates cells in meshgrid order).  Both models carry
    density_scale = 2^-16 (a power of two: exact) -- with density_scale = 1 the calibrated scene's mean density is in the thousands, far
    above density_thresh, and the threshold would not depend on the grid at all.
    On 4096 cells of each of three slices both A's and B's values pass the sigma bar at the slice's perturbed time; over the whole grid a
    bitfield bit differs only where the threshold separates, or nearly separates, the two values."""
    import raymarching
    scale = 2.0 ** -16
    a, b = _fresh_model(scale), _fresh_model(scale)
    torch.manual_seed(11)
    with torch.autocast("cuda", dtype=torch.float16):
        a.update_extra_state()
    assert 0 < a.mean_density < a.density_thresh, a.mean_density          # the threshold used is the mean: not vacuous
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
    da, db = a.density_grid, b.density_grid
    times = DS.update_times(b.times, tn, T_SLICES).reshape(-1).tolist()
    oracle = rig["oracle"]
    model_rows = _ModelRowOracle(BS.state_of(b), b)
    rng = np.random.default_rng(12)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (4096, 1))
    verdicts = []
    for t_idx in sorted({BS.slice_of(t, T_SLICES) for t in BS.TIMES}):
        cells = np.sort(rng.choice(H3, 4096, replace=False))
        ci = torch.from_numpy(cells).cuda()
        pts = DS.cell_points(cells, _np(by_cell[t_idx, 0][ci]))
        ref = BS.expected_f16(oracle, pts, d, times[t_idx])
        ref_m = BS.expected_f16(model_rows, pts, d, times[t_idx])
        for name, grid in (("A op-by-op", da), ("B native", db)):
            ok, stats = DS.sigma_bar(_np(grid[t_idx, 0][ci]), ref, scale)
            _, stats_m = DS.sigma_bar(_np(grid[t_idx, 0][ci]), ref_m, scale)
            print(f"slice {t_idx} t={times[t_idx]:.6f} {name}: failed {stats['sigma_failed']} worst/bar {stats['sigma_worst_of_bar']:.3f} "
                  f"| with the model's own row: failed {stats_m['sigma_failed']} worst/bar {stats_m['sigma_worst_of_bar']:.3f}")
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
    from dnerf_amd import fused
    from dnerf_amd.network_basis import NeRFNetwork
    m, f = rig["model"], rig["field"]
    with pytest.raises(NotImplementedError):
        fused.DensityGridUpdater(m, fp32=True)
    with pytest.raises(NotImplementedError, match="bg_radius"):
        NeRFNetwork(**{**BS.MODEL_KW, "bg_radius": 1.0}).use_native_density_update()
    with pytest.raises(NotImplementedError, match="architecture"):
        NeRFNetwork(**{**BS.MODEL_KW, "hidden_dim": 32}).use_native_density_update()
    out = torch.full((H3,), -1.0, device="cuda")
    row = _row(rig["oracle"], 0.5)
    with pytest.raises(sdn_backend.SdnError, match="bad argument"):
        f.query_cells(out, row, 0, 1.0, cells=rig["cells"][:64].contiguous(), cell_count=None)
    with pytest.raises(sdn_backend.SdnError, match="bad argument"):
        f.query_cells(out, row, 0, 1.0, n=H3 + 1)
    assert bool((out == -1).all())


def test_update_through_the_hook_after_training_steps():
    """Two op-by-op training steps of the mirror under autocast, then update_extra_state through the hook: the updater's field has the
    new weights and the new basis rows (one slice of its query equals the forward kernel of a freshly built field on the trained model),
    and a frame rendered natively with the new bitfield is finite and hits something."""
    from dnerf_amd import fused_basis, scene
    from dnerf_amd.renderer import DeviceLoop
    m = _fresh_model().train()
    up = m.use_native_density_update()
    ro, rd = scene.get_rays(scene.look_at_pose(30.0, 30.0), scene.intrinsics(64, 64), 64, 64)
    ro, rd = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    time = torch.tensor([[0.5]], dtype=torch.float32, device="cuda")
    target = torch.rand(1024, 3, generator=torch.Generator().manual_seed(1)).cuda()
    opt = torch.optim.Adam(m.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")
    before = [p.detach().clone() for p in (m.sigma_net[0].weight, m.basis_net[0].weight)]
    row_before = up.time_bias(time.reshape(-1)).clone()
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = m.render(ro[None, ::4].contiguous(), rd[None, ::4].contiguous(), time, staged=False, perturb=True, bg_color=1, force_all_rays=False)
            loss = ((out["image"][0] - target) ** 2).mean()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    assert all(not torch.equal(p, q) for p, q in zip(before, (m.sigma_net[0].weight, m.basis_net[0].weight)))
    with torch.autocast("cuda", dtype=torch.float16):
        m.update_extra_state()                   # the hook: refresh() + update()
    assert m.iter_density == 1 and m.mean_density > 0
    fresh = fused_basis.FusedBasisField(m, time)
    row = up.time_bias(time.reshape(-1))
    assert torch.equal(row[0], fresh.bias0) and not torch.equal(row, row_before)
    assert torch.equal(up.field.weights, fresh.weights) and torch.equal(up.field.table, fresh.table)
    noise = torch.rand(H3, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    got = up.query_cells(torch.full((H3,), -1.0, device="cuda"), row[0], 0, 1.0, n=H3, noise=noise)
    assert torch.equal(got, _forward(fresh, fresh.bias0, DS.torch_points(m, cells, noise)))
    m.eval()
    frame = DeviceLoop(m, fresh, ro.shape[0], "cuda").render(ro, rd, 0.5)
    torch.cuda.synchronize()
    depth_valid = torch.isfinite(frame["depth"]) & (frame["depth"] > 0)
    assert bool(torch.isfinite(frame["image"]).all()) and bool(depth_valid.any())
