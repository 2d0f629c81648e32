"""The temporal-basis model's fp32 fused field (csrc/field_basis_f32.hip behind `fused_basis.FusedBasisFieldF32`) and its density-grid
query on the device, held to ONE bar (tests/basis_f32_support.py: rtol 1e-4, atol 1e-6 on sigma and rgb; tests/test_basis_f32_cpu.py
shows three wrong wirings failing it): against the fp32 restatement of tests/basis_support.py, against the REFERENCE's own fp32 outputs
and frames in tests/golden/caller_basis.npz, against one-hot basis rows that pin every register of both contractions, through the
native frame drivers, `NeRFNetwork.forward`'s opt-in dispatch and `DensityGridUpdater`.  Run with -s for the measured figures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import basis_density_support as DS  # noqa: E402
import basis_f32_support as FS  # noqa: E402
import basis_support as BS  # noqa: E402
import field_probe_support as P  # noqa: E402

T = 0.5
H3, G, T_SLICES = DS.H3, DS.G, 64
N_RAYS = 64 * 64


def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _load(model, state):
    with torch.no_grad():
        for net in BS.NETS:
            for i, lin in enumerate(getattr(model, net)):
                lin.weight.copy_(torch.from_numpy(state[f"{net}.{i}.weight"]))
        model.encoder.embeddings.copy_(torch.from_numpy(state["encoder.embeddings"]))


def _set_row(field, row):
    """Hands the kernel this constants row (the restatement's, or a one-hot one) instead of the one `basis_net` gives."""
    field.bias0 = torch.from_numpy(np.ascontiguousarray(row, np.float32)).cuda()


def _tt(t):
    return torch.tensor([[t]], dtype=torch.float32, device="cuda")


class _RowOracle(BS.BasisOracle):
    """The fp32 restatement contracting with a given row instead of its own basis_net's."""

    def __init__(self, state, row):
        super().__init__(state, mode="fp32")
        self._row = np.asarray(row, np.float32)

    def basis(self, t):
        return self._row[:32], self._row[32:40]


@pytest.fixture(scope="module")
def rig():
    """The boosted-colour state (BS.boosted_colour: see there) on the device, its fp32 restatement on 513 fixture points at t = 0.5
    (computed once), and the field with the restatement's row."""
    from dnerf_amd import fused_basis
    model, bits = BS.mirror_model("cpu")
    fixture_state = BS.state_of(model)
    state = BS.boosted_colour(fixture_state)
    model = model.to("cuda")
    _load(model, state)
    fx = BS.load()
    oracle = BS.BasisOracle(state, mode="fp32")
    x, d = fx["x"][:513], fx["d"][:513]
    field = fused_basis.FusedBasisFieldF32(model, T)
    assert field.ctx_kind == 5 and field.table.data_ptr() == model.encoder.embeddings.data_ptr() and field.zero_deform == 0
    _set_row(field, oracle.row(T))
    ws, wc, _ = oracle.forward(x, d, T)
    return dict(model=model, bits=bits, field=field, oracle=oracle, x=x, d=d, want=(ws, wc), state=state, fixture_state=fixture_state,
                xg=torch.from_numpy(x).cuda(), dg=torch.from_numpy(d).cuda(), fx=fx)


def test_kernel_matches_the_fp32_restatement_at_every_launch_size(rig):
    """M = 1 (one lane), 31, 32 (a wave's points), 33, 127, 128 (a workgroup's), 129 and 513 (a ragged fifth workgroup): every launch
    within the bar, and the same bits as the first M points of the largest."""
    r = rig
    ws, wc = r["want"]
    s_all, c_all = (t.clone() for t in r["field"](r["xg"], r["dg"]))
    for M in (1, 31, 32, 33, 127, 128, 129, 513):
        s, c = r["field"](r["xg"][:M].contiguous(), r["dg"][:M].contiguous())
        ok, stats = FS.field_bar(_np(s), _np(c), ws[:M], wc[:M])
        print(M, stats)
        assert ok, (M, stats)
        assert torch.equal(s, s_all[:M]) and torch.equal(c, c_all[:M]), M


@pytest.mark.parametrize("t", BS.TIMES)
def test_kernel_reproduces_the_references_own_outputs(rig, t):
    """The fixture's state, all 2048 points: within the bar of the REFERENCE's fp32 `forward` (t*_sigma, t*_rgb), with the row the field
    itself computes (the mirror's basis_net without autocast), which equals the reference's basis at 2e-6."""
    from dnerf_amd import fused_basis
    r = rig
    _load(r["model"], r["fixture_state"])
    try:
        f = fused_basis.FusedBasisFieldF32(r["model"], t)
        row, flag, t_idx = f.time_constants(t)
        assert flag == 0 and t_idx == BS.slice_of(t, 64) and f.time_constants(float(np.float32(t)))[0] is row
        row = _np(row)
        assert row.shape == (128,) and not row[40:].any()
        np.testing.assert_allclose(row[:40], r["fx"][f"t{t}_basis"], rtol=0, atol=2e-6)
        s, c = f(torch.from_numpy(r["fx"]["x"]).cuda(), torch.from_numpy(r["fx"]["d"]).cuda())
        s, c = _np(s), _np(c)
    finally:
        _load(r["model"], r["state"])
    ok, stats = FS.field_bar(s, c, r["fx"][f"t{t}_sigma"], r["fx"][f"t{t}_rgb"])
    print(t, stats)
    assert ok, (t, stats)


def test_every_register_of_both_contractions(rig):
    """One-hot rows through `field.bias0`.  e_k, k = 0..31, color_basis zero: sigma = exp(coefficient k) and rgb = sigmoid(0) = 0.5
    exactly; e_{32 + j}, j = 0..7: sigma = exp(0) = 1 exactly and rgb[c] = sigmoid(colour coefficient (c, j)) -- every register of both
    lane halves of both cross-half sums, against the restatement with the same row.  The fixture's calibrated coefficients reach 300:
    where exp overflows float32 in the restatement the kernel must return the same infinity; everywhere else the bar holds as it is."""
    r = rig
    worst = [0.0, 0.0]
    for k in range(40):
        row = np.zeros(128, np.float32)
        row[k] = 1.0
        _set_row(r["field"], row)
        s, c = (_np(t) for t in r["field"](r["xg"], r["dg"]))
        with np.errstate(over="ignore"):
            ws, wc, _ = _RowOracle(r["state"], row).forward(r["x"], r["d"], T)
        if k < 32:
            coef = r["oracle"].coefficients(r["x"])[:, k]
            with np.errstate(over="ignore"):
                assert np.array_equal(ws, np.exp(coef).astype(np.float32))
            over = np.isinf(ws)
            assert np.array_equal(np.isinf(s), over) and (~over).sum() > 256, k
            assert (c == 0.5).all(), k
            fin = ~over
            ok, stats = FS.field_bar(s[fin], c[fin], ws[fin], wc[fin])
        else:
            assert (s == 1.0).all() and (ws == 1.0).all(), k
            assert np.abs(wc - 0.5).max() > 0.05, k            # (the coefficient shows in the output)
            ok, stats = FS.field_bar(s, c, ws, wc)
        worst = [max(worst[0], stats["sigma_worst_of_bar"]), max(worst[1], stats["rgb_worst_of_bar"])]
        assert ok, (k, stats)
    _set_row(r["field"], r["oracle"].row(T))
    print("one-hot rows: worst share of the bar, sigma / rgb:", worst)


@pytest.mark.parametrize("n", [0, 1, 130])
def test_live_list_evaluates_listed_slots_only(rig, n):
    r = rig
    M = 513
    f = r["field"]
    s_all, c_all = (t.clone() for t in f(r["xg"], r["dg"]))
    idx = torch.randperm(M, generator=torch.Generator().manual_seed(5))[:n].to(torch.int32)
    lst = torch.full((M,), 0, dtype=torch.int32)
    lst[:n] = idx
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    f._alloc(M)
    f._buf[0].fill_(-7.0)
    f._buf[1].fill_(-7.0)
    s, c = f(r["xg"], r["dg"], lst.cuda(), cnt)
    sel = torch.sort(idx).values.long().cuda()
    rest = torch.ones(M, dtype=torch.bool, device="cuda")
    rest[sel] = False
    assert bool((s[rest] == -7.0).all()) and bool((c[rest] == -7.0).all())
    assert torch.equal(s[sel], s_all[sel]) and torch.equal(c[sel], c_all[sel])


def test_faces_corners_and_points_outside_the_grid(rig):
    r = rig
    geo = P.Geometry(1)
    x, sets = P.point_sets(geo, n_uniform=64)
    d = np.resize(P.unit_dirs(), (x.shape[0], 3)).astype(np.float32)
    ws, wc, _ = r["oracle"].forward(x, d, T)
    logit = r["oracle"].density(x, T)["logit"]
    s, c = (_np(t) for t in r["field"](torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()))
    ok, stats = FS.field_bar(s, c, ws, wc)
    print(stats)
    assert ok, stats
    out = sets["outside"]
    assert (logit[out] == 0).all() and (s[out] == 1.0).all()       # zero features, no bias: sigma = density_scale * exp(0), exactly
    for name in ("corners", "faces", "edge_in"):
        assert np.isfinite(s[sets[name]]).all() and (np.abs(logit[sets[name]]) > 0).any(), name


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(rig):
    """The fixture's state and camera; the host-stepped frame with the fp32 field at the three stamps, rendered once."""
    from dnerf_amd import fused_basis, scene
    from dnerf_amd.renderer import render_frame
    model, _ = BS.mirror_model("cuda")
    ro, rd = scene.get_rays(scene.look_at_pose(30.0, 30.0), scene.intrinsics(64, 64), 64, 64)
    ro, rd = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    field = fused_basis.FusedBasisFieldF32(model, T)
    host = {}
    for t in BS.TIMES:
        field.set_time(t)
        o = render_frame(model, ro, rd, _tt(t), fp16=False, field=field)
        host[t] = {k: (o[k].clone() if isinstance(o[k], torch.Tensor) else o[k]) for k in ("image", "depth", "weights_sum", "trace", "n_samples")}
    return dict(model=model, ro=ro, rd=rd, field=field, host=host, fx=rig["fx"])


@pytest.mark.parametrize("t", BS.TIMES)
def test_render_frame_reproduces_the_reference_frames(frames, t):
    """`render_frame(field=FusedBasisFieldF32)`: the trace of the reference's own run_cuda exactly; image, weights_sum and depth on hits
    within 1e-4 (rtol and atol, as tests/test_gpu_field_f32.py::test_render_frame_fp32_through_the_fused_field_vs_oracle)."""
    out, fx = frames["host"][t], frames["fx"]
    assert np.array_equal(np.array([tuple(x) for x in out["trace"]], np.int32), fx[f"t{t}_trace"])
    np.testing.assert_allclose(_np(out["image"]).reshape(-1, 3), fx[f"t{t}_image"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(_np(out["weights_sum"]).reshape(-1), fx[f"t{t}_weights_sum"], rtol=1e-4, atol=1e-4)
    miss = np.isnan(fx[f"t{t}_depth"])
    depth = _np(out["depth"]).reshape(-1)
    assert np.array_equal(np.isnan(depth), miss) and (~miss).sum() > 100
    np.testing.assert_allclose(depth[~miss], fx[f"t{t}_depth"][~miss], rtol=1e-4, atol=1e-4)


def test_native_loops_equal_the_host_stepped_frame(frames):
    """`SdnRenderCtx.field_f32 == 5`: DeviceLoop, a two-frame group at two different stamps and the pipelined driver, bit for bit the
    host-stepped frame with the same field (same samples into the same kernel; a point's result does not depend on its tile)."""
    from dnerf_amd.renderer import DeviceLoop, PipelinedDeviceLoop
    fr = frames
    model, field, ro, rd, host = fr["model"], fr["field"], fr["ro"], fr["rd"], fr["host"]
    one = DeviceLoop(model, field, N_RAYS, "cuda")
    for t in BS.TIMES:
        a = one.render(ro, rd, t)
        torch.cuda.synchronize()
        assert torch.equal(a["image"], host[t]["image"]) and torch.equal(a["weights_sum"], host[t]["weights_sum"]), t
        assert torch.equal(torch.nan_to_num(a["depth"]), torch.nan_to_num(host[t]["depth"])), t
        assert [tuple(x) for x in a["trace"]] == [tuple(x) for x in host[t]["trace"]] and a["n_samples"] == host[t]["n_samples"] > 1000, t
    times = [0.0, 0.93]
    assert not torch.equal(host[0.0]["image"], host[0.93]["image"])
    grp = DeviceLoop(model, field, 2 * N_RAYS, "cuda", frames=2)
    out = grp.render(torch.cat([ro, ro]).contiguous(), torch.cat([rd, rd]).contiguous(), times)
    torch.cuda.synchronize()
    for f, t in enumerate(times):
        assert torch.equal(out["image"][f * N_RAYS:(f + 1) * N_RAYS], host[t]["image"]), t
    pl = PipelinedDeviceLoop(model, field, N_RAYS, "cuda", contexts=2)
    outs = [(torch.empty(N_RAYS, 3, device="cuda"), torch.empty(N_RAYS, device="cuda")) for _ in times]
    pl.render_frames([ro, ro], [rd, rd], times, outputs=outs)
    torch.cuda.synchronize()
    for f, t in enumerate(times):
        assert torch.equal(outs[f][0], host[t]["image"]), t


# ---- NeRFNetwork.forward's dispatch ----------------------------------------------------------------------------------------------------
def test_forward_dispatch_is_opt_in_and_leaves_every_other_path_alone(rig):
    from dnerf_amd.network_basis import NeRFNetwork
    m, x, d, t = rig["model"], rig["xg"], rig["dg"], _tt(T)
    assert NeRFNetwork.fused_inference_f32 is False and "fused_inference_f32" not in m.__dict__

    def op_by_op():
        sb, cb = m.basis(t)
        sigma, geo = m._sigma(x, sb)
        return sigma, m._color(d, geo, cb)

    with torch.no_grad():
        want = op_by_op()
        assert not m._fused_inference_ok(x, d)
        off = m(x, d, t)
        assert torch.equal(off[0], want[0]) and torch.equal(off[1], want[1]) and off[2] is None       # flag off: today's path, bit for bit
        with torch.autocast("cuda", dtype=torch.float16):
            assert m._fused_inference_ok(x, d) == 16
            half_before = [v.clone() for v in m(x, d, t)[:2]]
        m.fused_inference_f32 = True
        try:
            assert m._fused_inference_ok(x, d) == 32
            s, c, none = m(x, d, t)
            assert none is None and s.dtype == c.dtype == torch.float32
            ok, stats = FS.field_bar(_np(s), _np(c), _np(want[0]), _np(want[1]))
            print(stats)
            assert ok, stats
            assert m.__dict__["_fused_cache32"][1].ctx_kind == 5 and m.__dict__["_fused_cache32"][1] is not m.__dict__["_fused_cache"][1]
            with torch.autocast("cuda", dtype=torch.float16):       # under -O the flag changes nothing
                assert m._fused_inference_ok(x, d) == 16
                half_after = m(x, d, t)[:2]
            assert torch.equal(half_after[0], half_before[0]) and torch.equal(half_after[1], half_before[1])
            m.train()
            assert not m._fused_inference_ok(x, d)
            m.eval()
        finally:
            del m.fused_inference_f32
        again = m(x, d, t)
        assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
    with torch.enable_grad():
        m.fused_inference_f32 = True
        try:
            assert not m._fused_inference_ok(x, d)                  # with autograd: op by op
        finally:
            del m.fused_inference_f32


# ---- CELLS: the density-grid query -----------------------------------------------------------------------------------------------------
def _forward(field, row, x):
    field.bias0 = row
    return field(x, torch.zeros_like(x))[0].clone()


@pytest.fixture(scope="module")
def cells_rig(frames):
    model, field = frames["model"], frames["field"]
    g = torch.Generator(device="cuda").manual_seed(3)
    noise = torch.rand(H3, 3, device="cuda", generator=g)
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    return dict(model=model, field=field, noise=noise, cells=cells, x=DS.torch_points(model, cells, noise))


@pytest.mark.parametrize("t", [0.0, 0.93])
def test_query_is_bit_exact_against_the_forward_kernel(cells_rig, t):
    """n = 1, 127, 128 (a workgroup), 129 and a whole 128^3 slice, without a list and with one (unsorted, live count on the device): the
    query's density is the forward kernel's on points built by the reference's torch expressions, bit for bit; the rest of `out` keeps
    its fill."""
    r = cells_rig
    f = r["field"]
    row = f.time_constants(t)[0]
    perm = torch.randperm(H3, generator=torch.Generator().manual_seed(7)).to(torch.int32).cuda()
    for n in (1, 127, 128, 129, H3):
        out = torch.full((H3,), -1.0, device="cuda")
        f.query_cells(out, row, 0, 1.0, n=n, noise=r["noise"][:n].contiguous())
        want = _forward(f, row, r["x"][:n].contiguous())
        assert torch.equal(out[:n], want), (n, int((out[:n] != want).sum()))
        assert bool((out[n:] == -1).all()) and bool(torch.isfinite(out[:n]).all()) and float(out[:n].min()) >= 0, n
        if n == H3:
            assert float(out.std()) > 0
        # the same through a list of n cells in random order, n + 3 entries of which n are live
        lst = torch.cat([perm[:n], perm[:3]]).contiguous()
        nz = r["noise"][:n + 3].contiguous()
        out = torch.full((H3,), -1.0, device="cuda")
        f.query_cells(out, row, 0, 1.0, cells=lst, cell_count=torch.tensor([n], dtype=torch.int32, device="cuda"), noise=nz)
        idx = lst[:n].long()
        want = _forward(f, row, DS.torch_points(r["model"], lst[:n], nz[:n]))
        assert torch.equal(out[idx], want), n
        rest = torch.ones(H3, dtype=torch.bool, device="cuda")
        rest[idx] = False
        assert bool((out[rest] == -1).all()), n


def test_cascades_of_a_bound_2_model():
    from dnerf_amd import fused_basis
    from dnerf_amd.network_basis import NeRFNetwork
    torch.manual_seed(2)
    model = NeRFNetwork(**{**BS.MODEL_KW, "bound": 2})
    with torch.no_grad():
        model.encoder.embeddings.mul_(1e3)
    model = model.cuda().eval()
    assert model.cascade == 2
    f = fused_basis.FusedBasisFieldF32(model, 0.5)
    row = f.time_constants(0.5)[0]
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    noise = torch.rand(H3, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    outs = []
    for cas_bound in (1.0, 2.0):
        out = torch.full((H3,), -1.0, device="cuda")
        f.query_cells(out, row, 0, cas_bound, n=H3, noise=noise)
        assert torch.equal(out, _forward(f, row, DS.torch_points(model, cells, noise, cas_bound))), cas_bound
        assert bool(torch.isfinite(out).all()) and float(out.std()) > 0
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])


def test_query_refuses_bad_arguments(cells_rig):
    import sdn_backend
    r = cells_rig
    f = r["field"]
    row = f.time_constants(0.5)[0]
    out = torch.full((H3,), -1.0, device="cuda")
    with pytest.raises(sdn_backend.SdnError, match="bad argument"):
        f.query_cells(out, row, 0, 1.0, cells=r["cells"][:64].contiguous(), cell_count=None)
    with pytest.raises(sdn_backend.SdnError, match="bad argument"):
        f.query_cells(out, row, 0, 1.0, n=H3 + 1)
    assert bool((out == -1).all())


# ---- the updater ---------------------------------------------------------------------------------------------------------------------------
def _fresh_model(density_scale=None):
    model, _ = BS.mirror_model("cuda", check=False)
    if density_scale is not None:
        model.density_scale = density_scale
    assert model.iter_density == 0 and not bool(model.density_grid.any())
    return model


def test_full_update_against_the_op_by_op_fp32_mirror():
    """Model A: the mirror's update_extra_state op by op WITHOUT autocast.  Model B: the same torch.rand draws replayed into the native
    update through `FusedBasisFieldF32` (tests/test_gpu_basis_density.py::test_full_update_against_the_op_by_op_mirror has the replay).
    density_scale = 2^-16 (exact) keeps the mean below density_thresh, so that the threshold depends on the grid.  The grid within the
    bar on every cell A sets positive; a bitfield bit differs only at a cell whose density lies within the bar of a threshold."""
    import raymarching
    from dnerf_amd import fused, fused_basis
    scale = 2.0 ** -16
    a, b = _fresh_model(scale), _fresh_model(scale)
    torch.manual_seed(11)
    a.update_extra_state()
    assert 0 < a.mean_density < a.density_thresh, a.mean_density
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
    up = b.use_native_density_update(field=fused_basis.FusedBasisFieldF32(b, b.times[0].reshape(1, 1)))
    assert isinstance(up, fused.DensityGridUpdater) and up.fp32 and up.field.ctx_kind == 5
    mean = up.update(0.95, noise=by_cell, time_noise=tn)
    assert a.iter_density == b.iter_density == 1
    da, db = a.density_grid.double(), b.density_grid.double()
    pos = da > 0
    err = (db - da).abs() / (FS.ATOL + FS.RTOL * da.abs())
    thr_a, thr_b = min(a.mean_density, a.density_thresh), float(mean[1])
    print("cells A sets positive:", int(pos.sum()), "of", da.numel(), "| worst share of the bar:", float(err[pos].max()), "| cells over the bar:",
          int((err[pos] > 1).sum()), "| mean A", a.mean_density, "B", float(mean[0]), "thresholds", thr_a, thr_b)
    assert int(pos.sum()) > da.numel() // 2
    assert bool((err[pos] <= 1).all()), (float(err[pos].max()), int((err[pos] > 1).sum()))
    assert abs(thr_a - thr_b) <= FS.ATOL + FS.RTOL * thr_a
    assert torch.equal(b.density_bitfield, torch.stack([raymarching.packbits(b.density_grid[t], thr_b) for t in range(T_SLICES)]))
    diff = a.density_bitfield ^ b.density_bitfield
    n_bytes = int(diff.count_nonzero())
    n_cells = 0
    if n_bytes:
        bit = torch.arange(8, device="cuda", dtype=torch.uint8)
        cells = ((diff.view(T_SLICES, -1, 1) >> bit) & 1).bool().view(T_SLICES, 1, H3)
        n_cells = int(cells.sum())
        near = torch.zeros_like(cells)
        for v in (da, db):
            for thr in (thr_a, thr_b):
                near |= (v - thr).abs() <= FS.ATOL + FS.RTOL * thr
        assert bool(near[cells].all()), int((~near[cells]).sum())
    print("bitfield cells that differ:", n_cells, "in", n_bytes, "bytes")


def test_updater_follows_training_steps_after_refresh():
    """Two op-by-op fp32 training steps of the mirror, then `refresh()`: the updater's field carries the new weights, reads the new table
    in place and computes the new basis rows -- one slice of its query equals the forward kernel of a freshly built field."""
    from dnerf_amd import fused_basis, scene
    m = _fresh_model().train()
    time = _tt(0.5)
    up = m.use_native_density_update(field=fused_basis.FusedBasisFieldF32(m, time))
    ro, rd = scene.get_rays(scene.look_at_pose(30.0, 30.0), scene.intrinsics(64, 64), 64, 64)
    ro, rd = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    target = torch.rand(1024, 3, generator=torch.Generator().manual_seed(1)).cuda()
    opt = torch.optim.Adam(m.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    before = [p.detach().clone() for p in (m.sigma_net[0].weight, m.basis_net[0].weight, m.encoder.embeddings)]
    row_before = up.time_bias(time.reshape(-1)).clone()
    packed_before = up.field.weights.clone()
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        out = m.render(ro[None, ::4].contiguous(), rd[None, ::4].contiguous(), time, staged=False, perturb=True, bg_color=1, force_all_rays=False)
        ((out["image"][0] - target) ** 2).mean().backward()
        opt.step()
    assert all(not torch.equal(p, q) for p, q in zip(before, (m.sigma_net[0].weight, m.basis_net[0].weight, m.encoder.embeddings)))
    up.refresh()
    fresh = fused_basis.FusedBasisFieldF32(m, time)
    row = up.time_bias(time.reshape(-1))
    assert torch.equal(row[0], fresh.bias0) and not torch.equal(row, row_before)
    assert torch.equal(up.field.weights, fresh.weights) and not torch.equal(up.field.weights, packed_before)
    assert up.field.table.data_ptr() == m.encoder.embeddings.data_ptr()
    noise = torch.rand(H3, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    cells = torch.arange(H3, device="cuda", dtype=torch.int32)
    got = up.query_cells(torch.full((H3,), -1.0, device="cuda"), row[0], 0, 1.0, n=H3, noise=noise)
    assert torch.equal(got, _forward(fresh, fresh.bias0, DS.torch_points(m, cells, noise)))
