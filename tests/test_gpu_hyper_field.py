"""The fused field of the ambient-dimension model (csrc/field_hyper.hip behind dnerf_amd/fused_hyper.py) against the fp16 restatement of
tests/hyper_support.py (validated without a GPU by tests/test_hyper_cpu.py, where four wrong variants fail the same bars), against
probe weights that read every grid feature out bit for bit at ambient values on both sides of a cell boundary, on a wrapping index
and on the grid's faces, and -- with the fixture's weights -- against the reference's fp32 outputs at the distance the op-by-op `-O`
evaluation keeps.  Run with -s for the measured figures."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import field_probe_support as P  # noqa: E402
import hyper_support as HS  # noqa: E402
from oracle import oracle as O  # noqa: E402

T = 0.5


def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _load(model, state):
    with torch.no_grad():
        for net in HS.NETS:
            for i, lin in enumerate(getattr(model, net)):
                lin.weight.copy_(torch.from_numpy(state[f"{net}.{i}.weight"]))
        model.encoder.embeddings.copy_(torch.from_numpy(state["encoder.embeddings"]))


def _set_ambient(field, a):
    """Hands the kernel this ambient coordinate instead of the one `ambient_net` gives."""
    row = np.zeros(128, np.float32)
    row[0] = a
    field.bias0 = torch.from_numpy(row).cuda()


@pytest.fixture(scope="module")
def rig():
    from dnerf_amd import fused_hyper
    model, _ = HS.mirror_model("cpu")
    fixture_state = HS.state_of(model)
    state = HS.boosted_colour(fixture_state)
    model = model.to("cuda")
    _load(model, state)
    fx = HS.load()
    oracle = HS.HyperOracle(state, mode="fp16")
    x, d = fx["x"][:513], fx["d"][:513]
    field = fused_hyper.FusedHyperField(model, T)
    _set_ambient(field, oracle.ambient(T))
    return dict(model=model, field=field, oracle=oracle, x=x, d=d, ref=HS.expected_f16(oracle, x, d, T), state=state, fixture_state=fixture_state,
                xg=torch.from_numpy(x).cuda(), dg=torch.from_numpy(d).cuda(), fx=fx)


def _cut(ref, sel):
    return {k: v[sel] for k, v in ref.items()}


def test_kernel_matches_the_fp16_restatement_at_every_launch_size(rig):
    r = rig
    s_all, c_all = (t.clone() for t in r["field"](r["xg"], r["dg"]))
    for M in (1, 255, 256, 257, 513):
        s, c = r["field"](r["xg"][:M].contiguous(), r["dg"][:M].contiguous())
        ok, stats = HS.field_bars(_np(s), _np(c), _cut(r["ref"], slice(0, M)))
        print(M, stats)
        assert ok, (M, stats)
        assert torch.equal(s, s_all[:M]) and torch.equal(c, c_all[:M]), M


@pytest.mark.parametrize("n", [0, 1, 130])
def test_live_list_evaluates_listed_slots_only(rig, n):
    r = rig
    M = 513
    idx = torch.randperm(M, generator=torch.Generator().manual_seed(5))[:n].to(torch.int32)
    lst = torch.full((M,), 0, dtype=torch.int32)
    lst[:n] = idx
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    f = r["field"]
    f._alloc(M)
    f._buf[0].fill_(-7.0)
    f._buf[1].fill_(-7.0)
    s, c = f(r["xg"], r["dg"], lst.cuda(), cnt)
    s, c = _np(s), _np(c)
    sel = np.sort(idx.numpy())
    rest = np.setdiff1d(np.arange(M), sel)
    assert (s[rest] == -7.0).all() and (c[rest] == -7.0).all()
    if n:
        ok, stats = HS.field_bars(s[sel], c[sel], _cut(r["ref"], sel))
        assert ok, stats


@pytest.mark.parametrize("ambient", [-1.0, 1.0, 0.25, 1.5, -1.0000001])
def test_faces_corners_and_points_outside_the_grid(rig, ambient):
    """The 3-D point sets of the probe tests at an ambient coordinate inside, exactly on either face of the fourth dimension, and outside
    it: outside, every point has zero features and sigma == density_scale exactly."""
    r = rig
    x, sets = P.point_sets(P.Geometry(1), n_uniform=64)
    d = np.resize(P.unit_dirs(), (x.shape[0], 3)).astype(np.float32)
    a = np.float32(ambient)
    ref = HS.expected_f16(r["oracle"], x, d, T, ambient=a)
    _set_ambient(r["field"], a)
    try:
        s, c = (_np(t) for t in r["field"](torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()))
    finally:
        _set_ambient(r["field"], r["oracle"].ambient(T))
    ok, stats = HS.field_bars(s, c, ref)
    print(ambient, stats)
    assert ok, stats
    out = sets["outside"] if abs(ambient) <= 1 else np.arange(x.shape[0])
    assert (ref["logit"][out] == 0).all() and (s[out] == 1.0).all()
    if abs(ambient) <= 1:
        for name in ("corners", "faces", "edge_in"):
            assert np.isfinite(s[sets[name]]).all() and (np.abs(ref["logit"][sets[name]].astype(np.float32)) > 0).any(), name


def test_quad_and_pad_tables_give_identical_bits(rig):
    from dnerf_amd import fused_hyper
    r = rig
    fp = fused_hyper.FusedHyperField(r["model"], T, table_layout="pad")
    _set_ambient(fp, r["oracle"].ambient(T))
    assert r["field"].layout == "quad"
    sq, cq = (t.clone() for t in r["field"](r["xg"], r["dg"]))
    sp, cp = fp(r["xg"], r["dg"])
    assert torch.equal(sq, sp) and torch.equal(cq, cp)


def test_constants_row_is_the_models_autocast_ambient(rig):
    r = rig
    f = r["field"]
    for t in HS.TIMES:
        row, flag, t_idx = f.time_constants(t)
        assert flag == 0 and t_idx == HS.slice_of(t, 64) and f.time_constants(float(np.float32(t)))[0] is row
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            a = r["model"].ambient(torch.tensor([[t]], dtype=torch.float32, device="cuda"))
        assert a.dtype == torch.float16
        row = _np(row)
        assert row.shape == (128,) and not row[1:].any() and row[0] == float(a.float()) and row[0] == np.float32(np.float16(row[0]))
        assert abs(row[0] - float(r["fx"][f"t{t}_ambient"][0])) < 4e-3
    bias, mask, slices = f.group_constants([0.0, 0.93])
    assert tuple(bias.shape) == (2, 128) and mask == 0 and slices == [0, 59]


def test_3d_quad_table_is_unchanged_by_the_builders_dimension_argument():
    """The QUAD table of a 3-D grid (small geometry: 2^14 rows at most, two dense levels) from both entry points equals the formula of
    `Fp16Table._bind_table`'s comment restated in numpy: block off[l] + 2 l + r = rows {r, r+1, r+s1, r+s1+1} mod the level's size."""
    import sdn_backend
    from sdn_backend import check, ptr, stream
    off, pls = O.grid_offsets(3, 16, 2, 2, 16, 14, 2048, False)
    off = np.ascontiguousarray(off, np.int32)
    S = float(np.float32(np.log2(pls)))
    rows = int(off[-1])
    emb = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (rows, 2)).astype(np.float32)).cuda()
    want = np.zeros((rows + 32, 4, 2), np.float16)
    e16 = emb.cpu().numpy().astype(np.float16)
    for l in range(16):
        sc, res = ctypes.c_float(), ctypes.c_uint32()
        O.lib().orc_grid_level_params(O.u32(l), O.f32(S), O.u32(16), ctypes.byref(sc), ctypes.byref(res))
        a, hs = int(off[l]), int(off[l + 1] - off[l])
        s1 = int(res.value) + 1
        r = np.arange(hs)
        for k, dr in enumerate((0, 1, s1, s1 + 1)):
            want[a + 2 * l + r, k] = e16[a + (r + dr) % hs]
    outs = []
    for nd in (False, True):
        out = torch.full((rows + 32, 4, 2), 7.0, dtype=torch.float16, device="cuda")
        if nd:
            check(sdn_backend.lib.sdn_field_build_quad_table_nd(ptr(emb), sdn_backend.dtype_id(emb.dtype), 3, off.ctypes.data, S, 16, ptr(out), stream()), "nd")
        else:
            check(sdn_backend.lib.sdn_field_build_quad_table(ptr(emb), sdn_backend.dtype_id(emb.dtype), off.ctypes.data, S, 16, ptr(out), stream()), "3d")
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint16), want.view(np.uint16)) and np.array_equal(outs[1].view(np.uint16), want.view(np.uint16))


# ---- probe weights: every grid feature bit for bit ----------------------------------------------------------------------------------------
def _probe_state(j):
    """The density logit = grid feature j, carried through the ReLU layer as a +- pair; the colour net zero."""
    st = {f"{net}.{i}.weight": np.zeros(s, np.float32) for net, shapes in (("sigma_net", [(64, 32), (33, 64)]),
                                                                            ("color_net", [(64, 48), (64, 64), (3, 64)])) for i, s in enumerate(shapes)}
    P._pm(st["sigma_net.0.weight"], 0, j)
    st["sigma_net.1.weight"][0, 0], st["sigma_net.1.weight"][0, 1] = 1, -1
    return st


def test_grid_features_bit_for_bit_through_probe_weights(rig):
    """sigma reads out one grid feature (bias-free ReLU layers carry it exactly).  For each of the 32 features -- every level of every
    class -- and for ambient values just below and just above a level-0 cell boundary, on a wrapping index of the levels that wrap, and
    on both faces: float16(log sigma) equals the oracle's at::Half D = 4 forward."""
    from dnerf_amd import fused_hyper
    geo = HS.Geometry4(1)
    assert all(geo.classes[k] for k in geo.classes)
    # level 0: q = u scale + 0.5 crosses the integer 9 at u = 8.5 / scale
    edge = np.float32(2 * 8.5 / float(geo.levels[0]["scale"]) - 1)
    below, above = np.float32(edge - 1e-3), np.float32(edge + 1e-3)
    assert geo.cell_w(below, 0) + 1 == geo.cell_w(above, 0)
    wrap = np.float32(0.6)
    for l in geo.classes["w_wraps"]:
        assert geo.cell_w(wrap, l) * geo.levels[l]["s"][3] >= geo.levels[l]["hs"], l
    ambients = [below, above, wrap, np.float32(-1.0), np.float32(1.0)]
    table = HS.random_table(geo)
    model = rig["model"]
    keep = {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith("weight") or k == "encoder.embeddings"}
    try:
        with torch.no_grad():
            model.encoder.embeddings.copy_(torch.from_numpy(table.astype(np.float32)))
        x, sets = P.point_sets(P.Geometry(1), n_uniform=256)
        want = {float(a): HS.oracle_features(geo, geo.u4(x, a), table) for a in ambients}
        assert not np.array_equal(want[float(below)][:, :10], want[float(above)][:, :10])
        xg = torch.from_numpy(x).cuda()
        dg = torch.from_numpy(np.resize(P.unit_dirs(), (x.shape[0], 3))).cuda().contiguous()
        field = fused_hyper.FusedHyperField(model, T)
        acc = {"exact_pairs": 0}
        for j in range(32):
            st = _probe_state(j)
            with torch.no_grad():
                for net in ("sigma_net", "color_net"):
                    for i, lin in enumerate(getattr(model, net)):
                        lin.weight.copy_(torch.from_numpy(st[f"{net}.{i}.weight"]))
            field.weights.copy_(field._packed())
            for a in ambients:
                _set_ambient(field, a)
                s = _np(field(xg, dg)[0])
                ok, stats = P.grid_bar_f16(s, want[float(a)][:, j])
                assert ok.all(), (j, float(a), stats)
                assert (s[sets["outside"]] == 1.0).all(), (j, float(a))
                acc["exact_pairs"] += stats["exact_pairs"]
        print(P.line("hyper", "grid features x32 x5", acc))
    finally:
        with torch.no_grad():
            for k, v in keep.items():
                model.state_dict()[k].copy_(v)


# ---- full weights against the reference's fp32 outputs -----------------------------------------------------------------------------------
def parity_figures(model, fx, times=HS.TIMES):
    """(max, p99.9, mean) of the distance to the fixture's fp32 `forward` outputs, for sigma (relative, floor 1) and rgb, of the op-by-op
    `-O` evaluation (the mirror's unfused forward over the existing operators under autocast) and of the fused kernel."""
    x, d = torch.from_numpy(fx["x"]).cuda(), torch.from_numpy(fx["d"]).cuda()
    fig = {}
    for name, fused_on in (("op-by-op", False), ("fused", True)):
        model.fused_inference = fused_on
        gs, gc, ws, wc = [], [], [], []
        for t in times:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                s, c, _ = model(x, d, torch.tensor([[t]], dtype=torch.float32, device="cuda"))
            gs.append(_np(s)); gc.append(_np(c)); ws.append(fx[f"t{t}_sigma"]); wc.append(fx[f"t{t}_rgb"])
        fig[name] = {"sigma": HS.dist3(np.concatenate(gs), np.concatenate(ws), rel_floor=1.0), "rgb": HS.dist3(np.concatenate(gc), np.concatenate(wc))}
    del model.fused_inference
    return fig


def test_fused_forward_keeps_the_op_by_op_distance_and_the_mirror_dispatches(rig):
    """With the fixture's weights: the fused kernel (through NeRFNetwork.forward's dispatch) stays within twice each of max, p99.9 and
    mean of the distance the op-by-op autocast evaluation keeps to the reference's fp32 outputs (the bars of the basis test).  The
    dispatch returns the field's own bits; with gradients enabled `forward` stays on the operators."""
    from dnerf_amd import fused_hyper
    r = rig
    model = r["model"]
    _load(model, r["fixture_state"])
    try:
        fig = parity_figures(model.eval(), r["fx"])
        tt = torch.tensor([[T]], dtype=torch.float32, device="cuda")
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            s, c, _ = model(r["xg"], r["dg"], tt)
        field = fused_hyper.FusedHyperField(model, T)
        field.density_scale = 1.0
        fs, fc = field(r["xg"], r["dg"])
        assert torch.equal(s, fs) and torch.equal(c, fc)
        with torch.autocast("cuda", dtype=torch.float16):
            sg, _, _ = model(r["xg"], r["dg"], tt)
        assert sg.requires_grad and sg.grad_fn is not None
    finally:
        _load(model, r["state"])
    print(fig)
    for out in ("sigma", "rgb"):
        for i, what in enumerate(("max", "p99.9", "mean")):
            assert fig["fused"][out][i] <= 2 * fig["op-by-op"][out][i], (out, what, fig)
    assert fig["op-by-op"]["sigma"][2] > 0


def test_out_of_scope_configurations_are_refused(rig):
    from dnerf_amd import fused_hyper
    from dnerf_amd.fused import DensityGridUpdater
    from dnerf_amd.network_hyper import NeRFNetwork
    from dnerf_amd.train_native import NativeTrainStep
    model, field = rig["model"], rig["field"]
    with pytest.raises(NotImplementedError):
        fused_hyper.FusedHyperField(model, T, fp16=False)
    with pytest.raises(NotImplementedError):
        field.query_cells(None, None, 0, 1.0, n=8)
    with pytest.raises(NotImplementedError):
        DensityGridUpdater(model, field=field)
    with pytest.raises(NotImplementedError):
        NativeTrainStep(model, None, None, 1024, "cuda")
    with pytest.raises(NotImplementedError):
        fused_hyper.FusedHyperField(model, T, persistent=True)
    for kw in (dict(ambient_dim=2), dict(bg_radius=1.0)):
        other = NeRFNetwork(**{**HS.MODEL_KW, **kw})
        assert not fused_hyper.shapes_ok(other)
        with pytest.raises(NotImplementedError):
            fused_hyper.FusedHyperField(other, T)
