"""The fused field of the temporal-basis model (csrc/field_basis.hip behind dnerf_amd/fused_basis.py) against the fp16 restatement of
tests/basis_support.py (validated without a GPU by tests/test_basis_cpu.py, where three wrong variants fail the same bars), against
probe weights that pin every coefficient column and every position of the 3 x 8 colour contraction, and -- with the fixture's weights
-- against the reference's fp32 outputs at the distance the op-by-op `-O` evaluation keeps.  Run with -s for the measured figures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import basis_support as BS  # noqa: E402
import field_probe_support as P  # noqa: E402

T = 0.5


def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _load(model, state):
    with torch.no_grad():
        for net in BS.NETS:
            for i, lin in enumerate(getattr(model, net)):
                lin.weight.copy_(torch.from_numpy(state[f"{net}.{i}.weight"]))
        model.encoder.embeddings.copy_(torch.from_numpy(state["encoder.embeddings"]))


def _set_row(field, row):
    """Hands the kernel this constants row (the restatement's, or a probe's) instead of the one `basis_net` gives."""
    field.bias0 = torch.from_numpy(np.ascontiguousarray(row, np.float32)).cuda()


@pytest.fixture(scope="module")
def rig():
    from dnerf_amd import fused_basis
    model, _ = BS.mirror_model("cpu")
    fixture_state = BS.state_of(model)
    state = BS.boosted_colour(fixture_state)
    model = model.to("cuda")
    _load(model, state)
    fx = BS.load()
    oracle = BS.BasisOracle(state, mode="fp16")
    x, d = fx["x"][:513], fx["d"][:513]
    field = fused_basis.FusedBasisField(model, T)
    _set_row(field, oracle.row(T))
    return dict(model=model, field=field, oracle=oracle, x=x, d=d, ref=BS.expected_f16(oracle, x, d, T), state=state, fixture_state=fixture_state,
                xg=torch.from_numpy(x).cuda(), dg=torch.from_numpy(d).cuda(), fx=fx)


def _cut(ref, sel):
    return {k: v[sel] for k, v in ref.items()}


def test_kernel_matches_the_fp16_restatement_at_every_launch_size(rig):
    """M = 1 (one lane), 255, 256 (one tile), 257 and 513 (a ragged third tile): every launch within the bars, and the same bits as the
    first M points of the largest."""
    r = rig
    s_all, c_all = (t.clone() for t in r["field"](r["xg"], r["dg"]))
    for M in (1, 255, 256, 257, 513):
        s, c = r["field"](r["xg"][:M].contiguous(), r["dg"][:M].contiguous())
        ok, stats = BS.field_bars(_np(s), _np(c), _cut(r["ref"], slice(0, M)))
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
        ok, stats = BS.field_bars(s[sel], c[sel], _cut(r["ref"], sel))
        assert ok, stats


def test_faces_corners_and_points_outside_the_grid(rig):
    r = rig
    geo = P.Geometry(1)
    x, sets = P.point_sets(geo, n_uniform=64)
    d = np.resize(P.unit_dirs(), (x.shape[0], 3)).astype(np.float32)
    ref = BS.expected_f16(r["oracle"], x, d, T)
    s, c = r["field"](torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda())
    s, c = _np(s), _np(c)
    ok, stats = BS.field_bars(s, c, ref)
    print(stats)
    assert ok, stats
    out = sets["outside"]
    assert (ref["logit"][out] == 0).all() and (s[out] == 1.0).all()       # zero features, no bias: sigma = density_scale * exp(0), exactly
    for name in ("corners", "faces", "edge_in"):
        assert np.isfinite(s[sets[name]]).all() and (np.abs(ref["logit"][sets[name]].astype(np.float32)) > 0).any(), name


def test_quad_and_pad_tables_give_identical_bits(rig):
    from dnerf_amd import fused_basis
    r = rig
    fp = fused_basis.FusedBasisField(r["model"], T, table_layout="pad")
    _set_row(fp, r["oracle"].row(T))
    assert r["field"].layout == "quad"
    sq, cq = (t.clone() for t in r["field"](r["xg"], r["dg"]))
    sp, cp = fp(r["xg"], r["dg"])
    assert torch.equal(sq, sp) and torch.equal(cq, cp)


def test_basis_row_of_the_field_is_the_models_fp16_basis(rig):
    """`time_constants` runs the mirror's own encoder_time and basis_net under autocast: fp16 values in entries 0..39, zeros behind,
    at fp16 distance (5 fp16 Linear layers) of the fixture's fp32 basis; cached by value."""
    r = rig
    f = r["field"]
    for t in BS.TIMES:
        row, flag, t_idx = f.time_constants(t)
        assert flag == 0 and t_idx == BS.slice_of(t, 64) and f.time_constants(float(np.float32(t)))[0] is row
        row = _np(row)
        want = r["fx"][f"t{t}_basis"]
        assert row.shape == (128,) and not row[40:].any() and np.array_equal(row, row.astype(np.float16).astype(np.float32))
        assert np.abs(row[:40] - want).max() <= 16 * BS.ulp16(np.abs(want).max())
        assert np.abs(row[:40] - r["oracle"].row(t)[:40]).max() <= 8 * BS.ulp16(np.abs(want).max())
    bias, mask, slices = f.group_constants([0.0, 0.93])
    assert tuple(bias.shape) == (2, 128) and mask == 0 and slices == [0, 59]


# ---- probe weights: exact pins --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_rig(rig):
    from dnerf_amd import fused_basis
    geo = P.Geometry(1)
    table = P.random_table(geo)
    model = rig["model"]
    keep = {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith("weight") or k == "encoder.embeddings"}
    with torch.no_grad():
        model.encoder.embeddings.copy_(torch.from_numpy(table.astype(np.float32)))
    x, sets = P.point_sets(geo, n_uniform=256)
    f16 = P.oracle_features(geo, x, table)
    d = torch.from_numpy(np.resize(P.unit_dirs(), (x.shape[0], 3))).cuda().contiguous()
    field = fused_basis.FusedBasisField(model, T)
    yield dict(model=model, field=field, x=torch.from_numpy(x).cuda(), d=d, f16=f16, outside=sets["outside"])
    with torch.no_grad():
        for k, v in keep.items():
            model.state_dict()[k].copy_(v)


def _probe_state(j, out_row, c0_col=None, c2_row=None):
    """sigma-net output `out_row` = grid feature j (carried through the ReLU layer as a +- pair); with c0_col: colour-net output
    `c2_row` = GAIN * (colour input c0_col)."""
    st = {f"{net}.{i}.weight": np.zeros(s, np.float32) for net, shapes in (("sigma_net", [(64, 32), (64, 64)]),
                                                                            ("color_net", [(64, 48), (64, 64), (24, 64)])) for i, s in enumerate(shapes)}
    P._pm(st["sigma_net.0.weight"], 0, j)
    st["sigma_net.1.weight"][out_row, 0], st["sigma_net.1.weight"][out_row, 1] = 1, -1
    if c0_col is not None:
        P._pm(st["color_net.0.weight"], 0, c0_col)
        st["color_net.1.weight"][0, 0] = st["color_net.1.weight"][1, 1] = 1
        st["color_net.2.weight"][c2_row, 0], st["color_net.2.weight"][c2_row, 1] = P.GAIN, -P.GAIN
    return st


def _load_probe(pr, st):
    with torch.no_grad():
        for net in ("sigma_net", "color_net"):
            for i, lin in enumerate(getattr(pr["model"], net)):
                lin.weight.copy_(torch.from_numpy(st[f"{net}.{i}.weight"]))
    pr["field"].weights.copy_(pr["field"]._packed())


def test_every_density_coefficient_column_reads_its_basis_entry(probe_rig):
    """Coefficient k = grid feature k (bias-free ReLU layers passing one value through), sigma_basis[k] = 2^-1 and every other entry
    of the row 3 (a kernel that reads another entry, or another coefficient, is off by a factor or reads zero): the logit is
    feature x 2^-1, every rounding exact -- float16(log sigma) is that product bit for bit, for each of the 32 columns."""
    pr = probe_rig
    acc = {}
    for k in range(32):
        _load_probe(pr, _probe_state(k, k))
        row = np.zeros(128, np.float32)
        row[:40] = 3.0
        row[k] = 0.5
        _set_row(pr["field"], row)
        s = _np(pr["field"](pr["x"], pr["d"])[0])
        want = (pr["f16"][:, k].astype(np.float32) * np.float32(0.5)).astype(np.float16)
        ok, stats = P.grid_bar_f16(s, want)
        assert ok.all(), (k, stats)
        assert (s[pr["outside"]] == 1.0).all(), k
        acc["exact_pairs"] = acc.get("exact_pairs", 0) + stats["exact_pairs"]
    print(P.line("basis", "density columns x32", acc))


def test_every_position_of_the_colour_contraction(probe_rig):
    """Colour coefficient (c, k) = GAIN x geo_feat[g] = GAIN x one grid feature, color_basis[k] = 1 and every other entry 2: rgb[c] is
    sigmoid of that one value and the two other channels are sigmoid(0) = 0.5 exactly -- a `view(-1, 8, 3)` or a transposed register
    layout lands in another channel or doubles the logit.  All 3 x 8 positions, geo_feat index and grid feature varying with them."""
    pr = probe_rig
    for c in range(3):
        for k in range(8):
            pos = 8 * c + k
            g, j = (5 * pos + 3) % 32, pos % 32
            _load_probe(pr, _probe_state(j, 32 + g, c0_col=16 + g, c2_row=pos))
            row = np.zeros(128, np.float32)
            row[32:40] = 2.0
            row[32 + k] = 1.0
            _set_row(pr["field"], row)
            rgb = _np(pr["field"](pr["x"], pr["d"])[1]).astype(np.float64)
            cin = pr["f16"][:, j].astype(np.float64)[:, None]
            want, logit = P.expected_rgb(cin, (0,), True)
            bar = P.rgb_bar_f16(want, logit, (16,))           # (a geo_feat input: bit-exact, the bar is the output's own rounding)
            assert (np.abs(rgb[:, c:c + 1] - want) <= bar).all(), (c, k)
            others = [o for o in range(3) if o != c]
            assert (rgb[:, others] == 0.5).all(), (c, k)
            assert np.abs(want - 0.5).max() > 0.2


# ---- full weights against the reference's fp32 outputs -----------------------------------------------------------------------------------
def parity_figures(model, fx, times=BS.TIMES):
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
        fig[name] = {"sigma": BS.dist3(np.concatenate(gs), np.concatenate(ws), rel_floor=1.0), "rgb": BS.dist3(np.concatenate(gc), np.concatenate(wc))}
    del model.fused_inference
    return fig


def test_fused_forward_keeps_the_op_by_op_distance_to_the_reference(rig):
    """With the fixture's weights: the fused kernel (through NeRFNetwork.forward's dispatch) stays within twice each of max, p99.9 and
    mean of the distance the op-by-op autocast evaluation keeps to the reference's fp32 outputs -- both carry the same fp16 roundings in
    different accumulation orders; a factor of two separates reordering from a wrong operand.  Measured on an MI355X
    (profiles/basis_field_parity.txt): see there."""
    r = rig
    _load(r["model"], r["fixture_state"])
    try:
        fig = parity_figures(r["model"].eval(), r["fx"])
    finally:
        _load(r["model"], r["state"])
    print(fig)
    for out in ("sigma", "rgb"):
        for i, what in enumerate(("max", "p99.9", "mean")):
            assert fig["fused"][out][i] <= 2 * fig["op-by-op"][out][i], (out, what, fig)
    assert fig["op-by-op"]["sigma"][2] > 0        # (the bars are not vacuous: the op-by-op path is not the fp32 one)
