"""The fused field kernels at the edges of their operand ranges, and the inference compositor on an infinite sigma.  Section A: the
deformation model's fp32 kernels, kind 1 (csrc/field_f32.hip, fp32 MFMAs) and kind 2 (csrc/field_f32x3.hip, split fp16 operands);
section B: the fp16 kernels, kinds 0 (field.hip), 3 (field_basis.hip) and 4 (field_hyper.hip), forward and CELLS, on a freshly
initialised table; section C: the output stage of all six kinds (5: field_basis_f32.hip); section D: raymarching.composite_rays.
Probe states, the exact rescaling, the float64 restatement and every set of points a case names come from tests/field_range_support.py
(validated without a GPU by tests/test_field_ranges_cpu.py); the expected value is always that restatement, never another run of a
kernel.  Every launch is 513 points.  Run with -s for the measured distance to each bar.

Measured on an MI355X, worst error as a share of the bar that applies (sigma, rgb), over all magnitudes of the case:
  A.1 split, |x| 2^-8 .. 1023      D1 0.004, 0.000   D4 0.004, 0.000   S1 0.001, 0.001   C1 0.000, 0.001   (2^-7, the whole launch inside the
                                   envelope and held to the plain bar: the same figures)
  A.2 split, |x| 2^-12, 2^-16      D1 0.001, 0.000   D4 0.001, 0.000   S1 0.000, 0.000   C1 0.000, 0.000   (of the derived bar; under 0.01 of the
                                   plain bar too: on this hardware the subnormal lo parts are not lost -- the bound is the guarantee)
  A.3 split, |x| = 1100            every overflowing point non-finite (D1, D4: 103 of 103 in sigma and rgb; S1: 205 of 205 in both; C1: 205 of
                                   205 in rgb, sigma finite and right); the other points 0.004, 0.001.  On the parent commit D1, D4 and C1
                                   returned FINITE values on all of them (dx = 0, rgb = 0.5): the ReLU dropped NaNs with the sign bit set
  A.4 split, |w| 2^-10, 1, 255     0.001, 0.002;  256 refused (the parent packed an infinity)
  A   mfma32, |x| 2^-16 .. 2^12    D1 0.001, 0.001   D4 0.001, 0.001   S1 0.001, 0.001   C1 0.000, 0.003
  B   kinds 0, 3 and 4: the FIRST outcome for each -- the kernel agrees with the restatement that KEEPS subnormals, bit for bit in
      float16(log sigma), and so does the model's op-by-op -O forward.  max |sigma / ref - 1| of kernel and of op-by-op against "kept":
      1.2e-7, 0, 1.2e-7 (features 0, 1, 31) for every kind; against a flushed operand both would be off by 0.284, 0.221, 0.281 (kinds 0
      and 3) and 0.284, 0.221, 0.283 (kind 4).  Subnormal features of 513: 337, 337, 454 (kinds 0, 3) and 344, 344, 435 (kind 4, at its
      own ambient coordinate).  The CELLS kernel of each kind equals its forward kernel bit for bit on this table.
  C   sigma, rgb at density_scale 1 | 2^-8:  kind 0: 1.000, 0.000 | 0.233, 0.000;  kind 3: 1.000, 0.000 | 0.233, 0.000;  kind 4: 1.000,
      0.000 | 0.335, 0.000;  kind 1: 0.001, 0.000 both;  kind 2: 0.000, 0.000 both;  kind 5: 0.001, 0.000 both; infinite sets equal in
      all twelve runs.  (The 1.000 of the fp16 kinds at scale 1: exp(-103.94) is 2^-149 in the reference and 0 in the kernel -- one
      spacing of the float32 subnormals, the whole of that allowance.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import field_probe_support as P  # noqa: E402
import field_range_support as R  # noqa: E402
from oracle import oracle as O  # noqa: E402


def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _load(model, st):
    with torch.no_grad():
        for name, net in (("deform_net", model.deform_net), ("sigma_net", model.sigma_net), ("color_net", model.color_net)):
            for i, lin in enumerate(net):
                lin.weight.copy_(torch.from_numpy(st[f"{name}.{i}.weight"]))


def _repack(f, t=R.T):
    f.weights.copy_(f._packed())
    f.invalidate_time_cache()
    f._group_cache.clear()
    f.set_time(t)


def _set_table(model, table, fields=()):
    with torch.no_grad():
        model.encoder.embeddings.copy_(torch.from_numpy(table.astype(np.float32)))
    for f in fields:
        f.load_table(model.encoder.embeddings.detach())


@pytest.fixture(scope="module")
def rig():
    from dnerf_amd.bench_scene import build_model
    from dnerf_amd.fused_f32 import FusedFieldF32
    geo = P.Geometry(1)
    model = build_model(0, "cuda", 1)
    assert float(model.density_scale) == 1.0 and np.array_equal(model.encoder.offsets.cpu().numpy(), geo.offsets)
    table = R.a_table(geo)
    _set_table(model, table)
    x, d = R.a_points(geo)
    fields = {v: FusedFieldF32(model, R.T, variant=v) for v in ("mfma32", "split")}
    return dict(geo=geo, model=model, table=table, x=x, d=d, xg=torch.from_numpy(x).cuda(), dg=torch.from_numpy(d).cuda(), fields=fields)


def _run(r, variant, st):
    _load(r["model"], st)
    f = r["fields"][variant]
    _repack(f)
    s, c = f(r["xg"], r["dg"])
    return _np(s).astype(np.float64), _np(c).astype(np.float64)


def _share(got, ref, bar, sel=None):
    e = np.abs(got - ref) / bar
    return float(e.max() if sel is None else e[sel].max())


# ---- A: the split kernel inside, below and above its envelope; the fp32-MFMA kernel has none --------------------------------------------------
@pytest.mark.parametrize("stage", R.A_STAGES)
def test_split_kernel_holds_its_bar_across_the_documented_activation_envelope(rig, stage):
    """|x| entering the stage at 2^-8, 2^-2, 1, 2^9 and 1023 (target points; the others at 0.75 .. 0.91 of it): sigma and rgb within
    2.5e-4 (|ref| + 1e-2) of float64 -- the bar tests/test_gpu_field_f32.py holds the split variant to.  At 2^-8 the non-target points
    lie just below the envelope and get the derived allowance of the next test; the target points do not.
    Measured worst share of the bar (sigma, rgb): the module's docstring."""
    r = rig
    for a in R.A_INSIDE:
        st, L = R.a_state(stage, a)
        ref = R.forward64(st, r["geo"], r["table"], r["x"], r["d"])
        ds, dc, n = R.sub_envelope_bound(st, r["geo"], r["table"], r["x"], r["d"], L, ref)
        assert not n.any() or a == 2.0 ** -8
        s, c = _run(r, "split", st)
        bs, bc = R.split_bar(ref["sigma"]) + ds, R.split_bar(ref["rgb"]) + dc
        print(f"[field-range] A.1 split {stage} |x|={a:g}: sigma {_share(s, ref['sigma'], bs):.3f} rgb {_share(c, ref['rgb'], bc):.3f} of the bar")
        assert (np.abs(s - ref["sigma"]) <= bs).all() and (np.abs(c - ref["rgb"]) <= bc).all(), (stage, a)


@pytest.mark.parametrize("stage", R.A_STAGES)
def test_split_kernel_below_its_envelope_loses_one_lo_part_per_term_and_no_more(rig, stage):
    """|x| = 2^-12 and 2^-16: the lo part of 2^6 x is an fp16 subnormal and is lost, hi alone carries 11 bits: that term may be off by
    2^-11 of itself.  One weight takes at most 2^7 back (|w| <= 255), so at 2^-16 the next layer's operand (2^-9) is below the envelope
    too: the allowance is 2^-11 per such term, counted from the restatement's operands (`sub_envelope_bound`), plus the file's bar."""
    r = rig
    for a in R.A_BELOW:
        st, L = R.a_state(stage, a)
        ref = R.forward64(st, r["geo"], r["table"], r["x"], r["d"])
        ds, dc, n = R.sub_envelope_bound(st, r["geo"], r["table"], r["x"], r["d"], L, ref)
        assert (n >= 1).all() and n.max() <= 2
        s, c = _run(r, "split", st)
        bs, bc = R.split_bar(ref["sigma"]) + ds, R.split_bar(ref["rgb"]) + dc
        plain = max(_share(s, ref["sigma"], R.split_bar(ref["sigma"])), _share(c, ref["rgb"], R.split_bar(ref["rgb"])))
        print(f"[field-range] A.2 split {stage} |x|={a:g}: sigma {_share(s, ref['sigma'], bs):.3f} rgb {_share(c, ref['rgb'], bc):.3f} of the "
              f"derived bar ({int(n.max())} terms); {plain:.2f} of the plain bar")
        assert (np.abs(s - ref["sigma"]) <= bs).all() and (np.abs(c - ref["rgb"]) <= bc).all(), (stage, a)


@pytest.mark.parametrize("stage", R.A_STAGES)
def test_split_kernel_above_its_envelope_is_loud(rig, stage):
    """|x| = 1100 on the target points: 2^6 x is the fp16 infinity, its lo part the opposite one, the products NaN.  Every such point
    must come out non-finite in sigma or rgb -- a finite value there would be a wrong one -- and every other point of the same launch
    (825 .. 997) within the bar.  The sets come from the restatement's operands (`overflowing`), not from the kernel's output."""
    r = rig
    st, L = R.a_state(stage, R.A_ABOVE)
    ref = R.forward64(st, r["geo"], r["table"], r["x"], r["d"])
    over, inside = R.overflowing(ref, L)
    s, c = _run(r, "split", st)
    loud = ~np.isfinite(s) | ~np.isfinite(c).all(1)
    print(f"[field-range] A.3 split {stage}: {int(loud[over].sum())} of {int(over.sum())} overflowing points non-finite "
          f"(sigma {int((~np.isfinite(s[over])).sum())}, rgb {int((~np.isfinite(c[over]).all(1)).sum())}); others: sigma "
          f"{_share(s, ref['sigma'], R.split_bar(ref['sigma']), inside):.3f} rgb {_share(c, ref['rgb'], R.split_bar(ref['rgb']), inside):.3f} of the bar")
    assert loud[over].all(), (stage, int((~loud[over]).sum()), s[over][~loud[over]][:4], c[over][~loud[over]][:4])
    assert (np.abs(s - ref["sigma"]) <= R.split_bar(ref["sigma"]))[inside].all() and (np.abs(c - ref["rgb"]) <= R.split_bar(ref["rgb"]))[inside].all()


def test_split_kernel_weight_envelope_and_the_refusal_above_it(rig):
    """|w| = 2^-10, 1 and 255 on the last sigma layer (the density row the value itself, the geo row with a non-empty lo part): within
    the bar.  |w| = 256: `pack_weights_f32_split` refuses, naming the layer; the field keeps its previous weights."""
    import sdn_backend
    r = rig
    for w in R.A_WEIGHTS:
        st = R.weight_state(w)
        ref = R.forward64(st, r["geo"], r["table"], r["x"], r["d"])
        s, c = _run(r, "split", st)
        bs, bc = R.split_bar(ref["sigma"]), R.split_bar(ref["rgb"])
        print(f"[field-range] A.4 split |w|={w:g}: sigma {_share(s, ref['sigma'], bs):.3f} rgb {_share(c, ref['rgb'], bc):.3f} of the bar")
        assert (np.abs(s - ref["sigma"]) <= bs).all() and (np.abs(c - ref["rgb"]) <= bc).all(), w
    before = r["fields"]["split"].weights.clone()
    _load(r["model"], R.weight_state(256.0))
    with pytest.raises(sdn_backend.SdnError, match="S1"):
        _repack(r["fields"]["split"])
    assert torch.equal(r["fields"]["split"].weights, before)
    _repack(r["fields"]["mfma32"])                        # the fp32-MFMA kernel takes the same model


@pytest.mark.parametrize("stage", R.A_STAGES)
def test_fp32_mfma_kernel_has_no_envelope(rig, stage):
    """The same sweep, 2^-16 .. 2^12 (1100 included), through csrc/field_f32.hip: rtol 1e-4 / atol 1e-6 at every magnitude."""
    r = rig
    for a in R.A_MFMA32:
        st, _ = R.a_state(stage, a, cap=None)
        ref = R.forward64(st, r["geo"], r["table"], r["x"], r["d"])
        s, c = _run(r, "mfma32", st)
        bs, bc = R.mfma32_bar(ref["sigma"]), R.mfma32_bar(ref["rgb"])
        print(f"[field-range] A mfma32 {stage} |x|={a:g}: sigma {_share(s, ref['sigma'], bs):.3f} rgb {_share(c, ref['rgb'], bc):.3f} of the bar")
        assert (np.abs(s - ref["sigma"]) <= bs).all() and (np.abs(c - ref["rgb"]) <= bc).all(), (stage, a)


# ---- the six kinds behind one rig ------------------------------------------------------------------------------------------------------------------
KIND_MODEL = {0: "dnerf", 1: "dnerf", 2: "dnerf", 3: "basis", 4: "hyper", 5: "basis"}
HALF_KINDS = (0, 3, 4)


def _load_heads(model, st):
    with torch.no_grad():
        for key, w in st.items():
            net, i, _ = key.split(".")
            getattr(model, net)[int(i)].weight.copy_(torch.from_numpy(w))


def _refresh(f):
    """The probe weights now in the model -> the field's packed weights and its constants row (the basis model's row comes from the
    probe `basis_net`, the ambient model's from its own `ambient_net`)."""
    f.weights.copy_(f._packed())
    f.invalidate_time_cache()
    f._group_cache.clear()
    f.set_time(R.T)


def _kind_rig(kind, make_table, x):
    """Model, field and expected grid features of field kind `kind` on the table `make_table(geometry, half, dim)`.  Kinds 3 and 5: the
    temporal-basis mirror with `basis_net` replaced by a probe under which the model's own row is e_0 + e_32 (`R.basis_row`, also set
    with the `_set_row` technique); kind 4: the ambient-dimension mirror, its 4-D grid, the ambient coordinate its `ambient_net` gives."""
    half = kind in HALF_KINDS
    name = KIND_MODEL[kind]
    geo = P.Geometry(1)
    if name == "dnerf":
        from dnerf_amd import fused
        from dnerf_amd.bench_scene import build_model
        from dnerf_amd.fused_f32 import FusedFieldF32
        model = build_model(0, "cuda", 1).eval()
        table = make_table(geo, half, 3)
        _set_table(model, table)
        field = fused.FusedField(model, R.T) if kind == 0 else FusedFieldF32(model, R.T, variant="split" if kind == 2 else "mfma32")
        feats = P.oracle_features(geo, x, table)
    elif name == "basis":
        import basis_support as BS
        from dnerf_amd import fused_basis
        model, _ = BS.mirror_model("cuda", check=False)
        with torch.no_grad():
            for lin, w in zip(model.basis_net, R.basis_net_probe([tuple(l.weight.shape) for l in model.basis_net])):
                lin.weight.copy_(torch.from_numpy(w))
        table = make_table(geo, half, 3)
        _set_table(model, table)
        field = fused_basis.FusedBasisField(model, R.T) if kind == 3 else fused_basis.FusedBasisFieldF32(model, R.T)
        assert np.array_equal(_np(field.bias0), R.basis_row())               # the model's own row is the probe's
        field.bias0 = torch.from_numpy(R.basis_row()).cuda()
        feats = P.oracle_features(geo, x, table)
    else:
        import hyper_support as HS
        from dnerf_amd import fused_hyper
        model, _ = HS.mirror_model("cuda", check=False)
        geo4 = HS.Geometry4(1)
        table = make_table(geo4, half, 4)
        _set_table(model, table)
        field = fused_hyper.FusedHyperField(model, R.T, density_query=True)
        ambient = float(_np(field.bias0)[0])
        assert abs(ambient) < 1.0 and not _np(field.bias0)[1:].any()
        feats = HS.oracle_features(geo4, geo4.u4(x, ambient), table)
    assert float(model.density_scale) == 1.0
    return dict(kind=kind, name=name, half=half, geo=geo, model=model.eval(), table=table, field=field, feats=feats)


def _op_by_op(model, x, d, t):
    keep = model.__dict__.get("fused_inference")
    model.fused_inference = False
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            s, _, _ = model(x, d, torch.tensor([[t]], dtype=torch.float32, device="cuda"))
    finally:
        if keep is None:
            del model.fused_inference
        else:
            model.fused_inference = keep
    return _np(s)


# ---- B: the fp16 kernels on a freshly initialised table ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=HALF_KINDS)
def fresh(request):
    geo = P.Geometry(1)
    x, d, slab = R.b_points(geo)
    r = _kind_rig(request.param, lambda g, half, dim: R.b_table(g, dim=dim), x)
    r.update(x=x, d=d, slab=slab, xg=torch.from_numpy(x).cuda(), dg=torch.from_numpy(d).cuda())
    return r


@pytest.mark.parametrize("j", R.B_FEATURES)
def test_fp16_kernels_on_subnormal_grid_features(fresh, j):
    """Kinds 0, 3 and 4 on the table of an untrained `GridEncoder` (+-1e-4: most entries fp16 subnormals) with slabs of 1e-4, 2^-14,
    2^-15, 2^-20 and 2^-24 of either sign; density logit = 2^12 x feature j, so sigma = exp(2^12 f) separates a kept subnormal from a
    flushed one (2^-15: 1.133 against 1).  Against (a) the fp16 restatement with subnormals kept and (b) the model's own op-by-op forward
    under autocast.  Outcome (module docstring): the first for every kind -- kernel and op-by-op network both keep subnormals; asserted
    against (a) for both, with the kernels' existing sigma bar (float16(log sigma) is the logit bit for bit)."""
    r = fresh
    _load_heads(r["model"], R.b_state(j, r["name"]))
    _refresh(r["field"])
    got = _np(r["field"](r["xg"], r["dg"])[0])
    ops = _op_by_op(r["model"], r["xg"], r["dg"], R.T)
    f = r["feats"][:, j]
    kept, logit = R.b_expected(f)
    flushed, _ = R.b_expected(f, flush_subnormal_operands=True)
    sub = np.abs(f.astype(np.float32)) < 2.0 ** -14
    rel = lambda a, b: float(np.abs(a / b - 1).max())  # noqa: E731
    print(f"[field-range] B kind {r['kind']} feature {j}: {int(sub.sum())} subnormal features of {R.N}; max |sigma / ref - 1|: kernel vs kept "
          f"{rel(got, kept):.3g}, kernel vs flushed {rel(got, flushed):.3g}, op-by-op vs kept {rel(ops, kept):.3g}, op-by-op vs flushed "
          f"{rel(ops, flushed):.3g}, kernel vs op-by-op {rel(got, ops):.3g}")
    assert sub.sum() > R.N // 2 and rel(kept, flushed) > 0.05
    ok, stats = P.grid_bar_f16(got, logit)
    assert ok.all(), (r["kind"], j, stats)
    ok, stats = P.grid_bar_f16(ops, logit)
    assert ok.all(), (r["kind"], j, "op-by-op", stats)


def test_fp16_cells_kernels_equal_their_forward_kernels_on_the_fresh_table(fresh):
    """The CELLS variant of each of kinds 0, 3 and 4 on 513 listed cells of the occupancy grid against its forward kernel on the points
    the reference's torch expressions build for them (dnerf/renderer.py:480-490), bit for bit, on the subnormal table with the 2^12 gain."""
    import basis_density_support as DS
    r = fresh
    m, f = r["model"], r["field"]
    g = torch.Generator(device="cuda").manual_seed(33)
    cells = torch.randperm(m.grid_size ** 3, device="cuda", generator=g)[:R.N].to(torch.int32).contiguous()
    noise = torch.rand(R.N, 3, device="cuda", generator=g)
    pts = DS.torch_points(m, cells, noise)
    _, cell, _ = r["geo"].cell_rows(_np(pts), 0)
    assert np.isin(cell[:, 0], R.B_SLABS).sum() > 100               # a good share of the cells read a slab of listed values
    count = torch.tensor([R.N], dtype=torch.int32, device="cuda")
    for j in R.B_FEATURES:
        _load_heads(m, R.b_state(j, r["name"]))
        _refresh(f)
        out = torch.full((m.grid_size ** 3,), -1.0, device="cuda")
        f.query_cells(out, f.bias0, f.zero_deform, 1.0, cells=cells, cell_count=count, noise=noise)
        s = f(pts, torch.zeros_like(pts))[0]
        assert torch.equal(out[cells.long()], s), (r["kind"], j)
        assert int((out != -1).sum()) == R.N and float(s.max()) > 1.05 and float(s.min()) < 0.95


# ---- C: the output stage ---------------------------------------------------------------------------------------------------------------------------
# The existing sigma bars, relative on sigma: the fp16 kinds decode float16(log sigma) to the logit within 2e-6 + 1e-7 |logit|
# (field_probe_support.DECODE_BAR, basis_support.field_bars); kinds 1 and 5 rtol 1e-4; kind 2 2.5e-4.  A float32-subnormal sigma gets one
# spacing of the format there, 2^-149, on top: the fp16 kernels' exponential returns 0 where float64 rounds exp(-103.94) to 2^-149.
def _sigma_rel(kind, dl):
    if kind in HALF_KINDS:
        return 2e-6 + 1e-7 * np.abs(dl)
    return np.full(dl.shape, R.SPLIT_REL if kind == 2 else R.MFMA32_RTOL)


@pytest.mark.parametrize("scale", R.C_SCALES)
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5])
def test_output_stage_overflows_where_float64_does_and_nowhere_else(kind, scale):
    """Density logits 87, 88.5, 88.8, 100, -87 and -104 (slabs in x) and colour logits +-20, +-90 and 0 (slabs in y, on each channel in
    turn) in one launch, at density_scale 1 and 2^-8, through every field kind.  Expected: float64 exp cast to float32, times the scale
    (`c_expected`: the order in which the case table's 88.8 -> +inf holds at both scales) -- the set of infinite points equal to the
    reference's, the rest within the kernel's existing sigma bar (`_sigma_rel`), a subnormal within one subnormal spacing; rgb within the
    existing rgb bar of float64 sigmoid (fp16 kinds: one fp16 ulp of the output + 2^-20; fp32 kinds: their rtol + 1e-6), inside [0, 1]
    and never NaN; the two channels without a logit exactly 0.5."""
    geo = P.Geometry(1)
    x, d, sx, sy = R.c_points(geo)
    r = _kind_rig(kind, lambda g, half, dim: R.c_table(g, half, dim), x)
    f, half = r["field"], r["half"]
    f.density_scale = float(scale)
    xg, dg = torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()
    worst = [0.0, 0.0]
    for channel in range(3):
        _load_heads(r["model"], R.c_state(channel, r["name"]))
        _refresh(f)
        s, c = (_np(t).astype(np.float64) for t in f(xg, dg))
        dl, cl = R.c_logits(r["feats"], channel)
        assert np.abs(dl - np.asarray(R.C_DENSITY)[sx]).max() <= 0.25 and np.abs(cl[:, channel] - np.asarray(R.C_COLOUR)[sy]).max() <= 0.25
        want_s, want_c = R.c_expected(dl, cl, scale, half)
        inf = np.isinf(want_s)
        assert inf.sum() >= R.N // 6 and (~inf).sum() >= R.N // 2
        assert not np.isnan(s).any() and np.array_equal(np.isinf(s), inf), (kind, scale, channel, int((np.isinf(s) != inf).sum()))
        assert (s[inf] > 0).all()
        fin = ~inf
        bar_s = _sigma_rel(kind, dl)[fin] * np.abs(want_s[fin]) + 2.0 ** -149
        err_s = np.abs(s[fin] - want_s[fin].astype(np.float64))
        worst[0] = max(worst[0], float((err_s / bar_s).max()))
        assert (err_s <= bar_s).all(), (kind, scale, channel, worst)
        assert not np.isnan(c).any() and c.min() >= 0.0 and c.max() <= 1.0, (kind, scale, channel)
        bar = P.rgb_bar_f16(want_c, cl, (16, 16, 16)) if half else (R.SPLIT_REL if kind == 2 else R.MFMA32_RTOL) * np.abs(want_c) + 1e-6
        worst[1] = max(worst[1], float((np.abs(c - want_c) / bar).max()))
        assert (np.abs(c - want_c) <= bar).all(), (kind, scale, channel, worst)
        others = [o for o in range(3) if o != channel]
        assert (c[:, others] == 0.5).all()
    print(f"[field-range] C kind {kind} density_scale {scale:g}: sigma {worst[0]:.3f} rgb {worst[1]:.3f} of the bar")


# ---- D: the consumer of an infinite sigma ------------------------------------------------------------------------------------------------------------
def test_inference_compositor_on_infinite_huge_subnormal_and_zero_sigma():
    """raymarching.composite_rays against oracle.composite_rays on 65 rays x 4 steps (a wave plus one) whose sigmas hold +inf, 3e38, a
    float32 subnormal and 0 at the first, a middle and the last step of different rays, the rest ordinary: weights sum, depth and image
    under the comparison of test_inference_loop_bit_exact_counts (1e-6), all finite; the rays finished exactly where the oracle
    finishes them, the ray times bit for bit."""
    import raymarching
    n, steps = 65, 4
    rng = np.random.default_rng(51)
    sig = (rng.random((n, steps), dtype=np.float32) * 20).astype(np.float32)
    specials = (np.float32(np.inf), np.float32(3e38), np.float32(1e-41), np.float32(0.0))
    k = 0
    for v in specials:
        for step in (0, 2, 3):
            sig[k, step] = v
            k += 1
    sig[k, :] = np.float32(np.inf)
    sig[k + 1, :] = 0.0
    sig[64, 3] = np.float32(np.inf)                                   # the ray of the second wave
    rgb = rng.random((n * steps, 3), dtype=np.float32)
    deltas = np.stack([np.full(n * steps, 0.01, np.float32), np.full(n * steps, 0.0125, np.float32)], 1)
    deltas[4 * 20 + 2:4 * 21] = 0                                      # one ray that ran out of samples after two steps
    alive_r = np.arange(n, dtype=np.int32)[::-1].copy()
    t_r = (0.2 + 0.01 * np.arange(n)).astype(np.float32)
    ws_r, dp_r, im_r = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    alive, t, ws, dp, im = dev(alive_r), dev(t_r), dev(ws_r), dev(dp_r), dev(im_r)
    flat = sig.reshape(-1)
    O.composite_rays(n, steps, alive_r, t_r, flat, rgb, deltas, ws_r, dp_r, im_r, 1e-2)
    raymarching.composite_rays(n, steps, alive, t, dev(flat), dev(rgb), dev(deltas), ws, dp, im, 1e-2)
    assert np.array_equal(alive.cpu().numpy(), alive_r) and 0 < (alive_r < 0).sum() < n
    assert np.array_equal(t.cpu().numpy().view(np.uint32), t_r.view(np.uint32))
    for got, ref in ((ws, ws_r), (dp, dp_r), (im, im_r)):
        assert np.isfinite(ref).all() and bool(torch.isfinite(got).all())
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-6, atol=1e-7)
    assert ws_r.max() <= 1.0 + 1e-6 and (ws_r[::-1][:12] > 0).any()
