"""The fused field kernels (csrc/field_f16_net.h through field.hip / field_pp.inc, csrc/field_f32_net.h through field_f32.hip /
field_f32x3.hip) held stage by stage to the CPU oracle through probe weights (tests/field_probe_support.py: weights under which sigma
and rgb are read-outs of one internal stage; validated without a GPU by tests/test_field_probes_cpu.py).  No kernel, header or ABI is
touched: the probes are ordinary model weights, packed by `pack_weights` / the fp32 packers and launched through the existing entry points.
Run with -s for the measured distance to each derived bar, per stage and kernel variant."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import field_probe_support as P  # noqa: E402


def _load(model, st):
    with torch.no_grad():
        for name, net in (("deform_net", model.deform_net), ("sigma_net", model.sigma_net), ("color_net", model.color_net)):
            for i, lin in enumerate(net):
                lin.weight.copy_(torch.from_numpy(st[f"{name}.{i}.weight"]))


def _set_table(model, table, fields=()):
    with torch.no_grad():
        model.encoder.embeddings.copy_(torch.from_numpy(table.astype(np.float32)))
    for f in fields:
        f.load_table(model.encoder.embeddings.detach())


def _repack(f, t):
    """The probe weights now in the model -> the field's packed weights and the time constants computed from them."""
    f.weights.copy_(f._packed())
    f.invalidate_time_cache()
    f._group_cache.clear()
    f.set_time(t)


def _rig(bound, n_uniform):
    from dnerf_amd.bench_scene import build_model
    geo = P.Geometry(bound)
    model = build_model(0, "cuda", bound)
    assert float(model.density_scale) == 1.0 and np.array_equal(model.encoder.offsets.cpu().numpy(), geo.offsets)
    assert np.float32(np.log2(model.encoder.per_level_scale)) == geo.S
    table = P.random_table(geo)
    _set_table(model, table)
    x, sets = P.point_sets(geo, n_uniform=n_uniform)
    f16, f32r = P.oracle_features(geo, x, table), P.oracle_features(geo, x, table.astype(np.float32))
    P.assert_coverage(geo, x, sets, f16)
    d = torch.from_numpy(np.resize(P.unit_dirs(), (x.shape[0], 3))).cuda().contiguous()
    return dict(geo=geo, model=model, table=table, x=x, sets=sets, f16=f16, f32=f32r, xg=torch.from_numpy(x).cuda(), d=d,
                st=P.blank_state(geo, table))


@pytest.fixture(scope="module")
def rig():
    return _rig(1, 1536)


def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _check16(sig, f_ref, outside, what):
    ok, stats = P.grid_bar_f16(sig, f_ref)
    assert ok.all(), (what, stats)
    assert (sig[outside] == 1.0).all(), what          # zero features: sigma = density_scale * exp(0), exactly
    return stats


def _merge(acc, stats):
    for k, v in stats.items():
        if k == "strict_share":
            acc[k] = min(acc.get(k, v), v)
        else:
            acc[k] = max(acc.get(k, v), v) if k.startswith("worst") or k == "small_share" else acc.get(k, 0) + v
    return acc


def test_grid_stage_every_feature_through_the_quad_kernel(rig):
    """density logit = grid feature j, j = 0..31, on the engineered points (u in {0, 1}, just outside, wrap rows of every capped level,
    integer q, uniform): float16(log sigma) is the oracle's at::Half feature bit for bit; the canonical frame (t = 0: no deformation
    path) and t = 0.5 (x + 0) agree bit for bit."""
    from dnerf_amd import fused
    r = rig
    f = fused.FusedField(r["model"], 0.0, table_layout="quad")
    acc = {}
    for j in range(32):
        _load(r["model"], P.set_grid_probe(r["st"], j))
        _repack(f, 0.0)
        s0 = _np(f(r["xg"], r["d"])[0])
        f.set_time(0.5)
        s5 = _np(f(r["xg"], r["d"])[0])
        assert np.array_equal(s0, s5), j
        _merge(acc, _check16(s0, r["f16"][:, j], r["sets"]["outside"], j))
    assert acc["small_share"] <= P.MAX_SMALL_SHARE
    print(P.line("grid", "f16 quad one-tile x32", acc))


def test_grid_stage_every_fp16_variant_agrees_and_is_exact(rig):
    """A fixed subset of 8 features (both channels of level 0, the last dense level, the coarsest capped level, level 15) through the
    padded layout, the reference layout (direct sdn_field_forward_f16 call), launches of 1, 255, 256 and 257 points, a live list with
    the count on the device, and the persistent kernel at its smallest size + 77: each held to the oracle, all equal bit for bit."""
    import sdn_backend
    from sdn_backend import check, ptr, stream
    from dnerf_amd import fused
    r = rig
    x, d, n = r["xg"], r["d"], r["x"].shape[0]
    out = r["sets"]["outside"]
    fq = fused.FusedField(r["model"], 0.5, table_layout="quad")
    fp = fused.FusedField(r["model"], 0.5, table_layout="pad")
    emb = r["model"].encoder.embeddings.detach().half().contiguous()
    off = np.ascontiguousarray(r["geo"].offsets.astype(np.int32))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = 4 * cus * 256 + 77
    rep = np.resize(np.arange(n), big)
    xb, db = x[torch.from_numpy(rep).cuda()].contiguous(), d[torch.from_numpy(rep).cuda()].contiguous()
    idx = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))[: n // 3].to(torch.int32).contiguous()
    cnt = torch.tensor([idx.shape[0]], dtype=torch.int32, device="cuda")
    sel = sdn_backend.lib.sdn_field_select_kernel
    acc = {k: {} for k in ("quad", "pad", "reference", "sizes", "live list", "persistent")}
    try:
        for j in P.variant_features(r["geo"]):
            _load(r["model"], P.set_grid_probe(r["st"], j))
            ref = r["f16"][:, j]
            for t in (0.5, 0.0):
                _repack(fq, t); _repack(fp, t)
                sel(0)
                sq, cq = fq(x, d)
                sq, cq = sq.clone(), cq.clone()
                _merge(acc["quad"], _check16(_np(sq), ref, out, (j, t)))
                sp, cp = fp(x, d)
                assert torch.equal(sp, sq) and torch.equal(cp, cq), (j, t, "pad")
                _merge(acc["pad"], _check16(_np(sp), ref, out, (j, t, "pad")))
                sr, cr = torch.full_like(sq, -1.0), torch.full_like(cq, -1.0)
                check(sdn_backend.lib.sdn_field_forward_f16(ptr(x, torch.float32, "xyzs"), ptr(d, torch.float32, "dirs"), ptr(None), ptr(None), n,
                                                            ptr(fp.weights), ptr(fp.bias0), ptr(emb, torch.float16, "embeddings"), off.ctypes.data,
                                                            fp.S, fp.H, fp.bound, fp.density_scale, fp.zero_deform, ptr(sr), ptr(cr), stream()),
                      "field_forward_f16")
                assert torch.equal(sr, sq) and torch.equal(cr, cq), (j, t, "reference layout")
                _merge(acc["reference"], _check16(_np(sr), ref, out, (j, t, "reference")))
                for m in (1, 255, 256, 257):
                    sm, cm = fq(x[:m].contiguous(), d[:m].contiguous())
                    assert torch.equal(sm, sq[:m]) and torch.equal(cm, cq[:m]), (j, t, m)
                    ok, st = P.grid_bar_f16(_np(sm), ref[:m])
                    assert ok.all(), (j, t, m, st)
                    _merge(acc["sizes"], st)
                # live list: the listed slots exact, the others untouched
                fq._buf[0].fill_(-1.0); fq._buf[1].fill_(-1.0)
                sl, cl = fq(x, d, live_idx=idx, live_count=cnt)
                keep = torch.ones(n, dtype=torch.bool, device="cuda"); keep[idx.long()] = False
                assert bool((sl[keep] == -1).all()) and bool((cl[keep] == -1).all())
                assert torch.equal(sl[~keep], sq[~keep]) and torch.equal(cl[~keep], cq[~keep])
                ok, st = P.grid_bar_f16(_np(sl[~keep]), ref[_np(~keep).astype(bool)])
                assert ok.all(), (j, t, "live", st)
                _merge(acc["live list"], st)
            # the persistent two-set kernel against the one-tile kernel and the oracle (t = 0 left from the loop above: canonical frame)
            for t in (0.0, 0.5):
                fq.set_time(t)
                sel(0)
                s1, c1 = fq(xb, db)
                s1, c1 = s1.clone(), c1.clone()
                sel(1)
                s2, c2 = fq(xb, db)
                assert torch.equal(s1, s2) and torch.equal(c1, c2), (j, t, "persistent")
                ok, st = P.grid_bar_f16(_np(s2), ref[rep])
                assert ok.all(), (j, t, "persistent", st)
                _merge(acc["persistent"], st)
    finally:
        sel(-1)
    for k, v in acc.items():
        print(P.line("grid", "f16 " + k, v))


@pytest.mark.parametrize("variant", ["mfma32", "split"])
def test_grid_stage_fp32_kernels(rig, variant):
    """The same points and features through sdn_field_forward_f32 / _f32x3 against the oracle's float32 trilinear arithmetic."""
    from dnerf_amd.fused_f32 import FusedFieldF32
    r = rig
    f = FusedFieldF32(r["model"], 0.0, variant=variant)
    acc = {}
    dfm = torch.full((r["x"].shape[0], 3), -1.0, device="cuda")
    for j in P.variant_features(r["geo"]):
        _load(r["model"], P.set_grid_probe(r["st"], j))
        got = []
        for t in (0.0, 0.5):
            _repack(f, t)
            s, _ = f(r["xg"], r["d"], deform=dfm)
            got.append(_np(s))
            assert not dfm.any()
        assert np.array_equal(got[0], got[1]), j
        ok, st = P.grid_bar_f32(got[0], r["f32"][:, j], P.F32_BAR[variant])
        print(P.line("grid", f"f32 {variant} feature {j}", st))
        assert ok.all(), (j, st)
        assert (got[0][r["sets"]["outside"]] == 1.0).all()
        _merge(acc, st)
    print(P.line("grid", "f32 " + variant, acc))


@pytest.mark.parametrize("fp32", [False, True])
def test_grid_stage_cell_query(rig, fp32):
    """sdn_density_query_cells_f16 / _f32 with explicit noise (each cell's point is known: dnerf/renderer.py:480-490), two features, the
    first 32^3 cells of the slice."""
    import raymarching
    from dnerf_amd import fused
    from dnerf_amd.fused_f32 import FusedFieldF32
    r = rig
    m = r["model"]
    n = 32 ** 3
    g = torch.Generator(device="cuda").manual_seed(6)
    noise = torch.rand(n, 3, device="cuda", generator=g)
    coords = raymarching.morton3D_invert(torch.arange(n, device="cuda", dtype=torch.int32))
    half_grid = 1.0 / m.grid_size
    pts = (2 * coords.float() / (m.grid_size - 1) - 1) * (1.0 - half_grid)
    pts += (noise * 2 - 1) * half_grid
    xs = _np(pts)
    table = r["table"].astype(np.float32) if fp32 else r["table"]
    ref = P.oracle_features(r["geo"], xs, table)
    f = FusedFieldF32(m, 0.5, variant="mfma32") if fp32 else fused.FusedField(m, 0.5)
    acc = {}
    for j in (2 * r["geo"].capped[0], 31):
        _load(m, P.set_grid_probe(r["st"], j))
        _repack(f, 0.5)
        out = torch.full((m.grid_size ** 3,), -1.0, device="cuda")
        f.query_cells(out, f.bias0, f.zero_deform, 1.0, n=n, noise=noise)
        assert bool((out[n:] == -1).all())
        ok, st = P.grid_bar_f32(_np(out[:n]), ref[:, j], P.F32_BAR["mfma32"]) if fp32 else P.grid_bar_f16(_np(out[:n]), ref[:, j])
        assert ok.all(), (j, st)
        _merge(acc, st)
    print(P.line("grid", "cells " + ("f32" if fp32 else "f16"), acc))


def test_grid_stage_in_a_box_of_bound_2():
    """bound = 2: u = (x + 2) / 4, a finest level of 4096 and other level sizes; the same sets rebuilt for that geometry."""
    from dnerf_amd import fused
    from dnerf_amd.fused_f32 import FusedFieldF32
    r = _rig(2, 512)
    f = fused.FusedField(r["model"], 0.5, table_layout="quad")
    f3 = FusedFieldF32(r["model"], 0.5, variant="mfma32")
    acc, acc3 = {}, {}
    for j in P.variant_features(r["geo"]):
        _load(r["model"], P.set_grid_probe(r["st"], j))
        _repack(f, 0.5); _repack(f3, 0.5)
        _merge(acc, _check16(_np(f(r["xg"], r["d"])[0]), r["f16"][:, j], r["sets"]["outside"], j))
        ok, st = P.grid_bar_f32(_np(f3(r["xg"], r["d"])[0]), r["f32"][:, j], P.F32_BAR["mfma32"])
        assert ok.all(), (j, st)
        _merge(acc3, st)
    print(P.line("grid", "f16 quad bound 2", acc))
    print(P.line("grid", "f32 mfma32 bound 2", acc3))


def test_wiring_of_sigma_outputs_geo_features_and_sh_into_the_colour_net(rig):
    """sigma-net output k = feature k, colour logit c = GAIN * (one of the colour net's 31 inputs [SH(16), geo_feat(15)]), three inputs
    per launch: a swapped, negated or mis-scaled SH component or geo column moves rgb by far more than the bar (about 1e-3)."""
    from dnerf_amd import fused
    from dnerf_amd.fused_f32 import FusedFieldF32
    r = rig
    dirs = P.unit_dirs()
    n = dirs.shape[0]
    xs = r["x"][r["sets"]["uniform"][:n]]
    x, d = torch.from_numpy(xs).cuda(), torch.from_numpy(dirs).cuda()
    cin16 = P.colour_inputs(dirs, P.oracle_features(r["geo"], xs, r["table"]), True)
    cin32 = P.colour_inputs(dirs, P.oracle_features(r["geo"], xs, r["table"].astype(np.float32)), False)
    f = fused.FusedField(r["model"], 0.5)
    f32s = {v: FusedFieldF32(r["model"], 0.5, variant=v) for v in ("mfma32", "split")}
    worst, worst32 = 0.0, {v: 0.0 for v in f32s}
    for inputs in P.WIRING_LAUNCHES:
        _load(r["model"], P.set_wiring_probe(r["st"], inputs))
        _repack(f, 0.5)
        s, c = f(x, d)
        want, logit = P.expected_rgb(cin16, inputs, True)
        bar = P.rgb_bar_f16(want, logit, inputs)
        err = np.abs(_np(c) - want)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (inputs, float((err / bar).max()))
        ok, st = P.grid_bar_f16(_np(s), P.oracle_features(r["geo"], xs, r["table"])[:, 0])
        assert ok.all(), (inputs, st)
        want32, _ = P.expected_rgb(cin32, inputs, False)
        for v, ff in f32s.items():
            _repack(ff, 0.5)
            _, c3 = ff(x, d)
            rel = np.abs(_np(c3) - want32) / (P.F32_OUT_RTOL[v] * np.abs(want32) + 1e-6)
            worst32[v] = max(worst32[v], float(rel.max()))
            assert (rel <= 1).all(), (v, inputs, float(rel.max()))
    print(P.line("wiring", "f16 quad", {"worst_err_over_bar": worst, "points": n, "inputs": 31}))
    for v in f32s:
        print(P.line("wiring", "f32 " + v, {"worst_err_over_bar": worst32[v], "points": n, "inputs": 31}))


def test_frequency_encoder_deformation_chain_and_the_hand_off_to_the_grid():
    """dx[a] = DEFORM_G * (input cols[a] of the first deformation layer), the table a ramp of one axis, density logit = feature 0: sigma
    reads the coordinate that reached the grid.  All 63 columns of freq(x, 10) (their order inside the kernel) and the 13 time columns
    (the host's bias row, at a time that is neither 0 nor 0.5); dx is added in fp32 to the unrounded x; points that only the
    deformation carries out of the box read the zero-feature sigma; t = 0 ignores the deformation (bit 0 of zero_deform)."""
    from dnerf_amd import fused
    from dnerf_amd.bench_scene import build_model
    from dnerf_amd.fused_f32 import FusedFieldF32
    geo = P.Geometry(1)
    model = build_model(0, "cuda", 1)
    rng = np.random.default_rng(8)
    n, t = 1500, 0.37
    xs = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    x = torch.from_numpy(xs).cuda()
    d = torch.from_numpy(np.resize(P.unit_dirs(), (n, 3))).cuda().contiguous()
    enc = P.deform_inputs(xs, t)
    tables = [P.ramp_table(geo, a) for a in range(3)]
    _set_table(model, tables[0])
    st = P.set_grid_probe(P.blank_state(geo, tables[0]), 0)
    f = fused.FusedField(model, t)
    f32s = {v: FusedFieldF32(model, t, variant=v) for v in ("mfma32", "split")}
    packed, packed32 = [], {v: [] for v in f32s}
    for cols in P.DEFORM_LAUNCHES:
        _load(model, P.set_deform_probe(st, cols))
        _repack(f, t)
        packed.append((f.weights.clone(), f.bias0.clone()))
        for v, ff in f32s.items():
            _repack(ff, t)
            packed32[v].append((ff.weights.clone(), ff.bias0.clone()))
    acc, left_box, worst_dx = {}, 0, {v: 0.0 for v in f32s}
    dfm = torch.empty(n, 3, device="cuda")
    for axis in range(3):
        _set_table(model, tables[axis], [f] + list(f32s.values()))
        plain = P.oracle_features(geo, xs, tables[axis])[:, 0]
        for k, cols in enumerate(P.DEFORM_LAUNCHES):
            e = enc[:, list(cols)]
            f.weights.copy_(packed[k][0]); f.bias0 = packed[k][1]; f.zero_deform = 0
            sig = _np(f(x, d)[0])
            ok, stat = P.deform_bar_f16(geo, xs, e, cols, tables[axis], sig)
            assert ok.all(), (axis, cols, stat)
            xd = P.deformed_points_f16(xs, e)
            gone = ~((geo.u_of(xd) >= 0) & (geo.u_of(xd) <= 1)).all(1)
            assert (sig[gone & (np.abs(geo.u_of(xd) - 0.5) > 0.5 + 1e-4).any(1)] == 1.0).all()      # zero features: sigma = 1 exactly
            left_box += int(gone.sum())
            _merge(acc, stat)
            if k % 9 == 0:                     # the canonical frame with the same weights: the deformation is ignored
                f.zero_deform = 1
                ok0, st0 = P.grid_bar_f16(_np(f(x, d)[0]), plain)
                assert ok0.all(), (axis, cols, "t = 0", st0)
            if axis == 0 or k % 9 == 0:      # fp32 kernels: the deformation itself (every column once), and sigma through it
                for v, ff in f32s.items():
                    ff.weights.copy_(packed32[v][k][0]); ff.bias0 = packed32[v][k][1]; ff.zero_deform = 0
                    s3 = _np(ff(x, d, deform=dfm)[0])
                    dx_ref = (np.float32(P.DEFORM_G) * e).astype(np.float64)
                    tol = P.F32_OUT_RTOL[v] * np.abs(dx_ref) + 1e-6
                    err = np.abs(_np(dfm) - dx_ref)
                    worst_dx[v] = max(worst_dx[v], float((err / tol).max()))
                    assert (err <= tol).all(), (v, axis, cols, float((err / tol).max()))
                    u = (xs.astype(np.float64) + dx_ref + 1.0) / 2.0
                    safe = ((u > 1e-3) & (u < 1 - 1e-3)).all(1)          # (away from the range test: a 1e-4 dx must not flip it)
                    want = P.oracle_features(geo, (xs + dx_ref).astype(np.float32), tables[axis].astype(np.float32))[:, 0]
                    # feature 0 = (15 u + 0.5) / 16: slope 15 / 32 in x; + the float32 rounding of x + dx (2^-24) and the grid bar
                    bar = 15.0 / 32.0 * (tol.max(1) + 2.0 ** -23) + P.F32_BAR[v]
                    assert (np.abs(P.decode(s3) - want)[safe] <= bar[safe]).all(), (v, axis, cols)
    assert left_box > 0
    acc["left_the_box"] = left_box
    print(P.line("deform", "f16 quad 76 columns", acc))
    for v in f32s:
        print(P.line("deform", "f32 " + v, {"worst_dx_err_over_bar": worst_dx[v]}))
