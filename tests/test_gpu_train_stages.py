"""The native training steps (csrc/train.hip: sdn_train_step_f16 / sdn_train_step_f32) stage by stage on long, ragged rays.

One `grads_only` call per step and budget; every stage's outputs are then compared with the float64 restatement of THAT stage
(tests/train_stage_support.py, validated on the CPU by tests/test_train_stages_cpu.py) evaluated on the stage's own input buffers as
the GPU left them (`NativeTrainStep.view`).  Nothing chaotic sits between the two sides, so the bars are one stage's rounding and a
failure names the kernel.

The batch: 510 rays (not a multiple of the 4 rays of a compositing workgroup) of the 32 x 32 camera through a wedge-shaped slab whose
thickness grows across the image, so rays own 0 to more than 300 samples -- up to five 64-sample chunks of the wave-per-ray
compositing kernels -- with the density logit scaled so that rays stop in the first chunk, in a later one, or never.  The test asserts
that coverage itself, from the float64 reference on the GPU's sigmas / deltas / rays.  The workspace budget M is always a multiple of
128 (raymarching.py:200-203), so the kernels' `b < M` predicate cannot fail from this class; the partial tile that can be reached is
the 32-sample tile where the rays' samples end (rows behind it are the marcher's zero-filled padding, which the per-sample kernels
still evaluate): the number of owned samples is kept off a multiple of 32 and that tile is compared on its own.

Rays with a sample whose float64 transmittance is within 1e-4 (relative) of T_thresh are left out of the compositing comparisons
(the kernel's float32 prefix product may decide the other way there); at most 2 % of the rays may be.

Bars.  Structural results (zero rows / columns, copies, rows past the owned samples) are exact.  fp32 values against float64: 1e-4
relative with atol 1e-5 x the largest reference magnitude (the project's fp32 bar).  fp16 values that are one rounding of an fp32
result: 1.5 fp16 ulp (relative 1.5 * 2^-10, floor 2^-24).  Matrix-core stages (fp16 in, fp32 accumulate, one fp16 rounding per
layer): the bar of tests/test_gpu_ffmlp_parity.py::_close, 2 (L + 1) fp16 ulp on 99.9 % of the elements and 1 % norm-wise, L the depth
of the stage up to that buffer, per block and on the tail tile alone (a difference of one fp16 subnormal spacing is never counted).
Two allowances on top, in the fp16 step only, both zero for almost every element: (a) dh0 is a DIFFERENCE (T_behind c - (image -
running colour), raymarching.cu:655-675) of float32 prefix sums, so it is not one rounding of a well-conditioned float32 result: on
top of the 1.5 ulp it is allowed S.CANCEL_ULPS (one float32 ulp) of the magnitudes that cancel, a constant measured on the CPU from
a float32 restatement of the kernels against the float64 reference (tests/test_train_stages_cpu.py), not from the kernel; in the
fp32 step the restatement stays inside the plain fp32 bar, which is kept; (b) an fp16 colour whose float64 sigmoid lies within 2^-22
(relative; the bound of the float32 evaluation, derived in train_stage_support.colours) of the midpoint of two fp16 values may round
either way: what depends on it is allowed that one fp16 step, propagated linearly.

Measured on an MI355X (69 065 owned samples, M = 69 120, longest ray 308 samples; 209 rays stop in chunk 0 while owning more, 137 in
a later chunk, 76 rays with samples never stop; no ray near the threshold), worst error in units of its bar: each test's docstring."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import train_stage_support as S

pytestmark = pytest.mark.gpu

N_RAYS = 510
LOSS_SCALE = 1024.0          # the GradScaler's scale of the fp16 step: at 65536 the sums over ~1e5 samples of a weight gradient leave fp16
LOGIT_SCALE = 1.3            # row 0 of the last sigma layer (the density logit) x this: exp() spreads the per-sample densities, so that
                             # rays stop anywhere between the first chunk and never (the coverage asserts below hold the choice)
T_THRESH = float(np.float32(1e-4))


def _np(t):
    return t.detach().cpu().numpy()


_FAILED = {}


def _run(fp32, short):
    """The cached step of a case.  A case whose step raised is not launched again: the tests that share it fail with the same error."""
    if (fp32, short) in _FAILED:
        raise RuntimeError(f"the step of this case already failed: {_FAILED[(fp32, short)]!r}")
    try:
        return _step(fp32, short)
    except BaseException as exc:
        _FAILED[(fp32, short)] = exc
        raise


@functools.lru_cache(maxsize=None)
def _step(fp32, short):
    """One grads_only step; every buffer of it as numpy arrays."""
    from dnerf_amd import scene
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.network import NeRFNetwork
    from dnerf_amd.train_native import NativeTrainStep
    sc = build_scene(H=32, W=32, device="cuda", seed=0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).cuda().train()
    model.load_state_dict(sc.model.state_dict())
    bits = scene._occupancy_to_bitfield(S.wedge_occupancy(sc.pose, int(model.grid_size)), int(model.grid_size))
    with torch.no_grad():
        model.density_bitfield[sc.t_idx].copy_(torch.from_numpy(bits).cuda())       # in place through torch: version-keyed caches follow
        model.sigma_net[-1].weight[0].mul_(LOGIT_SCALE)
    for n in (N_RAYS, N_RAYS - 1):       # the owned samples must not end on a tile boundary: drop a ray if the scene gives a multiple of 32
        rays_o, rays_d = sc.rays_o[:n].contiguous(), sc.rays_d[:n].contiguous()
        model.local_step = 0
        model.step_counter.zero_()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            model.render(rays_o[None], rays_d[None], sc.time, staged=False, perturb=False, bg_color=1, force_all_rays=False)
        owned = int(model.step_counter[0, 0].item())
        if owned % 32 != 0:
            break
    model.mean_count = int(0.6 * owned) if short else owned
    model.local_step = 0
    model.step_counter.zero_()
    opt = torch.optim.Adam(model.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", enabled=not fp32, init_scale=LOSS_SCALE)
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(4)).cuda()
    e = torch.float32 if fp32 else torch.float16
    step = NativeTrainStep(model, opt, scaler, n, "cuda", perturb=False, T_thresh=1e-4)
    step._build()
    # the backward fills dcol_out / dh0 only for samples that are on and relies on the step clearing them first: start from a pattern
    step.view("dcol_out", e, (step._M, 16)).fill_(3.0)
    step.view("dh0", e, (step._M,)).fill_(3.0)
    loss = step(rays_o, rays_d, target, sc.time, grads_only=True)
    torch.cuda.synchronize()
    M = step._M
    f = torch.float32
    shapes = dict(xyzs=(f, (M, 3)), dirs=(f, (M, 3)), deltas=(f, (M, 2)), rays=(torch.int32, (n, 3)), enc_in=(e, (M, 80)), def_hidden=(e, (7, M, 128)),
                  def_out=(e, (M, 16)), xdef=(f, (M, 3)), grid_out=(e, (16, M, 2)), h1=(e, (M, 64)), hout=(e, (M, 16)), sigmas=(f, (M,)),
                  col_in=(e, (M, 32)), col_hidden=(e, (2, M, 64)), col_out=(e, (M, 16)), weights_sum=(f, (n,)), depth=(f, (n,)), image=(f, (n, 3)),
                  sq_err=(f, (n,)), dcol_out=(e, (M, 16)), dh0=(e, (M,)), col_bwd=(e, (2, M, 64)), dcol_in=(e, (M, 32)), dh=(e, (M, 16)),
                  dh1=(e, (M, 64)), denc=(e, (16, M, 2)), dx=(e, (M, 3)), ddef=(e, (M, 16)), def_bwd=(e, (7, M, 128)),
                  g_deform=(e, (S.DEF_FLAT,)), g_color=(e, (S.COL_FLAT,)), g_sigma0=(e, (64 * 32,)), g_sigma1=(e, (16 * 64,)))
    rows = int(model.encoder.offsets[-1].item())
    shapes.update(g_table=(e, (rows, 2)))
    if not fp32:
        shapes.update(enc_rm=(e, (M, 32)), w_sigma0=(e, (64, 32)), w_sigma1=(e, (16, 64)), w_table=(e, (rows, 2)), w_deform=(e, (S.DEF_FLAT,)),
                      w_color=(e, (S.COL_FLAT,)))
    r = SimpleNamespace(**{k: _np(step.view(k, dt, shape)) for k, (dt, shape) in shapes.items()})
    if fp32:
        with pytest.raises(ValueError):
            step.view("enc_rm", e, (M, 32))
        r.w_sigma0, r.w_sigma1 = _np(model.sigma_net[0].weight), _np(model.sigma_net[1].weight)
        # the fp32 step reads the model's parameters: the table in place, the MLPs padded into the flat geometry as k_f32_pack reads them
        r.table = _np(model.encoder.embeddings)
        r.def_mats = S.flat_from_parameters([_np(l.weight) for l in model.deform_net], S.DEF_IN, S.DEF_W, S.DEF_L)
        r.col_mats = S.flat_from_parameters([_np(l.weight) for l in model.color_net], S.COL_IN, S.COL_W, S.COL_L, split=16)
    else:
        r.table = r.w_table
        r.def_mats, r.col_mats = S.split_flat(r.w_deform, S.DEF_IN, S.DEF_W, S.DEF_L), S.split_flat(r.w_color, S.COL_IN, S.COL_W, S.COL_L)
    enc = model.encoder
    r.grid = SimpleNamespace(offsets=_np(enc.offsets).astype(np.int32), pls=enc.per_level_scale, H=int(enc.base_resolution),
                             S=float(np.float32(np.log2(enc.per_level_scale))))
    r.fp32, r.short, r.M, r.N, r.owned = fp32, short, M, n, owned
    r.time, r.bound, r.density_scale = float(sc.time.item()), float(model.bound), float(model.density_scale)
    r.target, r.pred, r.loss = _np(target), _np(step.image), float(loss)
    r.loss_scale = 1.0 if fp32 else LOSS_SCALE
    assert fp32 or scaler.get_scale() == LOSS_SCALE
    # the float64 compositing reference on the GPU's own sigmas / deltas / colour logits / ray table, shared by the tests below
    c, slack = S.colours(r.col_out, half=not fp32)
    r.fwd = S.composite_forward(r.sigmas, r.deltas, c, r.rays, T_THRESH, colour_slack=slack)
    r.flip = S.flip_rays(r.fwd, T_THRESH)                      # by ray index
    rs = r.fwd["rs"]
    r.sample_ok = np.ones(M, bool)                             # samples of the rays compared
    r.sample_ok[rs.idx[rs.valid & r.flip[rs.index][:, None]]] = False
    r.tail = slice((owned - 1) // 32 * 32, (owned - 1) // 32 * 32 + 32)
    # the backward's rows end earlier: the tile of the last sample that is on (rows of both kinds in one tile)
    last_on = int(rs.idx[r.fwd["on"]].max())
    r.grad_tail = slice(last_on // 32 * 32, last_on // 32 * 32 + 32)
    del step, model, opt
    torch.cuda.empty_cache()
    return r


def _close(r, got, ref, what, L, backward=False):
    """The stage bar of a per-sample buffer (rows = samples) for the step's precision, on the whole buffer and on the tail tile alone:
    the tile where the owned samples end, and for a backward buffer also the tile of the last sample with a gradient."""
    tails = [("tail tile", r.tail)] + ([("last tile with a gradient", r.grad_tail)] if backward else [])
    if backward:
        assert np.abs(ref[r.grad_tail]).max() > 0
    if r.fp32:
        S.fp32_close(got, ref, what)
        for name, t in tails:
            S.fp32_close(got[t], ref[t], f"{what} ({name})")
    else:
        S.mfma16_close(got, ref, what, L)
        for name, t in tails:
            S.mfma16_close(got[t], ref[t], f"{what} ({name})", L)


STEPS = pytest.mark.parametrize("fp32", [False, True], ids=["f16", "f32"])
BUDGETS = pytest.mark.parametrize("short", [False, True], ids=["full", "short"])


@STEPS
def test_batch_coverage(fp32):
    """Per-ray counts in every band (0, 1..63, 65..128, 129..192, > 192, one of exactly 64), rays that stop in chunk 0 while owning
    more, in a later chunk, and never (>= 8 each); owned samples not a multiple of 32; at most 2 % of the rays near the threshold."""
    r = _run(fp32, False)
    count, first_off = S.coverage(r.fwd, T_THRESH)
    assert int(count.sum()) == r.owned and r.owned % 32 != 0 and not (~r.fwd["rs"].kept & (r.fwd["rs"].count > 0)).any()
    print("[stage] coverage:", S.assert_coverage(count, first_off), "owned", r.owned, "M", r.M, "longest", int(count.max()), "flip rays", int(r.flip.sum()))
    assert r.flip.mean() <= 0.02


@STEPS
def test_encode_and_deformed_position(fp32):
    """k_train_encode, k_train_xdef.  fp16: enc_in within 1.5 fp16 ulp; fp32 and xdef: the fp32 bar; the padding columns are zero.
    Measured: enc_in 0.47 of the 1.5 ulp (fp16), 0.001 of the fp32 bar (fp32); xdef 0.001."""
    r = _run(fp32, False)
    ref = S.encode(r.xyzs, r.time)
    assert np.all(r.enc_in[:, 76:] == 0)
    (S.fp32_close if fp32 else S.ulp16_close)(r.enc_in, ref, "enc_in")
    (S.fp32_close if fp32 else S.ulp16_close)(r.enc_in[r.tail], ref[r.tail], "enc_in (tail tile)")
    S.fp32_close(r.xdef, S.deformed_position(r.xyzs, r.def_out, r.time, r.bound), "xdef")


@STEPS
def test_sigma_mlp_forward(fp32):
    """k_train_sigma_fwd (fp16) / k_f32_chain_fwd + k_f32_sigma_post (fp32) from grid_out, dirs and the step's own sigma matrices.
    Measured, fp16: no element of h1 / hout / col_in beyond its ulp bar, norm-wise 7e-6 / 2.1e-4 / 2.1e-4 (tail tile 2.6e-4); fp32: h1
    0.009, hout and col_in 0.003 of the fp32 bar; sigmas below 0.001 in both."""
    r = _run(fp32, False)
    if not fp32:
        assert np.array_equal(r.enc_rm, S.level_major_to_rows(r.grid_out))          # a transposition: exact
    h1, hout, col_in = S.sigma_forward(r.grid_out, r.dirs, r.w_sigma0, r.w_sigma1, half=not fp32)
    _close(r, r.h1, h1, "h1", 1)
    _close(r, r.hout, hout, "hout", 2)
    _close(r, r.col_in, col_in, "col_in", 2)
    assert np.array_equal(r.col_in[:, 16:], r.hout)                                   # the same values twice
    S.fp32_close(r.sigmas, S.sigmas_of(r.hout[:, 0], r.density_scale), "sigmas")       # trunc_exp of the log density AS STORED


@STEPS
@BUDGETS
def test_compositing_forward(fp32, short):
    """k_train_composite_fwd, k_train_loss: weights_sum, depth, image, the predicted colour, sq_err, loss at the fp32 bar; rays
    without samples and rays dropped for the budget (offset + count > M) show the background exactly.
    Measured (both budgets): weights_sum 0.001, depth 0.002, loss 0.001; image / image_out / sq_err 0.002 / 0.002 / 0.004 in the fp32
    step and 0.54 / 0.51 / 0.39 in the fp16 step (one ray there has a colour at a rounding midpoint: the allowance (b) above)."""
    r = _run(fp32, short)
    rs, fwd = r.fwd["rs"], r.fwd
    keep = ~r.flip
    assert (not short) or int((~rs.kept & (rs.count > 0)).sum()) >= 8
    slack = fwd["image_slack"]
    S.fp32_close(r.weights_sum[keep], fwd["weights_sum"][keep], "weights_sum")
    S.fp32_close(r.depth[keep], fwd["depth"][keep], "depth")
    S.fp32_close(r.image[keep], fwd["image"][keep], "image", extra=slack[keep])
    pred, sq, _ = S.loss_terms(fwd["image"], fwd["weights_sum"], r.target, np.ones(3))
    S.fp32_close(r.pred[keep], pred[keep], "image_out", extra=slack[keep])
    sq_slack = (2 * np.abs(pred - r.target) * slack + slack ** 2).sum(1)
    S.fp32_close(r.sq_err[keep], sq[keep], "sq_err", extra=sq_slack[keep])
    S.fp32_close(np.array([r.loss]), np.array([f64sum(r.sq_err) / 3.0 / r.N]), "loss")          # k_train_loss from ITS input, all rays
    empty = np.zeros(r.N, bool)
    empty[rs.index[~rs.kept]] = True
    assert empty.sum() >= 8
    assert np.all(r.weights_sum[empty] == 0) and np.all(r.depth[empty] == 0) and np.all(r.image[empty] == 0) and np.all(r.pred[empty] == 1)
    S.fp32_close(r.sq_err[empty], ((1.0 - r.target[empty].astype(np.float64)) ** 2).sum(1), "sq_err of background rays")


def f64sum(a):
    return float(np.asarray(a, np.float64).sum())


@STEPS
@BUDGETS
def test_compositing_backward(fp32, short):
    """k_train_composite_bwd from the forward's image / weights_sum and hout as stored.  Rows of samples that are off (behind a
    termination, never visited chunks, padding, dropped rays) and columns 3..15 are exactly zero.
    dcol_out and dh0 are filled with a pattern before the step, so the exact zeros test the step's own clear.
    Measured: fp16 dcol_out 0.74 of the 1.5 ulp, dh0 0.99 of 1.5 ulp plus allowance (a); fp32 dcol_out 0.003, dh0 0.09 of the plain bar."""
    r = _run(fp32, short)
    ref = S.composite_backward(r.fwd, r.image, r.weights_sum, r.target, np.ones(3), r.hout[:, 0], r.loss_scale, r.density_scale)
    ok, on = r.sample_ok, ref["on"]
    assert np.all(r.dcol_out[:, 3:] == 0)
    off = ok & ~on
    assert off.sum() > 0 and np.all(r.dcol_out[off] == 0) and np.all(r.dh0[off] == 0)
    assert np.all(r.dcol_out[r.owned:] == 0) and np.all(r.dh0[r.owned:] == 0)                  # rows past the owned samples: untouched
    m = ok & on
    if fp32:
        S.fp32_close(r.dcol_out[m, :3], ref["dcol_out"][m, :3], "dcol_out")
        S.fp32_close(r.dh0[m], ref["dh0"][m], "dh0")
    else:
        assert np.isfinite(r.dh0.astype(np.float32)).all()
        S.ulp16_close(r.dcol_out[m, :3], ref["dcol_out"][m, :3], "dcol_out", extra=ref["dcol_slack"][m])
        S.ulp16_close(r.dh0[m], ref["dh0"][m], "dh0", extra=S.CANCEL_ULPS * ref["dh0_cancel"][m] + ref["dh0_slack"][m])


@STEPS
def test_sigma_mlp_backward(fp32):
    """k_train_sigma_bwd (fp16) / k_f32_dh + k_f32_chain_bwd (fp32): dh is a copy (column 0 from dh0, 1..15 from dcol_in[:, 17:32]),
    dh1 gated by the GPU's own h1, denc in the grid encoder's [level][sample][2] layout.
    Measured, fp16: no element beyond its ulp bar, norm-wise dh1 3e-6, denc 1.8e-4 (single levels up to 2.3e-4; the last tile with a
    gradient, fp16 subnormals, 4.3e-3); fp32: dh1 0.002, denc
    0.005 of the fp32 bar."""
    r = _run(fp32, False)
    dh, dh1, denc = S.sigma_backward(r.dh0, r.dcol_in, r.h1, r.w_sigma0, r.w_sigma1, half=not fp32)
    assert np.array_equal(r.dh.astype(np.float64), dh)
    _close(r, r.dh1, dh1, "dh1", 1, backward=True)
    got, want = S.level_major_to_rows(r.denc), S.level_major_to_rows(denc)
    _close(r, got, want, "denc", 2, backward=True)
    for lvl in range(16):            # a wrong lane mapping moves whole levels: each level on its own
        _close(r, r.denc[lvl], denc[lvl], f"denc level {lvl}", 2)


@STEPS
def test_deformation_gradient(fp32):
    """k_train_deform_grad: dx / (2 bound) in columns 0..2, zero columns 3..15.  Measured: fp16 0.50 of the 1.5 ulp (an exact halving:
    the rounding alone), fp32 below 0.001 of the fp32 bar."""
    r = _run(fp32, False)
    ref = S.deform_gradient(r.dx, r.bound)
    assert np.all(r.ddef[:, 3:] == 0)
    (S.fp32_close if fp32 else S.ulp16_close)(r.ddef[:, :3], ref[:, :3], "ddef")
    for name, t in (("tail tile", r.tail), ("last tile with a gradient", r.grad_tail)):
        (S.fp32_close if fp32 else S.ulp16_close)(r.ddef[t, :3], ref[t, :3], f"ddef ({name})")


@STEPS
def test_weight_gradient_products(fp32):
    """All 13 products dW = A^T B from the two buffers the job list pairs, each in its block of the flat gradients.
    Measured, fp16: no element of any block beyond 4 ulp, norm-wise 1.8e-4 .. 2.3e-4 (the fp16 rounding of the result); fp32: at most
    0.046 of the fp32 bar."""
    r = _run(fp32, False)
    bufs = {k: getattr(r, k) for k in ("enc_in", "def_hidden", "def_bwd", "ddef", "col_in", "col_hidden", "col_bwd", "dcol_out", "h1", "dh1", "dh")}
    bufs["enc"] = S.level_major_to_rows(r.grid_out)
    ref, jobs = S.weight_gradients(bufs, fp32)
    for g, off, rows, cols, a, b in jobs:
        got, want = getattr(r, g)[off:off + rows * cols], ref[g][off:off + rows * cols]
        what = f"{g}[{off}:{off + rows * cols}] = {a[0]}^T {b[0]}"
        if fp32:
            S.fp32_close(got, want, what)
        else:
            assert np.abs(want).max() < 6e4, (what, "leaves fp16: lower LOSS_SCALE", float(np.abs(want).max()))
            S.mfma16_close(got, want, what, 1)


# ---- the packed MLP chains, layer by layer: every layer from the GPU's own stored input of THAT layer (depth 1 in the bar) --------------------------
def _at(r, L):
    """Where the gradient of hidden layer l's pre-activation is stored: [L - 1 - l] in the fp16 step, [l] in the fp32 step."""
    return (lambda l: l) if r.fp32 else (lambda l: L - 1 - l)


@STEPS
def test_deformation_mlp_forward(fp32):
    """sdn_ffh::forward_packed (fp16) / k_f32_chain_fwd (fp32) on 80 -> 128 x 7 -> 16: def_hidden[0] from enc_in, def_hidden[l] from
    def_hidden[l - 1], def_out from def_hidden[6]; output columns 3..15 and (fp16) the padding of the weight copy are exactly zero.
    Measured, fp16: no element of any layer beyond 4 ulp, norm-wise 2.07e-4 .. 2.08e-4 per hidden layer (tail tile up to 2.2e-4), def_out
    3.8e-4 (tail tile 5.2e-4); fp32: at most 0.017 of the fp32 bar (def_hidden[2]), def_out 0.009."""
    r = _run(fp32, False)
    m = r.def_mats
    if not fp32:
        assert np.all(m[0][:, 76:] == 0) and np.all(m[7][3:] == 0) and np.any(m[0][:, :76] != 0) and np.any(m[7][:3] != 0)
    x = r.enc_in
    for l in range(S.DEF_L):
        _close(r, r.def_hidden[l], S.mlp_layer_forward(x, m[l]), f"def_hidden[{l}]", 1)
        x = r.def_hidden[l]
    _close(r, r.def_out, S.mlp_layer_forward(x, m[S.DEF_L], relu=False), "def_out", 1)
    assert np.all(r.def_out[:, 3:] == 0) and np.any(r.def_out[:, :3] != 0)


@STEPS
def test_colour_mlp_forward(fp32):
    """forward_packed / k_f32_chain_fwd on 32 -> 64 x 2 -> 16: col_hidden[0] from col_in with the weight's input column 16 (the
    log-density column) zero, col_hidden[1], col_out; output columns 3..15 exactly zero.
    Measured, fp16: no element beyond 4 ulp, norm-wise 2.09e-4 / 2.07e-4 / 2.12e-4 (tail tile up to 2.7e-4); fp32: 0.012 / 0.015 / 0.007 of
    the fp32 bar."""
    r = _run(fp32, False)
    m = r.col_mats
    assert np.all(m[0][:, 16] == 0) and np.all(m[2][3:] == 0) and np.any(r.col_in[:, 16] != 0)
    _close(r, r.col_hidden[0], S.mlp_layer_forward(r.col_in, m[0]), "col_hidden[0]", 1)
    _close(r, r.col_hidden[1], S.mlp_layer_forward(r.col_hidden[0], m[1]), "col_hidden[1]", 1)
    _close(r, r.col_out, S.mlp_layer_forward(r.col_hidden[1], m[2], relu=False), "col_out", 1)
    assert np.all(r.col_out[:, 3:] == 0)


@STEPS
def test_colour_mlp_backward(fp32):
    """backward_packed with the input gradient / k_f32_chain_bwd: the two pre-activation gradients of col_bwd from dcol_out, gated
    by the GPU's own col_hidden, and dcol_in, whose column 16 is exactly zero (the weight column is structurally zero).
    Measured, fp16: no element beyond 4 ulp, norm-wise 2.1e-4 / 2.2e-4 / 2.3e-4 (the last tile with a gradient holds fp16 subnormals only: no element
    beyond the bar, norm-wise up to 8.8e-2 of a norm of ~1e-7, inside the bar's absolute 1e-6 term); fp32:
    0.002 / 0.004 / 0.007 of the fp32 bar."""
    r = _run(fp32, False)
    m, at = r.col_mats, _at(r, S.COL_L)
    _close(r, r.col_bwd[at(1)], S.mlp_layer_backward(r.dcol_out, m[2], r.col_hidden[1]), "col_bwd (layer 1)", 1, backward=True)
    _close(r, r.col_bwd[at(0)], S.mlp_layer_backward(r.col_bwd[at(1)], m[1], r.col_hidden[0]), "col_bwd (layer 0)", 1, backward=True)
    _close(r, r.dcol_in, S.mlp_layer_backward(r.col_bwd[at(0)], m[0]), "dcol_in", 1, backward=True)
    assert np.all(r.dcol_in[:, 16] == 0) and np.any(r.dcol_in[:, 17:] != 0)


@STEPS
def test_deformation_mlp_backward(fp32):
    """backward_packed WITHOUT the input gradient / k_f32_chain_bwd, seven layers deep: def_bwd layer 6 from ddef, layer l from the
    GPU's def_bwd layer l + 1, each gated by def_hidden[l]; rows of samples without a gradient are exactly zero.
    Measured, fp16: no element of any layer beyond 4 ulp, norm-wise 1.96e-4 (layer 6) .. 4.3e-4 (layer 0) (the
    last tile with a gradient holds values at the fp16 subnormal spacing: norm-wise up to 0.86 of a norm below 1e-7, inside the bar's
    absolute 1e-6 term); fp32: at most 0.008 of the
    fp32 bar (layer 0)."""
    r = _run(fp32, False)
    m, at = r.def_mats, _at(r, S.DEF_L)
    g = r.ddef
    for l in range(S.DEF_L - 1, -1, -1):
        _close(r, r.def_bwd[at(l)], S.mlp_layer_backward(g, m[l + 1], r.def_hidden[l]), f"def_bwd (layer {l})", 1, backward=True)
        g = r.def_bwd[at(l)]
    none = ~np.any(r.ddef != 0, axis=1)
    assert none.sum() > 0 and (~none).sum() > 0 and np.all(r.def_bwd[:, none] == 0)


# ---- the grid encoder inside the step ----------------------------------------------------------------------------------------------------------------
def _corners(r):
    if not hasattr(r, "corners"):
        r.corners = S.tiled_corners(r.xdef, r.grid.offsets, r.grid.S, r.grid.H)
    return r.corners


@STEPS
def test_grid_forward_in_step(fp32):
    """sdn_grid_encode_forward as the step calls it: grid_out (level-major) is bit-identical to the oracle on the GPU's xdef and the
    table the step read (the fp16 copy w_table / the fp32 parameter).
    Measured: bit-identical in both steps; the fp32 step's grid_out 0.010 of the fp32 bar from the float64 restatement."""
    from oracle import oracle as O
    r = _run(fp32, False)
    ref, _ = O.grid_encode_forward(r.xdef, r.table, r.grid.offsets, r.grid.pls, r.grid.H, False, 1, False, 0)
    got = S.level_major_to_rows(r.grid_out)
    bits = np.uint32 if fp32 else np.uint16
    assert got.dtype == ref.dtype and np.array_equal(got.view(bits), ref.view(bits))
    if fp32:      # and the float64 restatement the table-gradient tests rest on sees the same rows and weights
        S.fp32_close(got, S.level_major_to_rows(S.grid_forward64(_corners(r), r.table)), "grid_out against the float64 restatement")
    assert np.any(got != 0)


@STEPS
def test_grid_input_gradient_in_step(fp32):
    """k_grid_input_bwd: dx against the float64 sum of denc x the restated dy_dx.  fp32: the fp32 bar.  fp16: the kernel rounds every
    product and every partial sum to fp16 (Num<T>::rnd), 32 terms per element: 33 * 2^-11 * sum |g dy_dx| per element, plus 2^-24.
    Measured: fp32 0.002 of the fp32 bar; fp16 0.92 of the derived bound (which also has to cover the fp16 rounding of the kernel's own
    dy_dx, not restated here), and bit-equal to the oracle's serial fp16 grad_inputs."""
    from oracle import oracle as O
    r = _run(fp32, False)
    c = _corners(r)
    ref, mag = S.grid_input_gradient64(r.denc, S.grid_dy_dx64(c, r.table))
    assert np.abs(ref).max() > 0
    if fp32:
        S.fp32_close(r.dx, ref, "dx")
    else:
        _, dd = O.grid_encode_forward(r.xdef, r.table, r.grid.offsets, r.grid.pls, r.grid.H, True, 1, False, 0)
        _, gi = O.grid_encode_backward(S.level_major_to_rows(r.denc), r.xdef, r.table, r.grid.offsets, r.grid.pls, r.grid.H, dd, 1, False, 0)
        print("[stage] fp16 dx bit-equal to the oracle's serial fp16 grad_inputs:", bool(np.array_equal(r.dx.astype(np.float32), gi)))
        S.bound_close(r.dx, ref, 33 * 2.0 ** -11 * mag + S.F16_TINY, "dx", "33 * 2^-11 * sum |g dy_dx| + 2^-24")


@STEPS
def test_table_gradient_in_step(fp32):
    """k_grid_bwd's wave-level run merge on ray-ordered samples: g_table per level against the float64 scatter of denc at the GPU's
    own xdef.  fp32: the fp32 bar per level (the tight check of the merge: one template for both types, sums in fp32); fp16: the
    half-atomic bar of test_grid_encode_backward per level.  Rows no sample touches are exactly zero.  The batch must exercise the
    merge: on each of levels 0..3 a run of >= 8 lanes, >= 8 waves that merge, >= 1 row run continuing across a wave boundary.
    Measured on the wedge batch (corner 0, owned samples): longest run 54 / 39 / 29 / 20 lanes on levels 0 / 1 / 2 / 3, merging in all
    1080 waves, 1029 / 1030 / 994 / 960 row runs continuing across a wave boundary.  fp32: at most 0.001 of the fp32 bar on every
    level; fp16: 0.013 .. 0.056 of the half-atomic bar (level 0 the largest)."""
    r = _run(fp32, False)
    c = _corners(r)
    for l in range(4):
        rs = S.run_structure(np.where(c.valid, c.rows[l, :, 0], -1)[:r.owned])        # (owned samples only: the zero-filled padding rows behind them are one long run)
        print(f"[stage] level {l} corner 0: longest run {rs['longest']} lanes, {rs['merging_waves']} merging waves, {rs['crossings']} runs across a wave boundary")
        assert rs["longest"] >= 8 and rs["merging_waves"] >= 8 and rs["crossings"] >= 1, (l, rs["longest"], rs["merging_waves"], rs["crossings"])
    ref = S.grid_table_gradient64(r.denc, c)
    assert np.abs(ref).max() > 0
    touched = np.zeros(c.n_rows, bool)
    touched[c.rows[:, c.valid].reshape(-1)] = True
    assert (~touched).sum() > 0 and np.all(r.g_table[~touched] == 0)
    S.table_gradient_close(r.g_table, ref, r.grid.offsets, "g_table", fp32)
