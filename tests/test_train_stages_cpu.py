"""The float64 stage references of tests/train_stage_support.py, validated without a GPU: against the CPU oracle's sequential
compositing loops (in double), its frequency and SH encoders, and float64 torch autograd.  The GPU tests
(tests/test_gpu_train_stages.py) then hold each kernel of the native training steps to these functions."""
import numpy as np
import pytest
import torch

import train_stage_support as S
from oracle import oracle

T_THRESH = float(np.float32(1e-4))


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(float(np.abs(b).max()), 1e-300))


def _random_rays(rng, n_rays=200, longest=300, dropped=5, heavy=True):
    """Rays of 0..longest samples in shuffled order with shuffled `index`; the last `dropped` reach past M.  Densities are log-normal,
    so that rays stop in every chunk or never."""
    count = rng.integers(0, longest + 1, n_rays)
    count[:8] = [0, 0, 1, 63, 64, 65, 128, 129]
    order = rng.permutation(n_rays)
    offset = np.zeros(n_rays, np.int64)
    offset[order] = np.concatenate([[0], np.cumsum(count[order])[:-1]])
    M = int(count.sum()) - int(count[order[-dropped:]].sum()) + 3 if dropped else int(count.sum())
    rays = np.stack([rng.permutation(n_rays), offset, count], 1).astype(np.int32)
    total = int(count.sum())
    dt = 2 * np.sqrt(3) / 1024
    sig = np.exp(rng.normal(np.log(0.05 / dt), 1.5 if heavy else 0.3, total))
    deltas = np.stack([np.full(total, dt), np.full(total, dt) * rng.uniform(1, 3, total)], 1)
    col_out = rng.normal(0, 2, (total, 16))
    return rays, M, sig[:M], deltas[:M], col_out[:M]


def test_compositing_references_match_the_oracles_sequential_loops_in_double():
    """Forward and backward against oracle.composite_rays_train_forward / _backward evaluated in double (the same sequential loop
    and early stop as the float32 oracle): 1e-12 relative.  The float32 oracle itself agrees to float32 rounding."""
    rng = np.random.default_rng(0)
    rays, M, sig, deltas, col_out = _random_rays(rng)
    c, _ = S.colours(col_out)
    fwd = S.composite_forward(sig, deltas, c, rays, T_THRESH)
    ws, depth, image = oracle.composite_rays_train_forward(sig, c, deltas, rays, T_THRESH, dtype=np.float64)
    for got, want in ((fwd["weights_sum"], ws), (fwd["depth"], depth), (fwd["image"], image)):
        assert _rel(got, want) <= 1e-12
    ws32, depth32, image32 = oracle.composite_rays_train_forward(sig, c, deltas, rays, T_THRESH)
    assert _rel(fwd["weights_sum"], ws32) < 1e-4 and _rel(fwd["image"], image32) < 1e-4 and _rel(fwd["depth"], depth32) < 1e-4
    n = rays.shape[0]
    g_img, g_ws = rng.normal(0, 1, (n, 3)), rng.normal(0, 1, n)
    gs, gc, _, _ = S.composite_backward_core(fwd, g_img, g_ws, image, ws)
    gs_o, gc_o = oracle.composite_rays_train_backward(g_ws, g_img, sig, c, deltas, rays, ws, image, T_THRESH, dtype=np.float64)
    assert _rel(gs, gs_o) <= 1e-12 and _rel(gc, gc_o) <= 1e-12
    # and the float32 oracle that was there before, on its own forward results, to float32 rounding
    gs32, gc32 = oracle.composite_rays_train_backward(g_ws, g_img, sig, c, deltas, rays, ws32, image32, T_THRESH)
    assert _rel(gs, gs32) < 1e-4 and _rel(gc, gc32) < 1e-4
    # dropped rays (offset + count > M) and empty rays: nothing composited, no gradient row
    cov_count, first_off = S.coverage(fwd, T_THRESH)
    r = fwd["rs"]
    assert (~r.kept).sum() >= 7 and np.all(fwd["weights_sum"][r.index[~r.kept]] == 0)
    owned = np.zeros(M, bool)
    owned[r.idx[fwd["on"]]] = True
    assert np.all(gs[~owned] == 0) and np.all(gc[~owned] == 0) and (~owned).sum() > 0
    # this random batch has every class the GPU batch must have
    S.assert_coverage(cov_count, first_off)


def test_loss_and_its_gradient_match_float64_autograd():
    """pred = image + (1 - weights_sum) bg, loss = mean((pred - gt)^2), through sigmoid, density_scale and trunc_exp: the whole
    compositing backward against torch autograd in float64 on a short-ray batch (no sample near the threshold): 1e-10 relative."""
    rng = np.random.default_rng(1)
    rays, M, sig, deltas, col_out = _random_rays(rng, n_rays=40, longest=90, dropped=0, heavy=False)
    n = rays.shape[0]
    target, bg = rng.uniform(0, 1, (n, 3)), rng.uniform(0, 1, (n, 3))
    hout0 = np.log(sig / 0.7)
    hout0[:5] = [20.0, -20.0, 15.5, -15.5, 3.0]            # beyond the clamp: trunc_exp's backward uses exp(clamp(x))
    scale, ds = 128.0, 0.7
    sig = S.sigmas_of(hout0, ds)
    c, _ = S.colours(col_out)
    fwd = S.composite_forward(sig, deltas, c, rays, T_THRESH)
    assert not S.flip_rays(fwd, T_THRESH).any()
    pred, sq, loss = S.loss_terms(fwd["image"], fwd["weights_sum"], target, bg)
    ref = S.composite_backward(fwd, fwd["image"], fwd["weights_sum"], target, bg, hout0, scale, ds)

    class TruncExp(torch.autograd.Function):               # activation.py:5-17
        @staticmethod
        def forward(ctx, x):
            ctx.save_for_backward(x)
            return torch.exp(x)

        @staticmethod
        def backward(ctx, g):
            return g * torch.exp(ctx.saved_tensors[0].clamp(-15, 15))

    h = torch.tensor(hout0, requires_grad=True)
    co = torch.tensor(col_out[:, :3], requires_grad=True)
    s_t, c_t, d_t = TruncExp.apply(h) * ds, torch.sigmoid(co), torch.tensor(deltas)
    total = torch.zeros((), dtype=torch.float64)
    sq_t = torch.zeros(n, dtype=torch.float64)
    on = fwd["on"]
    for k in range(n):
        idx, o, cnt = int(rays[k, 0]), int(rays[k, 1]), int(rays[k, 2])
        keep = torch.tensor(on[k, :cnt])
        a = 1 - torch.exp(-s_t[o:o + cnt] * d_t[o:o + cnt, 0])
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1 - a[:-1]]), 0) if cnt else a
        w = a * T * keep
        img = (w[:, None] * c_t[o:o + cnt]).sum(0)
        p = img + (1 - w.sum()) * torch.tensor(bg[idx])
        sq_t[idx] = ((p - torch.tensor(target[idx])) ** 2).sum()
    total = sq_t.sum() / 3 / n
    (total * scale).backward()
    assert abs(loss - float(total.detach())) <= 1e-12 * abs(float(total.detach())) and _rel(sq, sq_t.detach().numpy()) <= 1e-12
    assert _rel(ref["dh0"], h.grad.numpy()) <= 1e-10 and _rel(ref["dcol_out"][:, :3], co.grad.numpy()) <= 1e-10
    assert np.all(ref["dcol_out"][:, 3:] == 0)


def test_sigma_mlp_references_match_float64_autograd_on_a_linear_stack():
    rng = np.random.default_rng(2)
    M = 77
    grid = rng.normal(0, 1, (16, M, 2))
    dirs = rng.normal(0, 1, (M, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    l1, l2 = torch.nn.Linear(32, 64, bias=False).double(), torch.nn.Linear(64, 16, bias=False).double()
    w1, w2 = l1.weight.detach().numpy(), l2.weight.detach().numpy()
    h1, hout, col_in = S.sigma_forward(grid, dirs, w1, w2)
    x = torch.tensor(S.level_major_to_rows(grid), requires_grad=True)
    h1_t = torch.relu(l1(x))
    hout_t = l2(h1_t)
    assert _rel(h1, h1_t.detach().numpy()) <= 1e-12 and _rel(hout, hout_t.detach().numpy()) <= 1e-12
    assert np.array_equal(col_in[:, 16:], hout)
    sh_o, _ = oracle.sh_encode_forward(dirs.astype(np.float32), 4)
    assert np.array_equal(col_in[:, :16], S.sh16(dirs)) and np.abs(S.sh16(dirs.astype(np.float32)) - sh_o).max() < 1e-6
    assert _rel(S.sigmas_of(hout[:, 0], 0.5), 0.5 * np.exp(hout[:, 0])) <= 1e-15
    # backward: dh = [dh0 | dcol_in[:, 17:32]]
    dh0, dcol_in = rng.normal(0, 1, M), rng.normal(0, 1, (M, 32))
    dh, dh1, denc = S.sigma_backward(dh0, dcol_in, h1, w1, w2)
    assert np.array_equal(dh[:, 0], dh0) and np.array_equal(dh[:, 1:], dcol_in[:, 17:])
    pre = l1(x)
    pre.retain_grad()
    l2(torch.relu(pre)).backward(torch.tensor(dh))
    assert _rel(dh1, pre.grad.numpy()) <= 1e-12
    assert denc.shape == (16, M, 2) and _rel(S.level_major_to_rows(denc), x.grad.numpy()) <= 1e-12
    # the fp16 variant rounds the hidden layers once and nothing else
    h1h, _, _ = S.sigma_forward(grid, dirs, w1, w2, half=True)
    assert np.array_equal(h1h, S.round16(h1))


def test_encoding_deformed_position_and_deformation_gradient():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    enc = S.encode(x, 0.5)
    assert enc.shape == (50, 80) and np.all(enc[:, 76:] == 0)
    assert np.abs(enc[:, :63] - oracle.freq_encode_forward(x, 10)).max() < 1e-6          # freqencoder.cu:30-58, in float32
    assert np.abs(enc[:, 63:76] - oracle.freq_encode_forward(np.full((50, 1), 0.5, np.float32), 6)).max() < 1e-6
    d = rng.normal(0, 0.05, (50, 16))
    for bound in (1.0, 2.0):
        assert np.allclose(S.deformed_position(x, d, 0.5, bound), (x + d[:, :3] + bound) / (2 * bound), rtol=1e-15)
        assert np.array_equal(S.deformed_position(x, d, 0.0, bound), (x.astype(np.float64) + bound) / (2 * bound))      # t == 0: no deformation
        g = S.deform_gradient(d[:, :3], bound)
        assert np.all(g[:, 3:] == 0) and np.allclose(g[:, :3] * 2 * bound, d[:, :3], rtol=1e-15)


def test_the_13_weight_gradient_jobs_reproduce_autograd_block_by_block():
    """A small float64 deformation / colour / sigma stack in the step's flat geometry: autograd's weight gradients against A^T B of
    the buffers the job list pairs, for the fp16 step's buffer order (hidden gradients last layer first) and the fp32 step's."""
    torch.manual_seed(0)
    M = 37
    lin = lambda i, o: torch.nn.Linear(i, o, bias=False).double()
    nets = {"g_deform": [lin(80, 128)] + [lin(128, 128) for _ in range(6)] + [lin(128, 16)],
            "g_color": [lin(32, 64), lin(64, 64), lin(64, 16)], "g_sigma": [lin(32, 64), lin(64, 16)]}

    def run(layers, x):
        pres, acts, h = [], [], x
        for layer in layers[:-1]:
            p = layer(h)
            p.retain_grad()
            h = torch.relu(p)
            pres.append(p)
            acts.append(h)
        out = layers[-1](h)
        out.retain_grad()
        return pres, acts, out

    enc_in, enc = torch.randn(M, 80, dtype=torch.float64), torch.randn(M, 32, dtype=torch.float64)
    dp, da, dout = run(nets["g_deform"], enc_in)
    sp, sa, hout = run(nets["g_sigma"], enc)
    col_in = torch.cat([torch.randn(M, 16, dtype=torch.float64), hout], 1)
    cp, ca, cout = run(nets["g_color"], col_in)
    (dout * torch.randn_like(dout)).sum().backward()
    ((cout * torch.randn_like(cout)).sum() + (hout[:, 0] * torch.randn(M, dtype=torch.float64)).sum()).backward()
    n = lambda t: t.detach().numpy()
    for fp32 in (False, True):
        order = (lambda xs: xs) if fp32 else (lambda xs: xs[::-1])
        bufs = {"enc_in": n(enc_in), "def_hidden": np.stack([n(a) for a in da]), "def_bwd": np.stack(order([n(p.grad) for p in dp])), "ddef": n(dout.grad),
                "col_in": n(col_in), "col_hidden": np.stack([n(a) for a in ca]), "col_bwd": np.stack(order([n(p.grad) for p in cp])), "dcol_out": n(cout.grad),
                "enc": n(enc), "h1": n(sa[0]), "dh1": n(sp[0].grad), "dh": n(hout.grad)}
        got, jobs = S.weight_gradients(bufs, fp32)
        assert len(jobs) == 13
        want = {"g_deform": np.concatenate([n(l.weight.grad).reshape(-1) for l in nets["g_deform"]]),
                "g_color": np.concatenate([n(l.weight.grad).reshape(-1) for l in nets["g_color"]]),
                "g_sigma0": n(nets["g_sigma"][0].weight.grad).reshape(-1), "g_sigma1": n(nets["g_sigma"][1].weight.grad).reshape(-1)}
        covered = {k: np.zeros(v.shape, bool) for k, v in want.items()}
        for g, off, rows, cols, _, _ in jobs:
            blk = slice(off, off + rows * cols)
            assert _rel(got[g][blk], want[g][blk]) <= 1e-12, (fp32, g, off)
            assert not covered[g][blk].any()
            covered[g][blk] = True
        assert all(c.all() for c in covered.values())           # the 13 blocks tile the four flat gradients


def test_fp16_colour_slack_marks_only_values_at_a_rounding_midpoint():
    x = np.linspace(-8, 8, 20001)[:, None].repeat(3, 1)
    c, slack = S.colours(x, half=True)
    assert np.array_equal(c, S.round16(1 / (1 + np.exp(-x)))) and (slack > 0).mean() < 1e-2
    x16 = np.float16(0.5)          # an exact midpoint, constructed: sigmoid^-1 of the midpoint of two neighbouring fp16 values
    mid = (float(x16) + float(np.nextafter(x16, np.float16(1)))) / 2
    c, slack = S.colours(np.full((1, 3), np.log(mid / (1 - mid))), half=True)
    assert np.all(slack == 2.0 ** -11)


def test_float32_sigmoid_stays_within_the_colour_slack_threshold():
    """1 / (1 + exp(-x)) in float32 on every finite fp16 input against float64: within 2^-22 relative, the threshold `colours` uses."""
    x = np.arange(65536, dtype=np.uint16).view(np.float16)
    x = x[np.isfinite(x)].astype(np.float32)
    with np.errstate(over="ignore"):
        y32 = np.float32(1) / (np.float32(1) + np.exp(-x))
        y64 = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    m = y64 > 2.0 ** -100
    assert float((np.abs(y32[m] - y64[m]) / y64[m]).max()) <= 2.0 ** -22


def _synthetic_batch(seed):
    rng = np.random.default_rng(seed)
    n = 510
    count = np.clip(((np.arange(n) % 32) * 11 - 20 + rng.integers(-5, 6, n)), 0, None)
    rays = np.stack([np.arange(n), np.concatenate([[0], np.cumsum(count)[:-1]]), count], 1).astype(np.int32)
    M = int(count.sum())
    dt = 2 * np.sqrt(3) / 1024
    sig = np.exp(rng.normal(np.log(0.05 / dt), 1.2, M)).astype(np.float32)
    return rng, rays, M, sig, np.full((M, 2), dt, np.float32)


def test_float32_restatement_of_the_compositing_kernels_stays_inside_the_dh0_bar():
    """The kernels' float32 order of operations (wave prefix product and sums per 64-sample chunk, chunk carry, float32 loss gradient)
    restated on the CPU, on a synthetic long-ray batch of the GPU test's shape, against the float64 reference on the restatement's own
    forward results: dcol_out inside the issue's bars as they stand, dh0 inside its bar plus S.CANCEL_ULPS of the cancelling
    magnitudes -- and NOT inside the plain bar, which is why the allowance exists.  The constant comes from this distance (measured
    worst 0.69 ulp over seeds 10..13, both precisions), never from the kernel."""
    for half, scale in ((False, 1.0), (True, 1024.0)):
        rng, rays, M, sig, deltas = _synthetic_batch(10)
        col_out = rng.normal(0, 2, (M, 16)).astype(np.float16 if half else np.float32)
        c, _ = S.colours(col_out, half)
        target = rng.uniform(0, 1, (rays.shape[0], 3)).astype(np.float32)
        hout0 = np.log(sig.astype(np.float64)).astype(np.float16 if half else np.float32)
        ws32, img32, gs32, gc32 = S.composite_f32_restatement(sig, deltas, c, rays, target, 1.0, scale, T_THRESH)
        fwd = S.composite_forward(sig, deltas, c, rays, T_THRESH)
        assert _rel(img32, fwd["image"]) < 1e-6 and _rel(ws32, fwd["weights_sum"]) < 1e-6
        ref = S.composite_backward(fwd, img32, ws32, target, np.ones(3), hout0, scale, 1.0)
        rs, flip = fwd["rs"], S.flip_rays(fwd, T_THRESH)
        ok = np.ones(M, bool)
        ok[rs.idx[rs.valid & flip[rs.index][:, None]]] = False
        m = ok & ref["on"]
        assert np.all(gs32[ok & ~ref["on"]] == 0)
        e32 = np.exp(np.clip(hout0.astype(np.float32), -15, 15))
        dh0 = (gs32 * np.float32(1.0)) * e32
        dcol = (gc32 * (1 - c.astype(np.float32))) * c.astype(np.float32)
        extra = S.CANCEL_ULPS * ref["dh0_cancel"][m]
        if half:
            S.ulp16_close(S.round16(dh0)[m], ref["dh0"][m], "restated dh0", extra=extra)
            worst_plain = np.abs(S.round16(dh0)[m] - ref["dh0"][m]) / np.maximum(1.5 * S.F16_ULP * np.abs(ref["dh0"][m]), S.F16_TINY)
        else:
            S.fp32_close(dh0[m], ref["dh0"][m], "restated dh0", extra=extra)
            S.fp32_close(dcol[m], ref["dcol_out"][m, :3], "restated dcol_out")
            worst_plain = np.abs(dh0[m] - ref["dh0"][m]) / (1e-4 * np.abs(ref["dh0"][m]) + 1e-5 * np.abs(ref["dh0"][m]).max())
        print("restated dh0 against the plain bar:", float(worst_plain.max()))
        if half:
            assert worst_plain.max() > 1.0        # one fp16 rounding of a float32 result it is not


def test_synthetic_long_ray_batch_has_the_coverage_and_few_threshold_flips():
    """A synthetic batch of the GPU test's shape (510 rays, counts sweeping 0 .. 320 across each image row, log-normal densities at
    the GPU test's median sigma * dt): every count band and termination class is present, and at most 2 % of the rays have a
    sample within 1e-4 (relative) of T_thresh -- the rays the GPU comparisons leave out."""
    rng = np.random.default_rng(4)
    n = 510
    count = np.clip(((np.arange(n) % 32) * 11 - 20 + rng.integers(-5, 6, n)), 0, None)
    count[100] = 64
    offset = np.concatenate([[0], np.cumsum(count)[:-1]])
    rays = np.stack([np.arange(n), offset, count], 1).astype(np.int32)
    M = int(count.sum())
    dt = 2 * np.sqrt(3) / 1024
    sig = np.exp(rng.normal(np.log(0.05 / dt), 1.2, M))
    fwd = S.composite_forward(sig, np.full((M, 2), dt), np.full((M, 3), 0.5), rays, T_THRESH)
    S.assert_coverage(*S.coverage(fwd, T_THRESH))
    assert S.flip_rays(fwd, T_THRESH).mean() <= 0.02


# ---- the packed MLP chains, the grid encoder, the optimizer pass ---------------------------------------------------------------------------------------
from oracle import ffmlp as FF  # noqa: E402


def _chain_case(seed, in_dim, W, L, B=37):
    rng = np.random.default_rng(seed)
    n = W * in_dim + (L - 1) * W * W + 16 * W
    flat = (rng.standard_normal(n) * (1.5 / np.sqrt(W))).astype(np.float16)
    x = rng.standard_normal((B, in_dim)).astype(np.float16)
    dy = (rng.standard_normal((B, 16)) * 0.1).astype(np.float16)
    return flat, x, dy


@pytest.mark.parametrize("in_dim,W,L", [(80, 128, 7), (32, 64, 2)], ids=["deformation", "colour"])
def test_one_layer_restatements_compose_to_the_ffmlp_oracle(in_dim, W, L):
    """mlp_layer_forward / mlp_layer_backward, composed with ONE fp16 rounding after each layer (of the float32
    accumulator, as the oracle rounds), reproduce the oracle's forward
    buffer, outputs, backward buffer (output side first) and input gradient bit for bit."""
    flat, x, dy = _chain_case(7, in_dim, W, L)
    mats = S.split_flat(flat, in_dim, W, L)
    assert [m.shape for m in mats] == [m.shape for m in FF.split_weights(flat, in_dim, W, L)] and all(np.array_equal(a, b) for a, b in zip(mats, FF.split_weights(flat, in_dim, W, L)))
    out_o, fwd_o = FF.ffmlp_forward(x, flat, in_dim, W, L, 0)
    h, hidden = x, []
    for l in range(L):
        h = S.round16_acc32(S.mlp_layer_forward(h, mats[l]))
        hidden.append(h)
        assert np.array_equal(h, fwd_o[l].astype(np.float64)), l
    assert np.array_equal(S.round16_acc32(S.mlp_layer_forward(h, mats[L], relu=False)), out_o.astype(np.float64))
    gi_o, _, bwd_o = FF.ffmlp_backward(dy, x, flat, fwd_o, in_dim, W, L, 0)
    g = dy
    for k in range(L):                                   # k-th backward layer: matrix L - k, gate: hidden layer L - 1 - k
        g = S.round16_acc32(S.mlp_layer_backward(g, mats[L - k], hidden[L - 1 - k]))
        assert np.array_equal(g, bwd_o[k].astype(np.float64)), k
        assert np.abs(g).max() > 0
    assert np.array_equal(S.round16_acc32(S.mlp_layer_backward(g, mats[0])), gi_o.astype(np.float64))


def test_flat_from_parameters_pads_and_splits_as_the_steps_pack():
    rng = np.random.default_rng(8)
    col = [rng.standard_normal((64, 31)), rng.standard_normal((64, 64)), rng.standard_normal((3, 64))]
    m = S.flat_from_parameters(col, 32, 64, 2, split=16)
    assert [a.shape for a in m] == [(64, 32), (64, 64), (16, 64)]
    assert np.array_equal(m[0][:, :16], col[0][:, :16]) and np.all(m[0][:, 16] == 0) and np.array_equal(m[0][:, 17:], col[0][:, 16:])
    assert np.array_equal(m[2][:3], col[2]) and np.all(m[2][3:] == 0)
    d = S.flat_from_parameters([rng.standard_normal((128, 76))] + [rng.standard_normal((128, 128))] * 6 + [rng.standard_normal((3, 128))], 80, 128, 7)
    assert d[0].shape == (128, 80) and np.all(d[0][:, 76:] == 0) and d[7].shape == (16, 128) and np.all(d[7][3:] == 0)


def _dnerf_grid():
    offsets, pls = oracle.grid_offsets(3, 16, 2, 2, 16, 19, 2048, False)
    return offsets, pls, float(np.float32(np.log2(pls))), 16


def _grid_points(rng, n):
    x = rng.random((n, 3), dtype=np.float32)
    x[0], x[1] = 0.0, 1.0
    x[2, 0], x[3, 2] = -1e-3, 1.0 + 1e-3
    x[4:40] = x[4] + rng.random((36, 3), dtype=np.float32) * 1e-3          # neighbours in one coarse cell
    return x


def test_level_scales_are_the_oracles():
    import ctypes
    offsets, pls, Sg, H = _dnerf_grid()
    scale, res = S.level_scales(16, Sg, H)
    for l in range(16):
        s, r = ctypes.c_float(), ctypes.c_uint32()
        oracle.lib().orc_grid_level_params(ctypes.c_uint32(l), ctypes.c_float(Sg), ctypes.c_uint32(H), ctypes.byref(s), ctypes.byref(r))
        assert np.float32(s.value) == scale[l] and int(r.value) == int(res[l]), l


def test_tiled_grid_restatements_match_the_oracle_on_500_points():
    """Indices exactly (a one-hot gradient through the oracle's backward names the rows it touches), values at the fp32 bar."""
    rng = np.random.default_rng(9)
    offsets, pls, Sg, H = _dnerf_grid()
    x = _grid_points(rng, 500)
    table = rng.uniform(-1, 1, (int(offsets[-1]), 2)).astype(np.float32)
    c = S.tiled_corners(x, offsets, Sg, H)
    assert not c.valid[2] and not c.valid[3] and c.valid[0] and c.valid[1] and c.valid.sum() == 498
    assert np.allclose(c.weights.sum(2)[:, c.valid], 1.0, atol=1e-12) and np.all(c.weights[:, ~c.valid] == 0)
    out_o, dd_o = oracle.grid_encode_forward(x, table, offsets, pls, H, True, 1, False, 0)
    S.fp32_close(S.level_major_to_rows(S.grid_forward64(c, table)), out_o, "grid forward")
    dd = S.grid_dy_dx64(c, table)
    S.fp32_close(dd.reshape(500, -1), dd_o, "dy_dx")
    g = rng.standard_normal((500, 32)).astype(np.float32)
    ge_o, gi_o = oracle.grid_encode_backward(g, x, table, offsets, pls, H, dd_o, 1, False, 0)
    denc = S.rows_to_level_major(g)
    ge = S.grid_table_gradient64(denc, c)
    S.table_gradient_close(ge_o, ge, offsets, "table gradient", fp32=True)
    gi, mag = S.grid_input_gradient64(denc, dd)
    S.fp32_close(gi, gi_o, "input gradient")
    assert np.all(mag >= np.abs(gi) - 1e-12)
    # indices: the rows the oracle's backward touches for a gradient of ones are exactly the restated rows, level by level
    ones = np.ones((500, 32), np.float32)
    touched_o, _ = oracle.grid_encode_backward(ones, x, table, offsets, pls, H, None, 1, False, 0)
    touched = np.zeros(int(offsets[-1]), bool)
    touched[c.rows[:, c.valid].reshape(-1)] = True
    nz = touched_o[:, 0] != 0
    assert np.array_equal(nz | ~touched, np.ones_like(nz)) and not (nz & ~touched).any()
    # (a corner of weight exactly 0 is restated but adds 0.0 in the oracle: every other restated row must be touched)
    w_row = np.zeros(int(offsets[-1]))
    np.add.at(w_row, c.rows[:, c.valid].reshape(-1), c.weights[:, c.valid].reshape(-1))
    assert np.array_equal(nz, w_row > 0)
    S.fp32_close(touched_o[:, 0], w_row, "row weights")


def test_run_structure_counts_runs_inside_waves_and_across_them():
    rows = np.array([5] * 3 + [7] * 61 + [7] * 2 + [-1] + [7] * 4 + [9] * 57 + [9] * 64 + [2] * 10)
    rs = S.run_structure(rows)
    assert rs["lengths"][:2].tolist() == [3, 61] and rs["lengths"][2:6].tolist() == [2, 1, 4, 57]
    assert rs["longest"] == 64 and rs["crossings"] == 2 and rs["merging_waves"] == 4
    assert int(rs["lengths"].sum()) == 256           # padded to whole waves with idle lanes
    assert S.run_structure(np.arange(100))["merging_waves"] == 0 and S.run_structure(-np.ones(70))["longest"] == 1


def _merge_case():
    """A ray-like batch on the small directed grid: blocks of identical points and a slow drift, so that runs start, end and continue
    at wave boundaries."""
    rng = np.random.default_rng(11)
    offsets, pls = oracle.grid_offsets(3, 4, 2, 2, 4, 8, None, False)
    Sg = float(np.float32(np.log2(pls)))
    x = np.repeat(rng.random((12, 3), dtype=np.float32), [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129], axis=0)
    x[300, 1] = 1.5
    denc = rng.standard_normal((4, x.shape[0], 2))
    return offsets, S.tiled_corners(x, offsets, Sg, 4), denc


@pytest.mark.parametrize("variant", ["last_lane", "cut_at_63"])
def test_table_gradient_bars_reject_a_wrong_run_merge(variant):
    """A run's last lane dropped from its sum / a run ending on lane 63 never issued: both bars (fp32, and the half-atomic bar the
    fp16 step gets) fail on the mutated restatement."""
    offsets, c, denc = _merge_case()
    ref = S.grid_table_gradient64(denc, c)
    drop = S.merge_mutation(c, variant)
    assert drop.any() and not drop[:, ~c.valid].any()
    wrong = S.grid_table_gradient64(denc, c, drop=drop)
    S.table_gradient_close(ref.astype(np.float32), ref, offsets, "table gradient", fp32=True)
    for fp32 in (True, False):
        with pytest.raises(AssertionError):
            S.table_gradient_close(wrong, ref, offsets, f"table gradient ({variant})", fp32=fp32)


def test_mlp_bars_reject_an_unzeroed_column_16_and_a_gate_from_the_wrong_layer():
    flat, x, dy = _chain_case(12, 32, 64, 2, B=64)
    mats = [m.astype(np.float64) for m in S.split_flat(flat, 32, 64, 2)]
    zeroed = mats[0].copy()
    zeroed[:, 16] = 0
    x = x.astype(np.float64)
    x[:, 16] = 3.0                                       # the log-density column carries a value
    ref = S.mlp_layer_forward(x, zeroed)
    wrong = S.mlp_layer_forward(x, mats[0])
    S.mfma16_close(S.round16(ref), ref, "col_hidden[0]", 1)
    S.fp32_close(ref.astype(np.float32), ref, "col_hidden[0]")
    for close in (lambda a, b: S.mfma16_close(S.round16(a), b, "col_hidden[0], column 16 kept", 1), lambda a, b: S.fp32_close(a, b, "col_hidden[0], column 16 kept")):
        with pytest.raises(AssertionError):
            close(wrong, ref)
    h0 = S.round16(ref)
    h1 = S.round16(S.mlp_layer_forward(h0, mats[1]))
    g_ref = S.mlp_layer_backward(dy, mats[2], h1)
    g_wrong = S.mlp_layer_backward(dy, mats[2], h0)
    assert (h0 > 0).mean() > 0.2 and ((h0 > 0) != (h1 > 0)).mean() > 0.1
    for close in (lambda a, b: S.mfma16_close(S.round16(a), b, "col_bwd, gate of the wrong layer", 1), lambda a, b: S.fp32_close(a, b, "col_bwd, gate of the wrong layer")):
        with pytest.raises(AssertionError):
            close(g_wrong, g_ref)
    # and the input gradient's column 16: exactly zero only with the zeroed weight column
    assert np.all(S.mlp_layer_backward(g_ref, zeroed)[:, 16] == 0) and np.any(S.mlp_layer_backward(g_ref, mats[0])[:, 16] != 0)


def test_adam_pass64_is_torch_adam_over_three_steps():
    rng = np.random.default_rng(13)
    p0 = rng.standard_normal(300)
    p_t = torch.tensor(p0.copy(), requires_grad=True)
    opt = torch.optim.Adam([p_t], lr=1e-2, betas=(0.9, 0.99), eps=1e-15, foreach=False)
    p, m, v = p0.copy(), np.zeros(300), np.zeros(300)
    for step in (1, 2, 3):
        g16 = (rng.standard_normal(300) * 1024).astype(np.float16)
        g16[::10] = 0
        p_t.grad = torch.tensor(g16.astype(np.float64) / 1024.0)
        opt.step()
        p, m, v = S.adam_pass64(p, m, v, g16, 1.0 / 1024.0, step, 1e-2, 0.9, 0.99, 1e-15)
        st = opt.state[p_t]
        assert _rel(p, p_t.detach().numpy()) <= 1e-13 and _rel(m, st["exp_avg"].numpy()) <= 1e-13 and _rel(v, st["exp_avg_sq"].numpy()) <= 1e-13


def test_adam_bars_reject_the_other_groups_step_count_and_a_missing_divisor():
    rng = np.random.default_rng(14)
    p0, m0, v0 = rng.standard_normal(500) * 0.1, rng.standard_normal(500) * 1e-3, rng.random(500) * 1e-6
    g16 = (rng.standard_normal(500) * 1024 * 1e-3).astype(np.float16)
    args = (1e-3, 0.9, 0.99, 1e-15)
    p, m, v = S.adam_pass64(p0, m0, v0, g16, 1.0 / 2048.0, 3, *args)
    for what, (pw, mw, vw) in (("step 2 for step 3", S.adam_pass64(p0, m0, v0, g16, 1.0 / 2048.0, 2, *args)),
                               ("no divisor", S.adam_pass64(p0, m0, v0, g16, 1.0 / 1024.0, 3, *args))):
        S.fp32_close((p - p0).astype(np.float32), p - p0, "update")
        with pytest.raises(AssertionError):
            S.fp32_close(pw - p0, p - p0, f"update ({what})", extra=2.0 ** -24 * np.abs(p0))
        if what == "no divisor":
            for got, ref in ((mw, m), (vw, v)):
                with pytest.raises(AssertionError):
                    S.fp32_close(got, ref, f"moment ({what})")


def test_nonfinite16_and_the_scaler_rule():
    g = np.zeros(64, np.float16)
    assert not S.nonfinite16(g)
    g[:] = 65504
    g[1::2] = -65504
    g[5] = np.float16(6e-8)
    assert not S.nonfinite16(g)
    for bad in (np.inf, -np.inf, np.nan):
        h = g.copy()
        h[63] = bad
        assert S.nonfinite16(h)
    # torch's own rule on the CPU, the sequence of the optimizer test: three clean steps grow, a found inf backs off
    scale, tracker = torch.tensor([1024.0]), torch.tensor([0], dtype=torch.int32)
    seen = []
    for found in (0.0, 0.0, 0.0, 1.0):
        torch._amp_update_scale_(scale, tracker, torch.tensor([found]), 2.0, 0.5, 3)
        seen.append((float(scale), int(tracker)))
    assert seen == [(1024.0, 1), (1024.0, 2), (2048.0, 0), (1024.0, 0)]
    assert S.ema_decay_of(0.95, 1) == 2.0 / 11.0 and S.ema_decay_of(0.95, 1000) == 0.95
    assert np.allclose(S.ema_pass64(np.ones(3), np.zeros(3), 0.75), 0.75)
