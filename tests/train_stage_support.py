"""Float64 restatements of the stages of the native training steps (csrc/train.hip: sdn_train_step_f16 / sdn_train_step_f32), one
function per stage, in numpy.  Each takes the stage's inputs as arrays -- in the GPU tests the step's own workspace buffers as the GPU
left them (tests/test_gpu_train_stages.py) -- and returns the stage's outputs in float64, so a comparison sees the rounding of ONE
stage and a failure names the kernel.  tests/test_train_stages_cpu.py checks these functions against the CPU oracle and float64
autograd, so they are not trusted blind.  Reference lines (relative to the reference tree) are the ones the kernels cite."""
import numpy as np

F16_ULP = 2.0 ** -10          # relative size of one fp16 ulp at the top of a binade
F16_TINY = 2.0 ** -24         # the fp16 subnormal spacing
# The allowance for dh0 on top of its rounding bar, in float32 ulps (2^-24) of the magnitudes that cancel in it (`dh0_cancel`).
# Why the plain bar is wrong for dh0: it is not one rounding of a well-conditioned float32 result but a DIFFERENCE,
# delta0 * sum_ch grad_image (T_behind c - (image - running colour)) (raymarching.cu:655-675), of float32 prefix sums taken in tree
# order, and grad_image = 2 (image + (1 - weights_sum) bg - target) scale / N / 3 is a difference too; a float32 evaluation's error
# scales with the magnitudes that cancel, not with the result.  The constant is MEASURED on the CPU, not on the kernel: the worst
# distance of `composite_f32_restatement` (the kernels' float32 order, operation by operation) from the float64 reference over eight
# synthetic 510-ray batches is 0.69 of one float32 ulp of those magnitudes; rounded up to 1.  tests/test_train_stages_cpu.py asserts that
# the restatement stays inside the resulting bar.
CANCEL_ULPS = 1.0 * 2.0 ** -24
DEF_IN, DEF_W, DEF_L = 80, 128, 7
SIG_IN, SIG_W, SIG_OUT = 32, 64, 16
COL_IN, COL_W, COL_L = 32, 64, 2
DEF_FLAT = DEF_W * DEF_IN + (DEF_L - 1) * DEF_W * DEF_W + 16 * DEF_W
COL_FLAT = COL_W * COL_IN + (COL_L - 1) * COL_W * COL_W + 16 * COL_W


def f64(a):
    return np.asarray(a).astype(np.float64)


def round16(a):
    """float64 -> nearest fp16 (one rounding), as float64."""
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def round16_acc32(a):
    """float64 -> float32 -> fp16: the rounding of a layer whose sums sit in a float32 accumulator before the store (what the
    matrix cores and oracle/ffmlp.py's `_linear` do; differs from `round16` only where the float32 rounding lands on an fp16 tie)."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float16).astype(np.float64)


# ---- encode and deformed position -----------------------------------------------------------------------------------------------------
def encode(xyzs, time):
    """freq(x, 10) ++ freq(t, 6), padded to 80 columns (dnerf/network.py:123-138; freqencoder.cu:30-58: x, then per frequency
    sin(2^f x + 0) and sin(2^f x + pi/2) with the float32 phase and the float32 sum the formula is written in)."""
    x = np.asarray(xyzs, np.float32).reshape(-1, 3)
    half_pi = np.float32(np.float32(np.pi) / np.float32(2))
    out = np.zeros((x.shape[0], DEF_IN))
    out[:, :3] = x
    for f in range(10):
        a = np.ldexp(x, f).astype(np.float32)
        out[:, 3 + 6 * f:6 + 6 * f] = np.sin(f64(a))
        out[:, 6 + 6 * f:9 + 6 * f] = np.sin(f64((a + half_pi).astype(np.float32)))
    t = np.float32(time)
    out[:, 63] = t
    for f in range(6):
        a = np.float32(np.ldexp(t, f))
        out[:, 64 + 2 * f] = np.sin(np.float64(a))
        out[:, 65 + 2 * f] = np.sin(np.float64(np.float32(a + half_pi)))
    return out


def deformed_position(xyzs, def_out, time, bound):
    """x + deform, deform = 0 on the canonical frame (dnerf/network.py:140-145), normalised to [0, 1] as GridEncoder.forward does
    (gridencoder/grid.py:146)."""
    x = f64(xyzs).reshape(-1, 3)
    v = x if float(time) == 0.0 else x + f64(def_out)[:, :3]
    return (v + float(bound)) / (2.0 * float(bound))


# ---- sigma MLP ----------------------------------------------------------------------------------------------------------------------------
_SH_C = (0.28209479177387814, 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.31539156525251999, 0.54627421529603959,
         0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769)


def sh16(dirs):
    """SH(d, 4) in the closed forms of shencoder.cu:49-121."""
    d = f64(dirs).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    c = _SH_C
    return np.stack([np.full_like(x, c[0]), -c[1] * y, c[1] * z, -c[1] * x, c[2] * xy, -c[2] * yz, c[3] * zz - c[4], -c[2] * xz,
                     c[5] * (xx - yy), c[6] * y * (-3 * xx + yy), c[7] * xy * z, c[8] * y * (1 - 5 * zz), c[9] * z * (5 * zz - 3),
                     c[8] * x * (1 - 5 * zz), c[10] * z * (xx - yy), c[6] * x * (-xx + 3 * yy)], axis=1)


def level_major_to_rows(grid):
    """The grid encoder's [levels][M][2] -> row-major [M, 2 levels] (feature 2 level + channel; an exact transposition)."""
    g = np.asarray(grid)
    return np.ascontiguousarray(g.transpose(1, 0, 2)).reshape(g.shape[1], g.shape[0] * g.shape[2])


def rows_to_level_major(rows):
    r = np.asarray(rows)
    return np.ascontiguousarray(r.reshape(r.shape[0], r.shape[1] // 2, 2).transpose(1, 0, 2))


def sigma_forward(grid_out, dirs, w1, w2, half=False):
    """dnerf/network.py:147-160: h1 = relu(W1 enc), hout = W2 h1 (column 0: the log density), the colour MLP's input row
    [SH(d, 4) 16 | hout 16].  half: the hidden layer is rounded to fp16 as autocast's F.linear does; products and sums stay exact.
    -> (h1 [M,64], hout [M,16], col_in [M,32])."""
    enc = f64(level_major_to_rows(grid_out))
    h1 = np.maximum(enc @ f64(w1).T, 0.0)
    if half:
        h1 = round16(h1)
    hout = h1 @ f64(w2).T
    return h1, hout, np.concatenate([sh16(dirs), hout], axis=1)


def sigmas_of(hout0, density_scale):
    """trunc_exp forward (activation.py:5-11) x density_scale (dnerf/renderer.py:307) of the log-density column as stored."""
    return float(density_scale) * np.exp(f64(hout0))


def sigma_backward(dh0, dcol_in, h1, w1, w2, half=False):
    """dh = [dh0 | columns 17..31 of the colour MLP's input gradient], dh1 = (dh W2) * relu'(h1) with the gate of the h1 given,
    denc = dh1 W1 in the grid encoder's [level][sample][2] layout.  half: dh1 is rounded to fp16.  -> (dh, dh1, denc)."""
    dh = np.concatenate([f64(dh0).reshape(-1, 1), f64(dcol_in)[:, 17:32]], axis=1)
    dh1 = (dh @ f64(w2)) * (f64(h1) > 0)
    if half:
        dh1 = round16(dh1)
    return dh, dh1, rows_to_level_major(dh1 @ f64(w1))


# ---- compositing ------------------------------------------------------------------------------------------------------------------------------
def colours(col_out, half=False):
    """sigmoid of the colour MLP's first three outputs (dnerf/network.py:166); half: rounded to fp16 (torch.sigmoid on a half tensor
    computes in float and rounds once).  -> (colour [M,3], slack [M,3]).  slack is non-zero only where the float64 sigmoid lies within
    2^-22 (relative) of the midpoint of two fp16 values: there a float32 evaluation may round to the other neighbour, and slack is the
    distance between the two.  2^-22 bounds the float32 evaluation 1 / (1 + expf(-x)): expf within 1 ulp (2^-23 relative, and the
    sum damps it by e / (1 + e) <= 1), the sum and the quotient one rounding (2^-24) each: 2^-23 + 2^-24 + 2^-24."""
    c = 1.0 / (1.0 + np.exp(-f64(col_out)[:, :3]))
    if not half:
        return c, np.zeros_like(c)
    c16 = round16(c)
    ulp = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(c16, 2.0 ** -14))) - 10), F16_TINY)
    near_mid = np.abs(np.abs(c - c16) - 0.5 * ulp) <= 4 * 2.0 ** -24 * c
    return c16, np.where(near_mid, ulp, 0.0)


class RaySamples:
    """The [N, longest ray] gather of a ray table (raymarching.cu:501-520: a ray with count == 0 or offset + count > M has no samples)."""

    def __init__(self, rays, M):
        r = np.asarray(rays).astype(np.int64).reshape(-1, 3)
        self.N, self.M = r.shape[0], int(M)
        self.index, self.offset, self.count = r[:, 0], r[:, 1], r[:, 2]
        self.kept = (self.count > 0) & (self.offset + self.count <= self.M)
        width = int(self.count[self.kept].max()) if self.kept.any() else 1
        k = np.arange(width)[None, :]
        self.valid = self.kept[:, None] & (k < self.count[:, None])
        self.idx = np.where(self.valid, self.offset[:, None] + k, 0)

    def gather(self, a, fill=0.0):
        return np.where(self.valid if a.ndim == 1 else self.valid[..., None], f64(a)[self.idx], fill)

    def scatter(self, values, mask, shape):
        out = np.zeros(shape)
        out[self.idx[mask]] = values[mask]
        return out


def composite_forward(sigmas, deltas, colour, rays, T_thresh=1e-4, colour_slack=None):
    """composite_rays_train forward (raymarching.cu:501-577), vectorised per ray: alpha = 1 - exp(-sigma delta0), T the exclusive
    cumulative product of (1 - alpha), sample i composited iff T_i >= T_thresh (the sequential loop's early stop: T never grows),
    t the running sum of delta1.  Results are indexed by the ray's `index` column.  -> dict with weights_sum [N], depth [N],
    image [N,3], and the per-sample terms the backward and the tests' coverage counts need (arrays [N, longest ray])."""
    rs = RaySamples(rays, np.asarray(sigmas).shape[0])
    d = f64(deltas).reshape(-1, 2)
    d0, d1 = rs.gather(d[:, 0]), rs.gather(d[:, 1])
    alpha = -np.expm1(-rs.gather(f64(sigmas)) * d0)
    T = np.cumprod(np.concatenate([np.ones((rs.N, 1)), 1.0 - alpha[:, :-1]], axis=1), axis=1)
    on = rs.valid & (T >= T_thresh)
    w = np.where(on, alpha * T, 0.0)
    t = np.cumsum(d1, axis=1)
    c = rs.gather(f64(colour))
    ws, depth, image = np.zeros(rs.N), np.zeros(rs.N), np.zeros((rs.N, 3))
    ws[rs.index], depth[rs.index], image[rs.index] = w.sum(1), (w * t).sum(1), (w[..., None] * c).sum(1)
    out = dict(rs=rs, alpha=alpha, T=T, on=on, w=w, c=c, d0=d0, weights_sum=ws, depth=depth, image=image)
    if colour_slack is not None:
        u = rs.gather(f64(colour_slack))
        out["u"] = u
        out["image_slack"] = np.zeros((rs.N, 3))
        out["image_slack"][rs.index] = (w[..., None] * u).sum(1)
    return out


def loss_terms(image, weights_sum, target, bg):
    """dnerf/renderer.py:318 and dnerf/utils.py:85, :125: pred = image + (1 - weights_sum) bg; per ray the sum over channels of
    (pred - target)^2; the loss is its mean over rays and channels.  -> (pred [N,3], sq_err [N], loss)."""
    pred = f64(image) + (1.0 - f64(weights_sum))[:, None] * f64(bg)
    sq = ((pred - f64(target)) ** 2).sum(1)
    return pred, sq, float(sq.sum() / 3.0 / sq.shape[0])


def loss_gradient(image, weights_sum, target, bg, loss_scale=1.0):
    """d(loss_scale * loss) / d(image, weights_sum): 2 (pred - target) loss_scale / N / 3, and -sum_ch of it times bg."""
    pred = f64(image) + (1.0 - f64(weights_sum))[:, None] * f64(bg)
    gi = 2.0 * (pred - f64(target)) * (float(loss_scale) / pred.shape[0] / 3.0)
    return gi, -(gi * f64(bg)).sum(1)


def composite_backward_core(fwd, grad_image, grad_ws, image, weights_sum, grad_image_mag=None):
    """composite_rays_train backward (raymarching.cu:602-682) on the forward's per-sample terms, with the forward's image and
    weights_sum as GIVEN (the operator reads them back): grad_rgb = grad_image * weight, grad_sigma = delta0 * (sum_ch grad_image
    (T_behind c - (image - running colour)) + grad_ws (1 - weights_sum)).  -> (grad_sigmas [M], grad_rgbs [M,3], cancel [M]);
    cancel is the sum of the magnitudes of the terms that cancel in grad_sigma (what a float32 evaluation's error scales with);
    grad_image_mag, if given, replaces |grad_image| there (a grad_image that is itself a difference, as the loss gradient is)."""
    rs, w, c, on = fwd["rs"], fwd["w"], fwd["c"], fwd["on"]
    gi, gws = f64(grad_image)[rs.index][:, None, :], f64(grad_ws)[rs.index][:, None]
    fin, wsf = f64(image)[rs.index][:, None, :], f64(weights_sum)[rs.index][:, None]
    run = np.cumsum(w[..., None] * c, axis=1)
    T_after = (fwd["T"] * (1.0 - fwd["alpha"]))[..., None]
    gs = fwd["d0"] * ((gi * (T_after * c - (fin - run))).sum(2) + gws * (1.0 - wsf))
    gm = np.abs(gi) if grad_image_mag is None else f64(grad_image_mag)[rs.index][:, None, :]
    gwm = np.abs(gws) if grad_image_mag is None else gm.sum(2)          # (bg <= 1: |grad_ws| <= the sum of the magnitudes)
    cancel = fwd["d0"] * ((gm * (T_after * c + np.abs(fin) + run)).sum(2) + gwm * (1.0 + np.abs(wsf)))
    if "u" in fwd:       # an fp16 colour that may round either way moves its own term and every running sum behind it
        cancel_u = fwd["d0"] * (np.abs(gi) * (T_after * fwd["u"] + np.cumsum(w[..., None] * fwd["u"], axis=1))).sum(2)
    else:
        cancel_u = np.zeros_like(gs)
    M = rs.M
    return (rs.scatter(gs, on, (M,)), rs.scatter(gi * w[..., None], on, (M, 3)), rs.scatter(cancel, on, (M,)), rs.scatter(cancel_u, on, (M,)))


def composite_backward(fwd, image, weights_sum, target, bg, hout0, loss_scale, density_scale):
    """The compositing backward of the training steps: the loss gradient (loss scale, / N / 3), composite_rays_train backward, then
    sigmoid backward (grad * (1 - y) * y on the colour as stored), density_scale and trunc_exp backward (activation.py:12-17:
    grad * exp(clamp(x, -15, 15))).  -> dict: dcol_out [M,16] (columns 3..15 zero), dh0 [M], both zero for samples that are off;
    dh0_cancel / dcol_slack: see composite_backward_core / colours."""
    gi, gws = loss_gradient(image, weights_sum, target, bg, loss_scale)
    # the loss gradient is itself a difference, image + (1 - weights_sum) bg - target: the magnitudes that cancel in it
    gi_mag = (np.abs(f64(image)) + np.abs(1.0 - f64(weights_sum))[:, None] * np.abs(f64(bg)) + np.abs(f64(target))) * (2.0 * float(loss_scale) / gi.shape[0] / 3.0)
    gs, grgb, cancel, cancel_u = composite_backward_core(fwd, gi, gws, image, weights_sum, gi_mag)
    rs = fwd["rs"]
    c = rs.scatter(fwd["c"], fwd["on"], (rs.M, 3))
    dcol = np.zeros((rs.M, 16))
    dcol[:, :3] = grgb * (1.0 - c) * c
    e = float(density_scale) * np.exp(np.clip(f64(hout0), -15.0, 15.0))
    out = dict(dcol_out=dcol, dh0=gs * e, dh0_cancel=cancel * e, dh0_slack=cancel_u * e, on=rs.scatter(fwd["on"].astype(np.float64), fwd["on"], (rs.M,)) > 0)
    if "u" in fwd:
        out["dcol_slack"] = np.abs(grgb * (1.0 - 2.0 * c)) * rs.scatter(fwd["u"], fwd["on"], (rs.M, 3))
    return out


def flip_rays(fwd, T_thresh=1e-4, rel=1e-4):
    """Rays (by `index`) with a sample whose transmittance in front of it is within `rel` (relative) of T_thresh: a float32 prefix
    product (good to ~1e-5 over 64 terms) may decide the other way there."""
    rs = fwd["rs"]
    near = rs.valid & (np.abs(fwd["T"] - T_thresh) <= rel * T_thresh)
    out = np.zeros(rs.N, bool)
    out[rs.index] = near.any(1)
    return out


def coverage(fwd, T_thresh=1e-4):
    """Per-ray sample counts and termination classes of a batch (rays in table order): count [N]; first_off [N]: the first sample
    with T < T_thresh in front of it, or -1 if the ray never terminates."""
    rs = fwd["rs"]
    off = rs.valid & (fwd["T"] < T_thresh)
    return np.where(rs.kept, rs.count, 0), np.where(off.any(1), off.argmax(1), -1)


# ---- deformation gradient ---------------------------------------------------------------------------------------------------------------------
def deform_gradient(dx, bound):
    """The gradient of the deformation MLP's 16-wide output: the grid input gradient / (2 bound) (gridencoder/grid.py:146's
    normalisation backwards) in columns 0..2, zero in 3..15."""
    out = np.zeros((np.asarray(dx).shape[0], 16))
    out[:, :3] = f64(dx).reshape(-1, 3) / (2.0 * float(bound))
    return out


# ---- weight gradients --------------------------------------------------------------------------------------------------------------------------
def weight_gradient_jobs(fp32):
    """The 13 products dW = A^T B of a step (csrc/train.hip: dw_job_list / dw32_jobs; ffmlp.cu:800-876 for the pairing): per job
    (gradient buffer, element offset of the block, rows, cols, (A buffer, layer or None), (B buffer, layer or None)).  The gradient of
    hidden layer l's pre-activation is def_bwd / col_bwd [L - 1 - l] in the fp16 step (the backward chain stores as it goes) and [l] in
    the fp32 step.  'enc' is the sigma MLP's row-major input (enc_rm, or grid_out transposed)."""
    jobs = []
    for g, A, H, X, ddown, W, cin, L in (("g_deform", "def_bwd", "def_hidden", "enc_in", "ddef", DEF_W, DEF_IN, DEF_L),
                                       ("g_color", "col_bwd", "col_hidden", "col_in", "dcol_out", COL_W, COL_IN, COL_L)):
        at = (lambda l: l) if fp32 else (lambda l, L=L: L - 1 - l)
        jobs.append((g, 0, W, cin, (A, at(0)), (X, None)))
        for l in range(1, L):
            jobs.append((g, W * cin + (l - 1) * W * W, W, W, (A, at(l)), (H, l - 1)))
        jobs.append((g, W * cin + (L - 1) * W * W, 16, W, (ddown, None), (H, L - 1)))
    jobs.append(("g_sigma0", 0, SIG_W, SIG_IN, ("dh1", None), ("enc", None)))
    jobs.append(("g_sigma1", 0, SIG_OUT, SIG_W, ("dh", None), ("h1", None)))
    return jobs


def weight_gradients(bufs, fp32):
    """All 13 blocks in float64 from the buffers the job list pairs.  bufs: name -> array ([M, width], or [L, M, width]).
    -> {gradient buffer: flat float64 array in the flat layout}, and the job list."""
    jobs = weight_gradient_jobs(fp32)
    out = {"g_deform": np.zeros(DEF_FLAT), "g_color": np.zeros(COL_FLAT), "g_sigma0": np.zeros(SIG_W * SIG_IN), "g_sigma1": np.zeros(SIG_OUT * SIG_W)}
    for g, off, rows, cols, (a, al), (b, bl) in jobs:
        A = f64(bufs[a] if al is None else bufs[a][al])
        B = f64(bufs[b] if bl is None else bufs[b][bl])
        assert A.shape[1] == rows and B.shape[1] == cols, (g, off, A.shape, B.shape)
        out[g][off:off + rows * cols] = (A.T @ B).reshape(-1)
    return out, jobs


# ---- the packed MLP chains, one layer at a time ---------------------------------------------------------------------------------------------------
def split_flat(flat, in_ld, W, L):
    """The flat weight layout [W, in_ld] ++ (L - 1) x [W, W] ++ [16, W] (ffmlp.cu:631) -> the L + 1 matrices [out, in], in layer order."""
    w = np.asarray(flat).reshape(-1)
    mats, off = [], 0
    for r, c in [(W, in_ld)] + [(W, W)] * (L - 1) + [(16, W)]:
        mats.append(w[off:off + r * c].reshape(r, c))
        off += r * c
    assert off == w.size, (off, w.size)
    return mats


def flat_from_parameters(params, in_ld, W, L, split=None):
    """The same L + 1 matrices from the model's parameters ([W, in], ..., [3, W]), padded with zeros as the steps pack them: the input
    layer to in_ld columns, the output layer to 16 rows; split: the flat input column that is structurally zero (the colour MLP's
    log-density column 16: the columns behind it sit one further right)."""
    mats = []
    for i, p in enumerate(params):
        p = f64(p)
        rows, cols = (W if i < L else 16), (in_ld if i == 0 else W)
        m = np.zeros((rows, cols))
        if i == 0 and split is not None:
            m[:p.shape[0], :split] = p[:, :split]
            m[:p.shape[0], split + 1:split + 1 + p.shape[1] - split] = p[:, split:]
        else:
            m[:p.shape[0], :p.shape[1]] = p
        mats.append(m)
    assert len(mats) == L + 1
    return mats


def mlp_layer_forward(x, W, relu=True):
    """ONE layer: x W^T, through the ReLU for a hidden layer.  Exact products, float64 sums, no rounding."""
    y = f64(x) @ f64(W).T
    return np.maximum(y, 0.0) if relu else y


def mlp_layer_backward(dy, W, act_out=None):
    """ONE layer backwards: dy W (W the [out, in] matrix dy came out of), gated by `act_out > 0` -- the stored post-activation of
    the layer the gradient arrives at (ReLU's derivative from its output, utils.h:538-541); None: the network's input, no gate."""
    g = f64(dy) @ f64(W)
    return g if act_out is None else g * (f64(act_out) > 0)


# ---- the tiled grid of the dnerf network: D = 3, C = 2, tiled, no align_corners, linear interpolation ------------------------------------------------
def level_scales(n_levels, S, H):
    """gridencoder.cu:138-139 as the host code evaluates it in float32: scale = exp2f(level * S) * H - 1, resolution = ceil(scale) + 1.
    (exp2 is taken in double and rounded once: the correctly rounded float32 result; tests/test_train_stages_cpu.py checks it against
    the oracle's own exp2f level by level.)"""
    p = (np.arange(n_levels, dtype=np.float32) * np.float32(S)).astype(np.float32)
    e = np.exp2(p.astype(np.float64)).astype(np.float32)
    scale = (e * np.float32(H)).astype(np.float32) - np.float32(1)
    return scale.astype(np.float32), np.ceil(scale.astype(np.float64)).astype(np.int64) + 1


class Corners:
    """What `tiled_corners` returns: rows [L, B, 8] (table row, level offset included; 0 where the point is out of range), weights
    [L, B, 8] float64 (0 there), frac [L, B, 3] the float32 in-cell position as float64, scale [L] float64, valid [B]."""

    def __init__(self, rows, weights, frac, scale, valid, n_rows):
        self.rows, self.weights, self.frac, self.scale, self.valid, self.n_rows = rows, weights, frac, scale, valid, n_rows


def tiled_corners(x, offsets, S, H):
    """Per level the 8 corner rows and trilinear weights of every point (gridencoder.cu:143-189, :66-84 with gridtype tiled): pos =
    x * scale + 0.5f and its floor are taken in FLOAT32, operation by operation, exactly as k_grid_bwd and the oracle take them (the
    cell a point falls in must not depend on who computes it); the in-cell position pos - floor is exact in float32, and the weights
    are its products in float64.  Corner idx has bit d set <=> +1 along d.  The row index is the tiled one: sum of pos_grid[d] *
    stride over the dimensions whose stride still fits the level, modulo the level's row count (uint32 arithmetic)."""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    off = np.asarray(offsets).astype(np.int64)
    L, B = off.size - 1, x.shape[0]
    scale, res = level_scales(L, S, H)
    valid = ~((x < 0) | (x > 1)).any(1)
    rows, weights, frac = np.zeros((L, B, 8), np.int64), np.zeros((L, B, 8)), np.zeros((L, B, 3))
    for l in range(L):
        pos = ((x * scale[l]).astype(np.float32) + np.float32(0.5)).astype(np.float32)
        fl = np.floor(pos).astype(np.float32)
        pg = np.where(valid[:, None], fl, 0).astype(np.int64)
        fr = (pos - fl).astype(np.float32).astype(np.float64)
        frac[l] = fr
        size = int(off[l + 1] - off[l])
        for idx in range(8):
            w, index, stride = np.ones(B), np.zeros(B, np.int64), 1
            for d in range(3):
                up = (idx >> d) & 1
                w = w * (fr[:, d] if up else 1.0 - fr[:, d])
                if stride <= size:
                    index = (index + (pg[:, d] + up) * stride) & 0xFFFFFFFF
                    stride = (stride * (int(res[l]) + 1)) & 0xFFFFFFFF
            rows[l, :, idx] = np.where(valid, off[l] + index % size, 0)
            weights[l, :, idx] = np.where(valid, w, 0.0)
    return Corners(rows, weights, frac, scale.astype(np.float64), valid, int(off[-1]))


def grid_forward64(corners, table):
    """[L, B, 2]: sum over the corners of weight x table row (gridencoder.cu:187-189), float64."""
    return (corners.weights[..., None] * f64(table)[corners.rows]).sum(2)


def grid_table_gradient64(denc, corners, drop=None):
    """[rows, 2]: every sample adds weight x its level's gradient to each of its 8 rows (gridencoder.cu:248-340), float64.
    denc: [L, B, 2].  drop: bool [L, B, 8], contributions to leave out (the wrong variants of the run merge)."""
    out = np.zeros((corners.n_rows, 2))
    contrib = corners.weights[..., None] * f64(denc)[:, :, None, :]
    keep = np.broadcast_to(corners.valid[None, :, None], corners.rows.shape)
    if drop is not None:
        keep = keep & ~drop
    np.add.at(out, corners.rows[keep], contrib[keep])
    return out


def grid_dy_dx64(corners, table):
    """[B, L, 3, 2]: d(feature) / d(x[gd]) = scale * sum over the 4 corners of the other two dimensions of their weights times
    (table row one step along gd - table row) (gridencoder.cu:193-236), float64; zero for a point out of range."""
    T = f64(table)[corners.rows]                                   # [L, B, 8, 2]
    L, B = corners.rows.shape[:2]
    out = np.zeros((B, L, 3, 2))
    fr = corners.frac
    for gd in range(3):
        others = [d for d in range(3) if d != gd]
        for idx in range(8):
            if (idx >> gd) & 1:
                continue
            w = corners.scale[:, None] * np.ones((L, B))
            for d in others:
                w = w * (fr[:, :, d] if (idx >> d) & 1 else 1.0 - fr[:, :, d])
            out[:, :, gd, :] += (w[..., None] * (T[:, :, idx | (1 << gd)] - T[:, :, idx])).transpose(1, 0, 2)
    return out * corners.valid[:, None, None, None]


def grid_input_gradient64(denc, dy_dx):
    """[B, 3] = sum over levels and channels of denc[l, b, c] * dy_dx[b, l, d, c] (gridencoder.cu:343-369), and the sum of the
    terms' magnitudes (what a rounded evaluation's error scales with).  denc: [L, B, 2]."""
    terms = f64(denc).transpose(1, 0, 2)[:, :, None, :] * f64(dy_dx)
    return terms.sum((1, 3)), np.abs(terms).sum((1, 3))


def run_structure(rows, wave=64):
    """The runs k_grid_bwd's wave-level merge sees on ONE corner of ONE level: rows[b] is sample b's row (negative: an idle lane --
    a point out of range; idle lanes never merge), lane = b % wave.  A run is a maximal stretch of equal rows inside one wave.
    -> dict: lengths (every run's length, in order), wave_of_run, longest, merging_waves (waves with a run longer than one lane),
    crossings (wave boundaries at which the same row continues: a row run the merge must cut there and finish with two atomics)."""
    r = np.asarray(rows).astype(np.int64).reshape(-1)
    n = r.size
    key = np.where(r < 0, -1 - np.arange(n), r)
    pad = (-n) % wave
    key = np.concatenate([key, -1 - n - np.arange(pad)])
    k = key.reshape(-1, wave)
    head = np.ones(k.shape, bool)
    head[:, 1:] = k[:, 1:] != k[:, :-1]
    starts = np.flatnonzero(head.ravel())
    lengths = np.diff(np.append(starts, key.size))
    wave_of_run = starts // wave
    crossings = int((k[1:, 0] == k[:-1, -1]).sum())
    return dict(lengths=lengths, wave_of_run=wave_of_run, longest=int(lengths.max()) if lengths.size else 0,
                merging_waves=int(np.unique(wave_of_run[lengths > 1]).size), crossings=crossings)


def merge_mutation(corners, variant, wave=64):
    """bool [L, B, 8]: the contributions a WRONG run merge loses.  'last_lane': the last lane of every run longer than one lane is left
    out of its run's sum (a scan that stops one offset early); 'cut_at_63': a run that ends on the wave's last lane is never issued (a
    tail test that looks only at the next lane's head bit)."""
    L, B, _ = corners.rows.shape
    drop = np.zeros(corners.rows.shape, bool)
    for l in range(L):
        for idx in range(8):
            rows = np.where(corners.valid, corners.rows[l, :, idx], -1)
            rs = run_structure(rows, wave)
            starts = np.concatenate([[0], np.cumsum(rs["lengths"])[:-1]])
            ends = starts + rs["lengths"] - 1
            if variant == "last_lane":
                lost = ends[rs["lengths"] > 1]
            elif variant == "cut_at_63":
                sel = ends % wave == wave - 1
                lost = np.concatenate([np.arange(s, e + 1) for s, e in zip(starts[sel], ends[sel])]) if sel.any() else np.zeros(0, np.int64)
            else:
                raise ValueError(variant)
            lost = lost[lost < B].astype(np.int64)
            drop[l, lost, idx] = corners.valid[lost]
    return drop


def table_gradient_close(got, ref, offsets, what, fp32):
    """The table gradient's bar, level by level.  fp32: the project's fp32 bar.  fp16 (packed-half atomics, every atomic rounds the
    running sum): the bar of tests/test_gpu_ops_parity.py::test_grid_encode_backward, rtol 2e-2 with atol 2e-3 x the level's largest
    reference magnitude.  -> the worst error over the levels, in units of the bar."""
    off = np.asarray(offsets).astype(np.int64)
    worst = 0.0
    for l in range(off.size - 1):
        g, r = f64(got)[off[l]:off[l + 1]], f64(ref)[off[l]:off[l + 1]]
        if fp32:
            worst = max(worst, fp32_close(g, r, f"{what} level {l}"))
        else:
            worst = max(worst, half_atomic_close(g, r, f"{what} level {l}", float(np.abs(r).max())))
    return worst


def half_atomic_close(got, ref, what, atol_scale):
    """rtol 2e-2 with atol 2e-3 x atol_scale: sums taken with packed-half atomics in the hardware's order."""
    got, ref = f64(got), f64(ref)
    tol = 2e-2 * np.abs(ref) + 2e-3 * float(atol_scale)
    r = np.abs(got - ref) / np.maximum(tol, 1e-300)
    worst = float(r.max()) if r.size else 0.0
    print(f"[stage] {what}: worst error {worst:.3f} of the half-atomic bar (max |ref| {float(np.abs(ref).max()) if ref.size else 0:.3e})")
    assert worst <= 1.0, f"{what}: {worst:.3f} x the half-atomic bar at {np.unravel_index(int(r.argmax()), r.shape)}"
    return worst


def bound_close(got, ref, tol, what, name):
    """|got - ref| <= tol element by element, tol a derived per-element bound.  -> the worst error in units of the bound."""
    got, ref, tol = f64(got), f64(ref), f64(tol)
    r = np.abs(got - ref) / np.maximum(tol, 1e-300)
    worst = float(r.max()) if r.size else 0.0
    print(f"[stage] {what}: worst error {worst:.3f} of {name} (max |ref| {float(np.abs(ref).max()) if ref.size else 0:.3e})")
    assert worst <= 1.0, f"{what}: {worst:.3f} x {name} at {np.unravel_index(int(r.argmax()), r.shape)}"
    return worst


# ---- the fp16 step's optimizer pass -------------------------------------------------------------------------------------------------------------------
def nonfinite16(g):
    """Is any fp16 element an inf or a NaN (all five exponent bits set)?"""
    bits = np.ascontiguousarray(np.asarray(g, np.float16)).view(np.uint16)
    return bool(((bits & 0x7C00) == 0x7C00).any())


def adam_pass64(p, m, v, g16, inv_scale, step, lr, b1, b2, eps):
    """torch.optim.Adam's single-tensor update (adam.py _single_tensor_adam; no weight decay, amsgrad or maximize) in float64 on the
    gradient GradScaler.unscale_ hands it, float(g16) * inv_scale: m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, 1 - b2);
    denom = sqrt(v) / sqrt(1 - b2^step) + eps; p.addcdiv_(m, denom, -lr / (1 - b1^step)).  -> (p, m, v)."""
    p, m, v = f64(p), f64(m), f64(v)
    g = f64(g16) * float(inv_scale)
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v


def ema_decay_of(decay, n_updates):
    """torch_ema's effective decay at its n-th update (num_updates is incremented before use): min(decay, (1 + n) / (10 + n))."""
    return min(float(decay), (1.0 + n_updates) / (10.0 + n_updates))


def ema_pass64(shadow, p, decay):
    """torch_ema: shadow -= (1 - decay) * (shadow - p)."""
    return f64(shadow) - (1.0 - decay) * (f64(shadow) - f64(p))


# ---- bars -------------------------------------------------------------------------------------------------------------------------------------
def fp32_close(got, ref, what, extra=0.0):
    """The project's fp32 bar: 1e-4 relative with atol = 1e-5 x the largest reference magnitude.  -> the worst error in units of the bar."""
    got, ref = f64(got), f64(ref)
    tol = 1e-4 * np.abs(ref) + 1e-5 * float(np.abs(ref).max()) + extra
    r = np.abs(got - ref) / np.maximum(tol, 1e-300)
    worst = float(r.max()) if r.size else 0.0
    print(f"[stage] {what}: worst error {worst:.3f} of the fp32 bar (max |ref| {float(np.abs(ref).max()) if ref.size else 0:.3e})")
    assert worst <= 1.0, f"{what}: {worst:.3f} x the fp32 bar at {np.unravel_index(int(r.argmax()), r.shape)}"
    return worst


def ulp16_close(got, ref, what, ulps=1.5, extra=0.0):
    """fp16 value that is one rounding of an fp32 result: within `ulps` fp16 ulp of the float64 value (relative ulps * 2^-10, absolute
    floor 2^-24 in the subnormal range)."""
    got, ref = f64(got), f64(ref)
    tol = np.maximum(ulps * F16_ULP * np.abs(ref), F16_TINY) + extra
    r = np.abs(got - ref) / tol
    worst = float(r.max()) if r.size else 0.0
    print(f"[stage] {what}: worst error {worst:.3f} of {ulps} fp16 ulp (max |ref| {float(np.abs(ref).max()) if ref.size else 0:.3e})")
    assert worst <= 1.0, f"{what}: {worst:.3f} x {ulps} fp16 ulp at {np.unravel_index(int(r.argmax()), r.shape)}"
    return worst


def mfma16_close(got, ref, what, L):
    """The bar of tests/test_gpu_ffmlp_parity.py::_close for fp16 in, fp32 accumulate, one fp16 rounding per layer: within
    2 (L + 1) fp16 ulp on 99.9 % of the elements, 1 % norm-wise.  That bar, with one addition: a difference of one fp16 subnormal
    spacing (2^-24, no multiplier) is never counted -- below 2^-14 fp16 values sit on that grid whatever the bar in ulps says."""
    a, b = np.asarray(got).astype(np.float32), np.asarray(ref).astype(np.float32)
    scale = float(np.abs(b).max()) + 1e-12
    ulps = 2 * (L + 1)
    bad = np.abs(a - b) > np.maximum(ulps * 2.0 ** -10 * np.maximum(np.abs(b), scale / 64), F16_TINY)
    rel = float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
    print(f"[stage] {what}: {bad.mean():.2e} of the elements beyond {ulps} ulp, norm-wise {rel:.2e}")
    assert bad.mean() <= 1e-3, f"{what}: {bad.mean():.2e} of the elements off by more than {ulps} ulp"
    assert np.linalg.norm(a - b) <= 1e-2 * np.linalg.norm(b) + 1e-6, f"{what}: norm-wise {rel:.2e}"
    return float(bad.mean()), rel


# ---- the batch --------------------------------------------------------------------------------------------------------------------------------
def wedge_occupancy(pose, grid_size=128, lo=-0.8, hi=0.8, thickest=1.0):
    """[H,H,H] bool in (ix, iy, iz) order: a slab through the origin, perpendicular to the camera's viewing direction, whose thickness
    grows linearly from 0 at camera-right coordinate `lo` to `thickest` at `hi` -- rays of one image row then own from 0 to
    thickest / dt samples."""
    c = (np.arange(grid_size, dtype=np.float64) + 0.5) * 2.0 / grid_size - 1.0
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    right, fwd = f64(pose[:3, 0]), f64(pose[:3, 2])
    u = X * right[0] + Y * right[1] + Z * right[2]
    w = X * fwd[0] + Y * fwd[1] + Z * fwd[2]
    thick = thickest * np.clip((u - lo) / (hi - lo), 0.0, 1.0)
    return np.abs(w) < 0.5 * thick


COUNT_BANDS = ((0, 0), (1, 63), (65, 128), (129, 192), (193, 1 << 30))


def assert_coverage(count, first_off, min_rays=8):
    """The coverage a long-ray batch must have (counts and termination from the float64 reference, not from the kernel under test)."""
    for lo, hi in COUNT_BANDS:
        n = int(((count >= lo) & (count <= hi)).sum())
        assert n >= min_rays, f"only {n} rays with {lo}..{hi} samples"
    assert int((count == 64).sum()) >= 1, "no ray with exactly 64 samples"
    classes = {"terminate in chunk 0, owning further chunks": (first_off >= 0) & (first_off < 64) & (count > 64),
               "terminate in a later chunk": first_off >= 64, "never terminate": (first_off < 0) & (count > 0)}
    for name, m in classes.items():
        assert int(m.sum()) >= min_rays, f"only {int(m.sum())} rays that {name}"
    return {k: int(v.sum()) for k, v in classes.items()}


# ---- float32 restatement of the wave-per-ray compositing (for deriving bars on the CPU, never compared with the GPU) --------------------------
def _wave_scan(v, op):
    """Inclusive Hillis-Steele scan over 64 lanes in float32 (csrc/train.hip: wave_incl_sum / wave_excl_product)."""
    v = v.copy()
    for o in (1, 2, 4, 8, 16, 32):
        u = v.copy()
        v[o:] = op(v[o:], u[:-o])
    return v


def _wave_sum(v):
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v[0]


def composite_f32_restatement(sigmas, deltas, colour, rays, target, bg_value, loss_scale, T_thresh=1e-4):
    """k_train_composite_fwd / _bwd restated in numpy float32, operation by operation: one ray per wave, 64-sample chunks, alpha from a
    correctly rounded exp, T as T_carry times the exclusive prefix PRODUCT over the lanes, running colours as acc_c plus the inclusive
    prefix SUM, per-lane accumulation over the chunks then a butterfly sum for the ray's totals, the carry of T and acc_c from lane
    63, the `T_carry >= T_thresh` loop exit, the loss gradient ((pred - gt) * 2) * ((scale / N) / 3) from the float32 forward results as
    the backward kernel reads them back.  -> (weights_sum, image, grad_sigmas [M], grad_rgbs [M,3])."""
    f = np.float32
    sig, d, col = np.asarray(sigmas, f), np.asarray(deltas, f).reshape(-1, 2), np.asarray(colour, f)
    r = np.asarray(rays).astype(np.int64).reshape(-1, 3)
    N, M, thr = r.shape[0], sig.shape[0], f(T_thresh)
    ws_out, img_out = np.zeros(N, f), np.zeros((N, 3), f)
    lane = np.arange(64)

    def chunks(offset, count):
        T_carry = f(1)
        for c0 in range(0, count, 64):
            if not T_carry >= thr:
                break
            in_ray = c0 + lane < count
            idx = np.where(in_ray, offset + c0 + lane, 0)
            d0 = np.where(in_ray, d[idx, 0], f(0)).astype(f)
            alpha = np.where(in_ray, f(1) - np.exp((-sig[idx] * d0).astype(np.float64)).astype(f), f(0)).astype(f)
            om = (f(1) - alpha).astype(f)
            inc = _wave_scan(om, np.multiply)
            T = (T_carry * np.concatenate([[f(1)], inc[:-1]]).astype(f)).astype(f)
            on = in_ray & (T >= thr)
            w = np.where(on, alpha * T, f(0)).astype(f)
            c = np.where(in_ray[:, None], col[idx], f(0)).astype(f)
            yield idx, d0, alpha, T, on, w, c
            T_carry = (T * om).astype(f)[63]

    kept = [(int(i), int(o), int(n)) for i, o, n in r if n > 0 and o + n <= M]
    for index, offset, count in kept:
        acc = np.zeros((64, 4), f)
        for idx, d0, alpha, T, on, w, c in chunks(offset, count):
            acc[:, 0] += w
            acc[:, 1:] += w[:, None] * c
        ws_out[index] = _wave_sum(acc[:, 0])
        img_out[index] = [_wave_sum(acc[:, 1 + ch]) for ch in range(3)]
    gt, bgc = np.asarray(target, f), f(bg_value)
    cg = f(f(f(loss_scale) / f(N)) / f(3))
    gs, grgb = np.zeros(M, f), np.zeros((M, 3), f)
    for index, offset, count in kept:
        fin, wsf = img_out[index], ws_out[index]
        gi = (((fin + (f(1) - wsf) * bgc).astype(f) - gt[index]) * f(2)).astype(f) * cg
        gws = f(0)
        for ch in range(3):
            gws = f(gws - f(gi[ch] * bgc))
        acc_c = np.zeros(3, f)
        for idx, d0, alpha, T, on, w, c in chunks(offset, count):
            run = np.stack([(acc_c[ch] + _wave_scan((w * c[:, ch]).astype(f), np.add)).astype(f) for ch in range(3)], 1)
            T_after = (T * (f(1) - alpha)).astype(f)
            g = gi[0] * (T_after * c[:, 0] - (fin[0] - run[:, 0]))
            g = g + gi[1] * (T_after * c[:, 1] - (fin[1] - run[:, 1]))
            g = g + gi[2] * (T_after * c[:, 2] - (fin[2] - run[:, 2]))
            g = (d0 * (g + gws * (f(1) - wsf))).astype(f)
            gs[idx[on]] = g[on]
            grgb[idx[on]] = (gi[None, :] * w[:, None]).astype(f)[on]
            acc_c = run[63]
    return ws_out, img_out, gs, grgb
