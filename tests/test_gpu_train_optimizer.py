"""The fp16 training step's optimizer pass (csrc/train.hip: k_train_check, k_train_prologue<true>, k_train_adam<_Float16>, and
k_train_copy16 at refresh) on gradients the test chose, so that its input is known bit for bit.

Injection.  `NativeTrainStep` with a `grad_sync` runs forward + backward (mode 1), hands each of `gradient_buffers()` to
`grad_sync._reduce`, then runs the optimizer alone (mode 2).  The stub below overwrites g_table, g_deform, g_sigma0, g_sigma1 and
g_color (padding included) through `step.view(...)` in that hook.  A data-parallel step keeps the deformation MLP in the pass on the
canonical frame (`keep_deform`: another rank's batch may carry its gradient); the stub clears that flag in the argument record before
the optimizer-only call unless `single_process=False`, so that the pass decides as a single-process step does -- the canonical
frame's frozen deformation segment is what the sequence below is about.  `test_canonical_frame_under_data_parallelism...` leaves it.

Reference: `S.adam_pass64` (torch's single-tensor Adam in float64, validated against torch.optim.Adam on the CPU) from the state read
before the pass; torch's own `torch._amp_update_scale_` on CPU tensors for the scaler; `S.nonfinite16` over what Adam consumes for
the skip decision.  Bars: exp_avg / exp_avg_sq: the fp32 bar; the update p_new - p_old: the fp32 bar plus 2^-24 |p_old| (the
rounding of the stored parameter); the EMA shadow's change: the same with |shadow_old|; everything structural (fp16 copies equal
p_new.half() with all padding zero, the cleared accumulator, a skipped or frozen segment, step counts, scale, tracker) exact.
The 12.2 M-element table is compared exactly on the device and in float64 on its dense head (4096), its dense tail (2048: the
last full 1024-block and the 880-element tail block) and a seeded sample of 200 000 rows.

Measured on an MI355X, worst error in units of its bar over all passes of this module: exp_avg 0.002, exp_avg_sq 0.001; the update
0.038 on the table and 0.80 on the MLPs (sigma_net.1, whose weights are largest: the rounding of the stored parameter, which the
2^-24 |p_old| term is there for); the EMA shadow's change 0.12 on the table and 0.75 on the MLPs; everything exact held exactly.
overlap_table_update is accepted together with a grad_sync and replays the sequence to the same bits."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import train_stage_support as S

pytestmark = pytest.mark.gpu

N_RAYS = 64
LR, LR_NET, B1, B2, EPS = 1e-2, 1e-3, 0.9, 0.99, 1e-15
F16 = torch.float16
DEF_OUT = S.DEF_W * S.DEF_IN + (S.DEF_L - 1) * S.DEF_W * S.DEF_W           # offset of the deformation MLP's output block
COL_OUT = S.COL_W * S.COL_IN + (S.COL_L - 1) * S.COL_W * S.COL_W
GRAD_BUFFERS = ("g_table", "g_deform", "g_sigma0", "g_sigma1", "g_color")


class Inject:
    """The stand-in for dnerf_amd.dist.GradSync: `.world` and `._reduce`."""

    def __init__(self):
        self.world, self.step, self.grads, self.single_process, self._calls = 1, None, None, True, 0

    def _reduce(self, g):
        self._calls += 1
        if self._calls % 2:              # (two buffers per step: act once, after the second)
            return
        for name, value in self.grads.items():
            self.step.view(name, F16, tuple(value.shape)).copy_(value)
        if self.single_process:
            self.step._rec.keep_deform = 0


def _segments(rows):
    """Parameter i -> (gradient buffer, copy buffer, element offset, rows, cols, leading dimension, split column, group, lr): the
    table of csrc/train.hip build_segments, restated."""
    seg = [("g_table", "w_table", 0, rows, 2, 2, None, 0, LR), ("g_deform", "w_deform", 0, S.DEF_W, 76, S.DEF_IN, None, 1, LR_NET)]
    for i in range(1, S.DEF_L):
        seg.append(("g_deform", "w_deform", S.DEF_W * S.DEF_IN + (i - 1) * S.DEF_W * S.DEF_W, S.DEF_W, S.DEF_W, S.DEF_W, None, 1, LR_NET))
    seg.append(("g_deform", "w_deform", DEF_OUT, 3, S.DEF_W, S.DEF_W, None, 1, LR_NET))
    seg.append(("g_sigma0", "w_sigma0", 0, S.SIG_W, S.SIG_IN, S.SIG_IN, None, 0, LR_NET))
    seg.append(("g_sigma1", "w_sigma1", 0, S.SIG_OUT, S.SIG_W, S.SIG_W, None, 0, LR_NET))
    seg.append(("g_color", "w_color", 0, S.COL_W, 31, S.COL_IN, 16, 0, LR_NET))
    seg.append(("g_color", "w_color", S.COL_W * S.COL_IN, S.COL_W, S.COL_W, S.COL_W, None, 0, LR_NET))
    seg.append(("g_color", "w_color", COL_OUT, 3, S.COL_W, S.COL_W, None, 0, LR_NET))
    return seg


def _consumed(buf, seg):
    """What Adam reads (or writes) of a flat buffer for one segment: [rows, cols]."""
    _, _, off, rows, cols, ld, split, _, _ = seg
    v = buf.reshape(-1)[off:off + rows * ld].view(rows, ld)
    return torch.cat([v[:, :split], v[:, split + 1:cols + 1]], 1) if split is not None else v[:, :cols]


@functools.lru_cache(maxsize=None)
def _ctx(ema_decay, overlap):
    from dnerf_amd.bench_scene import build_scene
    from dnerf_amd.network import NeRFNetwork
    from dnerf_amd.train_native import NativeTrainStep
    sc = build_scene(H=32, W=32, device="cuda", seed=0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).cuda().train()
    model.load_state_dict(sc.model.state_dict())
    model.mean_count = 2000
    opt = torch.optim.Adam(model.get_params(LR, LR_NET), betas=(B1, B2), eps=EPS)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=3)
    inject = Inject()
    step = NativeTrainStep(model, opt, scaler, N_RAYS, "cuda", ema_decay=ema_decay, perturb=False, T_thresh=1e-4, grad_sync=inject,
                           overlap_table_update=overlap)
    inject.step = step
    step._build()
    rows = int(model.encoder.offsets[-1].item())
    assert rows * 2 == 12239728 and rows * 2 % 1024 == 880
    c = SimpleNamespace(step=step, inject=inject, model=model, opt=opt, scaler=scaler, rows=rows, seg=_segments(rows), ema_decay=ema_decay,
                        rays_o=sc.rays_o[:N_RAYS].contiguous(), rays_d=sc.rays_d[:N_RAYS].contiguous(),
                        target=torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(4)).cuda(),
                        ref_scale=torch.tensor([1024.0]), ref_tracker=torch.zeros(1, dtype=torch.int32), history=[])
    c.shapes = dict(g_table=(rows * 2,), g_deform=(S.DEF_FLAT,), g_sigma0=(64 * 32,), g_sigma1=(16 * 64,), g_color=(S.COL_FLAT,),
                    w_table=(rows * 2,), w_deform=(S.DEF_FLAT,), w_sigma0=(64 * 32,), w_sigma1=(16 * 64,), w_color=(S.COL_FLAT,))
    g = torch.Generator().manual_seed(5)
    sample = torch.randperm(rows, generator=g)[:200000]
    idx = torch.cat([torch.arange(4096), torch.arange(rows * 2 - 2048, rows * 2), (sample[:, None] * 2 + torch.arange(2)[None, :]).reshape(-1)])
    c.idx = torch.unique(idx).cuda()
    _check_copies(c)                       # k_train_copy16 at the first refresh: copies of the initial parameters, zero padding
    return c


def _gradients(c, seed):
    """Seeded gradients for every buffer, padding included: normal values x 1024 over a spread of magnitudes, a tenth exact zeros,
    some fp16 subnormals, +-65504 and negative values; the table's dense in its first 4096 and last 2048 elements, sparse elsewhere."""
    gen = torch.Generator().manual_seed(seed)

    def draw(n):
        v = torch.randn(n, generator=gen) * 1024.0 * torch.pow(10.0, torch.rand(n, generator=gen) * 4.0 - 4.0)
        v[torch.rand(n, generator=gen) < 0.1] = 0.0
        v = v.clamp(-65504.0, 65504.0).to(F16)
        k = torch.randperm(n, generator=gen)[:max(n // 50, 4)]
        special = torch.tensor([6e-8, -6e-8, 3e-6, 65504.0, -65504.0, -1.0], dtype=torch.float32).to(F16)
        v[k] = special[torch.arange(k.numel()) % special.numel()]
        return v

    out = {}
    for name in GRAD_BUFFERS[1:]:
        out[name] = draw(c.shapes[name][0]).cuda()
    n = c.rows * 2
    t = torch.zeros(n, dtype=F16)
    t[:4096], t[n - 2048:] = draw(4096), draw(2048)
    where = torch.unique(torch.randint(4096, n - 2048, (300000,), generator=gen))      # (distinct: an indexed store with repeats has no defined winner)
    t[where] = draw(where.numel())
    out["g_table"] = t.cuda()
    return out


def _state(c):
    """Device clones of everything the pass may write."""
    st, step = SimpleNamespace(), c.step
    step.flush()
    torch.cuda.synchronize()
    st.p = [p.detach().clone() for p in step.params]
    st.m = [c.opt.state[p]["exp_avg"].clone() for p in step.params]
    st.v = [c.opt.state[p]["exp_avg_sq"].clone() for p in step.params]
    st.ema = [e.clone() for e in step.ema_shadow] if step.ema_shadow is not None else None
    st.w = {k: step.view(k, F16, c.shapes[k]).clone() for k in c.shapes if k.startswith("w_")}
    st.g_table = step.view("g_table", F16, c.shapes["g_table"]).clone()
    st.steps = [float(v) for v in step.adam_steps.tolist()]
    st.scale, st.tracker = float(c.scaler._scale.item()), int(c.scaler._growth_tracker.item())
    return st


def _check_copies(c):
    """Every fp16 copy equals p.half() in its place (the colour input layer's shifted columns included) and is zero everywhere else
    (input columns 76..79, output rows 3..15, the colour layer's column 16)."""
    c.step.flush()
    want = {k: torch.zeros(c.shapes[k], dtype=F16, device="cuda") for k in c.shapes if k.startswith("w_")}
    for p, seg in zip(c.step.params, c.seg):
        _, wname, off, rows, cols, ld, split, _, _ = seg
        v = want[wname][off:off + rows * ld].view(rows, ld)
        h = p.detach().half().view(rows, cols)
        if split is not None:
            v[:, :split], v[:, split + 1:cols + 1] = h[:, :split], h[:, split:]
        else:
            v[:, :cols] = h
    for k, w in want.items():
        assert torch.equal(c.step.view(k, F16, c.shapes[k]), w), k


def _pick(c, i, t):
    """Segment i's tensor as float64 numpy: all of an MLP's, the head / tail / sample of the table's."""
    t = t.reshape(-1)
    return (t[c.idx] if i == 0 else t).double().cpu().numpy()


def _pass(c, time, grads, world=1, single_process=True, full=True, what=""):
    """One optimizer pass on injected gradients, checked.  -> (found_inf, state after)."""
    step = c.step
    c.inject.grads, c.inject.world, c.inject.single_process = grads, world, single_process
    before = _state(c)
    n_ema = step.ema_updates + 1
    step(c.rays_o, c.rays_d, c.target, time)
    after = _state(c)
    frozen_deform = float(time) == 0.0 and single_process
    consumed = [_consumed(grads[seg[0]], seg) for seg in c.seg]
    active = [not (frozen_deform and 1 <= i <= 8) for i in range(14)]
    found = any(S.nonfinite16(g.cpu().numpy()) for g, a in zip(consumed, active) if a)
    # ---- the decision, the step counts, the scaler ----
    steps = list(before.steps)
    if not found:
        steps[0] += 1
        steps[1] += 0 if frozen_deform else 1
    assert after.steps == steps, (what, after.steps, steps)
    c.ref_scale.fill_(before.scale)
    c.ref_tracker.fill_(before.tracker)
    torch._amp_update_scale_(c.ref_scale, c.ref_tracker, torch.tensor([1.0 if found else 0.0]), c.scaler.get_growth_factor(), c.scaler.get_backoff_factor(),
                             c.scaler.get_growth_interval())
    assert (after.scale, after.tracker) == (float(c.ref_scale), int(c.ref_tracker)), (what, after.scale, after.tracker)
    assert not after.g_table.any(), what                      # the table's accumulator: cleared by every pass, skipped or not
    _check_copies(c)
    inv_scale = 1.0 / (before.scale * world)
    decay = S.ema_decay_of(c.ema_decay, n_ema) if c.ema_decay is not None else None
    for i, seg in enumerate(c.seg):
        name = f"{what} segment {i}"
        if found or not active[i]:
            assert torch.equal(after.p[i], before.p[i]) and torch.equal(after.m[i], before.m[i]) and torch.equal(after.v[i], before.v[i]), name
        elif full:
            p0, m0, v0 = (_pick(c, i, t[i]) for t in (before.p, before.m, before.v))
            g = _pick(c, i, consumed[i].contiguous()).astype(np.float16)
            p, m, v = S.adam_pass64(p0, m0, v0, g, inv_scale, steps[seg[7]], seg[8], B1, B2, EPS)
            S.fp32_close(_pick(c, i, after.m[i]), m, f"{name} exp_avg")
            S.fp32_close(_pick(c, i, after.v[i]), v, f"{name} exp_avg_sq")
            S.fp32_close(_pick(c, i, after.p[i]) - p0, p - p0, f"{name} update", extra=2.0 ** -24 * np.abs(p0))
            assert np.abs(p - p0).max() > 0
        else:
            assert not torch.equal(after.p[i], before.p[i]), name
        if decay is not None and (full or found):
            s0, p_new = _pick(c, i, before.ema[i]), _pick(c, i, after.p[i])
            S.fp32_close(_pick(c, i, after.ema[i]) - s0, S.ema_pass64(s0, p_new, decay) - s0, f"{name} EMA shadow", extra=2.0 ** -24 * np.abs(s0))
    for k in ("w_table", "w_deform", "w_sigma0", "w_sigma1", "w_color"):
        if found:
            assert torch.equal(after.w[k], before.w[k]), (what, k)
    return found, after


def _with(grads, name, index, value):
    g = dict(grads)
    g[name] = grads[name].clone()
    g[name][index] = value
    return g


def _sequence(c):
    """The main sequence of four passes; -> the states after each."""
    c.initial = _state(c)
    assert c.history == [] and c.initial.steps == [0.0, 0.0]
    out = []
    found, st = _pass(c, 0.5, _gradients(c, 100), what="pass 1")                       # every segment updates
    assert not found and st.steps == [1.0, 1.0] and (st.scale, st.tracker) == (1024.0, 1)
    out.append(st)
    g = _with(_gradients(c, 101), "g_deform", 5, float("inf"))                          # the canonical frame: the frozen segment is left out of the check
    found, st = _pass(c, 0.0, g, what="pass 2 (canonical frame)")
    assert not found and st.steps == [2.0, 1.0] and (st.scale, st.tracker) == (1024.0, 2)
    for i in range(1, 9):
        assert torch.equal(st.p[i], out[0].p[i]) and torch.equal(st.m[i], out[0].m[i]) and torch.equal(st.v[i], out[0].v[i])
    assert torch.equal(st.w["w_deform"], out[0].w["w_deform"])
    out.append(st)
    found, st = _pass(c, 0.5, _gradients(c, 102), what="pass 3")                       # bias corrections: step 3 and step 2; the scale grows
    assert not found and st.steps == [3.0, 2.0] and (st.scale, st.tracker) == (2048.0, 0)
    out.append(st)
    g = _with(_gradients(c, 103), "g_sigma1", 517, float("inf"))
    found, st = _pass(c, 0.5, g, what="pass 4 (one inf)")
    assert found and st.steps == [3.0, 2.0] and (st.scale, st.tracker) == (1024.0, 0)
    out.append(st)
    c.history = out
    return out


@pytest.mark.parametrize("ema_decay", [None, 0.95], ids=["vector-path", "ema-scalar-path"])
def test_optimizer_sequence_on_injected_gradients(ema_decay):
    """Four passes: 0.5 (all update, steps [1, 1]); 0.0 (the deformation segments bit-unchanged, an inf in g_deform does not skip,
    steps [2, 1]); 0.5 (bias corrections at steps 3 and 2, the tracker reaches the interval: scale 2048, tracker 0); one inf in
    g_sigma1 (nothing but the accumulator and the EMA shadows changes: scale 1024, tracker 0).  Without a shadow the table's full
    blocks take the vectorised path and its last 880 elements the scalar one; with a shadow every block takes the scalar path."""
    _sequence(_ctx(ema_decay, False))


def test_overlapped_table_update_is_bit_identical():
    """overlap_table_update=True (the table's segment on a second stream, the workgroup ranges of launch_adam re-based) replays the
    sequence to the same bits."""
    a = _ctx(None, False)
    ha = a.history or _sequence(a)
    b = _ctx(None, True)
    hb = _sequence(b)
    for i in range(14):
        assert torch.equal(a.initial.p[i], b.initial.p[i]), ("the two models do not start from the same parameters", i)
    for k, (sa, sb) in enumerate(zip(ha, hb)):
        for i in range(14):
            if not torch.equal(sa.p[i], sb.p[i]):
                d = torch.nonzero(sa.p[i].reshape(-1) != sb.p[i].reshape(-1)).reshape(-1)
                print(f"[stage] overlap: pass {k + 1} segment {i}: {d.numel()} elements differ, first {d[:8].tolist()}, last {d[-4:].tolist()}",
                      sa.p[i].reshape(-1)[d[:4]].tolist(), sb.p[i].reshape(-1)[d[:4]].tolist(), a.initial.p[i].reshape(-1)[d[:4]].tolist())
            assert torch.equal(sa.p[i], sb.p[i]) and torch.equal(sa.m[i], sb.m[i]) and torch.equal(sa.v[i], sb.v[i]), (k, i)
        assert all(torch.equal(sa.w[n], sb.w[n]) for n in sa.w) and sa.steps == sb.steps and (sa.scale, sa.tracker) == (sb.scale, sb.tracker)


def _settled(ema_decay=None):
    c = _ctx(ema_decay, False)
    if not c.history:
        _sequence(c)
    c.scaler._scale.fill_(1024.0)
    c.scaler._growth_tracker.zero_()
    return c


def test_world_size_two_divides_the_gradients():
    """grad_divisor: inv_scale = 1 / (scale * 2)."""
    c = _settled()
    found, _ = _pass(c, 0.5, _gradients(c, 110), world=2, what="world 2")
    assert not found


def test_canonical_frame_under_data_parallelism_keeps_the_deformation_mlp_in_the_pass():
    """keep_deform as a data-parallel step leaves it: at time 0 the deformation MLP takes part in the pass (another rank's batch may
    carry its gradient) -- it is updated from the reduced gradient, both step counts move, and an inf in g_deform skips the step."""
    c = _settled()
    before = _state(c).steps
    found, st = _pass(c, 0.0, _gradients(c, 111), single_process=False, what="canonical frame, data parallel")
    assert not found and st.steps == [before[0] + 1, before[1] + 1]
    c.scaler._scale.fill_(1024.0)
    found, st2 = _pass(c, 0.0, _with(_gradients(c, 112), "g_deform", 5, float("inf")), single_process=False, what="canonical frame, data parallel, inf")
    assert found and st2.steps == st.steps


PLACES = ([("g_table", 0), ("g_table", -1)] + [("g_sigma0", 1024 + k) for k in range(8)] + [("g_sigma1", 16 * 64 - 1), ("g_deform", 0), ("g_deform", DEF_OUT + 2 * 128 + 127),
          ("g_color", COL_OUT + 2 * 64 + 63), ("g_color", 15), ("g_color", 17), ("g_color", 63 * 32 + 17)])


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["inf", "-inf", "nan"])
def test_one_non_finite_gradient_anywhere_skips_the_step(value):
    """A single non-finite value at the first / last element of g_table, each of the 8 positions of one 16-byte group of g_sigma0,
    the last element of g_sigma1, the first and the last real element of g_deform, the last real element of g_color's output block,
    and around the masked column of g_color's input layer: each skips the step (nothing but the accumulator changes) and backs the
    scale off."""
    c = _settled()
    base = _gradients(c, 120)
    for name, index in PLACES:
        c.scaler._scale.fill_(1024.0)
        c.scaler._growth_tracker.zero_()
        found, st = _pass(c, 0.5, _with(base, name, index, value), full=False, what=f"{value} at {name}[{index}]")
        assert found and (st.scale, st.tracker) == (512.0, 0), (name, index)


def test_the_masked_column_and_the_largest_finite_gradients_do_not_skip():
    """An inf in the colour input layer's column 16 (rows 0 and 63: never consumed by Adam, masked by the check), and +-65504 in
    every element of every MLP gradient: a normal update."""
    c = _settled()
    base = _gradients(c, 121)
    for index in (16, 63 * 32 + 16):
        c.scaler._scale.fill_(1024.0)
        c.scaler._growth_tracker.zero_()
        found, st = _pass(c, 0.5, _with(base, "g_color", index, float("inf")), what=f"inf at g_color[{index}] (column 16)")
        assert not found and (st.scale, st.tracker) == (1024.0, 1)
    g = dict(base)
    for name in GRAD_BUFFERS[1:]:
        sign = torch.where(torch.arange(base[name].numel()) % 3 == 0, -1.0, 1.0).to(F16).cuda()
        g[name] = sign * 65504.0
    c.scaler._scale.fill_(1024.0)
    c.scaler._growth_tracker.zero_()
    found, st = _pass(c, 0.5, g, what="+-65504 everywhere")
    assert not found and (st.scale, st.tracker) == (1024.0, 1)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_a_nan_hidden_weight_of_the_deformation_mlp_skips_the_step():
    """One weight of a hidden row of deform_net is NaN: that neuron's pre-activation is NaN on every sample, and the ReLU of the MLP
    chains (csrc/ffmlp_kernels.h, the reference's x * (x > 0)) keeps it, so the loss is non-finite, the step is skipped, the scaler
    backs off and no parameter, moment or fp16 copy changes.  (A select-ReLU turned the NaN into a dead neuron: a finite loss, a
    normal update, and a zero gradient for the offending row for good.)  The step's own gradients are used: nothing is injected."""
    from dnerf_amd.bench_scene import build_scene
    c = _settled()
    c.inject.grads, c.inject.world, c.inject.single_process = {}, 1, True
    # 64 rays through the middle of the 32 x 32 image (the fixture's own first 64 are a corner of it and sample nothing)
    sc = build_scene(H=32, W=32, device="cuda", seed=0)
    idx = (torch.arange(14, 18)[:, None] * 32 + torch.arange(8, 24)[None, :]).reshape(-1).cuda()
    rays_o, rays_d = sc.rays_o[idx].contiguous(), sc.rays_d[idx].contiguous()
    clean = float(c.step(rays_o, rays_d, c.target, 0.5, grads_only=True))
    assert np.isfinite(clean) and bool(c.step.view("g_deform", F16, c.shapes["g_deform"]).any()), "the rays sample nothing"
    p = c.step.params[2]                                  # deform_net.1.weight [128, 128]
    assert tuple(p.shape) == (S.DEF_W, S.DEF_W)
    old = float(p.data[5, 7])
    try:
        p.data[5, 7] = float("nan")
        c.step.refresh()
        before = _state(c)
        loss = float(c.step(rays_o, rays_d, c.target, 0.5))
        after = _state(c)
        assert not np.isfinite(loss), loss
        assert after.steps == before.steps and (after.scale, after.tracker) == (before.scale * 0.5, 0)
        for i in range(14):
            assert torch.equal(_bits(after.p[i]), _bits(before.p[i])) and torch.equal(after.m[i], before.m[i]) and torch.equal(after.v[i], before.v[i]), i
        assert all(torch.equal(after.w[k].view(torch.int16), before.w[k].view(torch.int16)) for k in before.w)
        assert not after.g_table.any()
    finally:
        p.data[5, 7] = old
        c.step.refresh()
        c.scaler._scale.fill_(1024.0)
        c.scaler._growth_tracker.zero_()
